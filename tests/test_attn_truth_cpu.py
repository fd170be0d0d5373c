"""tests/attn_truth.py and the cases of tests/test_attn_exact_gpu.py, checked without a GPU.

emulate() is the attention kernels' arithmetic in plain torch (test-only code): fp32 scores; P = exp2(S - shift) rounded
to bf16 at a zero shift, the fixed shift floor(min(b_row + 60, 126 - b_row)) (b_row = |q_row| x the key bound), or the
online max per 64-key tile with the lazy rescale (a row moves its shift only when its tile max exceeds it by more than
24); the row sum of the rounded P; O = acc * (1 / lsum) rounded once to bf16; key splits as fp32 partials with lse =
shift + log2(lsum) merged by attn_merge_splits's formula (weights exp2(lse_s - max lse)); the gated pair's choice per
256-row block; the tail split of the last head's last rows.

For every GPU case: the premise holds (structured inputs have exact fp32 scores, Gaussian ones a worst-case score error
<= 2^-10 nats; the selector's gap is asserted by its builder) and the emulated output passes the case's own check
(test_attn_exact_gpu.check: torch.equal with v[pi], or error / bound <= 1). The same checks reject each wrong arithmetic
of MUTANTS on at least one of the cases listed for it:
  drop_last    the last key dropped            pad_key     one padded key admitted with score 0 (v of the last row)
  pi_off       rows off by one                 swap_cols   two head-dim columns swapped
  swap_bh      (b, h) strides exchanged        merge_w0    merge weights of split 0 used for every split
  merge_mx0    merge weights formed against split 0's lse, not the largest (the weights are then all scaled alike and
               cancel, until the spread passes fp32's exponent range: only the `far` cases see it)
  no_rescale   the online rescale skipped
"""
import math

import pytest
import torch

import attn_truth as T
import test_attn_exact_gpu as G

BF16 = torch.bfloat16
F32 = torch.float32


def _exp2_bf16(x):
    return torch.exp2(x.to(F32)).to(BF16).to(F32)


def _fixed_shift(qrow_norm, kb):
    b_row = (qrow_norm * kb).to(F32)
    return torch.floor(torch.minimum(b_row + 60.0, 126.0 - b_row))


def _attend(q, k, v, mode, kb, mut):
    """One (b, h), one key range: (o [Lq, 128] fp32 = acc / lsum, lse [Lq]). q, k, v fp32 [L, 128]."""
    S = q @ k.T
    if mut == "pad_key":
        S = torch.cat([S, torch.zeros(S.shape[0], 1)], 1)
        v = torch.cat([v, v[-1:]], 0)
    Lk = S.shape[1]
    if mode in ("zero", "fixed"):
        shift = torch.zeros(S.shape[0]) if mode == "zero" else _fixed_shift(q.norm(dim=-1), kb)
        P = _exp2_bf16(S - shift[:, None])
        lsum = P.double().sum(-1).to(F32)
        acc = (P.double() @ v.double()).to(F32)
    else:
        m = torch.zeros(S.shape[0])
        lsum = torch.zeros(S.shape[0])
        acc = torch.zeros(S.shape[0], v.shape[1])
        for t0 in range(0, Lk, T.KBLK):
            St = S[:, t0:t0 + T.KBLK] - m[:, None]
            mx = St.max(-1).values
            if t0 == 0:
                d, alpha = mx, torch.zeros_like(mx)
            else:
                d = torch.where(mx > T.LAZY, mx, torch.zeros_like(mx))
                alpha = torch.exp2(-d)
                if mut == "no_rescale":
                    alpha = torch.ones_like(mx)
            m = m + d
            P = _exp2_bf16(St - d[:, None])
            lsum = lsum * alpha + P.double().sum(-1).to(F32)
            acc = acc * alpha[:, None] + (P.double() @ v[t0:t0 + T.KBLK].double()).to(F32)
        shift = m
    inv = (1.0 / lsum).to(F32)
    return acc * inv[:, None], shift + torch.log2(lsum)


def _merge(parts, mut):
    o = torch.stack([p[0] for p in parts])      # [s, Lq, 128]
    lse = torch.stack([p[1] for p in parts])    # [s, Lq]
    mx = lse[0] if mut == "merge_mx0" else lse.max(0).values
    w = torch.exp2(lse - mx).to(F32)
    if mut == "merge_w0":
        w = w[:1].expand_as(w)
    w = torch.where(lse > -math.inf, w, torch.zeros_like(w))
    acc = (w[..., None] * o).sum(0)
    den = w.sum(0)
    inv = torch.where(den > 0, 1.0 / den, torch.zeros_like(den))
    return acc * inv[:, None]


def _one(q, k, v, mode, kb, n_split, mut):
    """One (b, h): the splits keep the launch's tile ranges; a dropped last key only shortens the last one, a padded
    key joins the last one (the ragged tile's)."""
    full = k.shape[0]
    Lk = full - (1 if mut == "drop_last" else 0)
    tps = -(-(-(-full // T.KBLK)) // n_split)
    parts = []
    for s in range(n_split):
        lo, hi = s * tps * T.KBLK, min(Lk, (s + 1) * tps * T.KBLK)
        if lo < hi:
            parts.append(_attend(q, k[lo:hi], v[lo:hi], mode, kb, None if mut == "pad_key" and hi != Lk else mut))
    return parts[0][0] if n_split == 1 else _merge(parts, mut)


def emulate(name, mut=None):
    """The case's output as the kernels' arithmetic gives it ([B, Lq, H, 128] bf16), or as a wrong one does."""
    c, d = G.case_data(name)
    route = c["route"]
    form = G.ROUTES[route][3]
    q = d["qn"] if c["kind"] in G.QN_KINDS else d["q"]
    nb, kmax = G.launch_bounds(c, d, q)
    kb = None if nb is None else float(torch.tensor(nb[1], dtype=F32))
    mode = "online" if nb is None else ("zero" if route in G.ZERO else "fixed")
    q, k, v = q.float(), d["k"].float(), d["v"].float()
    if mut == "swap_bh":
        assert c["B"] == c["H"]
        k, v = k.transpose(0, 2), v.transpose(0, 2)
    B, H, Lq = c["B"], c["H"], c["Lq"]
    out = torch.empty(B, Lq, H, T.D)
    for b in range(B):
        for h in range(H):
            qq, kk, vv = q[b, :, h], k[b, :, h], v[b, :, h]
            if form.get("gated"):
                kbg = float(torch.tensor(kmax, dtype=F32) * torch.tensor(1.001, dtype=F32))
                for r0 in range(0, Lq, 256):
                    blk = qq[r0:r0 + 256]
                    fixed_ok = blk.norm(dim=-1).max().item() * kmax * 1.001 <= 110.0
                    out[b, r0:r0 + 256, h] = _one(blk, kk, vv, "fixed" if fixed_ok else "online", kbg, c["n_split"], mut)
            elif c.get("tail"):
                o = _one(qq, kk, vv, mode, kb, 1, mut)
                if b == B - 1 and h == H - 1:
                    o[c["t0"]:] = _one(qq[c["t0"]:], kk, vv, mode, kb, c["tail_s"], mut)
                out[b, :, h] = o
            else:
                out[b, :, h] = _one(qq, kk, vv, mode, kb, c["n_split"], mut)
    if mut == "pi_off":
        out = out.roll(-1, 1)
    if mut == "swap_cols":
        out[..., [5, 6]] = out[..., [6, 5]]
    return c, d, out.to(BF16)


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_premise_and_emulation(name):
    c, d = G.case_data(name)
    form = G.ROUTES[c["route"]][3]
    q = d["qn"] if c["kind"] in G.QN_KINDS else d["q"]
    nb, _ = G.launch_bounds(c, d, q)
    qn, kn = T.norm_bounds(q, d["k"], 1.0)
    if nb is not None:  # the launch's bounds are bounds, and inside the window of the route under test
        assert nb[0] >= qn and nb[1] >= kn
        prod = nb[0] * nb[1]
        if form.get("fp8"):
            assert prod <= 60.0
        elif form.get("gated"):
            assert prod > 110.0
        elif c["route"] in G.ZERO:
            assert prod <= 96.0
        elif c["route"] in ("cross_fixed",):
            assert 96.0 < prod <= 98.0
        else:
            assert prod <= (110.0 if c["Lk"] > 4096 else 98.0)
    if c["kind"] in ("selector", "far"):
        assert T.exact_scores(q, d["k"])  # (the gap precondition is asserted by the builder)
        err = 0.0
    elif c["kind"] == "qnorm":
        assert d["top"] <= 110.0
        err = 0.0  # (exactness by the gap alone: a score error moves no P against the winner's)
    elif c["kind"] in ("uniform", "gap"):
        assert T.exact_scores(q, d["k"])
        err = 0.0
        if c["kind"] == "gap":  # the case is the case its name says
            s = torch.einsum("bqhd,bkhd->bhqk", q.float(), d["k"].float())
            first = s[..., :64].max(-1).values
            assert torch.equal(first, s[..., d["anchor"]])
            assert torch.equal(s[..., d["late"]] - first, d["d"].expand_as(first))
            assert d["late"] // 64 == (c["Lk"] - 1) // 64 and c["Lk"] % 64 != 0
            if c["n_split"] > 1:
                assert T.split_of(d["late"], c["Lk"], c["n_split"]) == c["n_split"] - 1
        else:
            lo = 126.0 - d["b_row"].max().item() * 1.0005 * 1.0005
            assert c["aligned"] or -d["b_row"].max().item() - math.floor(lo) >= -126.0  # the smallest term is normal
    elif c["kind"] == "qngap":
        err = T.score_error_nats(q, d["k"])
        s = torch.einsum("bqhd,bkhd->bhqk", q.float(), d["k"].float())
        first = s[..., :64].max(-1).values
        assert torch.equal(first, s[..., d["anchor"]])
        gap = (s[..., d["late"]] - first).permute(0, 2, 1)
        assert (gap - d["target"][None, :, None]).abs().max().item() < 0.1
        assert ((gap > T.LAZY) == (d["target"][None, :, None] > T.LAZY)).all()
        assert d["late"] // 64 == (c["Lk"] - 1) // 64 and c["Lk"] % 64 != 0
    else:
        err = T.score_error_nats(q, d["k"])
    if c.get("tie"):
        a, b = c["tie"]
        assert a // 64 != b // 64
        n = c.get("tail_s", c["n_split"])
        if n > 1:
            assert T.split_of(a, c["Lk"], n) != T.split_of(b, c["Lk"], n)
        if c.get("tail"):
            for n2 in range(2, 9):  # whatever split count the plan picks, the pair spans two tail splits
                if n2 <= -(-c["Lk"] // 64) and -(-(-(-c["Lk"] // 64)) // -(-(-(-c["Lk"] // 64)) // n2)) == n2:
                    assert T.split_of(a, c["Lk"], n2) != T.split_of(b, c["Lk"], n2)
            tr = d["tie_rows"][-1, :, -1]
            assert tr[c["t0"]:].any() and tr[:c["t0"]].any()
    assert err <= T.PREMISE, err
    _, _, o = emulate(name)
    ok, text = G.check(name, c, d, o)
    print(f"{text}; worst-case score error {err:.2e} nats")
    assert ok, text


MUTANTS = {
    "drop_last": ["sel-self_fixed-4097-s65", "sel-wq384-4200-s1", "sel-cross_zero-77-s1", "sel-f8_self-4200-s3"],
    "pad_key": ["uni-self_fixed-anti", "uni-cross_fixed-anti", "uni-wq384-anti"],
    "pi_off": ["sel-self_online-4200-s1", "sel-pers_zero-130-s1"],
    "swap_cols": ["sel-self_fixed-4200-s3", "sel-f8_cross-64-s1"],
    "swap_bh": ["sel-self_np_fixed-4200-s1", "sel-cross_gated-512-s3"],
    "merge_w0": ["sel-wq320-4200-s3", "sel-self_online-4097-s65", "tail-self_fixed"],
    "merge_mx0": ["far-self_online-s3", "far-wq384-s3", "far-cross_zero-s3"],
    "no_rescale": ["gap-self_online-s1", "gap-pers_online-s1", "sel-cross_online-512-s1", "qngap-online-rope1"],
}


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_wrong_arithmetic_is_rejected(mut):
    for name in MUTANTS[mut]:
        c, d, o = emulate(name, mut)
        ok, text = G.check(name, c, d, o)
        print(f"{mut}: {text}")
        assert not ok, (mut, name)


def test_reference_and_bound():
    """reference64 against an independent softmax in float64, and the bound's terms."""
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(1, n, 2, T.D, generator=g).to(BF16) for n in (5, 9, 9))
    ref, A = T.reference64(q, k, v, 0.3)
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * 0.3
    w = torch.exp2(s - s.max(-1, keepdim=True).values)
    w = w / w.sum(-1, keepdim=True)
    assert torch.allclose(ref, torch.einsum("bhqk,bkhd->bqhd", w, v.double()), rtol=1e-12, atol=1e-14)
    assert (A >= ref.abs() - 1e-12).all()
    assert torch.equal(T.bound(ref, A), 2.0 ** -9 * ref.abs() + 2.0 ** -8 * A)
    # 128 * 2^-24 * 110 * ln 2: every bounded route's worst case
    assert abs(T.D * 2.0 ** -24 * 110 * math.log(2.0) - 5.8e-4) < 1e-5 and T.D * 2.0 ** -24 * 184 * math.log(2.0) <= T.PREMISE


def test_selector_targets():
    """pi holds every named key and row, is injective while Lq <= Lk and differs between (b, h)."""
    keys, rows = T.key_targets(4097, (1, 3, 65)), T.row_targets(801, 384, 96)
    assert {0, 63, 64, 65, 4096, 4032, 4095}.issubset(keys) and {0, 800, 383, 384, 95, 96, 768}.issubset(rows)
    d = T.selector(2, 2, 801, 4097, *G.M90, 1, keys=keys, rows=rows)
    for b in range(2):
        for h in range(2):
            assert set(keys).issubset(set(d["pi"][b, h].tolist()))
            assert all(int(d["pi"][b, h, r]) in keys for r in rows[:len(keys)])
    assert not torch.equal(d["pi"][0, 0], d["pi"][0, 1]) and not torch.equal(d["pi"][0, 0], d["pi"][1, 0])
    d = T.selector(2, 2, 545, 3, *G.M90, 1, keys=T.key_targets(3), rows=T.row_targets(545, 256, 32))
    assert set(d["pi"].unique().tolist()) == {0, 1, 2}


def test_zero_shift_long_key_names_unreachable():
    """attn_fwd_m16<self, prescaled, zero shift> and the two attn_fwd_wq<.., zero shift> names of attn_route.h's table
    are routes of no launch: by attn_route, long keys (Lk > 4096) with bounds up to a product of 110 take mode 0, any
    other mode 2. Swept over the self forms, key counts on both sides of the width threshold, bound products 0.25 ..
    130 in steps of 0.25 (every window edge: 63, 96, 98, 110), prescaled with and without key slots; short keys do
    reach the zero shift (the sweep is not vacuous)."""
    from cosmos_predict2 import _native as N
    prev = N.attn_self_select(1)
    try:
        for form in (0, 1, 320, 384):
            N.attn_self_select(form)
            for i in range(1, 521):
                p = i / 4.0
                for Lk in (4097, 8192, 8193, 109120):
                    for pre in (True, 2):
                        nm = N.attn_kernel_name(Lk, norm_bounds=(p / 8.0, 8.0), prescaled=pre)
                        assert "zero shift" not in nm, (form, p, Lk, pre, nm)
                        if p <= 110.0 and pre is True:
                            assert "fixed shift" in nm, (form, p, Lk, nm)
            assert "zero shift" in N.attn_kernel_name(4096, norm_bounds=(90.0 / 8.0, 8.0), prescaled=True)
    finally:
        N.attn_self_select(prev)
