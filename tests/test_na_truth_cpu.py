"""tests/na_truth.py's known-answer material and the cases of tests/test_sparse_attn_exact_gpu.py, checked without a
GPU, in the manner of tests/test_attn_truth_cpu.py.

emulate() is cp25_attn_na3d's arithmetic in plain torch (test-only code), walking the same plan tables: tiles of 128
slots, a wave = 32 slots (an empty slot computes on the tile's first row and stores nothing); the box decoded from its
corner as the kernel does (key c -> jw = c mod Kw, jh = c div Kw mod Kh, jt = c div (Kw Kh)), 64-key tiles whose pads
repeat the box's last key and are masked to -inf; fp32 scores; the online max with the WAVE-level lazy rescale (when any
row of the wave has a tile max more than 24 above its shift, every row of the wave moves to max(shift, tile max));
P = exp2(S - shift) rounded to bf16 for P V, the row sum of the unrounded P; O = acc * (1 / sum) rounded once to bf16.

For every GPU case the premises hold (exact fp32 scores, the selector's gap and the lure's margin asserted by the
builders, the gap rows' and the staircase's tile maxima where the case says) and the emulation passes the case's own
check: bit for bit on the selector, lure and one-key cases, error / bound <= 1 on the bounded ones. That is a condition
on the inputs, not a tolerance. The same checks reject each wrong kernel of MUTANTS on the cases listed for it:
  ragged_off1  the ragged tile's mask off by one (the first pad, a copy of the last key, admitted)
  no_l_rescale the accumulator rescaled but not the row sum
  v_neighbor   a key's V row taken from the next key of its tile
  swap_hw      the box's h and w corners exchanged
  dil_axis     the dilations applied to the wrong axes
  store_empty  an empty slot's row stored (its id -1 clamped to token 0)
  stale_q      the second tile of a group reading the first tile's query rows
"""
import math

import numpy as np
import pytest
import torch

import attn_truth as AT
import na_truth as NT
import test_sparse_attn_exact_gpu as G
from cosmos_predict2 import sparse_attn as SA

BF16 = torch.bfloat16
F32 = torch.float32
KB = AT.KBLK


def emulate(grid_name, q, k, v, fused=False, ln2=False, mut=None):
    """[B, L, H, 128] bf16: what the kernel's arithmetic gives (the layout `fused` changes no bit), or a wrong one."""
    geo = NT.geometry(grid_name)
    q_tok, box = (torch.from_numpy(np.asarray(x)).long() for x in G.plan_host(grid_name))
    _, Hg, Wg = geo["grid"]
    _, Kh, Kw = geo["window"]
    dt, dh, dw = geo["dilation"]
    if mut == "dil_axis":
        dt, dh, dw = dh, dw, dt
    L, nk = geo["L"], geo["nkeys"]
    nt = -(-nk // KB)
    scale = float(torch.tensor(G.LN2, dtype=F32) * torch.tensor(1.4426950408889634, dtype=F32)) if ln2 else 1.0
    B, _, H, _ = q.shape
    qf, kf, vf = q.float(), k.float(), v.float()
    out = torch.full((B, L, H, AT.D), G.SENT, dtype=BF16)
    c = torch.arange(nt * KB).clamp(max=nk - 1)
    jw, jh, jt = c % Kw, c // Kw % Kh, c // Kw // Kh
    pad = torch.arange(nt * KB) >= (nk + 1 if mut == "ragged_off1" else nk)
    first = list(range(len(q_tok)))
    for t in range(1, len(q_tok)):
        if torch.equal(box[t], box[t - 1]):
            first[t] = first[t - 1]
    for tile in range(len(q_tok)):
        t0, h0, w0 = (int(x) for x in box[tile, :3])
        if mut == "swap_hw":
            h0, w0 = w0, h0
        ktok = (((t0 + jt * dt) * Hg + h0 + jh * dh) * Wg + w0 + jw * dw).clamp(0, L - 1)
        vtok = ktok.view(nt, KB).roll(-1, 1).reshape(-1) if mut == "v_neighbor" else ktok
        rows = q_tok[tile]
        src = q_tok[first[tile]] if mut == "stale_q" else rows
        qid = torch.where((src >= 0) & (src < L), src, src[0])
        for w in range(4):
            sl = slice(32 * w, 32 * w + 32)
            S = torch.einsum("bqhd,bkhd->bhqk", qf[:, qid[sl]], kf[:, ktok])  # [B, H, 32, nt 64]
            S = S.masked_fill(pad, -math.inf)
            m = torch.full((B, H, 32), -math.inf)
            lsum = torch.zeros(B, H, 32)
            acc = torch.zeros(B, H, 32, AT.D)
            for t in range(nt):
                St = S[..., t * KB:(t + 1) * KB]
                tmax = St.max(-1).values * scale
                lazy = (tmax > m + AT.LAZY).any(-1, keepdim=True)  # wave-uniform
                m_new = torch.maximum(m, tmax)
                alpha = torch.exp2(m - m_new)
                if mut != "no_l_rescale" or t == 0:
                    lsum = torch.where(lazy, lsum * alpha, lsum)
                acc = torch.where(lazy[..., None], acc * alpha[..., None], acc)
                m = torch.where(lazy, m_new, m)
                P = torch.exp2((St.double() * scale - m[..., None].double()).to(F32))
                lsum = (lsum.double() + P.double().sum(-1)).to(F32)
                vt = vf[:, vtok[t * KB:(t + 1) * KB]].double()  # [B, 64, H, D]
                acc = (acc.double() + torch.einsum("bhqk,bkhd->bhqd", P.to(BF16).double(), vt)).to(F32)
            o = (acc * (1.0 / lsum)[..., None]).to(BF16).permute(0, 2, 1, 3)  # [B, 32, H, D]
            live = (rows[sl] >= 0) & (rows[sl] < L)
            if mut == "store_empty":
                out[:, rows[sl].clamp(min=0)] = o
            else:
                out[:, rows[sl][live]] = o[:, live]
    return out


# ---------------------------------------------------------------------------------------------------------------------
# the geometry

FACTS = {  # name: (keys per box, live keys of the last key tile, groups, smallest and largest group)
    "one_key": (1, 1, 60, 1, 1), "k63": (63, 63, 4, 24, 30), "k65": (65, 1, 18, 10, 15),
    "k130_block": (130, 2, 4, 130, 130), "k195": (195, 3, 8, 24, 64), "k385_full": (385, 1, 1, 385, 385),
    "dil_t": (24, 24, 18, 12, 24),
}


@pytest.mark.parametrize("name", list(NT.NA_EXACT_CASES))
def test_boxes_against_the_plan(name):
    """The resolved mask and box_keys against sparse_attn.plan_tables: every token in exactly one slot, the box of its
    tile (decoded as the kernel decodes it) equal to its mask row, in box_keys' order; groups cut into tiles of 128 in
    ascending token order."""
    geo = NT.geometry(name)
    T, H, W = geo["grid"]
    L, win, dil = geo["L"], geo["window"], geo["dilation"]
    sizes = [len(qs) for qs, _ in geo["groups"]]
    assert FACTS[name] == (geo["nkeys"], (geo["nkeys"] - 1) % KB + 1, len(sizes), min(sizes), max(sizes))
    assert L <= 520 and (geo["mask"].sum(1) == geo["nkeys"]).all()
    q_tok, box = G.plan_host(name)
    live = q_tok[q_tok >= 0]
    assert sorted(live.tolist()) == list(range(L)) and (q_tok[:, 0] >= 0).all()
    seen = {}
    for row, (t0, h0, w0, _) in zip(q_tok, box.tolist()):
        keys = [((t0 + a * dil[0]) * H + h0 + b * dil[1]) * W + w0 + c * dil[2]
                for a in range(win[0]) for b in range(win[1]) for c in range(win[2])]
        toks = row[row >= 0].tolist()
        assert (row[len(toks):] == -1).all()
        gi = int(geo["group_of"][toks[0]])
        qs, ks = geo["groups"][gi]
        assert keys == ks, (name, gi)
        want = torch.zeros(L, dtype=torch.bool)
        want[keys] = True
        for tok in toks:
            assert torch.equal(geo["mask"][tok], want), (name, tok)
        seen.setdefault(gi, []).extend(toks)
        assert len(toks) == min(128, len(qs) - (len(seen[gi]) - len(toks)))  # full tiles first
    assert all(seen[gi] == qs for gi, (qs, _) in enumerate(geo["groups"]))


@pytest.mark.parametrize("name", sorted(NT.NA_CASES))
def test_resolved_forms_equal_the_parameter_forms(name):
    grid, params = NT.NA_CASES[name]
    _, win, st, dil = NT._resolve(*grid, params)
    assert torch.equal(NT.mask_resolved(grid, win, st, dil), NT.na_mask(*grid, params))
    assert NT.axis_sets_resolved(grid, win, st, dil) == NT.na_axis_sets(*grid, params)
    mask = NT.na_mask(*grid, params)
    for qs, ks in NT.box_keys(grid, win, st, dil):
        assert qs == sorted(qs) and all(mask[i].nonzero()[:, 0].tolist() == sorted(ks) for i in qs)


def test_a_window_of_one_key_is_one_key():
    assert NT.axis_sets_resolved((2, 5, 6), (1, 1, 1), (1, 1, 1), (1, 1, 1))[1] == [[i] for i in range(5)]
    assert torch.equal(NT.geometry("one_key")["mask"], torch.eye(60, dtype=torch.bool))
    assert NT.na_mask(2, 5, 6, dict(window_size=(1, 1, 1))).all()  # the parameter form: the full extent


def test_launch_shapes():
    """n_tiles H B below 8, no multiple of 8 and a multiple of 8; B != H somewhere; most launches on fused views."""
    wgs = {g: len(G.plan_host(g)[0]) * G.BH[g][0] * G.BH[g][1] for g in NT.NA_EXACT_CASES}
    assert wgs["k385_full"] == 4 and wgs["k63"] == 12 and G.BH["k130_block"] == (2, 2) and wgs["k130_block"] % 8 == 0
    assert any(b != h for b, h in G.BH.values())
    q_tok = G.plan_host("k130_block")[0]
    assert len(q_tok) == 8 and sorted((q_tok >= 0).sum(1).tolist()) == [2] * 4 + [128] * 4
    n = [G.launches(name) for name in G.CASES]
    assert sum(f for f, _ in n) >= sum(c for _, c in n)


# ---------------------------------------------------------------------------------------------------------------------
# the cases

def _box_scores(d, geo, gi):
    """fp32 scores of group gi's queries against its box, in box order: [B, H, n, nkeys]."""
    qs, ks = geo["groups"][gi]
    return torch.einsum("bqhd,bkhd->bhqk", d["q"][:, qs].float(), d["k"][:, ks].float())


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_premise_and_emulation(name):
    c, d = G.CASES[name], G.case_data(name)
    geo = NT.geometry(c["grid"])
    fam = c["family"]
    if fam in ("sel", "out"):
        base = d["base"] if fam == "out" else d
        assert AT.exact_scores(base["q"], base["k"])  # (the gap is asserted by the builder)
        targets = NT.box_targets(geo["window"])
        Kt, Kh, Kw = geo["window"]
        assert {0, geo["nkeys"] - 1, (Kh - 1) * Kw, Kw - 1, (Kt - 1) * Kh * Kw}.issubset(targets)
        assert {x for x in (63, 64, 65, 127, 128, 191, 192) if x < geo["nkeys"]}.issubset(targets)
        for qs, _ in geo["groups"]:
            for b in range(base["pos"].shape[0]):
                for h in range(base["pos"].shape[1]):
                    assert set(targets).issubset(set(base["pos"][b, h, qs].tolist()))
        if geo["nkeys"] > 1 and base["pos"][:, :, 0].numel() > 1:  # pi differs between (b, h)
            assert not torch.equal(base["pos"][0, 0], base["pos"][-1, -1])
        if fam == "out":
            n = len(geo["groups"])
            assert [lu["group"] for lu in d["lured"]] == sorted({0, n // 2, n - 1})
            axes = {a for lu in d["lured"] for a, _ in lu["steps"]}
            assert axes == {a for a in range(3) if geo["window"][a] * geo["dilation"][a] < geo["grid"][a]
                            or geo["dilation"][a] > 1}
            if c["grid"] == "dil_t":  # a token of the other dilation group, between two keys of the box, on every axis
                T, H, W = geo["grid"]
                for lu in d["lured"]:
                    ks = geo["groups"][lu["group"]][1]
                    for a, coord in enumerate((lambda x: x // (H * W), lambda x: x // W % H, lambda x: x % W)):
                        inside = sorted({coord(x) for x in ks})
                        assert any(ax == a and inside[0] < coord(t) < inside[-1] for ax, t in lu["steps"])
    elif fam == "uni":
        assert AT.exact_scores(d["q"], d["k"])
        for gi in range(len(geo["groups"])):
            s = _box_scores(d, geo, gi)
            assert torch.equal(s, s[..., :1].expand_as(s))
        assert sorted(set(d["b_row"].tolist())) == [0.0, 8.0, 32.0, 64.0][:max(1, min(4, geo["L"]))]
    elif fam == "gap":
        assert AT.exact_scores(d["q"], d["k"])
        for gi, (qs, ks) in enumerate(geo["groups"]):
            s = _box_scores(d, geo, gi)
            first = s[..., :KB].max(-1).values
            assert ks.index(d["anchors"][gi]) < KB and torch.equal(first, s[..., ks.index(d["anchors"][gi])])
            assert d["lates"][gi] == ks[-1] and (len(ks) - 1) // KB == -(-len(ks) // KB) - 1 and len(ks) % KB in (1, 2)
            assert torch.equal(s[..., -1] - first, d["d"][qs].expand_as(first))
            for w0 in range(0, len(qs), 32):  # odd slices straddle kLazy, even ones stay below
                dd = d["d"][qs[w0:w0 + 32]]
                if (w0 // 32) % 2 == 1 and len(dd) == 32:
                    assert (dd > AT.LAZY).any() and (dd < AT.LAZY).any()
                else:
                    assert (dd < AT.LAZY).all()
            assert len(d["probes"][gi]) >= 4 and (d["d"][d["probes"][gi]] == 22.0).all()
            pq = d["q"][:, d["probes"][gi]]
            assert torch.equal(pq, pq[:, :1].expand_as(pq))
    elif fam == "stair":
        assert AT.exact_scores(d["q"], d["k"])
        for gi, (qs, ks) in enumerate(geo["groups"]):
            s = _box_scores(d, geo, gi)
            nt = -(-len(ks) // KB)
            mx = torch.stack([s[..., j * KB:(j + 1) * KB].max(-1).values for j in range(nt)], -1)  # [B, H, n, nt]
            want = 20.0 + NT.STAIR_STEP * torch.arange(nt)
            want = want.flip(0) if c.get("reverse") else want
            assert torch.equal(mx, want * d["mag"][qs][None, None, :, None])
            assert nt == 7 and (NT.STAIR_STEP > AT.LAZY) and (0.5 * NT.STAIR_STEP < AT.LAZY)
            assert {float(x) for x in d["mag"][qs[:32]].tolist()} == {0.5, 1.0}
    else:
        assert fam == "one" and geo["nkeys"] == 1
    ok, text = G.evaluate(name, emulate)
    print(text)
    assert ok, text


MUTANTS = {
    "ragged_off1": ["gap-k385_full", "gap-k130_block", "uni-k65", "uni-k195"],
    "no_l_rescale": ["gap-k385_full", "gap-k130_block", "stair-k385_full"],
    "v_neighbor": ["sel-k63", "sel-k385_full", "selln2-dil_t", "out-k130_block"],
    "swap_hw": ["sel-k65", "out-k63", "sel-dil_t"],
    "dil_axis": ["sel-dil_t", "out-dil_t", "uni-dil_t"],
    "store_empty": ["sel-k130_block", "one-one_key", "uni-k65"],
    "stale_q": ["sel-k130_block", "sel-k385_full", "out-k130_block"],
}


@pytest.mark.parametrize("mut", list(MUTANTS))
def test_wrong_kernel_is_rejected(mut):
    for name in MUTANTS[mut]:
        ok, text = G.evaluate(name, lambda *a: emulate(*a, mut=mut))
        print(f"{mut}: {text}")
        assert not ok, (mut, name)


def test_reference_and_emulation_on_gaussian_data():
    """reference64_masked against na_attention_truth (an independent softmax), and the emulation on plain Gaussian data
    of every grid within the aggregate tolerance tests/test_sparse_attn_gpu.py holds the kernel to (rel-L2 <= 4e-3): it
    is a model of the kernel, not only of the structured cases."""
    for i, name in enumerate(NT.NA_EXACT_CASES):
        geo = NT.geometry(name)
        g = AT._gen(900 + i)
        q = (torch.randn(1, geo["L"], 2, AT.D, generator=g) * 0.25).to(BF16)
        k, v = (torch.randn(1, geo["L"], 2, AT.D, generator=g).to(BF16) for _ in range(2))
        ref, A = NT.reference64_masked(q, k, v, geo["mask"])
        truth = NT.na_attention_truth(q, k, v, geo["mask"], scale=math.log(2.0))
        assert torch.allclose(ref, truth, rtol=1e-12, atol=1e-14) and (A >= ref.abs() - 1e-12).all()
        err = ((emulate(name, q, k, v).double() - ref).norm() / ref.norm()).item()
        print(f"{name}: gaussian, emulation rel-L2 {err:.2e}")
        assert err <= 4e-3
