"""Ground truth for the DiT attention kernels: a float64 reference, the per-element bound and structured inputs whose
expected output is known without running any attention. No GPU, no product code (tests/test_attn_truth_cpu.py checks
all of it against an emulation of the kernels' arithmetic; tests/test_attn_exact_gpu.py runs the kernels on it).

Layout: q [B, Lq, H, 128], k / v [B, Lk, H, 128], bf16, as cosmos_predict2._native.attn_fwd takes them. Scores are in
log2 units: a prescaled q carries softmax_scale * log2 e, so softmax weights are exp2(q . k * log2_scale) with
log2_scale = 1; an unscaled launch has log2_scale = softmax_scale * log2 e.

Bound (tests/test_vae_attn_edges_gpu.py), per output element:

    |out - ref| <= 2^-9 |ref| + 2^-8 A,   A = sum_j softmax_j |v_jd|   (float64)

2^-9 |ref| is the output's bf16 rounding; half of 2^-8 A is P's bf16 rounding against the row sum, the other half the
allowance for the fp32 score and exp2 error, which holds while score_error_nats(...) <= 2^-10. It is never widened.

Structured inputs are +-1 codes times a magnitude with few mantissa bits, so that every q . k is (mq mk) x integer,
exact in fp32 in any summation order, also with the integer softmax shift added first.
"""
import math

import torch

BF16 = torch.bfloat16
D = 128
KBLK = 64          # keys per tile
LAZY = 24.0        # attn_route.h kLazy
PREMISE = 2.0 ** -10


def reference64(q, k, v, log2_scale=1.0):
    """float64 softmax attention of exactly these inputs: (ref, A), each [B, Lq, H, 128]."""
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * (log2_scale * math.log(2.0))
    w = torch.softmax(s, -1)
    ref = torch.einsum("bhqk,bkhd->bqhd", w, v.double())
    A = torch.einsum("bhqk,bkhd->bqhd", w, v.double().abs())
    return ref, A


def bound(ref, A):
    return 2.0 ** -9 * ref.abs() + 2.0 ** -8 * A


def ratio(out, ref, A):
    """Largest error / bound over the elements (a ratio above 1 is a finding)."""
    return ((out.double() - ref).abs() / bound(ref, A)).max().item()


def score_error_nats(q, k, log2_scale=1.0):
    """Worst-case error of an fp32 score of 128 products, in nats: 128 * 2^-24 * max_ij sum_d |q_id k_jd| * log2_scale
    * ln 2. Integer-valued codes times power-of-two-mantissa magnitudes (exact()) have none."""
    absdot = torch.einsum("bqhd,bkhd->bhqk", q.float().abs(), k.float().abs()).max().item()
    return D * 2.0 ** -24 * absdot * log2_scale * math.log(2.0)


def exact_scores(q, k):
    """True where every partial sum of every q . k is exact in fp32, also when an integer shift of up to 2^7 is added
    first: all elements are multiples of 2^-6 (so products are multiples of 2^-12) and the sums stay below 2^8, so every
    partial sum is a multiple of 2^-12 below 2^9: 21 bits of the 24-bit significand."""
    ok = all(torch.equal(t.float() * 64.0, (t.float() * 64.0).round()) for t in (q, k))
    absdot = torch.einsum("bqhd,bkhd->bhqk", q.float().abs(), k.float().abs()).max().item()
    return ok and absdot < 256.0


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _codes(g, shape):
    return (torch.randint(0, 2, shape, generator=g) * 2 - 1).float()


def _int_v(g, shape):
    """Values from {+-1 .. +-127}: bf16-exact integers, none near zero, each key row its own."""
    return (torch.randint(1, 128, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)).float()


def split_edges(Lk, n_split):
    """First and last key of every key-range split (split s owns the tiles [s tps, (s + 1) tps), tps = ceil(tiles /
    n_split), as attn_launch forms them)."""
    ntiles = -(-Lk // KBLK)
    tps = -(-ntiles // n_split)
    out = []
    for s in range(n_split):
        lo, hi = s * tps * KBLK, min(Lk, (s + 1) * tps * KBLK) - 1
        if lo <= hi:
            out += [lo, hi]
    return out


def split_of(key, Lk, n_split):
    ntiles = -(-Lk // KBLK)
    tps = -(-ntiles // n_split)
    return key // (tps * KBLK)


def key_targets(Lk, n_splits=(1,)):
    """Case 1's key positions: 0, 63, 64, 65, the last key, the first and last key of the ragged tile, the first and
    last key of every split of every split count."""
    t = [0, 63, 64, 65, Lk - 1, (Lk - 1) // KBLK * KBLK]
    for n in n_splits:
        if n <= -(-Lk // KBLK):
            t += split_edges(Lk, n)
    return sorted({x for x in t if 0 <= x < Lk})


def row_targets(Lq, rows_wg, rows_wave):
    """Case 1's query rows: 0, the last, R - 1 and R, the first and last row of each wave's slice of the first and of
    the last workgroup."""
    t = [0, Lq - 1, rows_wg - 1, rows_wg]
    last0 = (Lq - 1) // rows_wg * rows_wg
    for base in (0, last0):
        for w in range(rows_wg // rows_wave):
            t += [base + w * rows_wave, base + (w + 1) * rows_wave - 1]
    return sorted({x for x in t if 0 <= x < Lq})


def selector(B, H, Lq, Lk, mq, mk, seed, keys=(), rows=(), big_rows=None, big_mq=None, tie=None, pin=None):
    """Every query row selects one key. Key rows are random +-1 codes times mk, query row i is the code of key
    pi[b, h, i] times mq (big_mq for the rows big_rows), so its winning score is 128 mq mk log2 units and every other is
    mq mk x an integer far below. pi differs for every (b, h), is injective while Lq <= Lk, and sends the rows `rows`
    (then further rows) to the keys `keys`. tie = (a, b): key b is a copy of key a (v differs), so rows selecting
    either get (v[a] + v[b]) / 2 (held to bound(); all other rows stay exact). pin = {row: key}: further fixed
    entries of every (b, h)'s pi (Lq > Lk only, where pi is not injective anyway).

    Returns dict(q, k, v, pi, expected [B, Lq, H, 128] bf16 = v[pi], gap: the smallest winner - runner-up distance in
    log2 units, tie_rows: bool [B, Lq, H]). Asserts Lk * 2^-gap * 127 < 2^-10: the runners-up together move no output
    by 2^-10, so acc / lsum is within 2^-22 relative of v[pi] (the winner's bf16 P cancels against the row sum of the
    same P) and rounds back to it: the output must equal `expected` bit for bit."""
    g = _gen(seed)
    code = _codes(g, (B, Lk, H, D))
    v = _int_v(g, (B, Lk, H, D))
    if tie is not None:
        code[:, tie[1]] = code[:, tie[0]]
    keys = [x for x in dict.fromkeys(list(tie or ()) + list(keys)) if 0 <= x < Lk]
    rows = [x for x in dict.fromkeys(rows) if 0 <= x < Lq]
    named = set(rows)
    spare = [r for r in range(Lq) if r not in named]
    step = max(1, len(spare) // max(1, len(keys)))
    slots = (rows + spare[::step] + spare)  # distinct rows, the named ones first
    slots = list(dict.fromkeys(slots))
    pi = torch.empty(B, H, Lq, dtype=torch.long)
    for b in range(B):
        for h in range(H):
            perm = torch.randperm(Lk, generator=g)
            if Lq > Lk:
                perm = perm[torch.arange(Lq) % Lk].clone()
            for j, key in enumerate(keys):
                r = slots[(j + 3 * (b * H + h)) % len(slots)] if Lq > Lk else slots[j]
                if Lq > Lk:
                    perm[r] = key
                else:
                    p = (perm == key).nonzero()[0, 0].item()
                    perm[p], perm[r] = perm[r].item(), key
            for r, key in (pin or {}).items():
                assert Lq > Lk
                perm[r] = key
            pi[b, h] = perm[:Lq]
            if Lq <= Lk:
                assert pi[b, h].unique().numel() == Lq
    bi = torch.arange(B)[:, None, None]
    hi = torch.arange(H)[None, :, None]
    qcode = code[bi, pi, hi].permute(0, 2, 1, 3)  # [B, Lq, H, D]
    mag = torch.full((Lq,), float(mq))
    if big_rows is not None:
        mag[big_rows] = float(big_mq)
    q = (qcode * mag[None, :, None, None]).to(BF16)
    k = (code * mk).to(BF16)
    v = v.to(BF16)
    assert torch.equal(q.float(), qcode * mag[None, :, None, None]) and torch.equal(k.float(), code * mk)
    expected = v[bi, pi, hi].permute(0, 2, 1, 3).contiguous()
    # the gap: integer code products, exact in fp32 (one (b, h) at a time: Lq x Lk floats)
    gap = math.inf
    tie_rows = torch.zeros(B, Lq, H, dtype=torch.bool)
    most = 0
    for b in range(B):
        for h in range(H):
            n = qcode[b, :, h] @ code[b, :, h].T
            same = n == float(D)
            n[same] = -float(D)
            gap = min(gap, ((float(D) - n.max(-1).values) * mag * mk).min().item())
            tie_rows[b, :, h] = same.sum(-1) > 1
            most = max(most, int(same.sum(-1).max()))
    assert Lk * 2.0 ** -gap * 127 < PREMISE, gap
    if tie is None:
        assert not tie_rows.any()
    else:
        assert tie_rows.any() and most == 2
    return dict(q=q, k=k, v=v, pi=pi, expected=expected, gap=gap, tie_rows=tie_rows, log2_scale=1.0)


def far_split(B, H, Lq, Lk, mq, mk, seed, n_anti, late):
    """Every query row is one code u (times mq). Keys 0 .. n_anti - 1 are -u mk (the whole first split of the cases that
    use it: all of its scores are -128 mq mk), key `late` is +u mk, the others random codes. The output is v[late] for
    every row, exact by the selector's reasoning; the first split's lse sits 2 x 128 mq mk log2 units below the late
    key's, more than fp32's exponent range when that is > 128, so merge weights formed against anything but the row's
    largest lse overflow."""
    g = _gen(seed)
    u = _codes(g, (B, 1, H, D))
    code = _codes(g, (B, Lk, H, D))
    code[:, :n_anti] = -u
    code[:, late] = u[:, 0]
    v = _int_v(g, (B, Lk, H, D)).to(BF16)
    q = (u * mq).expand(B, Lq, H, D).contiguous().to(BF16)
    k = (code * mk).to(BF16)
    n = torch.einsum("bhd,bkhd->bhk", u[:, 0], code)
    n[:, :, late] = -float(D)
    gap = ((float(D) - n.max(-1).values) * mq * mk).min().item()
    assert Lk * 2.0 ** -gap * 127 < PREMISE, gap
    expected = v[:, late][:, None].expand(B, Lq, H, D).contiguous()
    return dict(q=q, k=k, v=v, expected=expected, gap=gap, spread=2 * D * mq * mk, log2_scale=1.0)


def uniform_rows(B, H, Lq, Lk, b_rows, mk, seed, aligned=True):
    """Every key is the same row u mk (-u mk: anti-aligned), query row i is u times a bf16 magnitude chosen so that its
    score against every key is +-b_rows[i % len(b_rows)] (to bf16's resolution; the exact value is returned in
    b_row). Every softmax weight is 1 / Lk, so the output is the float64 mean of v, held to bound(). v is Gaussian."""
    g = _gen(seed)
    u = _codes(g, (B, 1, H, D))
    v = torch.randn(B, Lk, H, D, generator=g).to(BF16)
    want = torch.tensor([b_rows[i % len(b_rows)] for i in range(Lq)], dtype=torch.float32)
    mag = (want / (D * mk)).to(BF16).float()
    q = (u * mag[None, :, None, None]).to(BF16)
    k = ((u if aligned else -u) * mk).expand(B, Lk, H, D).contiguous().to(BF16)
    assert torch.equal(q.float(), u * mag[None, :, None, None])
    ref = v.double().mean(1, keepdim=True).expand(B, Lq, H, D)
    A = v.double().abs().mean(1, keepdim=True).expand(B, Lq, H, D)
    return dict(q=q, k=k, v=v, ref=ref, A=A, b_row=mag * D * mk, log2_scale=1.0)


GAPS = (10.0, 22.0, 23.5, 24.5, 27.0, 60.0)  # around kLazy = 24


def gap_rows(B, H, Lq, Lk, seed, anchor=3, late=None, probe=5, rows_wave=32):
    """The online form's lazy rescale. Query rows are one code u times a per-row magnitude; the anchor key (first
    tile) is u x 1/2 and pins the first tile's row max, the late key is u x 3/4, so it sits d_i = 32 mq_i log2 units
    above the anchor: mq_i = GAPS[..] / 32 gives d_i in GAPS. Every other key is a random code x 1/8 (its scores stay
    below the anchor's: |n| <= 128 x 1/8 x mq < 64 mq). Even 32-row slices hold only rows below the threshold, so their
    wave never takes the rescale branch; odd slices cycle through all of GAPS, rows on both sides of the threshold in
    one wave. Row `probe` of every slice has d = 22: the same q row in both kinds of company (the kernel comments say a
    row's result does not depend on the other rows of its wave: those rows must agree bit for bit). Held to bound()
    against the float64 reference of the same inputs."""
    g = _gen(seed)
    late = Lk - 2 if late is None else late
    assert anchor < KBLK <= late < Lk
    u = _codes(g, (B, 1, H, D))
    code = _codes(g, (B, Lk, H, D))
    kmag = torch.full((Lk,), 0.125)
    code[:, anchor] = u[:, 0]
    code[:, late] = u[:, 0]
    kmag[anchor], kmag[late] = 0.5, 0.75
    d = torch.empty(Lq)
    below = [x for x in GAPS if x < LAZY]
    for i in range(Lq):
        sl, r = divmod(i, rows_wave)
        d[i] = 22.0 if r == probe else (below[r % len(below)] if sl % 2 == 0 else GAPS[r % len(GAPS)])
    mag = d / 32.0
    q = (u * mag[None, :, None, None]).to(BF16)
    k = (code * kmag[None, :, None, None]).to(BF16)
    v = torch.randn(B, Lk, H, D, generator=g).to(BF16)
    assert torch.equal(q.float(), u * mag[None, :, None, None])
    ref, A = reference64(q, k, v)
    probes = torch.arange(probe, Lq, rows_wave)
    return dict(q=q, k=k, v=v, ref=ref, A=A, d=d, probes=probes, late=late, anchor=anchor, log2_scale=1.0)


def _rms(t):
    return t * torch.rsqrt(t.pow(2).mean(-1, keepdim=True) + 1e-6)


def peaked(B, H, Lq, Lk, seed, norm_limit, fp8=False, abs_limit=184.0):
    """RMS-normed Gaussian q and k; q carries 128^-1/2 log2 e (prescaled) times the largest power of two that keeps
    max_ij sum_d |q k| <= abs_limit (184: the score error premise, 128 * 2^-24 * 184 ln 2 <= 2^-10) and max |q| max |k|
    x 1.02 <= norm_limit (the route's window for the bound product: 110 long-key fixed shift, 96 zero shift, 60 fp8
    Q K^T): the softmax then has a few significant keys per row and bound() is within a small factor of the real
    error. fp8: q and k are then rounded to e4m3 (q x 4, k / 4, the scales the DiT uses) and the returned q / k are the
    dequantised copies (q8 / k8 hold the bytes)."""
    g = _gen(seed)
    q0 = _rms(torch.randn(B, Lq, H, D, generator=g)) * (D ** -0.5 * math.log2(math.e))
    k = _rms(torch.randn(B, Lk, H, D, generator=g)).to(BF16)
    v = torch.randn(B, Lk, H, D, generator=g).to(BF16)
    absdot = torch.einsum("bqhd,bkhd->bhqk", q0.abs(), k.float().abs()).max().item()
    nprod = q0.norm(dim=-1).max().item() * k.float().norm(dim=-1).max().item() * 1.02
    p = math.floor(math.log2(min(abs_limit / (absdot * 1.01), norm_limit / (nprod * 1.07 if fp8 else nprod))))
    q = (q0 * 2.0 ** p).to(BF16)
    out = dict(power=p)
    if fp8:
        q8 = (q.float() * 4.0).to(torch.float8_e4m3fn)
        k8 = (k.float() / 4.0).to(torch.float8_e4m3fn)
        out.update(q8=q8.view(torch.uint8), k8=k8.view(torch.uint8))
        q, k = (q8.float() / 4.0).to(BF16), (k8.float() * 4.0).to(BF16)
        assert torch.equal(q.float() * 4.0, q8.float()) and torch.equal(k.float() / 4.0, k8.float())
    absdot = torch.einsum("bqhd,bkhd->bhqk", q.float().abs(), k.float().abs()).max().item()
    nprod = q.float().norm(dim=-1).max().item() * k.float().norm(dim=-1).max().item()
    assert absdot <= abs_limit and nprod * 1.001 <= norm_limit, (absdot, nprod)
    ref, A = reference64(q, k, v)
    out.update(q=q, k=k, v=v, ref=ref, A=A, absdot=absdot, log2_scale=1.0)
    return out


def norm_bounds(q, k, margin=1.001):
    """(max |q row|, max |k row|) x margin: data-tight bounds."""
    return (q.float().norm(dim=-1).max().item() * margin, k.float().norm(dim=-1).max().item() * margin)


def qnorm_rows(raw, weight, cos, sin, out_scale, eps=1e-6):
    """head_rmsnorm_rope's formula (tests/cpu_kernels.py) for raw [B, Lq, H, 128] bf16 rows, RoPE rows indexed by the
    query row: what the in-kernel q normalisation produces, up to the fp32 summation order."""
    xf = raw.float()
    xn = ((xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)) * weight.float()).to(BF16).float()
    if cos is not None:
        c = torch.cat([cos, cos], -1)[None, :raw.shape[1], None, :]
        s = torch.cat([sin, sin], -1)[None, :raw.shape[1], None, :]
        xn = xn * c + torch.cat([-xn[..., 64:], xn[..., :64]], -1) * s
    return (xn * out_scale).to(BF16)


def qnorm_selector(B, H, Lq, Lk, product, seed, rope, keys=(), rows=()):
    """The selector for the q_norm entry point. raw q rows are Gaussian; the designated key of row i is
    qnorm_rows(raw)[i] rescaled (by a power of two, exact) so that the winning score is about `product` log2 units; the
    other rows' normalised directions are the runners-up. The kernel's own normalisation may differ from the formula
    by an ulp of an element, which moves a score by ~2^-8 relative: nothing against the gap. Keys nobody selects (Lk >
    Lq) are random codes at the keys' typical magnitude."""
    assert Lq <= Lk
    g = _gen(seed)
    raw = (torch.randn(B, Lq, H, D, generator=g) * 3.0).to(BF16)
    w = (0.75 + 0.5 * torch.rand(D, generator=g)).to(BF16)
    cos = sin = None
    if rope:
        ang = torch.rand(Lq, 64, generator=g) * 50.0
        cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    c = D ** -0.5 * math.log2(math.e)
    qn = qnorm_rows(raw, w, cos, sin, c)
    qsq = qn.float().pow(2).sum(-1)  # [B, Lq, H]
    kscale = 2.0 ** math.floor(math.log2(product / qsq.max().item()))
    base = selector(B, H, Lq, Lk, 1.0, 1.0, seed + 1, keys=keys, rows=rows)
    pi = base["pi"]
    k = (base["k"].float() * (kscale * qsq.mean().sqrt().item() / D ** 0.5)).to(BF16)
    bi = torch.arange(B)[:, None, None]
    hi = torch.arange(H)[None, :, None]
    kq = (qn.float() * kscale).to(BF16)  # [B, Lq, H, D]: row i's key
    k[bi, pi, hi] = kq.permute(0, 2, 1, 3)
    v = base["v"]
    s = torch.einsum("bqhd,bkhd->bhqk", qn.float(), k.float())
    win = s.gather(-1, pi[..., None])[..., 0]
    s.scatter_(-1, pi[..., None], -1e30)
    gap = (win - s.max(-1).values).min().item()
    assert Lk * 2.0 ** -gap * 127 < PREMISE, gap
    return dict(raw=raw, weight=w, cos=cos, sin=sin, out_scale=c, qn=qn, k=k, v=v, pi=pi, expected=base["expected"],
                gap=gap, top=win.max().item(), log2_scale=1.0)


QN_ANCHOR, QN_LATE, QN_OTHER = 2.0, 7.0, 0.25  # key magnitudes of qnorm_gap_rows (late - anchor = 5)


def qnorm_gap_rows(B, H, Lq, Lk, seed, rope, anchor=3, late=None, probe=5, rows_wave=32):
    """gap_rows for the q_norm entry point. The RMSNorm removes a raw row's magnitude, so a row's gap is set through
    its direction: raw row i = 3 (t_i u + (1 - |t_i|) w_i) for the (b, h)'s code u and a Gaussian row w_i (its varied elements smooth raw's bf16 rounding), and t_i is
    bisected until the normalised row qn_i = qnorm_rows(raw)_i has the projection p_i = qn_i . u = d_i / 5. The anchor
    key (first tile) is 2 u, the late key 7 u, every other key a random code x 1/4 (|qn . code| / 4 stays below the
    anchor's 2 p_i >= 4), so the late key sits d_i = 5 p_i above the first tile's max; d_i follows gap_rows's layout
    (even 32-row slices below kLazy only, odd slices all of GAPS, row `probe` of every slice d = 22 with the same raw row
    and, with RoPE, the same cos / sin row, so those rows are the same q row in different company). RoPE angles are
    below 0.5 rad so that a rotated u keeps most of its projection on u. Scores are not exact here: score_error_nats of
    (qn, k) is the premise. The d reached is returned (asserted within 0.1 of its target, raw being bf16, and on the
    target's side of kLazy). The kernel's own normalisation can differ from the formula by a bf16 ulp of a rare element (a rounding
    tie of its fp32 value); that moves a score by at most 7 x 2^-8 |qn_d| < 0.01 log2 units, against rows whose second
    largest weight is below 2^-9: the output moves by less than 2^-16 A."""
    g = _gen(seed)
    late = Lk - 2 if late is None else late
    assert anchor < KBLK <= late < Lk
    u = _codes(g, (B, 1, H, D))
    w = torch.randn(B, Lq, H, D, generator=g)
    wt = (0.75 + 0.5 * torch.rand(D, generator=g)).to(BF16)
    c = D ** -0.5 * math.log2(math.e)
    probes = torch.arange(probe, Lq, rows_wave)
    w[:, probes] = w[:, probes[:1]].clone()
    cos = sin = None
    if rope:
        ang = torch.rand(Lq, 64, generator=g) * 0.5
        ang[probes] = ang[probes[0]].clone()
        cos, sin = torch.cos(ang).contiguous(), torch.sin(ang).contiguous()
    target = torch.empty(Lq)
    below = [x for x in GAPS if x < LAZY]
    for i in range(Lq):
        sl, r = divmod(i, rows_wave)
        target[i] = 22.0 if r == probe else (below[r % len(below)] if sl % 2 == 0 else GAPS[r % len(GAPS)])
    step = QN_LATE - QN_ANCHOR

    def rows(t):
        raw = ((t[..., None] * u + (1 - t.abs())[..., None] * w) * 3.0).to(BF16)
        qn = qnorm_rows(raw, wt, cos, sin, c)
        return raw, qn, (qn.float() * u).sum(-1) * step

    lo, hi = torch.full((B, Lq, H), -1.0), torch.full((B, Lq, H), 1.0)
    tgt = target[None, :, None].expand(B, Lq, H)
    for _ in range(30):
        mid = (lo + hi) / 2
        d = rows(mid)[2]
        lo, hi = torch.where(d < tgt, mid, lo), torch.where(d < tgt, hi, mid)
    raw, qn, d = rows((lo + hi) / 2)
    assert torch.equal(raw[:, probes], raw[:, probes[:1]].expand_as(raw[:, probes]))
    assert (d - tgt).abs().max().item() < 0.1 and ((d > LAZY) == (tgt > LAZY)).all()
    code = _codes(g, (B, Lk, H, D))
    kmag = torch.full((Lk,), QN_OTHER)
    code[:, anchor] = u[:, 0]
    code[:, late] = u[:, 0]
    kmag[anchor], kmag[late] = QN_ANCHOR, QN_LATE
    k = (code * kmag[None, :, None, None]).to(BF16)
    v = torch.randn(B, Lk, H, D, generator=g).to(BF16)
    ref, A = reference64(qn, k, v)
    return dict(raw=raw, weight=wt, cos=cos, sin=sin, out_scale=c, qn=qn, k=k, v=v, ref=ref, A=A, d=d, target=target,
                probes=probes, late=late, anchor=anchor, log2_scale=1.0)
