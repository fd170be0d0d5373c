"""CPU truth of the 3D neighborhood attention: a brute-force mask written independently of
cosmos_predict2/sparse_attn.py, and masked attention in float64.

The per-axis rule (length L, window K, stride s, dilation d), for index i:
    g = i mod d, p = i div d, Lg = L div d + (1 if g < L mod d else 0)
    leader = min((p div s) * s + s div 2, Lg - 1); start = clamp(leader - K div 2, 0, Lg - K)
    keys = { g + (start + j) * d : j = 0 .. K-1 }

The second half is the known-answer material of tests/test_na_truth_cpu.py and tests/test_sparse_attn_exact_gpu.py:
resolved (window, stride, dilation) forms of the mask (a window of one key is a window of one key there, not the full
extent), box_keys (every query group with its keys in the kernel's order), the grids of NA_EXACT_CASES and generators
of q / k / v [B, L, H, 128] bf16 whose answer is known without running attention, built from tests/attn_truth.py's
pieces. Scores are in log2 units (a prescaled q: softmax weights are exp2(q . k)).
"""
import functools
import math

import torch

import attn_truth as AT


def _axis_keys(L, K, s, d, i):
    g = i % d
    p = i // d
    Lg = L // d + (1 if g < L % d else 0)
    leader = min((p // s) * s + s // 2, Lg - 1)
    start = leader - K // 2
    if start < 0:
        start = 0
    if start > Lg - K:
        start = Lg - K
    return [g + (start + j) * d for j in range(K)]


def _resolve(T, H, W, params):
    """params: dict(window_size, stride=1, dilation=1) already adapted to the grid, except that window entries <= 1
    mean the full extent and scalars broadcast."""
    shape = (T, H, W)
    win = tuple(w if w > 1 else x for w, x in zip(params["window_size"], shape))
    st = params.get("stride", 1)
    st = (st,) * 3 if isinstance(st, int) else tuple(st)
    dil = params.get("dilation", 1)
    dil = (dil,) * 3 if isinstance(dil, int) else tuple(dil)
    return shape, win, st, dil


def na_axis_sets(T, H, W, params):
    """Per axis, the list (over the axis index) of key lists."""
    shape, win, st, dil = _resolve(T, H, W, params)
    return [[_axis_keys(shape[a], win[a], st[a], dil[a], i) for i in range(shape[a])] for a in range(3)]


def na_mask(T, H, W, params):
    """bool [L, L]: mask[q, k] is True where query token q attends key token k (token = (t H + h) W + w)."""
    shape, win, st, dil = _resolve(T, H, W, params)
    L = T * H * W
    mask = torch.zeros(L, L, dtype=torch.bool)
    for t in range(T):
        kt = _axis_keys(T, win[0], st[0], dil[0], t)
        for h in range(H):
            kh = _axis_keys(H, win[1], st[1], dil[1], h)
            for w in range(W):
                kw = _axis_keys(W, win[2], st[2], dil[2], w)
                q = (t * H + h) * W + w
                for a in kt:
                    for b in kh:
                        base = (a * H + b) * W
                        for c in kw:
                            mask[q, base + c] = True
    return mask


def na_attention_truth(q, k, v, mask, scale=None):
    """softmax over the masked keys of (q k^T scale) v in float64: q / k / v [B, L, H, D], mask bool [L, L];
    returns float64 [B, L, H, D]."""
    qd, kd, vd = (t.detach().cpu().double().transpose(1, 2) for t in (q, k, v))  # [B, H, L, D]
    sc = qd.shape[-1] ** -0.5 if scale is None else scale
    s = torch.matmul(qd, kd.transpose(-1, -2)) * sc
    s = s.masked_fill(~mask.cpu()[None, None], float("-inf"))
    return torch.matmul(torch.softmax(s, dim=-1), vd).transpose(1, 2)


# the kernel test shapes: name -> ((T, H, W), parameters)
NA_CASES = {
    "a_aligned": ((2, 8, 16), dict(window_size=(-1, 4, 8), stride=(1, 2, 4), dilation=1)),
    "b_ragged": ((3, 10, 13), dict(window_size=(2, 5, 6), stride=(1, 3, 4), dilation=1)),
    "c_dilated": ((2, 11, 9), dict(window_size=(-1, 3, 4), stride=1, dilation=(1, 3, 2))),
    "d_tiles": ((4, 16, 24), dict(window_size=(-1, 8, 8), stride=(1, 4, 8), dilation=1)),
    "e_full": ((2, 6, 8), dict(window_size=(-1, -1, -1))),
}


# ---------------------------------------------------------------------------------------------------------------------
# Known-answer material. Nothing below reads cosmos_predict2/sparse_attn.py: the boxes come from _axis_keys alone.

BF16 = torch.bfloat16
D = AT.D


def axis_sets_resolved(grid, window, stride, dilation):
    """na_axis_sets for already resolved per-axis triples: a window of 1 is one key."""
    return [[_axis_keys(grid[a], window[a], stride[a], dilation[a], i) for i in range(grid[a])] for a in range(3)]


def mask_resolved(grid, window, stride, dilation):
    """na_mask for already resolved per-axis triples."""
    T, H, W = grid
    sets = axis_sets_resolved(grid, window, stride, dilation)
    mask = torch.zeros(T * H * W, T * H * W, dtype=torch.bool)
    for t in range(T):
        for h in range(H):
            for w in range(W):
                keys = [(a * H + b) * W + c for a in sets[0][t] for b in sets[1][h] for c in sets[2][w]]
                mask[(t * H + h) * W + w, keys] = True
    return mask


def box_keys(grid, window, stride, dilation):
    """[(query tokens ascending, key tokens in the kernel's order: ascending per axis, w fastest)], one entry per query
    group (the queries with identical per-axis key sets), the groups sorted by their (t, h, w) key sets."""
    T, H, W = grid
    sets = axis_sets_resolved(grid, window, stride, dilation)
    groups = {}
    for t in range(T):
        for h in range(H):
            for w in range(W):
                key = (tuple(sets[0][t]), tuple(sets[1][h]), tuple(sets[2][w]))
                groups.setdefault(key, []).append((t * H + h) * W + w)
    return [(groups[key], [(a * H + b) * W + c for a in key[0] for b in key[1] for c in key[2]])
            for key in sorted(groups)]


# name -> ((T, H, W), window, stride, dilation), resolved; the box sizes and their last key tiles:
#   one_key 1 key; k63 63 (one short of a tile); k65 64 + 1; k130_block 128 + 2 keys, groups of 130 queries (a full
#   query tile and one with 2 live rows: its waves 1 - 3 are empty slots); k195 3 tiles, the last of 3; k385_full 6 tiles
#   + 1 key, 385 queries in one group; dil_t dilation on every axis, t included.
NA_EXACT_CASES = {
    "one_key": ((2, 5, 6), (1, 1, 1), (1, 1, 1), (1, 1, 1)),
    "k63": ((3, 4, 9), (3, 3, 7), (1, 1, 2), (1, 1, 1)),
    "k65": ((2, 7, 15), (1, 5, 13), (1, 2, 5), (1, 1, 1)),
    "k130_block": ((2, 10, 26), (2, 5, 13), (1, 5, 13), (1, 1, 1)),
    "k195": ((4, 6, 14), (3, 5, 13), (1, 2, 4), (1, 1, 1)),
    "k385_full": ((5, 7, 11), (5, 7, 11), (1, 1, 1), (1, 1, 1)),
    "dil_t": ((5, 9, 8), (2, 3, 4), (1, 1, 1), (2, 3, 2)),
}


@functools.lru_cache(maxsize=None)
def geometry(name):
    """The case's grid, parameters, mask and groups; group_of / pos_of [L]: a token's group and its rank in it (the
    kernel's plan cuts a group into tiles of 128 rows in that order, each wave taking 32). Never modified."""
    grid, window, stride, dilation = NA_EXACT_CASES[name]
    L = grid[0] * grid[1] * grid[2]
    groups = box_keys(grid, window, stride, dilation)
    group_of, pos_of = torch.empty(L, dtype=torch.long), torch.empty(L, dtype=torch.long)
    for gi, (qs, _) in enumerate(groups):
        group_of[qs] = gi
        pos_of[qs] = torch.arange(len(qs))
    return dict(name=name, grid=grid, window=window, stride=stride, dilation=dilation, L=L,
                nkeys=window[0] * window[1] * window[2], groups=groups, group_of=group_of, pos_of=pos_of,
                mask=mask_resolved(grid, window, stride, dilation))


def reference64_masked(q, k, v, mask, log2_scale=1.0):
    """attn_truth.reference64 over the masked keys only: (ref, A) float64 [B, L, H, 128]."""
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * (log2_scale * math.log(2.0))
    w = torch.softmax(s.masked_fill(~mask[None, None], -math.inf), -1)
    return (torch.einsum("bhqk,bkhd->bqhd", w, v.double()), torch.einsum("bhqk,bkhd->bqhd", w, v.double().abs()))


def box_targets(window):
    """The selector's key positions inside a box (kernel order): 0, 63, 64, 65, the last key, the first and last key of
    every 64-key tile and the eight corners."""
    Kt, Kh, Kw = window
    nk = Kt * Kh * Kw
    t = [0, 63, 64, 65, nk - 1]
    for j in range(0, nk, AT.KBLK):
        t += [j, min(j + AT.KBLK - 1, nk - 1)]
    t += [(a * Kh + b) * Kw + c for a in (0, Kt - 1) for b in (0, Kh - 1) for c in (0, Kw - 1)]
    return sorted({x for x in t if 0 <= x < nk})


def na_selector(geo, B, H, mq, mk, seed, dims=D):
    """Every query selects one key of its own box. Key rows are +-1 codes (in the first `dims` dims) x mk, query token i
    is the code of key pi[b, h, i] x mq: the winning score is dims mq mk log2 units, every other score of the box mq mk
    x an integer below. In every group and every (b, h), pi covers box_targets (on queries spread over the group, the
    rest of the group selects at random). Returns dict(q, k, v, pi [B, H, L] key token, pos [B, H, L] its position in
    the box, expected = v[pi], gap: the smallest winner - runner-up distance over each query's own box). Asserts
    nkeys 2^-gap 127 < 2^-10 (attn_truth.selector's reasoning): the output must equal `expected` bit for bit."""
    g = AT._gen(seed)
    L = geo["L"]
    code = torch.zeros(B, L, H, D)
    code[..., :dims] = AT._codes(g, (B, L, H, dims))
    v = AT._int_v(g, (B, L, H, D)).to(BF16)
    targets = box_targets(geo["window"])
    pi = torch.empty(B, H, L, dtype=torch.long)
    pos = torch.empty(B, H, L, dtype=torch.long)
    qcode = torch.empty(B, L, H, D)
    gap = math.inf
    for gi, (qs, ks) in enumerate(geo["groups"]):
        n, nk = len(qs), len(ks)
        assert n >= len(targets), (geo["name"], gi, n, len(targets))
        qs_t, ks_t = torch.tensor(qs), torch.tensor(ks)
        for b in range(B):
            for h in range(H):
                p = torch.randint(0, nk, (n,), generator=g)
                off = 5 * (b * H + h) + gi
                for j, t in enumerate(targets):
                    p[(j * n // len(targets) + off) % n] = t
                assert set(targets).issubset(set(p.tolist()))
                pos[b, h, qs_t] = p
                pi[b, h, qs_t] = ks_t[p]
                qc = code[b, ks_t[p], h]
                qcode[b, qs_t, h] = qc
                s = qc @ code[b, ks_t, h].T
                win = s == float(dims)
                assert (win.sum(-1) == 1).all() and win[torch.arange(n), p].all()
                gap = min(gap, ((float(dims) - s.masked_fill(win, -float(dims)).max(-1).values) * mq * mk).min().item())
    if geo["nkeys"] == 1:
        gap = math.inf
    assert geo["nkeys"] * 2.0 ** -gap * 127 < AT.PREMISE, gap
    q, k = (qcode * mq).to(BF16), (code * mk).to(BF16)
    assert torch.equal(q.float(), qcode * mq) and torch.equal(k.float(), code * mk)
    bi, hi = torch.arange(B)[:, None, None], torch.arange(H)[None, :, None]
    expected = v[bi, pi, hi].permute(0, 2, 1, 3).contiguous()
    return dict(q=q, k=k, v=v, pi=pi, pos=pos, expected=expected, gap=gap, log2_scale=1.0)


OUT_M = 1.5      # the outsider's selector magnitudes: 64 x 2.25 = 144 log2 units
OUT_LURE = 16.0  # lure magnitudes: 64 x 256 = 2^14 log2 units


def outside_steps(geo, gi):
    """Tokens one step outside group gi's box along each axis (below its first key, above its last, and, on a dilated
    axis, the next index after its first key, which belongs to another dilation group), the other two coordinates at
    the box's first key: [(axis, token)]."""
    T, H, W = geo["grid"]
    ks = geo["groups"][gi][1]
    coords = [sorted({x // (H * W) for x in ks}), sorted({x // W % H for x in ks}), sorted({x % W for x in ks})]
    out = []
    for a in range(3):
        for c in (coords[a][0] - 1, coords[a][-1] + 1, coords[a][0] + 1):
            if 0 <= c < geo["grid"][a] and c not in coords[a]:
                at = [coords[0][0], coords[1][0], coords[2][0]]
                at[a] = c
                out.append((a, (at[0] * H + at[1]) * W + at[2]))
    return list(dict.fromkeys(out))


def na_outsider(geo, B, H, seed, picks=None):
    """The lure. base: na_selector confined to dims 0 .. 63 at mq = mk = 1.5. For each picked group G (default the
    first, a middle and the last box): every key token outside G's box carries u x 16 in dims 64 .. 127, G's queries
    carry u x 16 there and every other query zeros, so no score of any query against a key of its own box moves by a
    bit, while any outside key read for a G query scores 2^14 log2 units: exp2 of it overflows. Returns dict(base,
    lured = [dict(group, q, k, steps)]); the premise (every lured score exceeds the winner by >= 1000) is asserted."""
    base = na_selector(geo, B, H, OUT_M, OUT_M, seed, dims=64)
    g = AT._gen(seed + 1)
    u = AT._codes(g, (B, 1, H, 64))
    n = len(geo["groups"])
    picks = sorted({0, n // 2, n - 1}) if picks is None else picks
    lured = []
    for gi in picks:
        qs, ks = geo["groups"][gi]
        outside = torch.ones(geo["L"], dtype=torch.bool)
        outside[ks] = False
        if not outside.any():
            continue
        q, k = base["q"].clone(), base["k"].clone()
        k[:, outside, :, 64:] = (u * OUT_LURE).to(BF16)
        q[:, qs, :, 64:] = (u * OUT_LURE).to(BF16)
        s = torch.einsum("bqhd,bkhd->bhqk", q[:, qs].float(), k.float())
        assert (s[..., outside].min() - 64 * OUT_M * OUT_M).item() >= 1000.0
        assert torch.equal(s[..., ~outside], torch.einsum("bqhd,bkhd->bhqk", base["q"][:, qs].float(),
                                                          base["k"][:, ~outside].float()))
        steps = outside_steps(geo, gi)
        assert all(outside[t] for _, t in steps)
        lured.append(dict(group=gi, q=q, k=k, steps=steps))
    return dict(base=base, lured=lured)


UNIFORM_B = (0.0, 8.0, 32.0, 64.0)


def na_uniform(geo, B, H, seed, mk=0.5):
    """attn_truth.uniform_rows per box: every key row is u mk, query token i is u times a magnitude that makes all of
    its scores UNIFORM_B[i % 4]; v is Gaussian. The answer is the float64 mean of v over the token's box."""
    g = AT._gen(seed)
    L = geo["L"]
    u = AT._codes(g, (B, 1, H, D))
    v = torch.randn(B, L, H, D, generator=g).to(BF16)
    want = torch.tensor([UNIFORM_B[i % len(UNIFORM_B)] for i in range(L)])
    mag = (want / (D * mk)).to(BF16).float()
    q = (u * mag[None, :, None, None]).to(BF16)
    k = (u * mk).expand(B, L, H, D).contiguous().to(BF16)
    assert torch.equal(q.float(), u * mag[None, :, None, None]) and torch.equal(mag * D * mk, want)
    ref, A = torch.empty(B, L, H, D, dtype=torch.float64), torch.empty(B, L, H, D, dtype=torch.float64)
    for qs, ks in geo["groups"]:
        ref[:, qs] = v[:, ks].double().mean(1, keepdim=True)
        A[:, qs] = v[:, ks].double().abs().mean(1, keepdim=True)
    return dict(q=q, k=k, v=v, ref=ref, A=A, b_row=want, log2_scale=1.0)


def _disjoint_boxes(geo):
    ks = [x for _, box in geo["groups"] for x in box]
    return len(ks) == len(set(ks))


def na_gap_rows(geo, B, H, seed, anchor=3, probe=5):
    """attn_truth.gap_rows in box order, for grids whose boxes are disjoint (each box gets its own keys). Query rows are
    one code u times a per-row magnitude; the box's key `anchor` (first key tile) is u x 1/2 and pins the first tile's
    row max, the box's LAST key (alone with few others in the ragged tile) is u x 3/4 and sits d = 32 mq log2 units
    above it, every other key is a random code x 1/8. d follows a query's rank r in its group: 32-row slices (a wave's
    rows) with an even index hold only d < kLazy, odd slices cycle through all of GAPS, rank `probe` of every slice has
    d = 22: the same q row in a wave that rescales and in one that does not. Returns ref / A (float64 masked
    attention), d [L], probes: per group the probe tokens, anchors / lates: per group the key tokens."""
    assert _disjoint_boxes(geo) and geo["nkeys"] > AT.KBLK and geo["nkeys"] % AT.KBLK != 0
    g = AT._gen(seed)
    L = geo["L"]
    u = AT._codes(g, (B, 1, H, D))
    code = AT._codes(g, (B, L, H, D))
    kmag = torch.full((L,), 0.125)
    below = [x for x in AT.GAPS if x < AT.LAZY]
    d = torch.empty(L)
    probes, anchors, lates = [], [], []
    for qs, ks in geo["groups"]:
        for tok, mag in ((ks[anchor], 0.5), (ks[-1], 0.75)):
            code[:, tok] = u[:, 0]
            kmag[tok] = mag
        anchors.append(ks[anchor])
        lates.append(ks[-1])
        for i, tok in enumerate(qs):
            sl, r = divmod(i, 32)
            d[tok] = 22.0 if r == probe else (below[r % len(below)] if sl % 2 == 0 else AT.GAPS[r % len(AT.GAPS)])
        probes.append([tok for i, tok in enumerate(qs) if i % 32 == probe])
    mag = d / 32.0
    q = (u * mag[None, :, None, None]).to(BF16)
    k = (code * kmag[None, :, None, None]).to(BF16)
    v = torch.randn(B, L, H, D, generator=g).to(BF16)
    assert torch.equal(q.float(), u * mag[None, :, None, None])
    ref, A = reference64_masked(q, k, v, geo["mask"])
    return dict(q=q, k=k, v=v, ref=ref, A=A, d=d, probes=probes, anchors=anchors, lates=lates, log2_scale=1.0)


STAIR_STEP = 30.0              # log2 units between the maxima of consecutive key tiles (> kLazy)
STAIR_MQ = (1.0, 1.0, 0.5, 1.0)  # by a query's rank in its group: rows at half the step share waves with full ones


def na_staircase(geo, B, H, seed, reverse=False):
    """A rescale at every key tile: key 64 j + 3 of the box (the last tile's only key where it has fewer) is u x
    (10 + 15 j) / 64, so for a q row u x 1 the max of key tile j is 20 + 30 j log2 units; every other key is a random
    code x 1/8 (|score| <= 16). Rows of magnitude 1/2 (steps of 15, below kLazy) sit in the same waves. reverse: the
    maxima descend instead, no rescale after the first tile and the late tiles' weights are tiny. Held to bound()."""
    assert _disjoint_boxes(geo)
    g = AT._gen(seed)
    L = geo["L"]
    u = AT._codes(g, (B, 1, H, D))
    code = AT._codes(g, (B, L, H, D))
    kmag = torch.full((L,), 0.125)
    nt = -(-geo["nkeys"] // AT.KBLK)
    mag = torch.empty(L)
    steps = []
    for qs, ks in geo["groups"]:
        toks = [ks[min(AT.KBLK * j + 3, len(ks) - 1)] for j in range(nt)]
        for j, tok in enumerate(toks):
            code[:, tok] = u[:, 0]
            kmag[tok] = (10.0 + 15.0 * (nt - 1 - j if reverse else j)) / 64.0
        steps.append(toks)
        for i, tok in enumerate(qs):
            mag[tok] = STAIR_MQ[i % len(STAIR_MQ)]
    q = (u * mag[None, :, None, None]).to(BF16)
    k = (code * kmag[None, :, None, None]).to(BF16)
    v = torch.randn(B, L, H, D, generator=g).to(BF16)
    assert torch.equal(k.float(), code * kmag[None, :, None, None])
    ref, A = reference64_masked(q, k, v, geo["mask"])
    return dict(q=q, k=k, v=v, ref=ref, A=A, mag=mag, steps=steps, log2_scale=1.0)


def na_one_key(geo, B, H, seed):
    """A box of one key: Gaussian q, k and v, the output is that key's v row bit for bit (P = exp2(0) = 1, row sum 1)."""
    assert geo["nkeys"] == 1
    g = AT._gen(seed)
    q, k, v = (torch.randn(B, geo["L"], H, D, generator=g).to(BF16) for _ in range(3))
    pi = torch.empty(geo["L"], dtype=torch.long)
    for qs, ks in geo["groups"]:
        pi[qs] = ks[0]
    return dict(q=q, k=k, v=v, expected=v[:, pi].contiguous(), log2_scale=1.0)
