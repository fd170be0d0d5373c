"""CPU truth of the 3D neighborhood attention: a brute-force mask written independently of
cosmos_predict2/sparse_attn.py, and masked attention in float64.

The per-axis rule (length L, window K, stride s, dilation d), for index i:
    g = i mod d, p = i div d, Lg = L div d + (1 if g < L mod d else 0)
    leader = min((p div s) * s + s div 2, Lg - 1); start = clamp(leader - K div 2, 0, Lg - K)
    keys = { g + (start + j) * d : j = 0 .. K-1 }
"""
import torch


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
