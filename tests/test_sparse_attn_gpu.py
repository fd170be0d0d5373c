"""cp25_attn_na3d (3D neighborhood attention, csrc/attn_na.hip) against the float64 masked attention of
tests/na_truth.py on the same bf16 q / k / v.

Reference op: NeighborhoodAttention.forward (modules/neighborhood_attn.py:172-252) as restated by the window rule in
cosmos_predict2/sparse_attn.py; the mask is na_truth.na_mask's brute-force loop. Tolerance: rel-L2 <= 4e-3, the bound
of tests/test_attn_m16_gpu.py (same numerics class: P rounded to bf16 before P.V, bf16 output); two bf16 kernels
against each other within 1.5 x that (two independent roundings). The membership test needs no tolerance on the mask:
with q = 0 the softmax is uniform over the box and one-hot position codes in v make every output column either 0 or
1 / K of its axis.
"""
import dataclasses
import functools

import pytest
import torch

import na_truth as NT
from cosmos_predict2 import _native as N
from cosmos_predict2 import sparse_attn as SA

pytestmark = pytest.mark.gpu

TOL = 4e-3
LOG2E = 1.4426950408889634
B, H, D = 2, 2, 128
CASES = sorted(NT.NA_CASES)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rms_rows(t, w):
    tf = t.float()
    return (tf * torch.rsqrt(tf.pow(2).mean(-1, keepdim=True) + 1e-6) * w).to(torch.bfloat16)


def _inputs(L, seed, wmax=1.5):
    """q / k RMS-normed rows with weights in [0.5, wmax], v normal (tests/test_attn_m16_gpu.py::_inputs), on the CPU."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = 0.5 + (wmax - 0.5) * torch.rand(128, generator=g)
    q = _rms_rows(torch.randn(B, L, H, 128, generator=g), w)
    k = _rms_rows(torch.randn(B, L, H, 128, generator=g), w)
    v = torch.randn(B, L, H, 128, generator=g).to(torch.bfloat16)
    return q, k, v


@functools.lru_cache(maxsize=None)
def _case(name):
    """(grid, params, mask, q, k, v, truth, q prescaled, truth of the prescaled q): computed once, never modified."""
    grid, params = NT.NA_CASES[name]
    L = grid[0] * grid[1] * grid[2]
    mask = NT.na_mask(*grid, params)
    q, k, v = _inputs(L, 700 + L)
    truth = NT.na_attention_truth(q, k, v, mask)
    qs = (q.float() * (D ** -0.5 * LOG2E)).to(torch.bfloat16)
    truth_s = NT.na_attention_truth(qs, k, v, mask, scale=1.0 / LOG2E)
    return grid, params, mask, q, k, v, truth, qs, truth_s


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("prescaled", [False, True])
def test_na3d_matches_float64_truth(device, name, prescaled):
    grid, params, mask, q, k, v, truth, qs, truth_s = _case(name)
    plan = SA.build_plan(grid, params, device)
    qin, ref = (qs, truth_s) if prescaled else (q, truth)
    out = N.attn_na3d(qin.to(device), k.to(device), v.to(device), plan, prescaled=prescaled)
    torch.cuda.synchronize()
    err = rel_l2(out.cpu(), ref)
    print(f"attn_na3d {name} prescaled={prescaled} tiles={plan.n_tiles} keys={plan.keys_per_query}: rel-L2 {err:.3e}")
    assert torch.isfinite(out).all()
    assert err <= TOL, err


def test_full_window_equals_dense_kernel(device):
    grid, params, mask, q, k, v, truth, _, _ = _case("e_full")
    assert mask.all()
    plan = SA.build_plan(grid, params, device)
    qd, kd, vd = q.to(device), k.to(device), v.to(device)
    out = N.attn_na3d(qd, kd, vd, plan)
    dense = N.attn_fwd(qd, kd, vd)
    torch.cuda.synchronize()
    err = rel_l2(out.cpu(), dense.cpu())
    print(f"attn_na3d full window vs attn_fwd: rel-L2 {err:.3e}")
    assert err <= 1.5 * TOL, err


@pytest.mark.parametrize("name", [c for c in CASES if c != "e_full"])
def test_exact_key_membership(device, name):
    """q = 0: uniform softmax over the box. v[token] holds one-hot codes of its t, h and w in three disjoint column
    ranges, so output column (axis, j) is 1 / K_axis where key index j is in the query's per-axis set and exactly 0
    elsewhere: any wrong, missing or extra key changes the zero pattern."""
    grid, params = NT.NA_CASES[name]
    T, Hg, Wg = grid
    L = T * Hg * Wg
    window, _, _ = SA.adaptive_parameters(params, grid)
    sets = NT.na_axis_sets(T, Hg, Wg, params)
    tok = torch.arange(L)
    coords = (tok // (Hg * Wg), (tok // Wg) % Hg, tok % Wg)
    offs = (0, T, T + Hg)
    assert T + Hg + Wg <= D
    v = torch.zeros(B, L, H, D)
    want = torch.zeros(L, D, dtype=torch.float64)
    for a in range(3):
        v[:, tok, :, offs[a] + coords[a]] = 1.0
        for i in range(L):
            for j in sets[a][int(coords[a][i])]:
                want[i, offs[a] + j] = 1.0 / window[a]
    g = torch.Generator().manual_seed(5)
    k = torch.randn(B, L, H, D, generator=g).to(torch.bfloat16)
    q = torch.zeros(B, L, H, D, dtype=torch.bfloat16)
    plan = SA.build_plan(grid, params, device)
    out = N.attn_na3d(q.to(device), k.to(device), v.to(torch.bfloat16).to(device), plan)
    torch.cuda.synchronize()
    out = out.cpu().double()
    for b in range(B):
        for h in range(H):
            o = out[b, :, h]
            assert torch.equal(o != 0, want != 0), (name, b, h)
            assert ((o - want).abs() <= want * 2.0 ** -8).all(), (name, b, h)  # bf16 rounding of 1 / K


def test_token_major_batch_inner_views_in_place(device):
    """The DiT's layout: q / k / v are column blocks of one token-major [n, B, 3 H D] buffer (batch inner), the output
    a [n, B, H D] buffer; same bits as contiguous tensors."""
    grid, params, mask, q, k, v, truth, _, _ = _case("b_ragged")
    L = q.shape[1]
    plan = SA.build_plan(grid, params, device)
    qkv = torch.empty(L, B, 3 * H * D, dtype=torch.bfloat16, device=device)
    for c, t in enumerate((q, k, v)):
        qkv[:, :, c * H * D:(c + 1) * H * D] = t.to(device).transpose(0, 1).reshape(L, B, H * D)
    views = [qkv[:, :, c * H * D:(c + 1) * H * D].view(L, B, H, D).transpose(0, 1) for c in range(3)]
    o = torch.full((L, B, H * D), float("nan"), dtype=torch.bfloat16, device=device)
    N.attn_na3d(*views, plan, out=o.view(L, B, H, D).transpose(0, 1))
    base = N.attn_na3d(q.to(device), k.to(device), v.to(device), plan)
    torch.cuda.synchronize()
    assert torch.equal(o.view(L, B, H, D).transpose(0, 1), base)
    assert rel_l2(base.cpu(), truth) <= TOL


def test_two_runs_are_bit_identical(device):
    grid, params, mask, q, k, v, truth, _, _ = _case("d_tiles")
    plan = SA.build_plan(grid, params, device)
    qd, kd, vd = q.to(device), k.to(device), v.to(device)
    a = N.attn_na3d(qd, kd, vd, plan)
    b = N.attn_na3d(qd, kd, vd, plan)
    torch.cuda.synchronize()
    assert torch.equal(a, b)


def test_bad_arguments_raise_value_error(device):
    grid, params = NT.NA_CASES["a_aligned"]
    L = grid[0] * grid[1] * grid[2]
    plan = SA.build_plan(grid, params, device)
    z = lambda *s: torch.zeros(*s, dtype=torch.bfloat16, device=device)  # noqa: E731
    with pytest.raises(ValueError):  # head dim
        N.attn_na3d(z(1, L, 2, 64), z(1, L, 2, 64), z(1, L, 2, 64), plan)
    with pytest.raises(ValueError):  # token stride not a multiple of 8 elements
        bad = z(1, L, 2 * 128 + 4)[:, :, :256].view(1, L, 2, 128)
        N.attn_na3d(bad, z(1, L, 2, 128), z(1, L, 2, 128), plan)
    with pytest.raises(ValueError):  # a window wider than the grid
        N.attn_na3d(z(1, L, 2, 128), z(1, L, 2, 128), z(1, L, 2, 128),
                    dataclasses.replace(plan, window=(grid[0], grid[1] + 1, plan.window[2])))
    with pytest.raises(ValueError):  # window x dilation wider than the grid
        N.attn_na3d(z(1, L, 2, 128), z(1, L, 2, 128), z(1, L, 2, 128), dataclasses.replace(plan, dilation=(1, 3, 1)))
    with pytest.raises(ValueError):  # tokens do not fill the grid
        N.attn_na3d(z(1, L + 1, 2, 128), z(1, L + 1, 2, 128), z(1, L + 1, 2, 128), plan)
    torch.cuda.synchronize()
