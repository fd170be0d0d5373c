"""cp25_plucker_tokens against the float64 truth of tests/camera_truth.py (get_plucker_rays restated + this build's
packing), F = 2 frames on a 2 x 3 patch grid (12 tokens of 16 x 16 pixels).

Gate per element: |out - truth64| <= half_ulp_bf16(truth64) + 2 E_ref, E_ref the largest absolute error of the
reference's fp32 op sequence (torch CPU) against the float64 truth on the same case; the factor 2 allows another,
equally valid fp32 evaluation order. tests/test_camera_cpu.py::test_plucker_gate_premise holds the reference sequence
to the gate with margin 1 and states why the first term is the half-ulp at the truth's magnitude.
Cases (camera_truth.plucker_cases): the identity; rotations up to 60 degrees about each axis with |t| <= 4; one pose
with t = 0; fx = fy in {0.5, 1, 1.5} x W_pix; the principal point at the centre and off it."""
import pytest
import torch

import camera_truth as ct
from cosmos_predict2 import _native as N
from cosmos_predict2 import camera as cam
from test_fp8_cast_exact_gpu import SENTINEL, guarded, guards_ok

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
HP, WP = ct.PLUCKER_HP, ct.PLUCKER_WP
CASES = ct.plucker_cases()


def _run(device, w2c, intr, Hp=HP, Wp=WP):
    n = w2c.shape[0] * Hp * Wp
    buf, out = guarded(n * 1536, BF16, device, SENTINEL)
    rows = N.plucker_tokens(w2c.to(device), intr.to(device), Hp, Wp, out=out.view(n, 1536))
    torch.cuda.synchronize()
    assert guards_ok(buf, n * 1536, SENTINEL)
    return rows.cpu()


@pytest.mark.parametrize("name", sorted(CASES))
def test_plucker_tokens(device, name):
    w2c, intr = CASES[name]
    t64 = ct.plucker_token_rows(w2c, intr, HP, WP, torch.float64)
    e_ref = (ct.plucker_token_rows(w2c, intr, HP, WP, torch.float32).double() - t64).abs().max().item()
    out = _run(device, w2c, intr)
    assert tuple(out.shape) == (12, 1536) and torch.isfinite(out.float()).all()
    err = (out.double() - t64).abs()
    bound = ct.bf16_half_ulp(t64) + 2 * e_ref
    over = (err - bound).max().item()
    print(f"{name}: E_ref {e_ref:.3e}, largest error beyond the bf16 half-ulp {(err - ct.bf16_half_ulp(t64)).max():.3e}")
    bad = (err > bound).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} elements over the gate by up to {over:.3e}, first {bad[:4].tolist()}"
    # the helper of the public module is the same kernel
    assert torch.equal(cam.plucker_camera_rows(w2c.to(device), intr.to(device), HP, WP).cpu(), out)


def test_feature_and_token_order(device):
    """A pose whose six channels occupy disjoint value ranges (told apart by sign and magnitude) over every pixel of
    every token: channel c must fill columns [256 c, 256 (c + 1)) of every row, pixels (m, n) row-major inside, tokens
    in (frame, hp, wp) order."""
    Hpx, Wpx = 16 * HP, 16 * WP
    eye = torch.eye(3, dtype=torch.float64)
    # camera centre o = (20, -5, 0) (t = -o), the principal point left of and below the image: x_c > 0 > y_c
    w2c = torch.stack([ct.pose(eye, [-20.0, 5.0, 0.0]), ct.pose(eye, [-22.0, 5.5, 0.0])])
    f = 4.0 * Wpx
    intr = torch.tensor([[f, f, -0.4 * Wpx, 0.5 * f + Hpx]] * 2)
    pl = ct.plucker_rays(w2c, ct.intrinsics_matrix(intr.double()), (Hpx, Wpx), torch.float64)  # [2, HW, 6]
    lo, hi = pl.amin(dim=(0, 1)), pl.amax(dim=(0, 1))
    order = torch.argsort(lo)
    tol = torch.maximum(ct.bf16_half_ulp(lo), ct.bf16_half_ulp(hi)) + 1e-5  # a bf16 rounding of the range's ends
    assert (lo[order][1:] - hi[order][:-1] > 2 * tol.max()).all(), "the six channels' ranges must stay disjoint"
    assert (lo[:3] < 0).all() and lo[3] > 0 and hi[4] < 0 and lo[5] > 0
    out = _run(device, w2c, intr).float()  # [12, 1536]
    blocks = out.view(12, 6, 256)
    for c in range(6):
        assert blocks[:, c].min() >= lo[c] - tol[c] and blocks[:, c].max() <= hi[c] + tol[c], f"channel {c}"
    # inside a token: x_c grows with n (columns), so the direction's x grows along n and is constant in sign along m;
    # y_c grows with m (rows). Across tokens: wp moves 16 columns, hp 16 rows, frame 1 has its own centre.
    d = blocks[:, 3:].view(2, HP, WP, 3, 16, 16)
    assert (d[..., 0, :, 1:] > d[..., 0, :, :-1]).float().mean() > 0.9   # d_x rises along n (bf16 ties aside)
    assert (d[..., 1, 1:, :] > d[..., 1, :-1, :]).float().mean() > 0.9   # d_y rises along m
    assert (d[:, :, 1:, 0, :, 0] > d[:, :, :-1, 0, :, 15]).all()          # next wp starts right of the last column
    assert (d[:, 1:, :, 1, 0, :] > d[:, :-1, :, 1, 15, :]).all()          # next hp starts below the last row
    m1 = blocks[:, 1].view(2, HP * WP, 256)
    assert (m1[1].mean() < m1[0].mean() - 1.0)                            # frame 1's centre: m_y = -o_x d_z, |o_x| larger
    t64 = ct.pack_tokens(pl, HP, WP)
    assert ((out.double() - t64).abs() <= ct.bf16_half_ulp(t64) + 1e-5).all()


def test_shapes_and_validation(device):
    """Another grid (1 x 1 and 3 x 2 patches, F = 3) keeps (frame, hp, wp) order; bad arguments raise."""
    w2c, intr = CASES["offcentre"]
    w3 = torch.cat([w2c, w2c[:1]])
    k3 = torch.cat([intr, intr[1:]])
    out = _run(device, w3, k3, 3, 2)
    t64 = ct.plucker_token_rows(w3, k3, 3, 2, torch.float64)
    assert ((out.double() - t64).abs() <= ct.bf16_half_ulp(t64) + 4e-6).all()
    one = _run(device, w2c[:1], intr[:1], 1, 1)
    assert torch.equal(one[0].view(6, 16, 16), out[0].view(6, 16, 16))  # token (0, 0, 0) does not depend on the grid
    with pytest.raises(ValueError):
        N.plucker_tokens(w2c.to(device)[:, :, :3], intr.to(device), 2, 3)
    with pytest.raises(ValueError):
        N.plucker_tokens(w2c.to(device), intr.to(device)[:1], 2, 3)
    with pytest.raises(ValueError):
        N.plucker_tokens(w2c.to(device), intr.to(device), 0, 3)
    with pytest.raises(ValueError):
        N.plucker_tokens(w2c.to(device).double(), intr.to(device), 2, 3)
    assert N.load_library().cp25_plucker_tokens(None, None, None, 1, 1, 1, N._stream(device)) == -22
