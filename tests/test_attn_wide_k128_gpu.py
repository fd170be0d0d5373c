"""attn_fwd_wq's 128-key iterations (attn_wide.hip: two 64-key images per LDS buffer, one barrier per 128 keys, nine DMA
pieces per wave for K and nine for V) against attn_fwd_m16 (form 0, untouched code) on the same inputs under
torch.equal, and against attn_truth's selector rows where an absolute answer is wanted.

What the two-tile iteration can get wrong and the 64-key loop could not: an odd tile count (the last iteration is half
full: its second image is a virtual tile of zero rows whose P.V must add exactly nothing), a ragged last tile in either
image and on either side of the 32-key half stage, a key-range split that ends in mid-iteration, pieces 16-17 of the two
images moved by different wave pairs, and the image offset of the fragment reads. So Lk takes 4097 (one key into an odd
tile), 4160 (65 tiles), 4224 (33 x 128) and 4225 / 4255 / 4257 / 4287 (ragged by 1 / 31 / 33 / 63 keys), each at 320
and 384 rows with Lq = 2 x rows + 33 (two full blocks and a ragged one). Splits at Lk 4200 (66 tiles): 1 and 3 (22
tiles each), and 2 and 6, whose 33 and 11 tiles per split are odd, so every split ends in a half-full iteration.
Every output is written into a buffer filled with a sentinel, so an unwritten row shows.
"""
import pytest
import torch

import attn_truth as T
from cosmos_predict2 import _native as N

pytestmark = pytest.mark.gpu

LOG2E = 1.4426950408889634
C = 128 ** -0.5 * LOG2E
WIDTHS = [320, 384]
SENTINEL = -1.5e30
TOL = 4e-3  # tests/test_attn_wide_gpu.py: rel-L2 of merged key splits against the whole launch, x 1.5
M90 = (15 / 16, 3 / 4)  # tests/test_attn_exact_gpu.py: 128 mq mk = 90 log2 units, a fixed-shift launch
RAGGED_LK = [4097, 4160, 4224, 4225, 4255, 4257, 4287]


def _name(width):
    return f"attn_fwd_wq<self, prescaled, {width} rows, fixed shift>"


def _rms_rows(t, w):
    tf = t.float()
    return (tf * torch.rsqrt(tf.pow(2).mean(-1, keepdim=True) + 1e-6) * w).to(torch.bfloat16)


def _inputs(device, B, H, Lq, Lk, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = 0.5 + torch.rand(128, generator=g)
    q = (_rms_rows(torch.randn(B, Lq, H, 128, generator=g), w).float() * C).to(torch.bfloat16).to(device)
    k = _rms_rows(torch.randn(B, Lk, H, 128, generator=g), w).to(device)
    v = torch.randn(B, Lk, H, 128, generator=g).to(device, torch.bfloat16)
    nb = (q.float().norm(dim=-1).max().item() * 1.01, k.float().norm(dim=-1).max().item() * 1.01)
    return q, k, v, nb


def _launch(device, form, q, k, v, **kw):
    """One launch under cp25_attn_self_select(form) into a sentinel-filled strided buffer: (output [B, Lq, H, 128],
    whether everything outside the output view still holds the sentinel)."""
    B, Lq, H = q.shape[0], q.shape[1], q.shape[2]
    prev = N.attn_self_select(form)
    try:
        buf = torch.full((Lq + 3, B, 2, H, 128), SENTINEL, dtype=torch.bfloat16, device=device)
        N.attn_fwd(q, k, v, out=buf[:Lq, :, 1].transpose(0, 1), **kw)
        torch.cuda.synchronize()
    finally:
        N.attn_self_select(prev)
    clean = bool((buf[:, :, 0] == SENTINEL).all()) and bool((buf[Lq:] == SENTINEL).all())
    return buf[:Lq, :, 1].transpose(0, 1).contiguous(), clean


def _assert_same_as_form0(device, R, q, k, v, **kw):
    prev = N.attn_self_select(R)
    try:
        assert N.attn_kernel_name(k.shape[1], norm_bounds=kw["norm_bounds"], prescaled=True) == _name(R)
    finally:
        N.attn_self_select(prev)
    a, _ = _launch(device, 0, q, k, v, **kw)
    b, clean = _launch(device, R, q, k, v, **kw)
    assert clean, "written outside the output view"
    assert not (b == SENTINEL).any(), "an output row was not written"
    assert torch.isfinite(b.float()).all()
    assert torch.equal(a, b), (R, tuple(q.shape), k.shape[1], (a.float() - b.float()).abs().max().item())


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("Lk", RAGGED_LK)
def test_k128_ragged_and_odd_tiles(device, R, Lk):
    q, k, v, nb = _inputs(device, 1, 2, 2 * R + 33, Lk, 100 + R + Lk)
    _assert_same_as_form0(device, R, q, k, v, prescaled=True, norm_bounds=nb, n_split=1)


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("n_split", [1, 3, 2, 6])
def test_k128_key_splits(device, R, n_split):
    q, k, v, nb = _inputs(device, 1, 2, 2 * R + 33, 4200, 200 + R + n_split)
    _assert_same_as_form0(device, R, q, k, v, prescaled=True, norm_bounds=nb, n_split=n_split)


@pytest.mark.parametrize("R", WIDTHS)
def test_k128_tail_split(device, R):
    """The smallest plan with a tail under the device's CU count (tests/test_attn_wide_gpu.py's recipe: 29 query blocks
    x enough heads to pass the CU count, an unsplit plan by cp25_attn_plan): the rows the plan computes whole are form
    0's bit for bit, the tail segment's rows (merged key splits, 173 / 144 tiles cut into splits of their own) within
    1.5 TOL of the whole launch."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    nqb = 29
    H = cus // nqb + 1
    L = nqb * R - 100
    t0 = (nqb - (nqb * H - cus)) * R
    assert N.attn_plan(1, H, L, L, 128) == 1
    prev = N.attn_self_select(R)
    try:
        assert N.load_library().cp25_attn_tail_workspace_bytes(1, H, L, L) > 0  # the plan has a tail here
    finally:
        N.attn_self_select(prev)
    q, k, v, nb = _inputs(device, 1, H, L, L, 300 + R)
    whole, _ = _launch(device, 0, q, k, v, prescaled=True, norm_bounds=nb, n_split=1)
    tail, clean = _launch(device, R, q, k, v, prescaled=True, norm_bounds=nb)
    assert clean and not (tail == SENTINEL).any()
    assert torch.equal(tail[:, :, :H - 1], whole[:, :, :H - 1])
    assert torch.equal(tail[0, :t0, H - 1], whole[0, :t0, H - 1])
    x, y = tail[0, t0:, H - 1].float(), whole[0, t0:, H - 1].float()
    e = ((x - y).norm() / y.norm()).item()
    print(f"width {R}: tail rows {t0}..{L} of the last head vs the whole launch: rel-L2 {e:.3e}")
    assert 0 < e <= 1.5 * TOL, e


@pytest.mark.parametrize("R", WIDTHS)
def test_k128_fused_qnorm_rope(device, R):
    """cp25_attn_fwd_prescaled_qnorm (q raw: RMSNorm + RoPE + prescale in the kernel) at 67 tiles, ragged by 31."""
    B, H, L = 1, 2, 4255
    g = torch.Generator(device="cpu").manual_seed(400 + R)
    w = (0.5 + torch.rand(128, generator=g)).to(torch.bfloat16)
    q = torch.randn(B, L, H, 128, generator=g).to(device, torch.bfloat16)
    k = _rms_rows(torch.randn(B, L, H, 128, generator=g), w.float()).to(device)
    v = torch.randn(B, L, H, 128, generator=g).to(device, torch.bfloat16)
    ang = torch.rand(L, 64, generator=g) * 50.0
    qn = dict(weight=w.to(device), cos=torch.cos(ang).to(device), sin=torch.sin(ang).to(device), out_scale=C)
    wb = 128 ** 0.5 * float(w.float().abs().max()) * 1.02
    _assert_same_as_form0(device, R, q, k, v, prescaled=True, norm_bounds=(wb * C, wb), q_norm=qn, n_split=1)


@pytest.mark.parametrize("R", WIDTHS)
def test_k128_selector_keys_around_the_iteration(device, R):
    """attn_truth's selector: every query row picks one key and must return that key's v row bit for bit. Named keys:
    positions 63, 64, 127, 128 and 129 of the first, a middle and the last whole 128-key iteration but one (the last
    key of image 0, both ends of image 1, the first keys of the next iteration's image 0), 63, 64 and 127 of the last
    whole one, and the last key, which at Lk = 4225 sits alone in the odd 67th tile, the half-full iteration."""
    B, H, Lq, Lk = 1, 2, 2 * R + 33, 4225
    last = (Lk // 128 - 1) * 128  # the last whole iteration: its position 128 is the last key
    keys = [b0 + p for b0 in (0, 16 * 128, last - 128) for p in (63, 64, 127, 128, 129)]
    keys += [last + 63, last + 64, last + 127, Lk - 1]
    assert last + 128 == Lk - 1 and len(set(keys)) == len(keys)
    d = T.selector(B, H, Lq, Lk, M90[0], M90[1], 500 + R, keys=keys, rows=T.row_targets(Lq, R, R // 4))
    assert all((d["pi"] == key).any() for key in keys)  # every named key is some row's answer
    nb = T.norm_bounds(d["q"], d["k"], 1.0005)
    prev = N.attn_self_select(R)
    try:
        assert N.attn_kernel_name(Lk, norm_bounds=nb, prescaled=True) == _name(R)
    finally:
        N.attn_self_select(prev)
    o, clean = _launch(device, R, d["q"].to(device), d["k"].to(device), d["v"].to(device), prescaled=True,
                       norm_bounds=nb, n_split=1)
    assert clean
    bad = (o.cpu() != d["expected"]).any(-1)
    assert not bad.any(), (int(bad.sum()), tuple(bad.nonzero()[0].tolist()), d["gap"])
