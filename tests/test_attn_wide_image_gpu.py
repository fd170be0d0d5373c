"""attn_fwd_wq's LDS image (csrc/attn_wq_image.h: a 64-key tile as 16 DMA pieces of four 256-B rows, rows r, r + 8,
r + 16, r + 24 of a 32-row group to a piece, pieces 1056 B apart) against attn_fwd_m16 (form 0, untouched code, its own
288-B image) on the same inputs under torch.equal, and against attn_truth's selector rows where an absolute answer is
wanted. B 1, H 2, Lq = 2 R + 33 (two full blocks and a ragged one), R in {320, 384}; every output is written into a
buffer filled with a sentinel, so an unwritten row shows.

What this image can get wrong and the row-major one could not:
* rows cut inside a piece: the ragged tile's bounds check is per DMA lane, and a piece's four rows are 8 keys apart,
  so the cut falls between rows of one piece. Lk = 4096 + m (the ragged tile is image 0 of its buffer) and 4160 + m
  (image 1) for m in {1, 7, 8, 9, 24, 31, 32, 33, 40, 63}: either side of the 8-row and the 32-row boundaries;
* a key's row or a 16-B chunk in the wrong slot: the selector with all 128 key positions of a middle iteration and of
  the last whole one named, so every row of both images of a K and a V buffer is some query row's answer and must
  come back as that key's v row bit for bit;
* key splits that end in mid-iteration (Lk 4200: 2, 3 and 6 splits) and on a ragged tile (Lk 4231, 3 splits);
* the fused q RMSNorm + RoPE entry (Lk 4255).
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
M90 = (15 / 16, 3 / 4)  # tests/test_attn_exact_gpu.py: 128 mq mk = 90 log2 units, a fixed-shift launch
CUTS = [1, 7, 8, 9, 24, 31, 32, 33, 40, 63]


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
@pytest.mark.parametrize("m", CUTS)
@pytest.mark.parametrize("base", [4096, 4160], ids=["image0", "image1"])
def test_image_rows_cut_inside_a_piece(device, R, base, m):
    Lk = base + m
    q, k, v, nb = _inputs(device, 1, 2, 2 * R + 33, Lk, 1000 + R + Lk)
    _assert_same_as_form0(device, R, q, k, v, prescaled=True, norm_bounds=nb, n_split=1)


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("Lk, n_split", [(4200, 2), (4200, 3), (4200, 6), (4231, 3)])
def test_image_key_splits(device, R, Lk, n_split):
    q, k, v, nb = _inputs(device, 1, 2, 2 * R + 33, Lk, 2000 + R + Lk + n_split)
    _assert_same_as_form0(device, R, q, k, v, prescaled=True, norm_bounds=nb, n_split=n_split)


@pytest.mark.parametrize("R", WIDTHS)
def test_image_fused_qnorm_rope(device, R):
    """cp25_attn_fwd_prescaled_qnorm (q raw: RMSNorm + RoPE + prescale in the kernel) at 67 tiles, ragged by 31."""
    B, H, Lq, Lk = 1, 2, 2 * R + 33, 4255
    g = torch.Generator(device="cpu").manual_seed(3000 + R)
    w = (0.5 + torch.rand(128, generator=g)).to(torch.bfloat16)
    q = torch.randn(B, Lq, H, 128, generator=g).to(device, torch.bfloat16)
    k = _rms_rows(torch.randn(B, Lk, H, 128, generator=g), w.float()).to(device)
    v = torch.randn(B, Lk, H, 128, generator=g).to(device, torch.bfloat16)
    ang = torch.rand(Lq, 64, generator=g) * 50.0
    qn = dict(weight=w.to(device), cos=torch.cos(ang).to(device), sin=torch.sin(ang).to(device), out_scale=C)
    wb = 128 ** 0.5 * float(w.float().abs().max()) * 1.02
    _assert_same_as_form0(device, R, q, k, v, prescaled=True, norm_bounds=(wb * C, wb), q_norm=qn, n_split=1)


@pytest.mark.parametrize("R", WIDTHS)
def test_image_selector_every_slot_of_an_iteration(device, R):
    """attn_truth's selector: every query row picks one key and must return that key's v row bit for bit. Named keys:
    all 128 positions of a middle 128-key iteration (keys 2048 ..) and of the last whole one (4096 .. 4223 of Lk =
    4225), so every row of both images of a buffer, every piece and every lane block of it, is some row's answer: a
    K row in the wrong slot picks another winner, a V row or 16-B chunk in the wrong slot returns other values."""
    B, H, Lq, Lk = 1, 2, 2 * R + 33, 4225
    last = (Lk // 128 - 1) * 128
    keys = [b0 + p for b0 in (16 * 128, last) for p in range(128)]
    assert last + 128 == Lk - 1 and len(set(keys)) == 256 and Lq >= len(keys)
    d = T.selector(B, H, Lq, Lk, M90[0], M90[1], 4000 + R, keys=keys, rows=T.row_targets(Lq, R, R // 4))
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
