"""cp25_rms_norm_silu at all five widths (C / 32 in {1, 2, 3, 6, 12}), SiLU on and off, against oracle.vae.rms_norm
(RMS_norm, tokenizers/wan2pt1.py:65-77: F.normalize over C, * sqrt(C), * gamma in bf16 tensor ops).

n_pix = 131 is no multiple of the 64 pixels per workgroup: the last workgroup holds 3 pixels. The output is a slice of a
sentinel-filled buffer and the elements around it must be untouched.

Exact-norm inputs: per pixel k entries are +-a and the rest are 0, a a power of two in [2^-3, 2^3], k = 16 (C = 32),
64 (C = 64, 96, 192) or 256 (C = 384). Then ||x|| = a sqrt(k) is exact in fp32 and in bf16, so no tie in the norm's
rounding can fall differently in the kernel and in torch, and the oracle equals the closed form
bf16(bf16(bf16(sign / sqrt k) * float32(sqrt C)) * gamma) bit for bit (asserted without a GPU in
test_exact_inputs_closed_form). With SiLU off the kernel must equal the oracle (torch.equal); with SiLU on every
element is within one bf16 ulp (expf against torch's) and at least 0.99 of them equal (test_vae_gpu.test_rms_norm_silu's
share).

Gaussian inputs: the two assertions of test_vae_gpu.test_rms_norm_silu, unchanged, for each width and SiLU setting.
"""
import functools

import pytest
import torch

from cosmos_predict2 import _native as N
from oracle import vae as ovae
from test_dit_ops_gpu import bf16_ulp_close

BF16 = torch.bfloat16
WIDTHS = (32, 64, 96, 192, 384)
N_PIX = 131
GUARD = 256
SENTINEL = -1.5e30


def _k(C):
    return {32: 16, 64: 64, 96: 64, 192: 64, 384: 256}[C]


@functools.lru_cache(maxsize=None)
def _inputs(C, kind):
    """x [N_PIX, C] bf16 (channels-last pixels), gamma [C] bf16."""
    g = torch.Generator().manual_seed(C + (1000 if kind == "exact" else 0))
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).to(BF16)
    if kind == "gauss":
        return torch.randn(N_PIX, C, generator=g).to(BF16), gamma
    k = _k(C)
    a = torch.pow(2.0, torch.randint(-3, 4, (N_PIX, 1), generator=g).float())
    sign = torch.randint(0, 2, (N_PIX, C), generator=g).float() * 2 - 1
    pos = torch.rand(N_PIX, C, generator=g).argsort(dim=1) < k  # k random positions per pixel
    return (a * sign * pos).to(BF16), gamma


@functools.lru_cache(maxsize=None)
def _reference(C, kind, silu):
    x, gamma = _inputs(C, kind)
    ref = ovae.rms_norm(x.t().reshape(1, C, 1, 1, N_PIX), gamma.reshape(C, 1, 1, 1))
    if silu:
        ref = ovae.silu(ref)
    return ref[0].reshape(C, N_PIX).t().contiguous()  # [N_PIX, C]


def _run(device, C, kind, silu):
    x, gamma = _inputs(C, kind)
    buf = torch.full((N_PIX * C + 2 * GUARD,), SENTINEL, dtype=BF16, device=device)
    out = buf[GUARD:GUARD + N_PIX * C].view(N_PIX, C)
    N.rms_norm_silu(x.to(device), gamma.to(device), silu=silu, out=out)
    torch.cuda.synchronize()
    buf = buf.cpu()
    guard = torch.full((GUARD,), SENTINEL, dtype=BF16)
    assert torch.equal(buf[:GUARD], guard), "wrote before the output"
    assert torch.equal(buf[GUARD + N_PIX * C:], guard), "wrote past the output"
    return buf[GUARD:GUARD + N_PIX * C].view(N_PIX, C)


@pytest.mark.parametrize("C", WIDTHS)
def test_exact_inputs_closed_form(C):
    """No kernel: on the exact-norm inputs the oracle is the closed form, so the GPU test's torch.equal has one answer."""
    x, gamma = _inputs(C, "exact")
    k = _k(C)
    assert ((x != 0).sum(1) == k).all()
    nrm = x.float().norm(2, dim=1)
    assert torch.equal(nrm, nrm.to(BF16).float())  # exact in bf16
    assert torch.equal(nrm, x.float().abs().amax(1) * k ** 0.5)
    y = (torch.sign(x.float()) / k ** 0.5).to(BF16)
    y = (y.float() * torch.tensor(C ** 0.5, dtype=torch.float32)).to(BF16)
    y = (y.float() * gamma.float()).to(BF16)
    assert torch.equal(y, _reference(C, "exact", False))


@pytest.mark.gpu
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("C", WIDTHS)
def test_rms_norm_exact_inputs(device, C, silu):
    out = _run(device, C, "exact", silu)
    ref = _reference(C, "exact", silu)
    if not silu:
        bad = (out != ref).nonzero()
        assert torch.equal(out, ref), f"{bad.shape[0]} elements differ, first (pixel, channel) {bad[:4].tolist()}"
    else:
        ok, eq = bf16_ulp_close(out, ref, min_equal=0.99)
        assert ok, eq


@pytest.mark.gpu
@pytest.mark.parametrize("silu", [False, True], ids=["plain", "silu"])
@pytest.mark.parametrize("C", WIDTHS)
def test_rms_norm_gaussian(device, C, silu):
    out = _run(device, C, "gauss", silu)
    ref = _reference(C, "gauss", silu)
    assert (out.float() - ref.float()).abs().max().item() <= 2 * 2 ** -7 * ref.float().abs().max().item()
    assert (out == ref).float().mean().item() >= 0.99


@pytest.mark.gpu
@pytest.mark.parametrize("C", [48, 128])
def test_rms_norm_rejects_width(device, C):
    """C = 48 is no multiple of 32; C = 128 is, but C / 32 = 4 has no instantiation."""
    x = torch.zeros(8, C, dtype=BF16, device=device)
    with pytest.raises(ValueError):
        N.rms_norm_silu(x, torch.ones(C, dtype=BF16, device=device))
