"""cp25_gemm_f32, bit for bit against float64 (the fp32 half of test_gemm_exact_gpu.py).

Premise: integer-valued fp32 operands (a in [-8, 8], [-64, 64] at K <= 96; w in [-4, 4]; integer addends in [-64, 64]),
so every product and partial sum is an integer below 2^24 and fp32 accumulation is exact in any order, the split-K
slices' partial sums and their reduction included: the kernel must equal a.double() @ w.double().T (+ addend) under
torch.equal, with split_k on and off. test_premise (no GPU) checks the abs-sum bound and torch's fp32 CPU product
against the fp64 one for every case.

What the cases reach (csrc/gemm_f32.hip): gemm_f32_kernel<ACT, ADD, split, kRB> with kRB = 1 (M <= 64: 64-row tiles)
and 2 (128-row tiles), ragged row tiles (M = 1, 62, 129, 300), N = 72 (a ragged 64-column tile), K = 32 (one chunk, never
split), 96 (three chunks: below the split's four-chunk minimum), 2048 and 5120 (split into up to 16 slices +
gemm_f32_reduce when split_k is on and the grid has fewer than 512 workgroups); the batched strided form (nb = 3, a as
column blocks of one [M, nb A] matrix) and addends as [N], [M, N], a strided column view and [nb, M, N], fused in the
kernel (no split) or in the reduce pass.

SiLU: the sums are scaled by 2^-6 (exact) so that SiLU(x) stays an fp32 normal, and compared per element in fp32 ulps
with float64 silu of the exact sum. Bound: twice the largest distance torch's own CPU fp32 F.silu shows against float64
on the same sums, at least 2 ulp. Measured in test_premise_silu: torch's CPU F.silu is 1.99 ulp away at K = 96, 2048 and
5120 (bound 3.98 ulp) and 1.12 ulp on the 64 sums of K = 32 (bound 2.24 ulp); the kernel measures the same 1.99 and 1.12.
"""
import functools
import zlib

import pytest
import torch
import torch.nn.functional as F

from cosmos_predict2 import _native as N

SENT = -1.5e30
GR = 3
MS, NS, KS = (1, 62, 129, 300), (64, 72, 192, 2048), (32, 96, 2048, 5120)
# every M x N at K = 96, every K at four (M, N), and the largest of each
SHAPES = sorted({(M, Nn, 96) for M in MS for Nn in NS}
                | {(M, Nn, K) for K in KS for M, Nn in ((62, 2048), (300, 72), (129, 192), (1, 64))}
                | {(300, 2048, 2048)})
SILU_SHAPES = [(62, 2048, 2048), (300, 72, 96), (129, 192, 5120), (1, 64, 32)]


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


@functools.lru_cache(maxsize=None)
def _data(M, Nn, K):
    g = _gen(f"f32_{M}_{Nn}_{K}")
    amax = 64 if K <= 96 else 8
    a, w = _ints(g, -amax, amax, (M, K)), _ints(g, -4, 4, (Nn, K))
    return dict(a=a, w=w, acc=a.double() @ w.double().t(), bias=_ints(g, -64, 64, (Nn,)),
                full=_ints(g, -64, 64, (M, 3 * Nn)))


def _ulps(got, truth):
    """|got - truth| in fp32 ulps of truth (float64), the ulp taken no smaller than the smallest normal's."""
    e = torch.floor(torch.log2(truth.abs().clamp_min(2.0 ** -126)))
    return ((got.double() - truth).abs() / torch.pow(2.0, e - 23)).max().item()


def _silu_bound(sums):
    """Twice torch's own CPU fp32 F.silu distance from float64 silu on the same sums, never below 2 ulp."""
    cpu = _ulps(F.silu(sums.float()), F.silu(sums))
    return max(2.0, 2.0 * cpu), cpu


@pytest.mark.parametrize("M,Nn,K", SHAPES)
def test_premise(M, Nn, K):
    d = _data(M, Nn, K)
    absum = (d["a"].double().abs() @ d["w"].double().abs().t()).max().item() + 64
    assert absum < 2 ** 24
    assert torch.equal((d["a"] @ d["w"].t()).double(), d["acc"])


@pytest.mark.parametrize("M,Nn,K", SILU_SHAPES)
def test_premise_silu(M, Nn, K):
    d = _data(M, Nn, K)
    sums = (d["acc"] + d["bias"].double()) * 2.0 ** -6
    assert F.silu(sums)[sums != 0].abs().min().item() >= 2.0 ** -126  # fp32 normals: no flush-to-zero question
    bound, cpu = _silu_bound(sums)
    print(f"silu M={M} N={Nn} K={K}: |x| <= {sums.abs().max().item():.1f}, torch CPU fp32 F.silu {cpu:.2f} ulp from "
          f"float64, bound {bound:.2f} ulp")
    assert cpu <= 4  # the reference's own error is a few ulp at the most: the bound stays meaningful


def _out(shape, device, pad=0):
    big = torch.full((*shape[:-2], shape[-2] + 2 * GR, shape[-1] + pad), SENT, device=device)
    return big, big[..., GR:GR + shape[-2], :shape[-1]]


def _untouched(big, out):
    chk = big.clone()
    chk[..., GR:GR + out.shape[-2], :out.shape[-1]] = SENT
    return torch.equal(chk, torch.full_like(chk, SENT))


def _mismatch(out, ref):
    bad = (out != ref).nonzero()
    first = ", ".join(f"{tuple(i.tolist())}: got {out[tuple(i)].item()} want {ref[tuple(i)].item()}" for i in bad[:6])
    return f"{bad.shape[0]} of {ref.numel()} elements differ; {first}"


@pytest.mark.gpu
@pytest.mark.parametrize("M,Nn,K", SHAPES)
def test_gemm_f32_exact(device, M, Nn, K):
    """Plain, + [N] bias, + [M, N] as a strided column view of [M, 3 N], split_k on and off, into a slice of a
    sentinel-filled buffer with ldc = N + 4."""
    d = _data(M, Nn, K)
    a, w = d["a"].to(device), d["w"].to(device)
    bias, full = d["bias"].to(device), d["full"].to(device)
    adds = ((None, 0), (bias, d["bias"].double()), (full[:, Nn:2 * Nn], d["full"][:, Nn:2 * Nn].double()))
    for add, add64 in adds:
        ref = (d["acc"] + add64).float().to(device)
        for split in (True, False):
            big, out = _out((M, Nn), device, pad=4)
            N.gemm_f32(a, w, add=add, out=out, split_k=split)
            assert _untouched(big, out), "wrote outside the output slice"
            assert torch.equal(out, ref), f"split_k={split} add={None if add is None else tuple(add.shape)}: {_mismatch(out, ref)}"


@pytest.mark.gpu
@pytest.mark.parametrize("M,Nn,K", SILU_SHAPES)
def test_gemm_f32_silu(device, M, Nn, K):
    d = _data(M, Nn, K)
    a, w, bias = (d["a"] * 2.0 ** -6).to(device), d["w"].to(device), (d["bias"] * 2.0 ** -6).to(device)
    sums = (d["acc"] + d["bias"].double()) * 2.0 ** -6
    truth = F.silu(sums)
    bound, cpu = _silu_bound(sums)
    for split in (True, False):
        assert torch.equal(N.gemm_f32(a, w, add=bias, split_k=split).cpu().double(), sums)  # the SiLU's input is exact
        got = N.gemm_f32(a, w, add=bias, act=N.ACT_SILU, split_k=split).cpu()
        u = _ulps(got, truth)
        print(f"silu M={M} N={Nn} K={K} split_k={split}: {u:.2f} ulp (torch CPU {cpu:.2f}, bound {bound:.2f})")
        assert u <= bound, (u, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("add_form", ["none", "n", "mn", "view", "bmn"])
def test_gemm_f32_batched_exact(device, add_form):
    """The AdaLN-LoRA form (test_gemm_f32_batched_strided_addend) at nb = 3, A = 64: a as column blocks of one
    [BT, nb A] matrix, w [nb, N, A], every addend form."""
    g = _gen("f32_batched")
    BT, nb, A, Nn = 62, 3, 64, 192
    a_all, w = _ints(g, -64, 64, (BT, nb * A)), _ints(g, -4, 4, (nb, Nn, A))
    a1 = a_all.view(BT, nb, A).transpose(0, 1)
    wide = _ints(g, -64, 64, (nb, BT, 3 * Nn))
    add = {"none": None, "n": wide[0, 0, :Nn], "mn": wide[0, :, :Nn].contiguous(), "view": wide[0, :, Nn:2 * Nn],
           "bmn": wide[:, :, 2 * Nn:]}[add_form]
    acc = torch.bmm(a1.double(), w.double().transpose(1, 2))
    assert (torch.bmm(a1.double().abs(), w.double().abs().transpose(1, 2)).max() + 64).item() < 2 ** 24
    ref = (acc if add is None else acc + add.double()).float().to(device)
    a_dev = a_all.to(device).view(BT, nb, A).transpose(0, 1)
    wide_dev = wide.to(device)
    add_dev = {"none": None, "n": wide_dev[0, 0, :Nn], "mn": wide_dev[0, :, :Nn].contiguous(),
               "view": wide_dev[0, :, Nn:2 * Nn], "bmn": wide_dev[:, :, 2 * Nn:]}[add_form]
    for split in (True, False):
        big, out = _out((nb, BT, Nn), device, pad=4)
        N.gemm_f32(a_dev, w.to(device), add=add_dev, out=out, split_k=split)
        assert _untouched(big, out), "wrote outside the output slice"
        assert torch.equal(out, ref), f"split_k={split}: {_mismatch(out, ref)}"


@pytest.mark.gpu
def test_gemm_f32_refuses_k_off_the_chunk(device):
    """K % 32 != 0 raises from the wrapper and launches nothing."""
    big, out = _out((8, 64), device)
    with pytest.raises(ValueError):
        N.gemm_f32(torch.ones(8, 48, device=device), torch.ones(64, 48, device=device), out=out)
    torch.cuda.synchronize()
    assert torch.equal(big, torch.full_like(big, SENT))
