"""The Reason1 text encoder's row kernels (csrc/text_ops.hip) against tests/reason1_truth.py.

Exact inputs (integer-valued bf16 rows, zero or integer row means: test_text_encoder_cpu.py asserts that their fp32 sums
equal the float64 sums in any order) must give the truth bit for bit: with exact sums every remaining step is one IEEE
operation and one bf16 rounding. Gaussian rows must be within one bf16 ulp of the truth everywhere; the share of
unequal elements is printed (DESIGN.md section 6i records it). Every output goes into a row (and, where the entry has a
leading dimension of its own, column) slice of a sentinel-filled buffer whose surroundings must stay untouched."""
import pytest
import torch
import torch.nn.functional as F

import reason1_truth as T
from cosmos_predict2 import _native as N

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SENT = -1.5e30
GR = 3  # sentinel rows before and after an output slice
DS = (512, 3584)
NS = (1, 63, 64, 65, 512)


def _framed(n, cols, device, pad=0):
    """(big, view): a sentinel-filled [n + 2 GR, cols + pad] buffer and its [n, cols] middle."""
    big = torch.full((n + 2 * GR, cols + pad), SENT, dtype=BF16, device=device)
    return big, big[GR:GR + n, :cols]


def _frame_untouched(big, n, cols):
    chk = big.clone()
    chk[GR:GR + n, :cols] = SENT
    return torch.equal(chk, torch.full_like(chk, SENT))


def _weight(D, seed):
    return (0.75 + 0.5 * torch.rand(D, generator=torch.Generator().manual_seed(seed))).to(BF16)


def _run_add_rmsnorm(device, x, y, w, h_ld):
    n, D = x.shape
    xbig, xv = _framed(n, D, device)
    xv.copy_(x)
    hbig, hv = _framed(n, h_ld, device)
    N.add_rmsnorm(xv, None if y is None else y.to(device), w.to(device), h_ld=h_ld, out=hv)
    torch.cuda.synchronize()
    assert _frame_untouched(xbig, n, D) and _frame_untouched(hbig, n, h_ld)
    return xv.cpu(), hv.cpu()


def _check_pad(h, D):
    if h.shape[1] > D:
        assert torch.equal(h[:, D].float(), torch.ones(h.shape[0]))
        assert not h[:, D + 1:].any()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_add_rmsnorm_exact(device, D, n):
    x = T.integer_rows(n, D, seed=n + D)
    y = T.integer_rows(n, D, seed=n + D + 1)
    w = _weight(D, 7)
    for h_ld in (D, D + 64):
        for yy in (y, None):
            xs = x.float() + y.float() if yy is not None else x.float()
            assert T.sums_exact(xs.to(BF16))
            want = T.rmsnorm(xs, w.float(), rounded=True).to(BF16)
            xo, h = _run_add_rmsnorm(device, x, yy, w, h_ld)
            assert torch.equal(xo, xs.to(BF16))
            assert torch.equal(h[:, :D], want), (D, n, h_ld)
            _check_pad(h, D)


@pytest.mark.parametrize("D", DS)
def test_add_rmsnorm_gaussian(device, D):
    g = torch.Generator().manual_seed(D)
    n = 512
    x = (torch.randn(n, D, generator=g) * 1.7).to(BF16)
    y = torch.randn(n, D, generator=g).to(BF16)
    w = _weight(D, 8)
    xs = T.rb(x.float() + y.float())
    want = T.rmsnorm(xs, w.float(), rounded=True).to(BF16)
    xo, h = _run_add_rmsnorm(device, x, y, w, D + 64)
    assert torch.equal(xo, xs.to(BF16))
    d = T.ulp_distance(h[:, :D], want)
    print(f"add_rmsnorm D={D}: {(d > 0).float().mean().item():.3e} of the elements differ from the truth, max {d.max().item()} ulp")
    assert d.max().item() <= 1
    _check_pad(h, D)


def _run_mean_normalize(device, x, col0, blocks):
    n, D = x.shape
    big, ov = _framed(n, blocks * D, device, pad=16)
    N.mean_normalize(x.to(device), ov, col0)
    torch.cuda.synchronize()
    chk = big.clone()
    chk[GR:GR + n, col0:col0 + D] = SENT
    assert torch.equal(chk, torch.full_like(chk, SENT))
    return ov[:, col0:col0 + D].cpu()


@pytest.mark.parametrize("D", DS)
@pytest.mark.parametrize("n", NS)
def test_mean_normalize_exact(device, D, n):
    for x in (T.integer_rows(n, D, seed=n + D, zero_mean=True), T.integer_mean_rows(n, D, seed=n + D + 1, mean=3),
              T.integer_mean_rows(n, D, seed=n + D + 2, mean=-2)):
        assert T.sums_exact(x, centered=True)
        want = T.mean_normalize(x.float(), rounded=True).to(BF16)
        assert want.float().std().item() > 0.5
        for col0 in (0, D):
            assert torch.equal(_run_mean_normalize(device, x, col0, 2), want), (D, n, col0)


@pytest.mark.parametrize("D", DS)
def test_mean_normalize_gaussian(device, D):
    g = torch.Generator().manual_seed(D + 1)
    x = (torch.randn(512, D, generator=g) * 2.5 + 0.3).to(BF16)
    want = T.mean_normalize(x.float(), rounded=True).to(BF16)
    got = _run_mean_normalize(device, x, D, 3)
    d = T.ulp_distance(got, want)
    print(f"mean_normalize D={D}: {(d > 0).float().mean().item():.3e} of the elements differ from the truth, max {d.max().item()} ulp")
    assert d.max().item() <= 1


def test_mean_normalize_constant_row(device):
    """std = 0: the reference divides by bf16(0 + 1e-8); a constant row gives 0 / 1e-8 = 0."""
    x = torch.full((2, 512), 3.0, dtype=BF16)
    got = _run_mean_normalize(device, x, 0, 1)
    assert torch.equal(got, T.mean_normalize(x.float(), rounded=True).to(BF16)) and not got.any()


def test_swiglu_all_gate_values(device):
    """All 65536 bf16 gate bit patterns at up = 1 equal PyTorch's device silu on the bf16 tensor, bit for bit (NaNs at
    the same places); against the CPU truth the count of differing inputs is printed and none is off by more than one
    ulp."""
    I = 1024
    g = torch.arange(65536, dtype=torch.int32).to(torch.int16).view(BF16).view(64, I)
    gu = torch.cat([g, torch.ones(64, I, dtype=BF16)], 1).to(device)
    big, ov = _framed(64, I, device, pad=8)
    N.swiglu(gu, out=ov)
    torch.cuda.synchronize()
    assert _frame_untouched(big, 64, I)
    got = ov.cpu()
    ref = F.silu(gu[:, :I]).cpu()
    assert torch.equal(got.isnan(), ref.isnan())
    assert torch.equal(torch.nan_to_num(got.float(), nan=0.0), torch.nan_to_num(ref.float(), nan=0.0))
    truth = T.swiglu(g.float(), torch.ones(64, I), rounded=True).to(BF16)
    fin = truth.float().isfinite() & got.float().isfinite()
    assert torch.equal(fin, truth.float().isfinite())
    d = T.ulp_distance(got[fin], truth[fin])
    print(f"swiglu: {(d > 0).sum().item()} of {fin.sum().item()} finite gate values differ from the CPU truth, max "
          f"{d.max().item()} ulp")
    assert d.max().item() <= 1


@pytest.mark.parametrize("n,I", [(1, 1024), (65, 1024), (64, 18944)])
def test_swiglu_rows(device, n, I):
    g = torch.Generator().manual_seed(n + I)
    gu = (torch.randn(n, 2 * I, generator=g) * 2.0).to(BF16)
    big, ov = _framed(n, I, device, pad=8)
    N.swiglu(gu.to(device), out=ov)
    torch.cuda.synchronize()
    assert _frame_untouched(big, n, I)
    ref = (F.silu(gu[:, :I].to(device)) * gu[:, I:].to(device)).cpu()  # two bf16 ops on the device
    assert torch.equal(ov.cpu(), ref)
    d = T.ulp_distance(ov.cpu(), T.swiglu(gu[:, :I].float(), gu[:, I:].float(), rounded=True).to(BF16))
    assert d.max().item() <= 1


@pytest.mark.parametrize("Hq,Hkv", [(4, 2), (28, 4)])
def test_rope_positions(device, Hq, Hkv):
    """Position 0 is the identity; rows L and L + 1 of a B = 2 buffer use positions 0 and 1; every row equals the
    truth's three rounded ops bit for bit; the v columns are not touched."""
    B, L = 2, 64
    g = torch.Generator().manual_seed(Hq)
    ld = (Hq + 2 * Hkv) * 128
    buf = (torch.randn(B * L, ld, generator=g) * 1.5).to(BF16)
    cos, sin = T.rope_tables(L)
    cos, sin = cos.to(BF16), sin.to(BF16)
    big, bv = _framed(B * L, ld, device)
    bv.copy_(buf)
    N.rope_qk(bv, cos.to(device), sin.to(device), heads=Hq + Hkv)
    torch.cuda.synchronize()
    assert _frame_untouched(big, B * L, ld)
    got = bv.cpu()
    qk = buf[:, :(Hq + Hkv) * 128].float().view(B, L, Hq + Hkv, 128)
    want = T.rope(qk, cos.float(), sin.float(), rounded=True).to(BF16).view(B * L, -1)
    assert torch.equal(got[:, :(Hq + Hkv) * 128], want)
    assert torch.equal(got[:, (Hq + Hkv) * 128:], buf[:, (Hq + Hkv) * 128:])
    assert torch.equal(got[0, :(Hq + Hkv) * 128], buf[0, :(Hq + Hkv) * 128])  # position 0
    assert torch.equal(got[L, :(Hq + Hkv) * 128], buf[L, :(Hq + Hkv) * 128])  # row L: position 0 again
    one = T.rope(buf[L + 1, :(Hq + Hkv) * 128].float().view(1, 1, -1, 128), cos[1:2].float(), sin[1:2].float(), True)
    assert torch.equal(got[L + 1, :(Hq + Hkv) * 128], one.to(BF16).view(-1))
    assert not torch.equal(got[1], buf[1])


@pytest.mark.parametrize("D", DS)
def test_gather(device, D):
    V = 1000
    g = torch.Generator().manual_seed(D)
    table = torch.randn(V, D, generator=g).to(BF16)
    tab = table.to(device)
    ids = torch.tensor([[0, V - 1, 5, 5, V - 1, 0, 17]], dtype=torch.int64)
    big, ov = _framed(7, D, device, pad=8)
    N.embed_gather(tab, ids, out=ov)
    torch.cuda.synchronize()
    assert _frame_untouched(big, 7, D)
    assert torch.equal(ov.cpu(), table[ids[0]])
    for bad in (V, -1, 2 ** 31 + 5):
        big.fill_(SENT)
        with pytest.raises(ValueError):
            N.embed_gather(tab, torch.tensor([3, bad, 4], dtype=torch.int64), out=big[GR:GR + 3, :D])
        torch.cuda.synchronize()
        assert torch.equal(big, torch.full_like(big, SENT))
    with pytest.raises(ValueError):
        N.embed_gather(tab, ids.to(device), out=ov)  # device ids cannot be validated before upload


def test_refused_calls_launch_nothing(device):
    """Arguments the C entries refuse (-22 / -95): a ValueError, and the outputs keep their sentinel."""
    lib = N.load_library()
    D = 512
    x = torch.full((4, D), SENT, dtype=BF16, device=device)
    h = torch.full((4, D + 64), SENT, dtype=BF16, device=device)
    w = torch.ones(D, dtype=BF16, device=device)
    st = torch.cuda.current_stream(device).cuda_stream
    p = lambda t: t.data_ptr()
    # h_ld not a multiple of 64, h_ld < D, D % 8, eps <= 0, misaligned x, D above the kernel's row capacity
    assert lib.cp25_add_rmsnorm(p(x), D, None, 0, p(w), p(h), D + 8, 4, D, 1e-6, st) == -22
    assert lib.cp25_add_rmsnorm(p(x), D, None, 0, p(w), p(h), D - 64, 4, D, 1e-6, st) == -22
    assert lib.cp25_add_rmsnorm(p(x), D, None, 0, p(w), p(h), 448, 4, 444, 1e-6, st) == -22
    assert lib.cp25_add_rmsnorm(p(x), D, None, 0, p(w), p(h), D, 4, D, 0.0, st) == -22
    assert lib.cp25_add_rmsnorm(p(x) + 2, D, None, 0, p(w), p(h), D, 2, D, 1e-6, st) == -22
    assert lib.cp25_add_rmsnorm(p(x), 16384, None, 0, p(w), p(h), 16384, 1, 16384, 1e-6, st) == -95
    assert lib.cp25_mean_normalize(p(x), D, p(h), D + 64, 128, 4, D, st) == -22  # col0 + D > out_ld
    assert lib.cp25_mean_normalize(p(x), D, p(h), D + 64, 4, 4, D, st) == -22    # col0 % 8
    assert lib.cp25_swiglu(p(h), D + 64, p(x), D, 4, D, st) == -22               # ld < 2 I
    assert lib.cp25_rope_qk(p(h), D + 64, 4, 3, 4, p(x), p(x), st) == -22        # n % L
    assert lib.cp25_rope_qk(p(h), D + 64, 4, 4, 5, p(x), p(x), st) == -22        # heads do not fit ld
    assert lib.cp25_embed_gather(p(x), 4, D, p(w), p(h), D - 8, 4, st) == -22    # out_ld < D
    torch.cuda.synchronize()
    assert torch.equal(x, torch.full_like(x, SENT)) and torch.equal(h, torch.full_like(h, SENT))
    with pytest.raises(ValueError):
        N.add_rmsnorm(x, None, w, h_ld=D + 8)
