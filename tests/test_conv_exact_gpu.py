"""cp25_conv3d, bit for bit against float64, in every kernel form a shape can take.

Premise: the inputs are small integers stored as bf16 (x in [-8, 8], w in [-4, 4], bias in [-8, 8], residual in
[-64, 64], seeded CPU generator). Every product is an integer and every partial sum stays below 2^24 as long as
conv(|x|, |w|) + |b| < 2^24 (the largest case here, 27 x 384 taps, reaches at most 3.4e5), so fp32 accumulation is
exact in any order and the only roundings left are the documented ones: bf16(acc + bias), then bf16(that + residual).
The kernel output must therefore equal F.conv3d in float64, rounded to bf16 at those two points, under torch.equal:
no tolerance. test_premise (no GPU) checks the premise for every case: the abs-sum bound, torch's fp32 CPU conv equal
to the fp64 one, and for the large-K cases a non-zero share of outputs that are exact bf16 ties (so round-to-nearest-
even is exercised, not only exact values).

Every case writes into a slice of a larger buffer pre-filled with a sentinel; the elements before and after the slice
must be untouched. Cases the default dispatch gives to conv3x3_halo_kernel run under all three cp25_conv3d_select
modes (0: 8 waves, 1: the per-tap kernel, 2: 4 waves); each must equal the reference. The other cases run the per-tap
kernel conv_igemm_kernel<BK, NT> (select 1, so that no later dispatch change moves them).

What the cases reach (csrc/vae_ops.hip):
  conv_igemm_kernel: all 12 (BK, NT) instantiations at M = 140 (a ragged second 128-pixel block); Cout 18 (nvalid = 2,
    out_C % 4 != 0, the scalar stores); Cout 160 (NT = 4 with a partial second tile); a residual; stride_hw = 2; the
    upsample gather; negative top / bottom pads; KT = 3 with a zero frame; the (3,1,1) time convs with stride_t = 2 and
    with out_split (the frame interleave of tokenizers/wan2pt1.py:139-141, split boundary on and inside a 32-channel
    block); the 1x1 conv 64 -> 288 (three NT = 4 tiles, the last partial).
  conv3x3_halo_kernel: nst = KT Cin / 16 of 1, 2 (both ways) and 3 (the pipeline prologue's own branches); Cout 64, 100
    and 160 (the zero-page weight guard and the scalar epilogue, alone and beside the vector one), with a residual;
    Ho = 1; a second row-tile of one row; 1, 2 and 3 column tiles; top / bottom pads of 0 and -1; the upsample gather;
    KT = 3 with stride_t = 2; a 9-workgroup grid (the XCD remap off a multiple of 8); and 27 x 384 taps.
"""
import dataclasses
import functools
from typing import Tuple

import pytest
import torch
import torch.nn.functional as F

from cosmos_predict2 import _native as N
from cosmos_predict2.vae import _Conv

BF16 = torch.bfloat16
GUARD = 256  # sentinel elements before and after the output slice (512 B: the slice keeps its 16-B alignment)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    cin: int
    cout: int
    H: int
    W: int
    k: Tuple[int, int, int] = (1, 3, 3)     # KT, KH, KW
    frames: Tuple[int, ...] = (1,)          # 1: a data frame, 0: None (a causal zero frame)
    tout: int = 1
    stride_t: int = 1
    stride_hw: int = 1
    pad: Tuple[int, int, int, int] = (1, 1, 1, 1)  # top, left, bottom, right
    up: bool = False
    split: int = 0
    res: bool = False
    halo: bool = False                      # the default dispatch takes conv3x3_halo_kernel

    def __str__(self):
        return self.name


def _tap(name, cin, cout, H=7, W=20, **kw):
    return Case("tap_" + name, cin, cout, H, W, **kw)


def _halo(name, cin, cout, H=5, W=32, **kw):
    return Case("halo_" + name, cin, cout, H, W, halo=True, **kw)


CASES = (
    # all 12 (BK, NT): BK = 16 / 32 / 64 by Cin, NT = 1 / 2 / 3 / 4 by Cout; M = 140
    [_tap(f"bk{cin}_cout{cout}", cin, cout) for cin in (16, 32, 64) for cout in (18, 40, 96, 160)]
    + [
        _tap("res_cout18", 32, 18, res=True),
        _tap("res_cout96", 32, 96, res=True),
        _tap("stride2_9x20", 32, 96, H=9, W=20, stride_hw=2, pad=(0, 0, 1, 1)),
        _tap("stride2_8x21", 32, 96, H=8, W=21, stride_hw=2, pad=(0, 0, 1, 1)),
        _tap("upsample_5x6", 32, 96, H=5, W=6, up=True),
        _tap("pad_m1_1_m1_1", 32, 96, pad=(-1, 1, -1, 1)),
        _tap("pad_0_1_m1_1", 32, 96, pad=(0, 1, -1, 1)),
        _tap("kt3_zero_frame", 32, 96, k=(3, 3, 3), frames=(0, 1, 1, 1, 1), tout=3),
        _tap("time_stride2", 32, 96, k=(3, 1, 1), frames=(0, 1, 1, 1, 1, 1, 1), tout=3, stride_t=2, pad=(0, 0, 0, 0)),
        _tap("time_split96", 96, 192, k=(3, 1, 1), frames=(0, 1, 1, 1), tout=2, pad=(0, 0, 0, 0), split=96),
        _tap("time_split36", 32, 72, k=(3, 1, 1), frames=(0, 1, 1, 1), tout=2, pad=(0, 0, 0, 0), split=36),
        _tap("1x1_64_288", 64, 288, k=(1, 1, 1), pad=(0, 0, 0, 0)),
        # stage counts nst = KT Cin / 16
        _halo("nst1", 16, 96),
        _halo("nst2_cin32", 32, 96),
        _halo("nst2_kt2", 16, 96, k=(2, 3, 3), frames=(1, 1)),
        _halo("nst3_first_frame", 16, 96, k=(3, 3, 3), frames=(0, 0, 1)),
        # partial 96-channel tiles
        _halo("cout64", 32, 64),
        _halo("cout100", 32, 100),
        _halo("cout160", 32, 160),
        _halo("cout100_res", 32, 100, res=True),
        _halo("cout160_res", 32, 160, res=True),
        # tile geometry
        _halo("ho1", 32, 96, H=1),
        _halo("ho17", 32, 96, H=17),
        _halo("wo64", 32, 96, H=3, W=64),
        _halo("wo96", 32, 96, H=3, W=96),
        _halo("pad_0_1_0_1", 32, 96, H=6, pad=(0, 1, 0, 1)),
        _halo("pad_m1_1_m1_1", 32, 96, H=6, pad=(-1, 1, -1, 1)),
        _halo("pad_m1_1_1_1", 32, 96, H=6, pad=(-1, 1, 1, 1)),
        _halo("upsample_3x16", 32, 96, H=3, W=16, up=True),
        _halo("kt3_stride_t2", 32, 96, k=(3, 3, 3), frames=(1, 1, 1, 1, 1), tout=2, stride_t=2),
        _halo("tout3_wo96", 16, 96, H=3, W=96, k=(3, 3, 3), frames=(0, 1, 1, 1, 1), tout=3),  # 9 workgroups
        _halo("k27x384", 384, 96, H=4, k=(3, 3, 3), frames=(1, 1, 1)),
    ]
)
LARGE_K = 27 * 96  # cases with at least this many taps must show exact bf16 ties


def _out_hw(c: Case):
    Hu, Wu = (2 * c.H, 2 * c.W) if c.up else (c.H, c.W)
    return ((Hu + c.pad[0] + c.pad[2] - c.k[1]) // c.stride_hw + 1,
            (Wu + c.pad[1] + c.pad[3] - c.k[2]) // c.stride_hw + 1)


def _takes_halo(c: Case) -> bool:
    """cp25_conv3d's halo_ok (csrc/vae_ops.hip) under select 0."""
    return (c.k[1] == 3 and c.k[2] == 3 and c.stride_hw == 1 and c.split == 0 and c.pad[1] == 1 and c.pad[3] == 1
            and c.cout >= 64 and c.k[0] <= 3 and _out_hw(c)[1] % 32 == 0)


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).to(BF16)


@functools.lru_cache(maxsize=None)
def _data(c: Case):
    """Inputs and the float64 reference of a case, computed once and shared by the premise and the GPU tests.
    x [n_frames, H, W, Cin] (channels-last frames; frames[i] == 0 rows are zero and passed as None), w
    [Cout, Cin, KT, KH, KW], b [Cout], res / ref in the output layout [Tout (2 Tout), Ho, Wo, Cout (split)]."""
    g = torch.Generator().manual_seed(sum(map(ord, c.name)))
    KT, KH, KW = c.k
    x = _randint(g, -8, 8, (len(c.frames), c.H, c.W, c.cin))
    x = x * torch.tensor(c.frames, dtype=BF16).view(-1, 1, 1, 1)
    w = _randint(g, -4, 4, (c.cout, c.cin, KT, KH, KW))
    b = _randint(g, -8, 8, (c.cout,))

    def conv(xx, ww, dtype):
        clip = xx.to(dtype).permute(3, 0, 1, 2).unsqueeze(0)  # [1, Cin, T, H, W]
        if c.up:
            clip = clip.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)  # nearest 2x
        clip = F.pad(clip, (c.pad[1], c.pad[3], c.pad[0], c.pad[2], 0, 0))  # negative pads crop
        y = F.conv3d(clip, ww.to(dtype), stride=(c.stride_t, c.stride_hw, c.stride_hw))
        return y[0, :, :c.tout]  # [Cout, Tout, Ho, Wo]

    acc = conv(x, w, torch.float64)
    acc32 = conv(x, w, torch.float32)
    absum = conv(x.abs(), w.abs(), torch.float64) + b.double().abs().view(-1, 1, 1, 1)
    pre = acc + b.double().view(-1, 1, 1, 1)  # exact; every |value| < 2^24, so fp64 -> bf16 rounds once
    y = pre.to(BF16)
    if c.split:
        # Resample.forward's interleave (tokenizers/wan2pt1.py:139-141): reshape(b, 2, c, t, h, w), stack the two halves
        # on a new axis after t, reshape(b, c, 2 t, h, w)
        Ho, Wo = y.shape[2:]
        y6 = y.unsqueeze(0).reshape(1, 2, c.split, c.tout, Ho, Wo)
        y = torch.stack((y6[:, 0], y6[:, 1]), 3).reshape(1, c.split, 2 * c.tout, Ho, Wo)[0]
    y = y.permute(1, 2, 3, 0).contiguous()  # [T, Ho, Wo, C]
    res = None
    if c.res:
        res = _randint(g, -64, 64, tuple(y.shape))
        y = (y.double() + res.double()).to(BF16)
    return dict(x=x, w=w, b=b, res=res, ref=y, acc=acc, acc32=acc32, absum=absum, pre=pre)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_premise(case):
    """No kernel: the integer inputs make fp32 accumulation exact, the dispatch is the one the case is named for, and
    the large-K cases round ties."""
    d = _data(case)
    assert d["absum"].max().item() < 2 ** 24
    assert torch.equal(d["acc32"].double(), d["acc"])
    assert d["ref"].shape[1:3] == _out_hw(case)
    assert _takes_halo(case) == case.halo
    assert (case.tout - 1) * case.stride_t + case.k[0] == len(case.frames)
    taps = case.k[0] * case.k[1] * case.k[2] * case.cin
    if taps >= LARGE_K:
        pre = d["pre"]
        ulp = torch.pow(2.0, torch.floor(torch.log2(pre.abs().clamp_min(1.0))) - 7)
        ties = ((pre - pre.to(BF16).double()).abs() * 2 == ulp).double().mean().item()
        inexact = (pre != pre.to(BF16).double()).double().mean().item()
        print(f"{case.name}: {taps} taps, {inexact:.1%} of outputs rounded, {ties:.1%} exact bf16 ties")
        assert ties > 0


def test_premise_has_large_k_cases():
    assert sum(c.k[0] * c.k[1] * c.k[2] * c.cin >= LARGE_K for c in CASES) >= 1
    assert len({c.name for c in CASES}) == len(CASES)


def _run(case: Case, device, conv: _Conv, d, select: int):
    """One launch of cp25_conv3d under conv3d_select(select) into a slice of a sentinel-filled buffer."""
    KT, KH, KW = case.k
    xd = d["x"].to(device)
    frames = [xd[i] if on else None for i, on in enumerate(case.frames)]
    ref = d["ref"]
    res = None if d["res"] is None else d["res"].to(device)
    n = ref.numel()
    buf = torch.full((n + 2 * GUARD,), -1.5e30, dtype=BF16, device=device)
    out = buf[GUARD:GUARD + n].view(ref.shape)
    prev = N.conv3d_select(select)
    try:
        N.conv3d(frames, conv.w, conv.b, out, Hin=case.H, Win=case.W, Cin=conv.cin_p, Cout=case.cout, Tout=case.tout,
                 KT=KT, KH=KH, KW=KW, stride_t=case.stride_t, stride_hw=case.stride_hw, pad=case.pad,
                 upsample=case.up, out_split=case.split, residual=res)
        torch.cuda.synchronize()
    finally:
        N.conv3d_select(prev)
    return buf.cpu()


def _mismatch(out, ref):
    bad = (out != ref).nonzero()
    first = ", ".join(f"{tuple(i.tolist())}: got {out[tuple(i)].item()} want {ref[tuple(i)].item()}" for i in bad[:6])
    return f"{bad.shape[0]} of {ref.numel()} elements differ; (t, h, w, c) {first}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_conv_exact(device, case):
    d = _data(case)
    ref = d["ref"]
    conv = _Conv(d["w"], d["b"], device)
    n = ref.numel()
    for select in ((0, 1, 2) if case.halo else (1,)):
        buf = _run(case, device, conv, d, select)
        sentinel = torch.full((GUARD,), -1.5e30, dtype=BF16)
        assert torch.equal(buf[:GUARD], sentinel), f"{case.name} select {select}: wrote before the output"
        assert torch.equal(buf[GUARD + n:], sentinel), f"{case.name} select {select}: wrote past the output"
        out = buf[GUARD:GUARD + n].view(ref.shape)
        assert torch.equal(out, ref), f"{case.name} select {select}: {_mismatch(out, ref)}"


@pytest.mark.gpu
def test_conv_host_checks(device):
    """Arguments cp25_conv3d refuses before any launch: each is a ValueError."""
    def call(cin=32, cout=96, n_frames=3, tout=1, stride_t=1, kt=3, split=0):
        x = torch.zeros(4, 4, cin, dtype=BF16, device=device)
        w = torch.zeros(cout, kt, 1, 1, cin, dtype=BF16, device=device)
        out = torch.zeros((2 if split else 1) * tout, 4, 4, split or cout, dtype=BF16, device=device)
        prev = N.conv3d_select(0)
        try:
            N.conv3d([x] * n_frames, w, None, out, Hin=4, Win=4, Cin=cin, Cout=cout, Tout=tout, KT=kt, KH=1, KW=1,
                     stride_t=stride_t, out_split=split)
        finally:
            N.conv3d_select(prev)

    call()  # the base arguments are accepted
    call(cout=192, split=96)
    with pytest.raises(ValueError):
        call(cin=24)
    with pytest.raises(ValueError):
        call(n_frames=4, tout=2, stride_t=2)  # (Tout - 1) stride_t + KT = 5 > 4 frames
    with pytest.raises(ValueError):
        call(cout=96, split=96)  # out_split with Cout != 2 out_split
    with pytest.raises(ValueError):
        call(n_frames=25)
