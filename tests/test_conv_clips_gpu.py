"""cp25_conv3d_clips (several independent clips in one launch) against one cp25_conv3d call per clip, bit for bit.

Every layer kind the VAE runs at dim = 96, n_clips 2 and 3, 1 and 2 output frames per clip, at 8 x 12 pixels, at
20 x 36 (720 pixels: a partial 128-pixel tile, several workgroups) and, for the 3x3x3 convs, at 16 x 32, the smallest
width the halo kernel takes, under every cp25_conv3d_select mode. The clips start differently: clip 0's history is
zero (NULL) frames, clip 1's is real frames, clip 2's is one of each, so a window that read a neighbour's run, or a
NULL entry taken from the wrong clip, changes the result. The output is a slice of a sentinel-filled buffer.
"""
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2 import _native as N
from cosmos_predict2.vae import _Conv

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
GUARD = 4096
SENTINEL = -1.5e30

# name: (cin, cout, (KT, KH, KW), dict of conv options, residual)
KINDS = {
    "causal_16_96": (16, 96, (3, 3, 3), dict(pad=(1, 1, 1, 1)), False),
    "causal_96_96": (96, 96, (3, 3, 3), dict(pad=(1, 1, 1, 1)), False),
    "causal_96_96_res": (96, 96, (3, 3, 3), dict(pad=(1, 1, 1, 1)), True),
    "to_qkv_1x1": (384, 1152, (1, 1, 1), dict(), False),
    "time_conv_out_split": (192, 384, (3, 1, 1), dict(out_split=192), False),
    "time_conv_stride_t2": (192, 192, (3, 1, 1), dict(stride_t=2), False),
    "upsample_3x3": (192, 96, (1, 3, 3), dict(pad=(1, 1, 1, 1), upsample=True), False),
    "down_stride_hw2": (96, 96, (1, 3, 3), dict(stride_hw=2, pad=(0, 0, 1, 1)), False),
}
SIZES = [(8, 12), (20, 36)]
CASES = [(k, hw) for k in KINDS for hw in SIZES] + [(k, (16, 32)) for k in KINDS if k.startswith("causal")]


def _weights(kind, device):
    cin, cout, k, _, _ = KINDS[kind]
    g = torch.Generator().manual_seed(sorted(KINDS).index(kind))
    fan = cin * k[0] * k[1] * k[2]
    w = (torch.randn((cout, cin) + k, generator=g) / fan ** 0.5).to(BF16)
    b = (0.1 * torch.randn(cout, generator=g)).to(BF16)
    return _Conv(w, b, device)


def _out_shape(kind, H, W, tout):
    _, cout, k, o, _ = KINDS[kind]
    pad, s = o.get("pad", (0, 0, 0, 0)), o.get("stride_hw", 1)
    Hu, Wu = (2 * H, 2 * W) if o.get("upsample") else (H, W)
    Ho, Wo = (Hu + pad[0] + pad[2] - k[1]) // s + 1, (Wu + pad[1] + pad[3] - k[2]) // s + 1
    split = o.get("out_split", 0)
    return (2 * tout, Ho, Wo, split) if split else (tout, Ho, Wo, cout)


def _tables(kind, H, W, n_clips, Tc, device, g):
    """Per clip the Fc table entries: its history (KT - 1 entries: all NULL for clip 0, all real for clip 1, NULL then
    real for clip 2) and then its own frames."""
    cin, _, k, o, _ = KINDS[kind]
    Fc = (Tc - 1) * o.get("stride_t", 1) + k[0]
    tabs = []
    for c in range(n_clips):
        x = torch.randn((Fc, H, W, cin), generator=g).to(BF16).to(device)
        n_null = min(k[0] - 1, (2 - c) % 3)
        tabs.append([None if i < n_null else x[i] for i in range(Fc)])
    return Fc, tabs


@pytest.mark.parametrize("kind,hw", CASES, ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_clips_equal_one_call_per_clip(device, kind, hw):
    cin, cout, k, o, with_res = KINDS[kind]
    H, W = hw
    conv = _weights(kind, device)
    kw = dict(Hin=H, Win=W, Cin=conv.cin_p, Cout=cout, KT=k[0], KH=k[1], KW=k[2], **o)
    g = torch.Generator().manual_seed(H * W)
    halo = k == (3, 3, 3) and W % 32 == 0
    for n_clips in (2, 3):
        for Tc in (1, 2):
            Fc, tabs = _tables(kind, H, W, n_clips, Tc, device, g)
            shape = _out_shape(kind, H, W, n_clips * Tc)
            per_clip = shape[0] // n_clips
            res = torch.randn(shape, generator=g).to(BF16).to(device) if with_res else None
            for select in ((0, 1, 2) if halo else (0, 1)):
                n = torch.Size(shape).numel()
                buf = torch.full((n + 2 * GUARD,), SENTINEL, dtype=BF16, device=device)
                out = buf[GUARD:GUARD + n].view(shape)
                want = torch.empty(shape, dtype=BF16, device=device)
                prev = N.conv3d_select(select)
                try:
                    N.conv3d_clips([f for t in tabs for f in t], n_clips, conv.w, conv.b, out, Tout=n_clips * Tc,
                                   residual=res, **kw)
                    for c in range(n_clips):
                        sl = slice(c * per_clip, (c + 1) * per_clip)
                        N.conv3d(tabs[c], conv.w, conv.b, want[sl], Tout=Tc,
                                 residual=None if res is None else res[sl], **kw)
                finally:
                    N.conv3d_select(prev)
                tag = f"{kind} {H}x{W} n_clips {n_clips} Tc {Tc} select {select}"
                sent = torch.tensor(SENTINEL, dtype=BF16, device=device)
                assert (buf[:GUARD] == sent).all() and (buf[GUARD + n:] == sent).all(), f"{tag}: guard written"
                assert torch.isfinite(want.float()).all() and want.any(), tag
                bad = (out != want).flatten(1).any(1).nonzero().flatten().tolist()
                assert torch.equal(out, want), f"{tag}: output frames {bad} differ"


def test_one_clip_is_conv3d(device):
    """n_clips = 1 of the clips entry is cp25_conv3d: same bits, surplus table entries allowed."""
    kind, (H, W) = "causal_96_96", (16, 32)
    cin, cout, k, o, _ = KINDS[kind]
    conv = _weights(kind, device)
    g = torch.Generator().manual_seed(1)
    x = torch.randn((5, H, W, cin), generator=g).to(BF16).to(device)
    tab = [None, x[0], x[1], x[2], x[3], x[4]]  # 6 entries, Tout = 3 reads 5
    kw = dict(Hin=H, Win=W, Cin=conv.cin_p, Cout=cout, Tout=3, KT=3, KH=3, KW=3, **o)
    a = N.conv3d(tab, conv.w, conv.b, torch.empty((3, H, W, cout), dtype=BF16, device=device), **kw)
    b = N.conv3d_clips(tab, 1, conv.w, conv.b, torch.empty((3, H, W, cout), dtype=BF16, device=device), **kw)
    assert torch.equal(a, b) and a.any()


def test_rejections_write_nothing(device):
    """n_clips < 1, Tout % n_clips != 0, n_clips * Fc > 24 and n_clips * Fc != n_frames: -22 before any launch."""
    H, W, cin, cout = 4, 4, 32, 96
    x = torch.ones(H, W, cin, dtype=BF16, device=device)
    w = torch.ones(cout, 3, 1, 1, cin, dtype=BF16, device=device)

    def call(n_frames, n_clips, tout, stride_t=1):
        out = torch.full((tout, H, W, cout), SENTINEL, dtype=BF16, device=device)
        with pytest.raises(ValueError, match="-22"):
            N.conv3d_clips([x] * n_frames, n_clips, w, None, out, Hin=H, Win=W, Cin=cin, Cout=cout, Tout=tout, KT=3,
                           KH=1, KW=1, stride_t=stride_t)
        torch.cuda.synchronize()
        assert (out == torch.tensor(SENTINEL, dtype=BF16, device=device)).all()

    call(3, 0, 1)
    call(3, -1, 1)
    call(10, 2, 3)        # Tout % n_clips
    call(24, 3, 21)       # Fc = 9: 27 entries > 24
    call(24, 4, 8, 2)     # stride_t 2: Fc = 5 ... 20 entries != 24
    call(7, 2, 2)         # Fc = 3: 6 entries != 7
    call(5, 2, 2)         # ... != 5
    # the accepted neighbours of those
    out = torch.empty((2, H, W, cout), dtype=BF16, device=device)
    N.conv3d_clips([x] * 6, 2, w, None, out, Hin=H, Win=W, Cin=cin, Cout=cout, Tout=2, KT=3, KH=1, KW=1)
    assert torch.equal(out, torch.full_like(out, 96.0))


def test_conv_wrapper_splits_and_trims(device):
    """vae._Conv over clips: launches of at most 24 entries, a clip whose run alone overflows the table (30 frames of a
    1x1 conv) on the one-clip path, and runs longer than the frames read (a stride-2 time conv over an even count)
    trimmed to Fc, each against one call per clip."""
    g = torch.Generator().manual_seed(7)
    H, W = 8, 12
    for kind, n_clips, Tc, L in (("causal_96_96", 8, 2, 4), ("to_qkv_1x1", 2, 30, 30), ("time_conv_stride_t2", 3, 1, 4)):
        cin, cout, k, o, _ = KINDS[kind]
        conv = _weights(kind, device)
        x = torch.randn((n_clips, L, H, W, cin), generator=g).to(BF16).to(device)
        tab = [x[c, i] for c in range(n_clips) for i in range(L)]
        got = conv(tab, n_clips * Tc, H, W, n_clips=n_clips, **o)
        for c in range(n_clips):
            want = conv([x[c, i] for i in range(L)], Tc, H, W, **o)
            assert torch.equal(got[c * Tc:(c + 1) * Tc], want) and want.any(), (kind, c)
