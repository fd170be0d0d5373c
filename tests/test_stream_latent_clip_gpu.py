"""cp25_stream_latent_clip on the device: one frame of the token-major streaming state -> the VAE decoder's un-normalised
channels-last input, bit for bit the torch ops it replaces (written out below: from_patch_layout per session, the stack,
the decode's permute + contiguous, `/ inv_std + mean` on bf16 tensors).

Shapes (Hp, Wp, B): one token; odd, non-square grids with B = 2, 3; 16 x 16 x 16 (several blocks). A trained-range
mean / std table and a random one. One case holds every one of the 65 536 bf16 bit patterns in each of the 16 channels
(4096 tokens, B = 4): NaN results must be NaN in the same places, every other element must have the same bits.
Rejections: a misaligned pointer, B, Hp or Wp = 0 (-22 from the C entry, ValueError from the binding).
"""
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2 import _native as N
from cosmos_predict2 import vae as V
from cosmos_predict2.model import from_patch_layout

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


def _tables(kind, device):
    if kind == "trained":
        mean = torch.tensor(V._MEAN, dtype=BF, device=device)
        std = torch.tensor(V._STD, dtype=BF, device=device)
    else:
        g = torch.Generator().manual_seed(3)
        mean = torch.randn(16, generator=g).to(device, BF)
        std = (0.3 + 2.7 * torch.rand(16, generator=g)).to(device, BF)
    return mean, 1.0 / std  # as WanVAE holds them


def _torch_ops(xs, mean, inv_std, Hp, Wp, B):
    """What the chunk loop does with a frame of StreamingBatchRun.out: latents() and the head of _decode_clip."""
    rows = xs.view(Hp * Wp, B, 64)
    z = torch.stack([from_patch_layout(rows[:, b].reshape(-1, 64), 1, 2 * Hp, 2 * Wp) for b in range(B)], 0)
    zl = z.permute(0, 2, 3, 4, 1).contiguous().flatten(0, 1)  # [B, H, W, 16]
    return zl / inv_std + mean


def _same_bits(out, ref):
    nan = ref.isnan()
    assert torch.equal(out.isnan(), nan)
    assert torch.equal(out.view(torch.int16)[~nan], ref.view(torch.int16)[~nan])


@pytest.mark.parametrize("table", ["trained", "random"])
@pytest.mark.parametrize("Hp,Wp,B", [(1, 1, 1), (4, 6, 3), (3, 5, 2), (16, 16, 16)])
def test_equals_the_torch_ops(device, Hp, Wp, B, table):
    mean, inv_std = _tables(table, device)
    g = torch.Generator().manual_seed(Hp * 100 + Wp * 10 + B)
    xs = (torch.randn(Hp * Wp * B, 64, generator=g) * 1.5).to(device, BF)
    out = N.stream_latent_clip(xs.view(Hp * Wp, B, 64), inv_std, mean, Hp, Wp)
    assert out.dtype == BF and tuple(out.shape) == (B, 2 * Hp, 2 * Wp, 16)
    ref = _torch_ops(xs, mean, inv_std, Hp, Wp, B)
    assert torch.equal(out, ref)
    _same_bits(out, ref)
    # into a given buffer
    buf = torch.full_like(out, 7.0)
    assert N.stream_latent_clip(xs.view(Hp * Wp, B, 64), inv_std, mean, Hp, Wp, out=buf) is buf
    assert torch.equal(buf, ref)


@pytest.mark.parametrize("table", ["trained", "random"])
def test_every_bf16_bit_pattern_in_every_channel(device, table):
    Hp = Wp = 64
    B = 4
    mean, inv_std = _tables(table, device)
    # element (row, p, c) holds pattern ((row * 4 + p) * odd + c * 4099) mod 2^16: a bijection of the 65 536 (row, p)
    # slots onto the patterns, for every channel c
    slot = torch.arange(Hp * Wp * B * 4, dtype=torch.int64).view(-1, 4, 1)
    c = torch.arange(16, dtype=torch.int64).view(1, 1, 16)
    pat = (slot * 40503 + c * 4099) & 0xFFFF
    for ch in (0, 7, 15):
        assert pat[:, :, ch].unique().numel() == 65536
    xs = (pat - ((pat >> 15) << 16)).to(torch.int16).view(Hp * Wp * B, 64).to(device).view(BF)
    assert int(xs.isnan().sum()) == 16 * 2 * 127  # the NaN patterns are in
    out = N.stream_latent_clip(xs.view(Hp * Wp, B, 64), inv_std, mean, Hp, Wp)
    _same_bits(out, _torch_ops(xs, mean, inv_std, Hp, Wp, B))


def test_rejections(device):
    mean, inv_std = _tables("trained", device)
    lib = N.load_library()
    xs = torch.zeros((4 * 6 * 3 + 1, 64), dtype=BF, device=device)
    dst = torch.zeros((3 * 8 * 12 + 1, 16), dtype=BF, device=device)
    tab = torch.zeros(32, dtype=BF, device=device)
    st = N._stream(device)

    def call(x=xs.data_ptr(), i=inv_std.data_ptr(), m=mean.data_ptr(), d=dst.data_ptr(), B=3, Hp=4, Wp=6):
        return lib.cp25_stream_latent_clip(x, i, m, d, B, Hp, Wp, st)

    assert call() == 0
    assert call(x=xs.data_ptr() + 2) == -22 and call(d=dst.data_ptr() + 8) == -22
    assert call(i=tab.data_ptr() + 2) == -22 and call(m=tab.data_ptr() + 4) == -22
    assert call(x=None) == -22 and call(d=None) == -22
    for bad in (dict(B=0), dict(Hp=0), dict(Wp=0), dict(B=-1), dict(Hp=-2)):
        assert call(**bad) == -22
    torch.cuda.synchronize(device)
    rows = xs[:72].view(24, 3, 64)
    with pytest.raises(ValueError):
        N.stream_latent_clip(rows, inv_std, mean, 4, 5)  # 20 tokens announced, 24 given
    with pytest.raises(ValueError):
        N.stream_latent_clip(rows.float(), inv_std, mean, 4, 6)
    with pytest.raises(ValueError):
        N.stream_latent_clip(rows, inv_std[:8], mean, 4, 6)
    with pytest.raises(ValueError):
        N.stream_latent_clip(rows[:, :2], inv_std, mean, 4, 6)  # not contiguous
    with pytest.raises(ValueError):
        N.stream_latent_clip(xs[:0].view(0, 3, 64), inv_std, mean, 0, 6)
