"""WanVAE.decode_stream on the device: the decoder fed one latent frame per push over a feature cache it keeps between
calls gives decode's frames bit for bit.

Synthetic weights, latent [B, 16, 5, 8, 12] (64 x 96 pixels, 17 frames), B = 1 and 3 distinct clips. The pushes of
frames 0 .. 4 (t = 1, then 4 each) concatenated along t are torch.equal to decode(z); the push_u8 results to decode_u8(z)
in both layouts; the un-normalised channels-last input form gives the same; a decode of another latent, an encode and a
second, interleaved stream on the same WanVAE between pushes change nothing; under a context-parallel group
decode_stream raises. decode(z) is computed once per module.
"""
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2.vae import DecodeStream, Wan2pt1VAEInterface, init_vae_state_dict

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
H, W, T = 64, 96, 5


@pytest.fixture(scope="module")
def vae(device):
    tok = Wan2pt1VAEInterface(init_vae_state_dict(seed=3), device=device)
    g = torch.Generator().manual_seed(21)
    z = torch.randn(3, 16, T, H // 8, W // 8, generator=g).to(BF16).to(device)
    other = torch.randn(2, 16, 2, H // 8, W // 8, generator=g).to(BF16).to(device)
    video = (torch.rand(2, 3, 5, H, W, generator=g) * 2 - 1).to(BF16).to(device)
    d = dict(tok=tok, z=z, other=other, video=video, dec={})

    def decode(B):
        if B not in d["dec"]:
            d["dec"][B] = tok.decode(z[:B])
        return d["dec"][B]

    d["decode"] = decode
    return d


def _frames(z):
    return [z[:, :, i: i + 1] for i in range(z.shape[2])]


@pytest.mark.parametrize("B", [1, 3])
def test_pushes_concatenate_to_decode(vae, B):
    tok, z, want = vae["tok"], vae["z"][:B], vae["decode"](B)
    assert tuple(want.shape) == (B, 3, 1 + 4 * (T - 1), H, W)
    s = tok.decode_stream(B)
    assert isinstance(s, DecodeStream) and s.n_clips == B
    parts = [s.push_video(f) for f in _frames(z)]
    assert [p.shape[2] for p in parts] == [1] + [4] * (T - 1)
    assert all(p.dtype == BF16 and p.is_contiguous() for p in parts)
    assert torch.equal(torch.cat(parts, 2), want)
    assert s.frames == T
    # push itself: channels-last, clip-major
    s = tok.model.decode_stream(B)
    raw = [s.push(f) for f in _frames(z)]
    assert tuple(raw[0].shape) == (B, H, W, 3) and tuple(raw[1].shape) == (B * 4, H, W, 3)
    got = torch.cat([r.unflatten(0, (B, -1)) for r in raw], 1).permute(0, 4, 1, 2, 3)
    assert torch.equal(got, want)
    if B > 1:
        assert not torch.equal(want[0], want[1])


@pytest.mark.parametrize("B", [1, 3])
def test_unnormalised_channels_last_input(vae, B):
    """The [B, h, w, 16] form: what cp25_stream_latent_clip writes, here made by decode's own torch ops."""
    tok, z, want = vae["tok"], vae["z"][:B], vae["decode"](B)
    m = tok.model
    s = tok.decode_stream(B)
    parts = []
    for f in _frames(z):
        zl = f.permute(0, 2, 3, 4, 1).contiguous().flatten(0, 1) / m.inv_std + m.mean
        parts.append(s.push_video(zl))
    assert torch.equal(torch.cat(parts, 2), want)


@pytest.mark.parametrize("B", [1, 3])
def test_push_u8_equals_decode_u8(vae, B):
    tok, z = vae["tok"], vae["z"][:B]
    for layout, dim in (("THWC", 0 if B == 1 else 1), ("NCTHW", 2)):
        want = tok.decode_u8(z, layout)
        s = tok.decode_stream(B)
        parts = [s.push_u8(f, layout) for f in _frames(z)]
        assert all(p.dtype == torch.uint8 for p in parts)
        assert torch.equal(torch.cat(parts, dim), want), layout
    with pytest.raises(ValueError):
        tok.decode_stream(B).push_u8(z[:, :, :1], "HWC")


@pytest.mark.parametrize("B", [1, 3])
def test_other_calls_between_pushes(vae, B):
    """decode of another latent (another clip count), an encode and a second stream, interleaved with the pushes."""
    tok, z, want = vae["tok"], vae["z"][:B], vae["decode"](B)
    a, b = tok.decode_stream(B), tok.decode_stream(B)
    pa, pb = [], []
    zb = z.flip(0) if B > 1 else z * 0.5
    for i, f in enumerate(_frames(z)):
        pa.append(a.push_video(f))
        if i == 1:
            tok.decode(vae["other"])
        if i == 2:
            tok.encode(vae["video"])
        if i >= 1:  # the second stream runs one frame behind
            pb.append(b.push_video(zb[:, :, i - 1: i]))
    pb.append(b.push_video(zb[:, :, T - 1:]))
    assert torch.equal(torch.cat(pa, 2), want)
    want_b = want.flip(0) if B > 1 else tok.decode(zb)
    assert torch.equal(torch.cat(pb, 2), want_b)
    assert tok.model._nb == 1


def test_rejections(vae):
    tok, z = vae["tok"], vae["z"]
    s = tok.decode_stream(3)
    for bad in (z[:2, :, :1], z[:, :, :2], z[:, :8, :1], z[:, :, 0], z[:, :, 0].permute(0, 2, 3, 1).float()):
        with pytest.raises(ValueError):
            s.push(bad)
    s.push(z[:, :, :1])
    with pytest.raises(ValueError):
        s.push(z[:, :, :1, :4])  # another latent size in the same stream
    with pytest.raises(ValueError):
        tok.decode_stream(0)
    tok.set_context_parallel_group(object())
    try:
        with pytest.raises(ValueError):
            tok.decode_stream(1)
        with pytest.raises(ValueError):
            tok.model.decode_stream(1)
        with pytest.raises(ValueError):
            s.push(z[:, :, 1:2])  # a group set after the stream was opened
    finally:
        tok.set_context_parallel_group(None)
    assert s.frames == 1
