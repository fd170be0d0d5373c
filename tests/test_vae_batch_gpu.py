"""The VAE on B clips in lock-step against the stack of its own B = 1 calls, bit for bit.

Synthetic weights, 64 x 96 pixels (an 8 x 12 latent), B = 2 and 3 clips that differ from each other: decode of T = 4
latent frames, encode of 1 frame and of 13 frames, encode_u8 and decode_u8, through WanVAE and through the
Wan2pt1VAEInterface wrappers. One case has more clips than one frame table holds (B = 8 at two frames per clip: the 3x3x3
convs' runs of 4 entries fit 6 clips per launch), so the clips split over two launches. The B = 1 results are made once
per module and shared.
"""
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2.vae import Wan2pt1VAEInterface, clip_table_layout, init_vae_state_dict

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
H, W = 64, 96
BMAX = 8


@pytest.fixture(scope="module")
def vae(device):
    """The tokenizer, BMAX distinct inputs of every kind and each one's B = 1 result."""
    tok = Wan2pt1VAEInterface(init_vae_state_dict(seed=3), device=device)
    g = torch.Generator().manual_seed(11)
    d = dict(tok=tok, refs={})
    d["z4"] = torch.randn(BMAX, 16, 4, H // 8, W // 8, generator=g).to(BF16).to(device)
    d["z2"] = torch.randn(BMAX, 16, 2, H // 8, W // 8, generator=g).to(BF16).to(device)
    d["v1"] = (torch.rand(BMAX, 3, 1, H, W, generator=g) * 2 - 1).to(BF16).to(device)
    d["v13"] = (torch.rand(3, 3, 13, H, W, generator=g) * 2 - 1).to(BF16).to(device)
    d["v5"] = (torch.rand(BMAX, 3, 5, H, W, generator=g) * 2 - 1).to(BF16).to(device)
    d["u1"] = torch.randint(0, 256, (3, 3, 1, H, W), generator=g, dtype=torch.uint8).to(device)
    d["u13"] = torch.randint(0, 256, (3, 3, 13, H, W), generator=g, dtype=torch.uint8).to(device)

    def ref(fn, key, b):
        if (fn, key, b) not in d["refs"]:
            d["refs"][(fn, key, b)] = getattr(tok, fn)(d[key][b: b + 1])
        return d["refs"][(fn, key, b)]

    d["ref"] = ref
    return d


def _check(vae, fn, key, B, **kw):
    tok = vae["tok"]
    got = getattr(tok, fn)(vae[key][:B], **kw)
    want = [vae["ref"](fn, key, b) for b in range(B)]
    assert got.shape[0] == B and tuple(got.shape[1:]) == tuple(want[0].shape[1:]), (got.shape, want[0].shape)
    assert got.dtype == want[0].dtype
    assert not torch.equal(want[0], want[1])  # the clips differ
    for b in range(B):
        assert torch.equal(got[b: b + 1], want[b]), f"{fn}({key}) B = {B}: clip {b} differs from its B = 1 call"
    assert torch.isfinite(got.float()).all()
    return got


@pytest.mark.parametrize("B", [2, 3])
def test_decode_batch(vae, B):
    got = _check(vae, "decode", "z4", B)
    assert tuple(got.shape) == (B, 3, 13, H, W)


@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("key", ["v1", "v13"])
def test_encode_batch(vae, B, key):
    got = _check(vae, "encode", key, B)
    assert tuple(got.shape) == (B, 16, 1 if key == "v1" else 4, H // 8, W // 8)


@pytest.mark.parametrize("B", [2, 3])
def test_encode_u8_batch(vae, B):
    _check(vae, "encode_u8", "u1", B)
    _check(vae, "encode_u8", "u13", B)
    # a strided (non-contiguous) batch, as a frame slice of a longer video is
    tok = vae["tok"]
    got = tok.encode_u8(vae["u13"][:B, :, :1])
    for b in range(B):
        assert torch.equal(got[b: b + 1], tok.encode_u8(vae["u13"][b: b + 1, :, :1]))


@pytest.mark.parametrize("B", [2, 3])
def test_decode_u8_batch(vae, B):
    tok = vae["tok"]
    z = vae["z2"][:B]
    thwc = tok.decode_u8(z)
    ncthw = tok.decode_u8(z, "NCTHW")
    assert thwc.dtype == torch.uint8 and tuple(thwc.shape) == (B, 5, H, W, 3)
    assert tuple(ncthw.shape) == (B, 3, 5, H, W)
    for b in range(B):
        assert torch.equal(thwc[b], tok.decode_u8(z[b: b + 1]))
        assert torch.equal(ncthw[b: b + 1], tok.decode_u8(z[b: b + 1], "NCTHW"))
    assert torch.equal(thwc.permute(0, 4, 1, 2, 3), ncthw)


def test_more_clips_than_one_table(vae):
    """B = 8: the decoder's time convs see one frame per clip, the encoder's second chunk (5-frame clips: 1 + 4) four
    per clip, the decoder's later frames two after the upsample3d interleave: tables of 8 x 3, 8 x 6 and 8 x 4 entries
    against the 24 one launch holds."""
    Fc, launches = clip_table_layout(2, 1, 3, BMAX)
    assert BMAX * Fc > 24 and len(launches) == 2
    _check(vae, "decode", "z2", BMAX)
    _check(vae, "encode", "v5", BMAX)
