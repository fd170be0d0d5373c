"""The batch entry points of ActionStreamingInference end to end on the device: tiny action net, synthetic VAE weights,
64 x 96 pixels, 24 actions (two chunks), B = 3 sessions with distinct frames, actions and seeds.

generate_action_streaming_batch has the stated shape, is finite and within [-1, 1]; session b equals
generate_action_streaming of that session's inputs (attention key split pinned to 1, as in
tests/test_stream_batch_gpu.py); the generator's pieces concatenate to it; the host and device pixel paths agree
exactly; an int seed gives every session the one-session result of that seed; every stream_gemm mode runs.
"""
import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2 import _native as N
from cosmos_predict2.interactive import MODEL_NAME, ActionStreamingInference
from cosmos_predict2.net_config import tiny_dit
from cosmos_predict2.pipeline import Video2WorldInference

pytestmark = pytest.mark.gpu

CFG = tiny_dit(num_blocks=1, action_dim=7, action_per_latent_frame=4, timestep_scale=1.0, use_wan_fp32_strategy=False)
B = 3
SEEDS = [5, 9, 2]
KW = dict(num_steps=2, cache_frame_size=2)


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.RandomState(8)
    imgs = [rng.randint(0, 256, size=(64, 96, 3), dtype=np.uint8) for _ in range(B)]
    acts = (rng.randn(B, 24, 7) * 0.5).astype(np.float32)
    emb = torch.from_numpy(rng.randn(512, CFG.crossattn_proj_in_channels).astype(np.float32))
    return imgs, acts, emb


@pytest.fixture
def no_attn_split():
    prev = N.set_attn_split(1)
    yield
    N.set_attn_split(prev)


def _infer(device, emb, path, stream_gemm=None):
    return ActionStreamingInference(emb, Video2WorldInference(MODEL_NAME, device=device, net_cfg=CFG, pixel_path=path),
                                    stream_gemm=stream_gemm)


def test_batch_equals_the_sessions_alone(device, inputs, no_attn_split):
    imgs, acts, emb = inputs
    host = _infer(device, emb, "host")
    video = host.generate_action_streaming_batch(imgs, acts, (64, 96), seed=SEEDS, **KW)
    assert video.dtype == torch.float32 and tuple(video.shape) == (B, 3, 1 + 2 * 12, 64, 96)
    assert torch.isfinite(video).all() and float(video.abs().max()) <= 1.0
    assert float(video[:, :, 1:].std()) > 0
    singles = [host.generate_action_streaming(imgs[b], acts[b], (64, 96), seed=SEEDS[b], **KW) for b in range(B)]
    assert not torch.equal(singles[0][:, 1:], singles[1][:, 1:])
    for b in range(B):
        assert torch.equal(video[b], singles[b]), f"session {b} differs from generate_action_streaming of its inputs"
    # the generator: the input frames, then each chunk's 12 frames
    pieces = list(host.stream_action_chunks_batch(imgs, acts, (64, 96), seed=SEEDS, **KW))
    assert [tuple(p.shape) for p in pieces] == [(B, 3, 1, 64, 96), (B, 3, 12, 64, 96), (B, 3, 12, 64, 96)]
    assert torch.equal(torch.cat(pieces, dim=2), video)
    # an int seed: every session the one-session result of that seed
    same = host.generate_action_streaming_batch([imgs[1]] * 2, np.stack([acts[1]] * 2), (64, 96), seed=SEEDS[1], **KW)
    assert torch.equal(same[0], singles[1]) and torch.equal(same[1], singles[1])
    del host
    # the device pixel path agrees exactly
    dev = _infer(device, emb, "device")
    assert torch.equal(dev.generate_action_streaming_batch(imgs, acts, (64, 96), seed=SEEDS, **KW), video)


@pytest.mark.parametrize("mode", ["small", "small_splitk"])
def test_stream_gemm_modes(device, inputs, no_attn_split, mode):
    imgs, acts, emb = inputs
    inf = _infer(device, emb, "device", stream_gemm=mode)
    video = inf.generate_action_streaming_batch(imgs, acts[:, :12], (64, 96), seed=SEEDS, **KW)
    assert tuple(video.shape) == (B, 3, 13, 64, 96)
    assert torch.isfinite(video).all() and float(video.abs().max()) <= 1.0
    if mode == "small":  # the small-M family's exact form: the bits of "tile256"
        base = _infer(device, emb, "device").generate_action_streaming_batch(imgs, acts[:, :12], (64, 96), seed=SEEDS,
                                                                             **KW)
        assert torch.equal(video, base)


def test_rejections(device, inputs):
    imgs, acts, emb = inputs
    inf = _infer(device, emb, "host")
    with pytest.raises(ValueError):
        inf.generate_action_streaming_batch([imgs[0], imgs[1][:48]], acts[:2], None)  # unequal sizes
    with pytest.raises(ValueError):
        inf.generate_action_streaming_batch(imgs, acts[:2], (64, 96))  # 2 action sequences for 3 frames
    with pytest.raises(ValueError):
        inf.generate_action_streaming_batch(imgs, acts[0], (64, 96))
    with pytest.raises(ValueError):
        inf.generate_action_streaming_batch(imgs, acts, (64, 96), seed=[1, 2])
