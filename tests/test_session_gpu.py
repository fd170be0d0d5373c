"""Closed-loop sessions (ActionStreamingInference.open_session) end to end on the device, against the open-loop entry
points fed the same actions, bit for bit.

Tiny action net, synthetic VAE weights, 64 x 96 pixels, num_steps = 2, cache_frame_size = 2, B = 3 sessions with distinct
frames, actions and seeds (the shapes of tests/test_stream_batch_inference_gpu.py). 6 steps after first_frames are
generate_action_streaming_batch of the same 24 actions; 5 steps are its first 1 + 20 frames (a frame does not depend on
later actions); output="u8" is decode_u8 of each chunk's latents from frame 1 on; the host and device pixel paths agree;
stream_gemm="small" equals the default; B = 1 equals the batch entry point of one session; replace() restarts one session
at a chunk start and leaves the others alone, and raises elsewhere; a wrong action shape raises. The open-loop videos
are made once per module.
"""
import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2.interactive import MODEL_NAME, ActionSession, ActionStreamingInference, chunk_seeds
from cosmos_predict2.model import StreamingBatchRun
from cosmos_predict2.net_config import tiny_dit
from cosmos_predict2.pipeline import Video2WorldInference

pytestmark = pytest.mark.gpu

CFG = tiny_dit(num_blocks=1, action_dim=7, action_per_latent_frame=4, timestep_scale=1.0, use_wan_fp32_strategy=False)
B = 3
SEEDS = [5, 9, 2]
RES = (64, 96)
KW = dict(num_steps=2, cache_frame_size=2)


def _infer(device, emb, path, stream_gemm=None):
    return ActionStreamingInference(emb, Video2WorldInference(MODEL_NAME, device=device, net_cfg=CFG, pixel_path=path),
                                    stream_gemm=stream_gemm)


@pytest.fixture(scope="module")
def world(device):
    rng = np.random.RandomState(8)
    imgs = [rng.randint(0, 256, size=(64, 96, 3), dtype=np.uint8) for _ in range(B + 1)]
    acts = (rng.randn(B, 24, 7) * 0.5).astype(np.float32)
    emb = torch.from_numpy(rng.randn(512, CFG.crossattn_proj_in_channels).astype(np.float32))
    dev = _infer(device, emb, "device")
    video = dev.generate_action_streaming_batch(imgs[:B], acts, RES, seed=SEEDS, **KW)  # [B, 3, 25, 64, 96]
    return dict(imgs=imgs, acts=acts, emb=emb, dev=dev, video=video)


def _steps(sess, acts, n, first=0):
    return [sess.step(acts[:, 4 * k: 4 * k + 4]) for k in range(first, first + n)]


def test_six_steps_equal_the_open_loop_video(device, world):
    sess = world["dev"].open_session(world["imgs"][:B], RES, seed=SEEDS, **KW)
    assert isinstance(sess, ActionSession) and sess.at_chunk_start and sess.steps_done == 0
    ff = sess.first_frames
    assert ff.dtype == torch.float32 and tuple(ff.shape) == (B, 3, 1, 64, 96) and not ff.is_cuda
    out = []
    for k in range(6):
        assert sess.at_chunk_start == (k % 3 == 0) and sess.steps_done == k
        a = world["acts"][:, 4 * k: 4 * k + 4]
        out.append(sess.step(torch.from_numpy(a) if k % 2 else a))  # numpy or tensor
    assert all(o.dtype == torch.float32 and tuple(o.shape) == (B, 3, 4, 64, 96) and not o.is_cuda for o in out)
    got = torch.cat([ff] + out, dim=2)
    video = world["video"]
    assert torch.isfinite(got).all() and float(got.abs().max()) <= 1.0 and float(got[:, :, 1:].std()) > 0
    assert not torch.equal(video[0], video[1])
    assert torch.equal(got, video)
    assert sess.at_chunk_start and sess.steps_done == 6


def test_five_steps_equal_the_first_21_frames(device, world):
    """A frame does not depend on later actions: stop inside the second chunk."""
    sess = world["dev"].open_session(world["imgs"][:B], RES, seed=SEEDS, **KW)
    got = torch.cat([sess.first_frames] + _steps(sess, world["acts"], 5), dim=2)
    assert torch.equal(got, world["video"][:, :, :21])
    assert not sess.at_chunk_start and sess.steps_done == 5


def test_u8_output_equals_decode_u8_of_the_chunk(device, world):
    dev, acts = world["dev"], world["acts"]
    sess = dev.open_session(world["imgs"][:B], RES, seed=SEEDS, output="u8", **KW)
    out = _steps(sess, acts, 3)
    assert all(o.dtype == torch.uint8 and o.is_cuda and tuple(o.shape) == (B, 4, 64, 96, 3) for o in out)
    # the first chunk's latents, as the chunk loop makes them
    model = dev.pipe.model
    frame = torch.stack([dev._first_frame(f, RES) for f in world["imgs"][:B]], 0).to(device)
    gt = model.encode_conditioning(frame[:, :, None], 1, 4)
    a = torch.from_numpy(acts[:, :12]).float().to(device, torch.bfloat16)
    run = StreamingBatchRun(model, gt, dev._ctx_batch, a, seed=chunk_seeds(SEEDS, B, 0), n_steps=2, cache_frame_size=2)
    while not run.done:
        run.next_frame()
    want = model.tokenizer.decode_u8(run.latents())  # [B, 13, H, W, 3]
    assert torch.equal(torch.cat(out, dim=1), want[:, 1:])
    assert not torch.equal(want[0], want[1])


def test_host_and_device_pixel_paths_agree(device, world):
    host = _infer(device, world["emb"], "host")
    sess = host.open_session(world["imgs"][:B], RES, seed=SEEDS, **KW)
    got = torch.cat([sess.first_frames] + _steps(sess, world["acts"], 4), dim=2)
    assert torch.equal(got, world["video"][:, :, :17])
    u8 = host.open_session(world["imgs"][:B], RES, seed=SEEDS, output="u8", **KW)
    d8 = world["dev"].open_session(world["imgs"][:B], RES, seed=SEEDS, output="u8", **KW)
    for k in range(4):
        a = world["acts"][:, 4 * k: 4 * k + 4]
        assert torch.equal(u8.step(a), d8.step(a))


def test_small_stream_gemm_equals_the_default(device, world):
    small = _infer(device, world["emb"], "device", stream_gemm="small")
    sess = small.open_session(world["imgs"][:B], RES, seed=SEEDS, **KW)
    got = torch.cat([sess.first_frames] + _steps(sess, world["acts"], 4), dim=2)
    assert torch.equal(got, world["video"][:, :, :17])


def test_one_session(device, world):
    dev, img, acts = world["dev"], world["imgs"][1:2], world["acts"][1:2]
    want = dev.generate_action_streaming_batch(img, acts, RES, seed=SEEDS[1], **KW)
    sess = dev.open_session(img, RES, seed=SEEDS[1], **KW)
    got = torch.cat([sess.first_frames] + _steps(sess, acts, 6), dim=2)
    assert tuple(got.shape) == (1, 3, 25, 64, 96) and torch.equal(got, want)
    u8 = dev.open_session(img, RES, seed=SEEDS[1], output="u8", **KW).step(acts[:, :4])
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1, 4, 64, 96, 3)


def test_replace_restarts_one_session(device, world):
    dev, imgs, acts = world["dev"], world["imgs"], world["acts"]
    new_frame, s = imgs[B], 31
    sess = dev.open_session(imgs[:B], RES, seed=SEEDS, **KW)
    _steps(sess, acts, 1)
    with pytest.raises(RuntimeError):
        sess.replace(1, new_frame, seed=s)  # inside a chunk
    _steps(sess, acts, 2, first=1)
    assert sess.at_chunk_start
    with pytest.raises(ValueError):
        sess.replace(B, new_frame)
    with pytest.raises(ValueError):
        sess.replace(1, new_frame[:, :, :2])
    sess.replace(1, new_frame, seed=s)
    later = torch.cat(_steps(sess, acts, 3, first=3), dim=2)  # [B, 3, 12, H, W]
    # session 1: chunk 0 of (new_frame, s) under actions 12 .. 23
    fresh = dev.generate_action_streaming_batch([imgs[0], new_frame, imgs[2]], acts[:, 12:], RES,
                                                seed=[SEEDS[0], s, SEEDS[2]], **KW)
    assert torch.equal(later[1], fresh[1, :, 1:])
    # sessions 0 and 2: the uninterrupted run
    video = world["video"]
    assert torch.equal(later[0], video[0, :, 13:]) and torch.equal(later[2], video[2, :, 13:])
    assert not torch.equal(later[1], video[1, :, 13:])
    # a replace without a seed keeps the session's seed and restarts its chunk count
    sess.replace(0, imgs[0])
    again = sess.step(acts[:, :4])
    assert torch.equal(again[0], video[0, :, 1:5])


def test_rejections(device, world):
    dev, imgs, acts = world["dev"], world["imgs"], world["acts"]
    sess = dev.open_session(imgs[:B], RES, seed=SEEDS, **KW)
    for bad in (acts[:, :3], acts[:, :8], acts[:2, :4], acts[:, :4, :6], acts[0, :4], None):
        with pytest.raises(ValueError):
            sess.step(bad)
    assert sess.steps_done == 0 and sess.at_chunk_start
    with pytest.raises(ValueError):
        dev.open_session(imgs[:B], RES, seed=[1, 2], **KW)
    with pytest.raises(ValueError):
        dev.open_session([imgs[0], imgs[1][:48]], None, **KW)
    with pytest.raises(ValueError):
        dev.open_session(imgs[:B], RES, output="uint8", **KW)
    with pytest.raises(ValueError):
        dev.open_session([], RES, **KW)
    with pytest.raises(ValueError):
        dev.open_session([imgs[0]] * 17, RES, **KW)
