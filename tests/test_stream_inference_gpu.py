"""ActionStreamingInference end to end on the device (tiny action net, synthetic VAE weights, 64 x 96 pixels, 24 actions =
two chunks): 1 + 2 x 12 finite frames, the generator form yields the batch form's frames chunk by chunk, and the host
and device pixel paths agree exactly (tests/test_pixels_gpu.py's requirement for every pipeline)."""
import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2.interactive import MODEL_NAME, ActionStreamingInference
from cosmos_predict2.net_config import tiny_dit
from cosmos_predict2.pipeline import Video2WorldInference

pytestmark = pytest.mark.gpu

CFG = tiny_dit(num_blocks=1, action_dim=7, action_per_latent_frame=4, timestep_scale=1.0, use_wan_fp32_strategy=False)


@pytest.fixture(scope="module")
def inputs():
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, size=(64, 96, 3), dtype=np.uint8)
    acts = (rng.randn(24 + 5, 7) * 0.5).astype(np.float32)  # 29 actions: two whole chunks, the rest dropped
    emb = torch.from_numpy(rng.randn(512, CFG.crossattn_proj_in_channels).astype(np.float32))
    return img, acts, emb


def _infer(device, emb, path):
    return ActionStreamingInference(emb, Video2WorldInference(MODEL_NAME, device=device, net_cfg=CFG, pixel_path=path))


def test_two_chunks_host_device_and_generator(device, inputs, tmp_path):
    img, acts, emb = inputs
    host = _infer(device, emb, "host")
    video = host.generate_action_streaming(img, acts, (64, 96), num_steps=2, seed=5, cache_frame_size=2)
    assert video.dtype == torch.float32 and tuple(video.shape) == (3, 1 + 2 * 12, 64, 96)
    assert torch.isfinite(video).all() and float(video.abs().max()) <= 1.0
    assert torch.equal(video[:, 0], torch.from_numpy(img).permute(2, 0, 1).float() / 128 - 1)
    assert float(video[:, 1:].std()) > 0  # the generated frames are not a constant
    # the generator form: the input frame, then each chunk's 12 frames as it is decoded
    pieces = list(host.stream_action_chunks(img, acts, (64, 96), num_steps=2, seed=5, cache_frame_size=2))
    assert [p.shape[1] for p in pieces] == [1, 12, 12]
    assert torch.equal(torch.cat(pieces, dim=1), video)
    # the second chunk depends on its own seed and on the first chunk's last frame
    other = host.generate_action_streaming(img, acts[:12], (64, 96), num_steps=2, seed=5, cache_frame_size=2)
    assert tuple(other.shape) == (3, 13, 64, 96) and torch.equal(other, video[:, :13])
    assert not torch.equal(video[:, 1:13], video[:, 13:])
    del host
    dev = _infer(device, emb, "device")
    got = dev.generate_action_streaming(img, acts, (64, 96), num_steps=2, seed=5, cache_frame_size=2)
    assert torch.equal(got, video)
    # an image path, resized to the target resolution (exact 2:1), runs the same loop
    from PIL import Image

    big = np.repeat(np.repeat(img, 2, axis=0), 2, axis=1)
    Image.fromarray(big).save(tmp_path / "in.png")
    from_file = dev.generate_action_streaming(str(tmp_path / "in.png"), acts[:12], (64, 96), num_steps=1, seed=5)
    assert tuple(from_file.shape) == (3, 13, 64, 96) and torch.isfinite(from_file).all()


def test_rejections(device, inputs):
    img, acts, emb = inputs
    with pytest.raises(ValueError):
        ActionStreamingInference(emb, Video2WorldInference("2B/robot/action-cond", device=device,
                                                           net_cfg=tiny_dit(num_blocks=1, action_dim=7,
                                                                            action_per_latent_frame=4)))
    inf = _infer(device, emb, "host")
    with pytest.raises(ValueError):
        inf.generate_action_streaming(img, acts[:, :6], (64, 96))
    with pytest.raises(ValueError):
        inf.generate_action_streaming(img[:60], acts, None)  # 60 rows: not a multiple of 16
