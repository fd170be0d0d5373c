"""Actions supplied per frame: a StreamingBatchRun / StreamingRun built with actions=None and stepped with
next_frame(action) against the run built with the whole action array, on the device.

Tiny action net (one block), T = 4 latent frames on the 4 x 6 patch grid, num_steps = 2, a bounded cache
(cache_frame_size = 2), B = 1 and 3 distinct sessions: the latents are torch.equal after every frame (a frame never
reads a later frame's actions), frame_rows(f) is the frame's [hw, B, 64] state rows, and through cp25_stream_latent_clip
they are the un-normalised decoder input of latents()[:, :, f]. The misuse forms raise ValueError.
"""
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2 import _native as N
from cosmos_predict2.dit import init_state_dict
from cosmos_predict2.model import (StreamingBatchRun, StreamingRun, Video2WorldModelRectifiedFlow, to_patch_layout)
from cosmos_predict2.net_config import SAMPLER_ACTION_STREAMING, tiny_dit

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
T, H, W = 4, 8, 12
SEEDS = [11, 12, 13]
CFG = tiny_dit(num_blocks=1, action_dim=7, action_per_latent_frame=4, timestep_scale=1.0, use_wan_fp32_strategy=False)
KW = dict(n_steps=2, cache_frame_size=2)


@pytest.fixture(scope="module")
def tiny(device):
    sd = {"net." + k: v for k, v in init_state_dict(CFG, seed=21, zero_adaln_out=False).items()}
    model = Video2WorldModelRectifiedFlow(CFG, SAMPLER_ACTION_STREAMING, device=device)
    model.load_state_dict(sd)
    g = torch.Generator().manual_seed(77)
    d = dict(gt=torch.randn(3, 16, T, H, W, generator=g), actions=(torch.randn(3, 12, 7, generator=g) * 0.5).to(BF16),
             ctx=torch.randn(1, 512, CFG.crossattn_proj_in_channels, generator=g).to(BF16))
    return model, d


@pytest.mark.parametrize("B", [1, 3])
def test_batch_run_with_actions_per_frame(device, tiny, B):
    model, d = tiny
    gt, acts = d["gt"][:B], d["actions"][:B]
    whole = StreamingBatchRun(model, gt, d["ctx"], acts, seed=SEEDS[:B], **KW)
    loop = StreamingBatchRun(model, gt, d["ctx"], None, seed=SEEDS[:B], **KW)
    assert loop.actions is None and loop.action_shape == (B, 4, 7)
    assert whole.next_frame() == 0 and loop.next_frame() == 0  # the prefill takes no action
    for f in range(1, T):
        assert whole.next_frame() == f
        a = acts[:, 4 * (f - 1): 4 * f]
        assert loop.next_frame(a if f % 2 else a.to(device)) == f  # a host or a device tensor
        assert torch.equal(loop.latents(), whole.latents()), f  # later frames still zero in both
        rows = loop.frame_rows(f)
        assert tuple(rows.shape) == (H // 2 * (W // 2), B, 64) and rows.data_ptr() == loop.out[f].data_ptr()
        for b in range(B):
            assert torch.equal(rows[:, b], to_patch_layout(whole.latents()[b, :, f: f + 1]))
    assert loop.done and float(loop.latents()[:, :, 1:].float().std()) > 0
    if B > 1:
        assert not torch.equal(loop.latents()[0], loop.latents()[1])
    # the rows through the kernel: the decoder's un-normalised input of that latent frame
    mean = torch.linspace(-1, 1, 16).to(device, BF16)
    inv_std = 1.0 / torch.linspace(0.5, 3, 16).to(device, BF16)
    z = whole.latents()[:, :, 2]  # [B, 16, H, W]
    assert torch.equal(N.stream_latent_clip(loop.frame_rows(2), inv_std, mean, H // 2, W // 2),
                       z.permute(0, 2, 3, 1).contiguous() / inv_std + mean)
    with pytest.raises(RuntimeError):
        loop.next_frame(acts[:, :4])


def test_one_session_run_with_actions_per_frame(device, tiny):
    model, d = tiny
    gt, acts = d["gt"][:1], d["actions"][:1]
    whole = StreamingRun(model, gt, d["ctx"], acts, seed=5, **KW)
    loop = StreamingRun(model, gt, d["ctx"], None, seed=5, **KW)
    whole.next_frame(), loop.next_frame()
    for f in range(1, T):
        whole.next_frame()
        loop.next_frame(acts[:, 4 * (f - 1): 4 * f])
    assert torch.equal(loop.latents(), whole.latents())
    assert tuple(loop.frame_rows(3).shape) == (24, 1, 64)


def test_misuse_raises(device, tiny):
    model, d = tiny
    gt, acts = d["gt"][:2], d["actions"][:2]
    for cls, g, a in ((StreamingBatchRun, gt, acts), (StreamingRun, gt[:1], acts[:1])):
        loop = cls(model, g, d["ctx"], None, seed=1, **KW)
        with pytest.raises(ValueError):
            loop.frame_rows(0)  # not run yet
        with pytest.raises(ValueError):
            loop.next_frame(a[:, :4])  # the prefill takes none
        assert loop.frame == 0
        loop.next_frame()
        with pytest.raises(ValueError):
            loop.next_frame()  # a missing action
        for bad in (a[:, :3], a[:, :4, :6], a[0, :4], a[:, :8], a[:, :4].tolist()):
            with pytest.raises(ValueError):
                loop.next_frame(bad)
        if cls is StreamingBatchRun:
            with pytest.raises(ValueError):
                loop.next_frame(a[:1, :4])  # one session's actions for two
        assert loop.frame == 1  # nothing ran
        assert loop.next_frame(a[:, :4]) == 1
        with pytest.raises(ValueError):
            loop.frame_rows(2)
        # a run that has its action array takes none per frame
        whole = cls(model, g, d["ctx"], a, seed=1, **KW)
        with pytest.raises(ValueError):
            whole.next_frame(a[:, :4])
        whole.next_frame()
        with pytest.raises(ValueError):
            whole.next_frame(a[:, :4])
        assert whole.next_frame() == 1
        assert torch.equal(whole.latents(), loop.latents())
