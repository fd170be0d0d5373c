"""The camera-conditioned sampler (model.CameraSamplingRun, generate_camera_samples) and the public interface
(camera.CameraInference) on the GPU.

Plumbing: with a deterministic stub net evaluated on the CPU for both sides, the three-segment setup and the loop of
tests/camera_truth.py (the reference's generate_samples_from_batch restated over oracle.sampler / oracle.unipc) and the
fused device loop must agree bit for bit over the whole trajectory: the standard of
tests/test_dit_gpu.py::test_sampler_plumbing_bit_exact."""
import dataclasses
import functools

import pytest
import torch

import camera_truth as ct
from cosmos_predict2 import camera as cam
from cosmos_predict2.config import SetupArguments
from cosmos_predict2.model import CameraSamplingRun, Video2WorldModelRectifiedFlow
from cosmos_predict2.net_config import SamplerConfig, tiny_dit

pytestmark = pytest.mark.gpu

CFG = tiny_dit(camera_dim=1536)
SAMPLER = SamplerConfig(use_kerras_sigma_at_inference=False, conditional_frame_timestep=0.1, state_t=2)
C, TS, H, W = 16, 2, 8, 12  # the latent is 16 x 6 x 8 x 12: three 2-frame segments
STEPS, GUIDANCE, SEED = 4, 1.5, 3
CTX_C, CTX_U = torch.zeros(1, 4, 8), torch.ones(1, 4, 8)


def _fake(xv, tv, b):
    """Deterministic stand-in denoiser evaluated on the CPU (same bits on both paths)."""
    return torch.sin(xv.float() * (1.0 + 0.25 * b) + tv)


def _source():
    return torch.randn(1, C, TS, H, W, generator=torch.Generator().manual_seed(21))


@functools.lru_cache(maxsize=None)
def _truth(n):
    def oracle_fn(c, s, x, t, ctx, mask):
        b = 0 if ctx is CTX_C else 1
        ts = (t.float() * CFG.timestep_scale)[0]  # [T]
        return _fake(x, ts[None, None, :, None, None], b)

    return ct.camera_generate(dataclasses.asdict(CFG), None, _source(), CTX_C, CTX_U, num_cond=n, guidance=GUIDANCE,
                              seed=SEED, num_steps=STEPS, cond_frame_t=SAMPLER.conditional_frame_timestep,
                              dit_fn=oracle_fn, return_trajectory=True)


def _device_fn(rows, t_B_T, geo):
    r = rows.cpu()[:, 0, :64].view(-1, 16, 4).transpose(1, 2).reshape(-1, 64)  # (c p) -> (p c)
    tok_t = torch.arange(geo.n_tok) // geo.hw
    outs = [_fake(r, t_B_T.cpu()[b][tok_t][:, None], b) for b in range(2)]
    return torch.stack(outs, 1).to(rows.device)


@pytest.mark.parametrize("n", [1, 2])
def test_camera_sampler_plumbing_bit_exact(device, n):
    (want0, want1), want_final, traj = _truth(n)
    model = Video2WorldModelRectifiedFlow(CFG, SAMPLER, device=device)
    src = _source()
    run = CameraSamplingRun(model, src.to(device), CTX_C, CTX_U, None, num_conditional_frames=n, guidance=GUIDANCE,
                            seed=SEED, num_steps=STEPS, net_fn=_device_fn)
    assert run.num_evals == len(traj) == STEPS and not run._graphable
    # the initial state: both target segments start from the same seeded noise, the source segment is the source latent
    x0 = run.latents().cpu()
    seg = torch.chunk(x0, 3, dim=2)
    assert torch.equal(seg[0], seg[2]) and torch.equal(seg[1], src) and seg[0].std() > 0.5
    want_mask = torch.zeros(3 * TS)
    want_mask[n:2 * n] = 1
    assert torch.equal(run.frame_mask.cpu(), want_mask)
    gt = run.gtp.cpu()  # zero outside the source segment
    hw = (H // 2) * (W // 2)
    assert (gt[: TS * hw] == 0).all() and (gt[2 * TS * hw:] == 0).all() and gt[TS * hw: 2 * TS * hw].abs().sum() > 0
    for i in range(STEPS):
        assert run.step() == i
        assert torch.equal(run.latents().cpu(), traj[i]), f"step {i}"
    assert run.done
    got0, got1 = run.target_latents()
    assert torch.equal(got0.cpu(), want0) and torch.equal(got1.cpu(), want1)
    assert tuple(got0.shape) == tuple(got1.shape) == (1, C, TS, H, W)
    if n == 1:
        # the mask sits on frame 1 of target 0 (the literal [n, 2n) rule), the only thing that tells the two targets
        # apart under a stub net that sees neither the camera nor the position
        assert not torch.equal(got0, got1) and torch.equal(got0[:, :, 0], got1[:, :, 0])
    if n == 2:
        assert torch.equal(got0, got1)
        # the mask covers the source segment: its velocity is noise - gt = 0 there, so the state stays the source latent
        # up to the solver's own fp32 arithmetic (x' = a x + b x0 with x0 = x and a + b = 1 only in exact arithmetic:
        # the reference's loop, restated in camera_truth, moves these values by 4.8e-7 too; the device equals it bit for
        # bit above). Bound: two coefficient roundings, two products and a sum per step, 4 eps of max |x| each.
        final = run.latents().cpu()[:, :, TS:2 * TS]
        bound = STEPS * 4 * torch.finfo(torch.float32).eps * src.abs().max().item()
        assert (final - src).abs().max().item() <= bound
        assert torch.equal(final, want_final[:, :, TS:2 * TS])


def test_generate_camera_samples_with_stub_net(device):
    """generate_camera_samples: the source latent in, cameras in arrival order [source | target 0 | target 1] (only
    their shape is read with a stub net), the same two latents out as the run above."""
    (want0, want1), _, _ = _truth(1)
    model = Video2WorldModelRectifiedFlow(CFG, SAMPLER, device=device)
    camera = torch.zeros(3 * TS, H // 2, W // 2, 1536, dtype=torch.bfloat16)
    got0, got1 = model.generate_camera_samples(CTX_C, CTX_U, camera, source_latent=_source().to(device),
                                               num_conditional_frames=1, guidance=GUIDANCE, seed=SEED,
                                               num_steps=STEPS, net_fn=_device_fn)
    assert torch.equal(got0.cpu(), want0) and torch.equal(got1.cpu(), want1)
    with pytest.raises(ValueError, match="expected"):
        model.generate_camera_samples(CTX_C, CTX_U, camera[:-1], source_latent=_source().to(device), net_fn=_device_fn)
    with pytest.raises(ValueError, match="exactly one"):
        model.generate_camera_samples(CTX_C, CTX_U, camera, net_fn=_device_fn)
    with pytest.raises(ValueError, match="needs `camera`"):
        CameraSamplingRun(model, _source().to(device), CTX_C, CTX_U, None)
    karras = Video2WorldModelRectifiedFlow(CFG, dataclasses.replace(SAMPLER, use_kerras_sigma_at_inference=True),
                                           device=device)
    with pytest.raises(ValueError, match="Karras"):
        CameraSamplingRun(karras, _source().to(device), CTX_C, CTX_U, None, net_fn=_device_fn)


def _trajectories(delta=0.0):
    """w2c [3, 5, 3, 4], intrinsics [3, 5, 4] for 5 pixel frames at 64 x 96: a static source camera, target 0 moving
    right, target 1 turning about y (by delta more)."""
    eye = torch.eye(3, dtype=torch.float64)
    w2c = torch.stack([
        torch.stack([ct.pose(eye, [0.0, 0.0, 0.0]) for _ in range(5)]),
        torch.stack([ct.pose(eye, [-0.1 * f, 0.0, 0.0]) for f in range(5)]),
        torch.stack([ct.pose(ct.rot("y", 4.0 * f + delta), [0.0, 0.0, 0.1 * f]) for f in range(5)])])
    k = torch.tensor([96.0, 96.0, 48.0, 32.0]).expand(3, 5, 4).contiguous()
    return w2c, k


def test_camera_inference_end_to_end(device, tmp_path):
    """CameraInference.generate on the tiny net at 64 x 96 pixels, 3 x 5 frames: two uint8 videos of the right shape,
    deterministic in the seed, and different once a target trajectory changes."""
    setup = SetupArguments(output_dir=tmp_path, model="2B/camera-cond", context_parallel_size=1)
    inf = cam.CameraInference(setup, net_cfg=CFG, sampler_cfg=SAMPLER, device=device)
    args = cam.CameraInferenceArguments(name="s", prompt="a street at dusk", input_path=tmp_path / "in.mp4",
                                        cameras_path=tmp_path / "c.npz", seed=5, num_steps=2, resolution="64,96")
    video = torch.randint(0, 256, (1, 3, 5, 64, 96), dtype=torch.uint8, generator=torch.Generator().manual_seed(1))
    a = inf.generate(args, output_dir=False, input_video=video, cameras=_trajectories())
    assert len(a) == 2 and all(v.dtype == torch.uint8 and tuple(v.shape) == (5, 64, 96, 3) for v in a)
    assert all(v.float().std() > 0 for v in a)
    b = inf.generate(args, output_dir=False, input_video=video, cameras=_trajectories())
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    c = inf.generate(args, output_dir=False, input_video=video, cameras=_trajectories(delta=20.0))
    assert not all(torch.equal(x, y) for x, y in zip(a, c))
    # a ready camera tensor (the reference's contract) replaces the packing: the same features, the same videos
    rows = cam.camera_rows_from_trajectories(*_trajectories(), 2, 4, 6, device)
    e = inf.generate(args, output_dir=False, input_video=video, camera_tensor=rows)
    assert all(torch.equal(x, y) for x, y in zip(a, e))
    # written through the existing muxer (the videos of the first run, not generated again)
    inf.generate_videos = lambda *_a, **_k: a
    paths = inf.generate(args)
    assert [p.split("/")[-1] for p in paths] == ["s_target0.mp4", "s_target1.mp4"]
    assert all((tmp_path / n).stat().st_size > 0 for n in ("s_target0.mp4", "s_target1.mp4", "s.json"))
    with pytest.raises(ValueError, match="camera-conditioned net"):
        cam.CameraInference(setup, net_cfg=tiny_dit(), sampler_cfg=SAMPLER, device=device)
