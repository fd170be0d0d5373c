"""Host side of the distilled (DMD2 / TrigFlow) sampler: tables, step list, config entries, refusals (no GPU).

The float64 tables (cosmos_predict2/trigflow.py) are checked against closed forms: under rectified-flow scaling with
sigma_data = 1 the four student times (pi / 2, atan 15, atan 5, atan 5/3) are rectified-flow t = s / (1 + s) for
s = tan(time) = inf, 15, 5, 5/3, i.e. c_noise = 1, 15/16, 5/6, 5/8, c_skip = c_in and c_out = -c_noise. Bound: 2 ulp
of float64 (cos, sin and one division, each within an ulp, on values of order 1), stated before any run.
"""
import math
import types

import pytest
import torch

import distill_truth as DT
from cosmos_predict2 import trigflow
from cosmos_predict2.config import SetupArguments
from cosmos_predict2.model import Video2WorldModelRectifiedFlow
from cosmos_predict2.net_config import (DIT_2B, DIT_2B_DISTILLED, MODELS, SAMPLER_2B_DISTILLED,
                                        SAMPLER_2B_POST_TRAINED, SamplerConfig)

TIMES = (math.pi / 2, math.atan(15), math.atan(5), math.atan(5 / 3))
ULP = 2.0 ** -52


def _within_ulps(a: torch.Tensor, b, n: int) -> bool:
    b = torch.as_tensor(b, dtype=torch.float64)
    return bool(((a - b).abs() <= n * ULP * b.abs().clamp_min(2.0 ** -60)).all())


def test_rectified_flow_tables_closed_form():
    t = torch.tensor(TIMES, dtype=torch.float64)
    c_skip, c_out, c_in, c_noise = trigflow.trig_scaling(t, "rectified_flow", 1.0)
    assert all(c.dtype == torch.float64 for c in (c_skip, c_out, c_in, c_noise))
    assert _within_ulps(c_noise, [1.0, 15 / 16, 5 / 6, 5 / 8], 2)
    assert torch.equal(c_skip, c_in)
    assert torch.equal(c_out, -c_noise)
    # c_skip = c_in = 1 / (cos + sin) = sqrt(1 + s^2) / (1 + s): the TrigFlow state is cos x0 + sin eps, the
    # rectified-flow state (1 - t) x0 + t eps divided by (1 - t) sqrt(1 + s^2)
    s = torch.tensor([15.0, 5.0, 5 / 3], dtype=torch.float64)
    assert _within_ulps(c_skip[:1], [1.0], 2)
    assert _within_ulps(c_skip[1:], torch.sqrt(1 + s * s) / (1 + s), 4)  # + the closed form's own roundings
    # and the truth's restatement of the wrapper gives the same bits
    for s, sd in (("rectified_flow", 1.0), ("rectified_flow", 0.8), ("edm", 1.0), ("edm", 0.5)):
        for a, b in zip(trigflow.trig_scaling(t, s, sd), DT.scaling_from_time(t, s, sd)):
            assert torch.equal(a, b)


def test_rectified_flow_tables_sigma_data():
    """sigma_data != 1: c_noise = sd sin / (cos + sd sin) = sd s / (1 + sd s) with s = tan(time)."""
    t = torch.tensor(TIMES[1:], dtype=torch.float64)
    for sd in (0.5, 0.8):
        c_skip, c_out, c_in, c_noise = trigflow.trig_scaling(t, "rectified_flow", sd)
        s = torch.tensor([15.0, 5.0, 5 / 3], dtype=torch.float64)
        assert _within_ulps(c_noise, sd * s / (1 + sd * s), 4)  # + the closed form's own two roundings
        assert torch.equal(c_skip, c_in) and torch.equal(c_out, -c_noise)


def test_edm_tables_closed_form():
    t = torch.tensor(TIMES[1:], dtype=torch.float64)
    for sd in (1.0, 0.5):
        c_skip, c_out, c_in, c_noise = trigflow.trig_scaling(t, "edm", sd)
        s = torch.tensor([15.0, 5.0, 5 / 3], dtype=torch.float64)  # tan(time)
        assert _within_ulps(c_skip, sd / torch.sqrt(1 + s * s), 4)
        assert _within_ulps(c_out, sd * s / torch.sqrt(1 + s * s), 4)
        assert torch.equal(c_in, torch.ones_like(t))
        assert bool(((c_noise - 0.25 * torch.log(sd * s)).abs() <= 4 * ULP).all())
    with pytest.raises(ValueError):
        trigflow.trig_scaling(t, "vp", 1.0)
    with pytest.raises(ValueError):
        trigflow.trig_scaling(t.float(), "edm", 1.0)


def test_conditional_frame_time():
    mask = torch.tensor([1.0, 1.0, 0.0, 0.0])
    for sd, sc in ((1.0, 1e-4), (0.5, 1e-4), (0.8, 0.02)):
        tf = trigflow.frame_times(TIMES[2], mask, sc, sd)
        assert tf.dtype == torch.float64 and tf.shape == (4,)
        assert _within_ulps(tf[:2], [math.atan(sc / sd)] * 2, 1)
        assert torch.equal(tf[2:], torch.tensor([TIMES[2]] * 2, dtype=torch.float64))
    # no conditioning: every frame at t
    assert torch.equal(trigflow.frame_times(TIMES[0], torch.zeros(3), 1e-4, 1.0),
                       torch.full((3,), TIMES[0], dtype=torch.float64))
    # the truth's per-frame time (denoise_edm :257-260) gives the same bits
    m5 = mask.view(1, 1, 4, 1, 1).expand(1, 1, 4, 2, 2)
    _, _, st = DT.net_input(torch.zeros(1, 16, 4, 2, 2), torch.tensor([TIMES[2]], dtype=torch.float64),
                            torch.zeros(1, 16, 4, 2, 2), m5, sigma_data=0.5)
    assert torch.equal(st["time"].flatten(), trigflow.frame_times(TIMES[2], mask, 1e-4, 0.5))


def test_step_list_and_renoise_scalars():
    for n, want in ((1, TIMES[:1]), (2, TIMES[:2]), (3, TIMES[:3]), (4, TIMES), (35, TIMES)):
        assert trigflow.step_times(TIMES, n) == list(want) + [0.0]
    with pytest.raises(ValueError):
        trigflow.step_times(TIMES, 0)
    with pytest.raises(ValueError):
        trigflow.step_times((), 4)
    assert trigflow.renoise_scalars(TIMES[1]) == (math.cos(TIMES[1]), math.sin(TIMES[1]), False)
    assert trigflow.renoise_scalars(0.0)[2] and trigflow.renoise_scalars(1e-5)[2]
    assert not trigflow.renoise_scalars(2e-5)[2]


def test_net_timesteps_cast():
    """bf16(bf16(c_noise) * timestep_scale) widened to fp32; the float64 -> bf16 cast rounds through fp32."""
    c = torch.tensor([1.0, 15 / 16, 5 / 6, 5 / 8, 1e-4], dtype=torch.float64)
    for scale in (1.0, 0.001):
        got = trigflow.net_timesteps(c, scale)
        assert got.dtype == torch.float32 and got.shape == (1, 5)
        assert torch.equal(got[0], (c.float().to(torch.bfloat16) * scale).float())
    assert trigflow.net_timesteps(c, 1.0)[0, 2].item() == 0.83203125  # bf16(5 / 6)


def test_model_entry_and_names(tmp_path):
    net, smp = MODELS["2B/distilled"]
    assert net is DIT_2B_DISTILLED and smp is SAMPLER_2B_DISTILLED
    assert net == DIT_2B.replace(timestep_scale=1.0, use_wan_fp32_strategy=False)
    assert smp.sampler == "dmd2" and smp.selected_sampling_time == TIMES and smp.trig_scaling == "rectified_flow"
    assert (smp.sigma_data, smp.sigma_conditional, smp.state_t) == (1.0, 1e-4, 24)
    assert smp.denoise_replace_gt_frames and not smp.change_time_embed
    assert SetupArguments(output_dir=tmp_path, model="2B/distilled").model == "2B/distilled"
    with pytest.raises(ValueError):
        SetupArguments(output_dir=tmp_path, model="2B/distilled-8step")


def test_sampler_config_defaults_unchanged():
    d = SamplerConfig()
    assert (d.state_ch, d.state_t, d.shift, d.use_kerras_sigma_at_inference, d.conditional_frame_timestep,
            d.denoise_replace_gt_frames, d.cfg_mode, d.resolution) == (16, 24, 5.0, False, -1.0, True, "video2world",
                                                                       "720")
    assert (d.sampler, d.selected_sampling_time, d.trig_scaling, d.sigma_data, d.sigma_conditional,
            d.change_time_embed) == ("unipc", (), "rectified_flow", 1.0, 1e-4, False)
    assert SAMPLER_2B_POST_TRAINED.sampler == "unipc"
    for name, (_, s) in MODELS.items():
        assert (s.sampler == "dmd2") == (name == "2B/distilled"), name


def test_distilled_sampler_refuses_action_and_views():
    """begin_sampling's routing refuses what the distilled loop does not serve, before anything is built."""
    stub = types.SimpleNamespace(config=SAMPLER_2B_DISTILLED)
    kw = dict(state_shape=(16, 3, 8, 12), num_conditional_frames=1, guidance=7.0, seed=0, num_steps=4)
    with pytest.raises(ValueError, match="action"):
        Video2WorldModelRectifiedFlow.begin_sampling(stub, None, torch.zeros(1, 4, 8), None, action=torch.zeros(1, 12, 7),
                                                     **kw)
    with pytest.raises(ValueError, match="view_indices"):
        Video2WorldModelRectifiedFlow.begin_sampling(stub, None, torch.zeros(1, 4, 8), None,
                                                     view_indices=torch.tensor([0, 1]), **kw)
    bad = types.SimpleNamespace(config=SamplerConfig(sampler="ddim"))
    with pytest.raises(ValueError, match="sampler"):
        Video2WorldModelRectifiedFlow.begin_sampling(bad, None, torch.zeros(1, 4, 8), None, **kw)
    uni = types.SimpleNamespace(config=SamplerConfig())
    with pytest.raises(ValueError, match="init_noise"):
        Video2WorldModelRectifiedFlow.begin_sampling(uni, None, torch.zeros(1, 4, 8), None,
                                                     init_noise=torch.zeros(1, 16, 3, 8, 12), **kw)


def test_student_forward_small_frames_cpu():
    """The student net's arithmetic (timestep_scale 1, bf16 conditioning) at a 4 x 6 latent, where every gated residual
    is unfused and the bf16 final layer's LN-mod takes the last MLP residual: host path on the CPU stand-ins against
    the oracle, timesteps = bf16 c_noise values. (The stride refusal this used to hit is the device wrapper's;
    tests/test_distill_gpu.py covers it there.)"""
    import dataclasses

    import cpu_kernels
    from cosmos_predict2.dit import MinimalV1LVGDiT, init_state_dict
    from cosmos_predict2.net_config import tiny_dit
    from oracle import dit as odit

    cfg = tiny_dit(num_blocks=2, timestep_scale=1.0, use_wan_fp32_strategy=False)
    sd = {"net." + k: v for k, v in init_state_dict(cfg, seed=1, zero_adaln_out=False).items()}
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 16, 3, 4, 6, generator=g)
    mask = torch.zeros(1, 1, 3, 4, 6)
    mask[:, :, :1] = 1
    t = torch.tensor([[1e-4, 5 / 6, 5 / 6]]).to(torch.bfloat16).float()
    ctx = torch.randn(1, 512, cfg.crossattn_proj_in_channels, generator=g).to(torch.bfloat16)
    ref = odit.dit_forward(dataclasses.asdict(cfg), sd, x, t, ctx, mask)
    with cpu_kernels.patched(), torch.no_grad():
        net = MinimalV1LVGDiT(cfg, device="cpu")
        net.load_state_dict(sd)
        out = net(x.to(torch.bfloat16), t, ctx, condition_video_input_mask_B_C_T_H_W=mask)
    rel = ((out.float() - ref).norm() / ref.norm()).item()
    print(f"student net forward at a 4 x 6 latent (CPU stand-ins) vs oracle rel-L2: {rel:.3e}")
    assert rel <= 1e-2, rel


def test_double_rounding_premise():
    """The GPU rounding test's premise: among 2^22 seeded normals times c_in(atan 5) at least 16 round differently
    float64 -> bf16 directly and through fp32, and torch's `.to(bfloat16)` is the two-step rounding on every one."""
    c_in = trigflow.trig_scaling(torch.tensor([TIMES[2]], dtype=torch.float64), "rectified_flow", 1.0)[2].item()
    xs = DT.double_rounding_inputs(c_in)
    assert xs.numel() >= 16, xs.numel()
    x = torch.randn(1 << 22, generator=torch.Generator().manual_seed(0))
    p = x.double() * c_in
    assert torch.equal(p.to(torch.bfloat16), p.float().to(torch.bfloat16))
    # the one-step rounding is a correct rounding: never farther from the float64 value than torch's
    d1 = (DT.bf16_direct(p).double() - p).abs()
    d2 = (p.to(torch.bfloat16).double() - p).abs()
    assert bool((d1 <= d2).all()) and bool((d1 < d2).sum() == xs.numel())
