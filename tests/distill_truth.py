"""The distilled (DMD2 / TrigFlow) student's sampling loop restated in CPU torch: TEST INFRASTRUCTURE, like oracle/.

Follows, in cosmos_predict2/_src/predict2/, with the reference's exact dtype sequence:
  distill/models/video2world_model_distill_dmd2.py:421-492   generate_samples_from_batch: float64 state, `.float()`
                                                             into the denoiser, python-scalar re-noising, nan_to_num
  models/video2world_model_rectified_flow.py:214-346         denoise_edm, net_type "student": float64 times and
                                                             coefficients, `.to(bfloat16)` of the float64 net input and
                                                             of c_noise, `.float()` of the net output, the mask
                                                             arithmetic as written
  modules/denoiser_scaling.py:28-67                          EDM_sCMWrapper / RectifiedFlow_sCMWrapper
  configs/video2world/defaults/conditioner.py:45-143         the frame mask (oracle.sampler.frame_mask)
The noise is this build's arch_invariant_rand(seed) unless init_noise is given (the reference draws from a device
torch.Generator). `dit_fn(cfg, sd, x, t, ctx, mask)` defaults to the oracle DiT, as in
oracle.sampler.generate; x and t arrive in bf16 as the reference's tensor_kwargs cast makes them.
"""
from __future__ import annotations

import math

import torch

from oracle import dit as odit
from oracle import sampler as osamp

F64 = torch.float64
BF16 = torch.bfloat16
TIMES_4STEP = (math.pi / 2, math.atan(15), math.atan(5), math.atan(5 / 3))


def scaling_from_time(trigflow_t: torch.Tensor, scaling: str, sigma_data: float):
    """denoiser_scaling.py: RectifiedFlow_sCMWrapper.__call__ (:50-67) / EDM_sCMWrapper.__call__ (:32-43)."""
    dtype = trigflow_t.dtype
    trigflow_t = trigflow_t.to(F64)
    if scaling == "edm":
        sigma = torch.tan(trigflow_t) * sigma_data
        c_skip = sigma_data * torch.cos(trigflow_t)
        c_out = sigma_data * torch.sin(trigflow_t)
        c_in = torch.ones_like(trigflow_t)
        c_noise = 0.25 * sigma.log()
    else:
        c_skip = sigma_data / (torch.cos(trigflow_t) + sigma_data * torch.sin(trigflow_t))
        c_out = -sigma_data * torch.sin(trigflow_t) / (torch.cos(trigflow_t) + sigma_data * torch.sin(trigflow_t))
        c_in = sigma_data / (torch.cos(trigflow_t) + sigma_data * torch.sin(trigflow_t))
        c_noise = sigma_data * torch.sin(trigflow_t) / (torch.cos(trigflow_t) + sigma_data * torch.sin(trigflow_t))
    return c_skip.to(dtype), c_out.to(dtype), c_in.to(dtype), c_noise.to(dtype)


def net_input(xt, time_B, gt, mask, *, scaling="rectified_flow", sigma_data=1.0, sigma_conditional=1e-4,
              change_time_embed=False):
    """denoise_edm :239-309 up to the net call. xt [B, C, T, H, W] fp32, time_B [B] float64, gt the x0 latent, mask
    [B, 1, T, H, W]. Returns (x bf16 [B, C, T, H, W], timesteps bf16 [B, T], state for x0_from_net)."""
    time_B_T = time_B[:, None]
    time5 = time_B_T[:, None, :, None, None]  # b 1 t 1 1
    is_video = xt.shape[2] > 1
    C = xt.shape[1]
    cvm = None
    if is_video:
        cvm = mask.repeat(1, C, 1, 1, 1).type_as(xt)
        cvm_t = cvm.mean(dim=[1, 3, 4], keepdim=True).type_as(time5)
        t_cond = torch.atan(torch.ones_like(time5) * (sigma_conditional / sigma_data))
        time5 = t_cond * cvm_t + time5 * (1 - cvm_t)
    c_skip, c_out, c_in, c_noise = scaling_from_time(time5, scaling, sigma_data)
    net_in = xt * c_in
    if change_time_embed:
        c_noise = time5
    if is_video:
        cond_in = gt.type_as(net_in) / sigma_data
        cvm = mask.repeat(1, C, 1, 1, 1).type_as(net_in)
        net_in = cond_in * cvm + net_in * (1 - cvm)
    t_B_T = c_noise.squeeze(dim=[1, 3, 4]).to(BF16)
    return net_in.to(BF16), t_B_T, dict(c_skip=c_skip, c_out=c_out, c_in=c_in, c_noise=c_noise, cvm=cvm, time=time5)


def x0_from_net(xt, net_out, gt, state, *, replace_gt=True):
    """denoise_edm :322-336: net_out is the net's bf16 (or stand-in) output; returns x0 (float64)."""
    net_out = net_out.float().to(dtype=xt.dtype)
    x0 = state["c_skip"] * xt + state["c_out"] * net_out
    cvm = state["cvm"]
    if replace_gt and cvm is not None:
        gtf = gt.type_as(x0)
        x0 = gtf * cvm.type_as(x0) + x0 * (1 - cvm)
    return x0


def denoise_edm(cfg_dit, sd, xt, time_B, ctx, gt, mask, *, replace_gt=True, dit_fn=None, **kw):
    x, t_B_T, state = net_input(xt, time_B, gt, mask, **kw)
    fn = dit_fn or odit.dit_forward
    net_out = fn(cfg_dit, sd, x, t_B_T, ctx, mask.to(BF16))
    return x0_from_net(xt, net_out, gt, state, replace_gt=replace_gt)


def renoise(x0_f64, t_next, init_noise, sigma_data):
    """dmd2 :487-488 (init_noise stays the float32 tensor it was drawn as)."""
    return math.cos(t_next) * x0_f64 / sigma_data + math.sin(t_next) * init_noise


def generate(cfg_dit, sd, gt, ctx, *, num_cond, seed, num_steps, selected_sampling_time=TIMES_4STEP,
             scaling="rectified_flow", sigma_data=1.0, sigma_conditional=1e-4, change_time_embed=False,
             replace_gt=True, dit_fn=None, init_noise=None, state_shape=None):
    """generate_samples_from_batch (:421-492). gt: x0 latent [1, C, T, H, W] fp32 (None with num_cond = 0: the mask is
    zero and the frames never enter). Returns the fp32 samples."""
    if gt is None:
        gt = torch.zeros((1,) + tuple(state_shape), dtype=torch.float32)
    B, C, T, H, W = gt.shape
    mask = osamp.frame_mask(B, T, H, W, num_cond, dtype=gt.dtype)
    if init_noise is None:
        init_noise = osamp.arch_invariant_rand((B, C, T, H, W), seed)
    x = init_noise.to(F64)
    ones = torch.ones(x.size(0), dtype=x.dtype)
    t_steps = list(selected_sampling_time)[:num_steps] + [0]
    for t_cur, t_next in zip(t_steps[:-1], t_steps[1:]):
        x = denoise_edm(cfg_dit, sd, x.float(), t_cur * ones, ctx, gt, mask, replace_gt=replace_gt, dit_fn=dit_fn,
                        scaling=scaling, sigma_data=sigma_data, sigma_conditional=sigma_conditional,
                        change_time_embed=change_time_embed).to(F64)
        if t_next > 1e-5:
            x = renoise(x, t_next, init_noise, sigma_data)
    samples = x.float()
    return torch.nan_to_num(samples)


# ---------------------------------------------------------------- float64 -> bf16: one rounding against torch's two
def bf16_direct(v: torch.Tensor) -> torch.Tensor:
    """Round float64 values to bf16 in ONE round-to-nearest-even step (finite, normal values). torch's
    `.to(bfloat16)` rounds float64 -> float32 -> bf16; the two differ where the float32 rounding lands exactly on a
    bf16 tie that the float64 value was not on."""
    f = v.float()
    lo = ((f.view(torch.int32) >> 16) << 16).view(torch.float32)  # f's magnitude truncated to bf16
    hi = (lo.view(torch.int32) + 0x10000).view(torch.float32)
    mid = (lo.double() + hi.double()) / 2
    odd = ((lo.view(torch.int32) >> 16) & 1).bool()
    up = (v.abs() > mid.abs()) | ((v.abs() == mid.abs()) & odd)
    return torch.where(up, hi, lo).to(BF16)


def double_rounding_inputs(c_in: float, n: int = 1 << 22, seed: int = 0) -> torch.Tensor:
    """fp32 normals x (seeded) on which bf16(float(double(x) * c_in)) != the direct float64 -> bf16 rounding."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    p = x.double() * c_in
    two_step = p.to(BF16)
    return x[two_step != bf16_direct(p)]
