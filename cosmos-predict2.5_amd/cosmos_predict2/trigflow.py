"""Host arithmetic of the distilled (DMD2 / TrigFlow) student sampler: per-frame times and EDM-style scaling tables.

Reference: cosmos_predict2/_src/predict2/modules/denoiser_scaling.py (EDM_sCMWrapper :28-43, RectifiedFlow_sCMWrapper
:46-67), models/video2world_model_rectified_flow.py denoise_edm :247-270 (conditional-frame time, c_noise) and :303-309
(the timesteps' cast to the net dtype), distill/models/video2world_model_distill_dmd2.py :480-488 (the step list and
the re-noising scalars, which the reference takes from Python's math module as well).

Everything here is a handful of float64 values per latent frame, computed with CPU torch ops in the reference's order;
the per-element work is cp25_trig_patchify_ld / cp25_trig_x0_step. Deviation: the reference evaluates
atan / cos / sin / tan / log of these tables on CUDA float64 tensors and this build on the host, so agreement in the
last ulp of those functions is not pinned.

stream_scaling / stream_renoise are the same tables for the streaming causal student (interactive/models/
action_video2world_self_forcing.py:185-203, 441-443), whose times and coefficients are bf16 tensors: a few bf16 values
per evaluation, made with CPU torch bf16 ops; the per-element work is cp25_stream_patchify_ld / cp25_stream_x0_step.
"""
from __future__ import annotations

import math
from typing import List, Sequence, Tuple

import torch

F64 = torch.float64
SCALINGS = ("rectified_flow", "edm")
LAST_STEP_EPS = 1e-5  # video2world_model_distill_dmd2.py:487: a next time at or below this ends the loop without noise


def trig_scaling(t_frames: torch.Tensor, scaling: str, sigma_data: float) -> Tuple[torch.Tensor, ...]:
    """TrigFlow time(s) -> (c_skip, c_out, c_in, c_noise), float64, operation for operation as
    RectifiedFlow_sCMWrapper.__call__ (denoiser_scaling.py:59-66) or EDM_sCMWrapper.__call__ (:35-42)."""
    if t_frames.dtype != F64:
        raise ValueError(f"trig_scaling takes float64 times (the loop's dtype), got {t_frames.dtype}")
    t = t_frames
    if scaling == "rectified_flow":
        c_skip = sigma_data / (torch.cos(t) + sigma_data * torch.sin(t))
        c_out = -sigma_data * torch.sin(t) / (torch.cos(t) + sigma_data * torch.sin(t))
        c_in = sigma_data / (torch.cos(t) + sigma_data * torch.sin(t))
        c_noise = sigma_data * torch.sin(t) / (torch.cos(t) + sigma_data * torch.sin(t))
    elif scaling == "edm":
        sigma = torch.tan(t) * sigma_data
        c_skip = sigma_data * torch.cos(t)
        c_out = sigma_data * torch.sin(t)
        c_in = torch.ones_like(t)
        c_noise = 0.25 * sigma.log()
    else:
        raise ValueError(f"trig_scaling: unknown scaling {scaling!r} (one of {SCALINGS})")
    return c_skip, c_out, c_in, c_noise


def frame_times(t: float, frame_mask: torch.Tensor, sigma_conditional: float, sigma_data: float) -> torch.Tensor:
    """Per-frame TrigFlow time [T] float64: conditioning frames sit at t_cond = atan(sigma_conditional / sigma_data)
    (denoise_edm :257-260: t_cond * mask + t * (1 - mask), the mask cast to the time's float64)."""
    m = frame_mask.detach().to("cpu", F64)
    time = t * torch.ones_like(m)  # t_cur * ones (dmd2 :486)
    t_cond = torch.atan(torch.ones_like(time) * (sigma_conditional / sigma_data))
    return t_cond * m + time * (1 - m)


def step_times(selected_sampling_time: Sequence[float], num_steps: int) -> List[float]:
    """selected_sampling_time[:num_steps] + [0] (dmd2 :482-484): num_steps above the list's length runs all of it."""
    if num_steps < 1:
        raise ValueError("num_steps must be at least 1")
    if not selected_sampling_time:
        raise ValueError("the distilled sampler needs SamplerConfig.selected_sampling_time")
    return [float(t) for t in selected_sampling_time][:num_steps] + [0.0]


def renoise_scalars(t_next: float) -> Tuple[float, float, bool]:
    """(cos t_next, sin t_next, last) of one step (dmd2 :487-488, Python's math as there)."""
    return math.cos(t_next), math.sin(t_next), not (t_next > LAST_STEP_EPS)


BF16 = torch.bfloat16


def stream_scaling(t: float, frame_mask: float, scaling: str, sigma_data: float,
                   sigma_conditional: float) -> Tuple[float, float, float, torch.Tensor]:
    """The streaming student's coefficients of one evaluation at TrigFlow time t (denoise_edm_seq,
    interactive/models/action_video2world_self_forcing.py:185-203): (c_skip, c_out, c_in) as Python floats holding bf16
    values, and c_noise as a bf16 [1] tensor for net_timesteps. There the time is a bf16 tensor (torch.full(...,
    dtype=bfloat16), :420, or zeros in the net dtype, :524), the mask's mean is cast to it, and
    `t_cond * mask + time * (1 - mask)` is four bf16 ops, written out here though this loop's mask is always 0; the
    sCM wrappers compute in float64 and return the coefficients cast back to the time's bf16
    (modules/denoiser_scaling.py:33-34, 43, 51-52, 67)."""
    time = torch.full((1,), float(t), dtype=BF16)
    m = torch.full((1,), float(frame_mask), dtype=BF16)
    t_cond = torch.atan(torch.ones_like(time) * (sigma_conditional / sigma_data))
    time = t_cond * m + time * (1 - m)
    c_skip, c_out, c_in, c_noise = (c.to(BF16) for c in trig_scaling(time.to(F64), scaling, sigma_data))
    return float(c_skip), float(c_out), float(c_in), c_noise


def stream_renoise(t_next: float) -> Tuple[float, float]:
    """(cos, sin) of the 0-dim bf16 tensor torch.tensor(t_next, dtype=bfloat16) (:441-443), each a bf16 value."""
    tn = torch.tensor(float(t_next), dtype=BF16)
    return float(torch.cos(tn)), float(torch.sin(tn))


def net_timesteps(c_noise: torch.Tensor, timestep_scale: float) -> torch.Tensor:
    """What the student net's embedder sees, [1, T] fp32: c_noise cast to the net dtype (denoise_edm :307-309; a float64
    tensor's .to(bfloat16) rounds through fp32) and scaled there (minimal_v1_lvg_dit.py:55, a bf16 product)."""
    t = c_noise.to(torch.bfloat16) * timestep_scale
    return t.float()[None, :]
