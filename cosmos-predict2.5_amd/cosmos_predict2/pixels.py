"""The device-resident uint8 pixel path: resize + centre crop, uint8 -> VAE clip, VAE clip -> uint8.

Host side of csrc/pixel_ops.hip. `aa_tables` restates the separable triangle filter that
`F.interpolate(mode="bilinear", align_corners=False, antialias=True)` applies (the host path's
`pipeline.resize_input`); `resize_input_device` / `process_video_frames_device` are the device forms of
`pipeline.resize_input` / `pipeline.process_video_frames` (inference/video2world.py:75-97, :145-233), and
`video_to_clip` / `clip_to_uint8` wrap the two conversion kernels. Unsupported shapes raise ValueError; nothing
here falls back to the host path.
"""
from __future__ import annotations

import math
from typing import Dict, Tuple

import numpy as np
import torch

from . import _native as N

_TABLES: Dict[tuple, tuple] = {}


def _aa_tables_np(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    scale = n_in / n_out
    support = scale if scale >= 1.0 else 1.0
    inv = 1.0 / max(scale, 1.0)
    starts = np.zeros(n_out, np.int32)
    counts = np.zeros(n_out, np.int32)
    rows = []
    for i in range(n_out):
        center = scale * (i + 0.5)
        start = max(int(center - support + 0.5), 0)
        end = min(int(center + support + 0.5), n_in)
        j = np.arange(end - start, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((j + start - center + 0.5) * inv))
        rows.append(w / w.sum())
        starts[i], counts[i] = start, end - start
    taps = int(counts.max())
    weights = np.zeros((n_out, taps), np.float32)
    for i, w in enumerate(rows):
        weights[i, : len(w)] = w
    return starts, counts, weights


def aa_tables(n_in: int, n_out: int, device=None):
    """Filter tables of one axis of the antialiased bilinear resize n_in -> n_out: (start int32 [n_out],
    count int32 [n_out], weights fp32 [n_out, taps]); output i is sum_j weights[i, j] * in[start[i] + j] over
    j < count[i]. numpy arrays for device=None, else tensors on `device`; cached per (n_in, n_out, device)."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"aa_tables: sizes must be positive, got {n_in} -> {n_out}")
    key = (n_in, n_out, None if device is None else str(torch.device(device)))
    hit = _TABLES.get(key)
    if hit is None:
        if device is None:
            hit = _aa_tables_np(n_in, n_out)
        else:
            hit = tuple(torch.from_numpy(a).to(device) for a in aa_tables(n_in, n_out))
        _TABLES[key] = hit
    return hit


def resize_geometry(orig_hw, resolution):
    """resize_input's arithmetic: ((rh, rw) resized extent, (top, left) of the centre crop)."""
    orig_h, orig_w = orig_hw
    th, tw = resolution
    r = max(tw / orig_w, th / orig_h)
    rh, rw = int(math.ceil(r * orig_h)), int(math.ceil(r * orig_w))
    return (rh, rw), (int(round((rh - th) / 2.0)), int(round((rw - tw) / 2.0)))


def resize_input_device(video_u8: torch.Tensor, resolution, layout: str = "TCHW") -> torch.Tensor:
    """pipeline.resize_input on the device in one kernel launch: uint8 [T, C, H, W] (layout "TCHW") or
    [T, H, W, C] ("THWC") device tensor of any strides -> contiguous uint8 [T, C, th, tw] / [T, th, tw, C]."""
    if layout not in ("TCHW", "THWC"):
        raise ValueError(f"layout must be 'TCHW' or 'THWC', got {layout!r}")
    if video_u8.dtype != torch.uint8 or video_u8.dim() != 4:
        raise ValueError(f"resize_input_device: a 4-D uint8 tensor is needed, got {video_u8.dtype} {tuple(video_u8.shape)}")
    if not video_u8.is_cuda:
        raise ValueError("resize_input_device: the video must be on the GPU (pipeline.resize_input is the host path)")
    src = video_u8 if layout == "TCHW" else video_u8.permute(0, 3, 1, 2)
    T, C, H, W = src.shape
    th, tw = (int(v) for v in resolution)
    (rh, rw), (top, left) = resize_geometry((H, W), (th, tw))
    if layout == "TCHW":
        out = torch.empty((T, C, th, tw), dtype=torch.uint8, device=src.device)
        dst = out
    else:
        out = torch.empty((T, th, tw, C), dtype=torch.uint8, device=src.device)
        dst = out.permute(0, 3, 1, 2)
    N.resize_crop_u8(src, dst, aa_tables(H, rh, src.device), aa_tables(W, rw, src.device), (top, left, th, tw))
    return out


def process_video_frames_device(frames_T_H_W_C_u8: torch.Tensor, resolution, num_video_frames: int,
                                num_latent_conditional_frames: int = 2, validate: bool = True,
                                device="cuda") -> torch.Tensor:
    """pipeline.process_video_frames on the device: keep the last 4(n-1)+1 decoded frames, resize them, and pad
    to num_video_frames with copies of the last resized frame (a resize is per frame, so this equals resizing
    the padded video). Only the kept frames are uploaded. -> uint8 [1, 3, num_video_frames, th, tw] on `device`."""
    n = num_latent_conditional_frames
    if validate and n not in (1, 2):
        raise ValueError(f"num_latent_conditional_frames must be 1 or 2, but got {n}")
    fr = frames_T_H_W_C_u8
    if fr.dtype != torch.uint8 or fr.dim() != 4:
        raise ValueError(f"frames must be a uint8 [T, H, W, C] tensor, got {fr.dtype} {tuple(fr.shape)}")
    need = 4 * (n - 1) + 1
    if fr.shape[0] < need:
        raise ValueError(f"Video has only {fr.shape[0]} frames but needs at least {need} frames")
    if need > num_video_frames:
        raise ValueError(f"{need} conditioning frames do not fit {num_video_frames} video frames")
    kept = fr[fr.shape[0] - need:]
    kept = kept.to(device) if not kept.is_cuda else kept
    th, tw = (int(v) for v in resolution)
    C = kept.shape[3]
    full = torch.empty((1, C, num_video_frames, th, tw), dtype=torch.uint8, device=kept.device)
    src = kept.permute(0, 3, 1, 2)  # [T, C, H, W] view
    (rh, rw), (top, left) = resize_geometry(src.shape[2:], (th, tw))
    dst = full[0, :, :need].permute(1, 0, 2, 3)  # [T, C, th, tw] view of the planar video
    N.resize_crop_u8(src, dst, aa_tables(src.shape[2], rh, kept.device), aa_tables(src.shape[3], rw, kept.device),
                     (top, left, th, tw))
    if need < num_video_frames:
        full[:, :, need:] = full[:, :, need - 1: need]
    return full


def video_to_clip(video_u8: torch.Tensor) -> torch.Tensor:
    """uint8 [1, C, T, H, W] or [C, T, H, W] device video (any strides) -> the VAE encoder's clip [T, H, W, 16] bf16."""
    if video_u8.dim() == 5:
        if video_u8.shape[0] != 1:
            raise ValueError(f"video_to_clip: batch 1 only, got {video_u8.shape[0]}")
        video_u8 = video_u8[0]
    return N.u8_to_clip(video_u8)


def clip_to_uint8(clip: torch.Tensor, layout: str = "THWC") -> torch.Tensor:
    """The decoder's bf16 [T, H, W, 3] result -> uint8 [T, H, W, 3] ("THWC") or [1, 3, T, H, W] ("NCTHW")."""
    if clip.dim() != 4:
        raise ValueError(f"clip_to_uint8: a [T, H, W, C] clip is needed, got {tuple(clip.shape)}")
    T, H, W, C = clip.shape
    if layout == "THWC":
        out = torch.empty((T, H, W, C), dtype=torch.uint8, device=clip.device)
        N.clip_to_u8(clip, out)
    elif layout == "NCTHW":
        out = torch.empty((1, C, T, H, W), dtype=torch.uint8, device=clip.device)
        N.clip_to_u8(clip, out[0].permute(1, 2, 3, 0))
    else:
        raise ValueError(f"layout must be 'THWC' or 'NCTHW', got {layout!r}")
    return out
