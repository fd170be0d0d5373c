"""Camera-conditioned Video2World on MI355X: one source video and two target camera trajectories in, two re-rendered
videos out.

Reference: cosmos_predict2/_src/predict2/camera/ (net camera/networks/minimal_v4_dit_camera_conditioned.py and
camera_conditioned_minimal_v1_lvg_dit.py, conditioner configs/camera_conditioned/conditioner.py:42-68, model
models/camera_conditioned_video2world_model_rectified_flow.py:155-327) and the ray arithmetic of
_src/imaginaire/modules/camera.py:172-236 (get_plucker_rays). The net takes `camera` as a [B, T, Hp, Wp, 1536] tensor
on the patch grid (:1650-1658) and a caller may pass such a tensor ready made: that is the reference's own contract.

The reference holds NO code that packs per-pixel rays into that 1536-wide token feature (its camera datasets are
mocks). The packing offered here (plucker_camera_rows: "(c m n)", c over [moment | direction], m / n the 16 x 16
pixels of a token) and the choice of the pose of pixel frame 4 t for latent frame t (poses_for_latent_frames) are this
build's own helpers; parity of them is unpinned. A net post-trained with another packing takes its
features through the ready-tensor path.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Any, List, Optional, Tuple

import numpy as np
import pydantic
import torch

from . import _native as N

MODEL_NAME = "2B/camera-cond"
CAMERA_DIM = 1536  # 6 Pluecker channels x 16 x 16 pixels per token (8x VAE, 2x patch)


# ----------------------------------------------------------------------------- camera features
def reorder_source_first(x: torch.Tensor, dim: int = 1) -> torch.Tensor:
    """[source | target 0 | target 1] along `dim` (the order cameras arrive in the data batch) -> the latent time
    axis's [target 0 | source | target 1]: cat(chunks[1], chunks[0], chunks[2])
    (camera_conditioned_video2world_model_rectified_flow.py:186-187)."""
    if x.shape[dim] % 3:
        raise ValueError(f"{x.shape[dim]} entries along dim {dim} are not three equal segments")
    c = torch.chunk(x, 3, dim=dim)
    return torch.cat((c[1], c[0], c[2]), dim=dim)


def poses_for_latent_frames(per_pixel_frame: torch.Tensor, n_latent: Optional[int] = None) -> torch.Tensor:
    """Per-pixel-frame camera data [F_pix, ...] -> one entry per latent frame: latent frame t takes pixel frame 4 t
    (the causal VAE's latent frame t covers pixel frames 4 t - 3 .. 4 t, and frame 0 alone for t = 0). This build's
    own choice: the reference ships no such selection."""
    F_pix = per_pixel_frame.shape[0]
    T = 1 + (F_pix - 1) // 4 if n_latent is None else int(n_latent)
    if T < 1 or 4 * (T - 1) >= F_pix:
        raise ValueError(f"{F_pix} pixel frames do not cover {T} latent frames (needs frame {4 * (T - 1)})")
    return per_pixel_frame[0: 4 * (T - 1) + 1: 4]


def plucker_camera_rows(w2c: torch.Tensor, intrinsics: torch.Tensor, Hp: int, Wp: int) -> torch.Tensor:
    """Device tensors in, rows out (cp25_plucker_tokens): w2c [F, 3, 4] world-to-camera poses and intrinsics [F, 4]
    (fx, fy, cx, cy at the pixel size (16 Hp, 16 Wp)), one per latent frame -> [F * Hp * Wp, 1536] bf16, the rows
    MinimalV1LVGDiT.prepare_camera takes. The packing is this build's own (module docstring)."""
    if not w2c.is_cuda:
        raise RuntimeError("plucker_camera_rows runs on the GPU: pass device tensors")
    return N.plucker_tokens(w2c.float(), intrinsics.to(w2c.device).float(), int(Hp), int(Wp))


def camera_rows_from_trajectories(w2c: torch.Tensor, intrinsics: torch.Tensor, T_seg: int, Hp: int, Wp: int,
                                  device) -> torch.Tensor:
    """w2c [3, F_pix, 3, 4], intrinsics [3, F_pix, 4] in source, target 0, target 1 order -> the net's camera tensor
    [3 T_seg, Hp, Wp, 1536] bf16 in the same (arrival) order, one pose per latent frame."""
    if w2c.dim() != 4 or tuple(w2c.shape[0:1] + w2c.shape[2:]) != (3, 3, 4):
        raise ValueError(f"w2c must be [3, F_pix, 3, 4] (source, target 0, target 1), got {tuple(w2c.shape)}")
    if tuple(intrinsics.shape) != (3, w2c.shape[1], 4):
        raise ValueError(f"intrinsics must be [3, {w2c.shape[1]}, 4], got {tuple(intrinsics.shape)}")
    p = torch.stack([poses_for_latent_frames(w2c[s], T_seg) for s in range(3)]).reshape(3 * T_seg, 3, 4)
    k = torch.stack([poses_for_latent_frames(intrinsics[s], T_seg) for s in range(3)]).reshape(3 * T_seg, 4)
    rows = plucker_camera_rows(p.to(device), k.to(device), Hp, Wp)
    return rows.view(3 * T_seg, Hp, Wp, CAMERA_DIM)


# ----------------------------------------------------------------------------- public interface
class CameraInferenceArguments(pydantic.BaseModel):
    """One camera-conditioned sample. The reference has no inference script for this model; the fields follow
    InferenceArguments (config.py) and generate_samples_from_batch's defaults (guidance 1.5, 35 steps,
    camera_conditioned_video2world_model_rectified_flow.py:236-249)."""

    model_config = pydantic.ConfigDict(extra="forbid", frozen=True)

    name: str
    prompt: Optional[str] = None
    prompt_path: Optional[Path] = None
    negative_prompt: Optional[str] = None  # None: the zeroed text embedding of the conditioner's text dropout
    input_path: Path  # the source video (.mp4)
    # .npz with w2c [3, F_pix, 3, 4] and intrinsics [3, F_pix, 4] (fx, fy, cx, cy at the generation resolution), in
    # source, target 0, target 1 order
    cameras_path: Path
    seed: int = 1
    guidance: float = pydantic.Field(1.5, ge=0.0)
    num_steps: pydantic.PositiveInt = 35
    resolution: str = "none"
    num_conditional_frames: pydantic.NonNegativeInt = 1

    @pydantic.model_validator(mode="before")
    @classmethod
    def _prompt(cls, data: Any) -> Any:
        if isinstance(data, dict) and data.get("prompt") is None and data.get("prompt_path") is not None:
            data = dict(data)
            data["prompt"] = Path(data["prompt_path"]).read_text().strip()
        return data

    @pydantic.model_validator(mode="after")
    def _check(self):
        if self.prompt is None:
            raise ValueError("one of prompt / prompt_path is required")
        if self.input_path.suffix != ".mp4":
            raise ValueError(f"input_path has unsupported file extension '{self.input_path.suffix}'")
        if self.cameras_path.suffix != ".npz":
            raise ValueError(f"cameras_path must be an .npz file, got '{self.cameras_path.suffix}'")
        if self.resolution != "none":
            try:
                h, w = (int(v) for v in self.resolution.split(","))
            except ValueError:
                raise ValueError(f"resolution must be 'H,W' or 'none', got {self.resolution!r}") from None
            if h <= 0 or w <= 0 or h % 16 or w % 16:
                raise ValueError(f"resolution {self.resolution}: both sides must be positive multiples of 16")
        return self


def load_cameras(path) -> Tuple[torch.Tensor, torch.Tensor]:
    """cameras_path -> (w2c [3, F_pix, 3, 4], intrinsics [3, F_pix, 4]) fp32 host tensors."""
    with np.load(os.fspath(path)) as z:
        if "w2c" not in z or "intrinsics" not in z:
            raise ValueError(f"{path}: expected arrays 'w2c' and 'intrinsics', found {sorted(z.files)}")
        w2c, k = torch.from_numpy(z["w2c"].astype(np.float32)), torch.from_numpy(z["intrinsics"].astype(np.float32))
    if w2c.dim() != 4 or w2c.shape[0] != 3 or tuple(w2c.shape[2:]) != (3, 4) or tuple(k.shape) != (3, w2c.shape[1], 4):
        raise ValueError(f"{path}: w2c {tuple(w2c.shape)} / intrinsics {tuple(k.shape)}, expected [3, F_pix, 3, 4] / "
                         "[3, F_pix, 4]")
    return w2c, k


class CameraInference:
    """`generate(args)` over one pipeline object (tokenizer + the camera-conditioned net). `setup` is a
    config.SetupArguments (model "2B/camera-cond"); pipe_kwargs go to Video2WorldInference (net_cfg / sampler_cfg
    overrides for tests, ...)."""

    def __init__(self, setup, text_encoder=None, pipe=None, **pipe_kwargs):
        from .pipeline import Video2WorldInference

        torch.set_grad_enabled(False)
        self.setup_args = setup
        if pipe is None:
            if (setup.context_parallel_size or 1) > 1:
                raise ValueError("a camera-conditioned net combined with context parallelism is not built")
            pipe = Video2WorldInference(setup.model, ckpt_path=setup.checkpoint_path,
                                        tokenizer_path=setup.tokenizer_path, state_t=setup.state_t,
                                        text_encoder=text_encoder, pixel_path=setup.pixel_path,
                                        lora_path=setup.lora_path, lora_alpha=setup.lora_alpha,
                                        lora_scale=setup.lora_scale,
                                        text_encoder_path=getattr(setup, "text_encoder_path", None),
                                        text_tokenizer_path=getattr(setup, "text_tokenizer_path", None),
                                        offload_text_encoder=getattr(setup, "offload_text_encoder", False),
                                        **pipe_kwargs)
        self.pipe = pipe
        if not pipe.model.net_cfg.camera_dim:
            raise ValueError(f"CameraInference needs a camera-conditioned net (model {MODEL_NAME!r}), got "
                             f"{getattr(setup, 'model', None)!r}")

    # ------------------------------------------------------------------ the source clip
    def _source_video(self, input_path, hw: Tuple[int, int], frames: int) -> torch.Tensor:
        """uint8 [1, 3, frames, H, W]: the first `frames` frames of the source video (padded with the last), resized
        and centre-cropped; on the GPU under pixel_path="device"."""
        if isinstance(input_path, torch.Tensor):
            return input_path
        from .video_io import read_mp4

        v = torch.from_numpy(read_mp4(os.fspath(input_path)))  # [T, H, W, 3] uint8
        if v.shape[0] < frames:
            v = torch.cat([v, v[-1:].expand(frames - v.shape[0], -1, -1, -1)], 0)
        v = v[:frames]
        if self.pipe.pixel_path == "device":
            from .pixels import resize_input_device

            out = resize_input_device(v.to(self.pipe.device), hw, layout="THWC")  # [T, h, w, 3]
            return out.permute(3, 0, 1, 2).unsqueeze(0)
        from .pipeline import resize_input

        return resize_input(v.permute(0, 3, 1, 2), hw).permute(1, 0, 2, 3).unsqueeze(0)

    # ------------------------------------------------------------------ generation
    @torch.no_grad()
    def generate_videos(self, args: CameraInferenceArguments, input_video: Optional[torch.Tensor] = None,
                        cameras: Optional[Tuple[torch.Tensor, torch.Tensor]] = None,
                        camera_tensor: Optional[torch.Tensor] = None) -> List[torch.Tensor]:
        """-> the two target videos, uint8 [T_pix, H, W, 3] on the host. input_video (uint8 [1, 3, T, H, W]) and
        cameras ((w2c, intrinsics)) replace the files of args; camera_tensor [3 T_seg, Hp, Wp, 1536] in source,
        target 0, target 1 order replaces the Pluecker packing altogether (the reference's contract)."""
        from .net_config import VIDEO_RES_SIZE_INFO

        pipe = self.pipe
        model, dev = pipe.model, pipe.device
        if args.resolution == "none":
            h, w = VIDEO_RES_SIZE_INFO[model.config.resolution]["9,16"]
        else:
            h, w = (int(v) for v in args.resolution.split(","))
        Ts = model.config.state_t
        frames = model.tokenizer.get_pixel_num_frames(Ts)
        vid = self._source_video(args.input_path if input_video is None else input_video, (h, w), frames)
        if vid.dtype != torch.uint8 or tuple(vid.shape) != (1, 3, frames, h, w):
            raise ValueError(f"source video {vid.dtype} {tuple(vid.shape)}: expected uint8 [1, 3, {frames}, {h}, {w}]")
        Hp, Wp = h // 16, w // 16
        if camera_tensor is None:
            w2c, k = load_cameras(args.cameras_path) if cameras is None else cameras
            camera_tensor = camera_rows_from_trajectories(w2c, k, Ts, Hp, Wp, dev)
        ctx_c = pipe.text_encoder(args.prompt).to(dev, torch.bfloat16)
        if args.negative_prompt is None:
            ctx_u = torch.zeros_like(ctx_c)  # TextAttr dropout zeroes the embedding
        else:
            ctx_u = pipe.text_encoder(args.negative_prompt).to(dev, torch.bfloat16)
        lat0, lat1 = model.generate_camera_samples(ctx_c, ctx_u, camera_tensor, source_video=vid,
                                                   num_conditional_frames=args.num_conditional_frames,
                                                   guidance=args.guidance, seed=args.seed, num_steps=args.num_steps)
        out = []
        for lat in (lat0, lat1):
            if pipe.pixel_path == "device":
                out.append(model.tokenizer.decode_u8(lat, "THWC").cpu())
            else:
                v = model.decode(lat).float()[0]  # [3, T, H, W] in [-1, 1]
                out.append((((1.0 + v) / 2) * 255.0).clamp(0, 255).to(torch.uint8).permute(1, 2, 3, 0).cpu())
        return out

    def generate(self, args: CameraInferenceArguments, output_dir: Optional[Path] = None, **inputs):
        """The two target videos of one sample: written as <name>_target0.mp4 / <name>_target1.mp4 under output_dir
        (default: the setup's) and returned as their paths; output_dir=False returns the uint8 videos instead."""
        videos = self.generate_videos(args, **inputs)
        if output_dir is False:
            return videos
        from .video_io import write_mp4

        out_dir = Path(self.setup_args.output_dir if output_dir is None else output_dir)
        out_dir.mkdir(parents=True, exist_ok=True)
        (out_dir / f"{args.name}.json").write_text(args.model_dump_json())
        return [write_mp4(np.ascontiguousarray(v.numpy()), str(out_dir / f"{args.name}_target{i}.mp4"), fps=16)
                for i, v in enumerate(videos)]
