"""Video2WorldModelRectifiedFlow for MI355X: conditioning, CFG velocity and the UniPC sampling loop.

Reference: cosmos_predict2/_src/predict2/models/video2world_model_rectified_flow.py (denoise :77-138,
velocity_fn :140-212) and text2world_model_rectified_flow.py (generate_samples_from_batch :516-599,
_normalize_video_databatch_inplace :703-737, encode/decode :864-870).

Hot-loop layout (DESIGN.md "Sampler"): the latent state, the noise and the ground-truth latent live
in HBM in *patch layout* [tokens, 64] fp32 (token = (t, h/2, w/2), feature (p1 p2 C)); a context-
parallel rank owns a contiguous token range. One sampler step is
    patchify (HIP) -> DiT forward on the CFG batch [cond, uncond] (B = 2)
    -> GT-frame velocity replacement + CFG (HIP, reads the final layer's output in place)
    -> fused UniPC corrector/predictor update (HIP)
with the only inter-GPU traffic the K/V all-gather inside self-attention.

A model whose SamplerConfig.sampler is "dmd2" samples with the DMD2-distilled few-step student instead
(DistilledSamplingRun; reference: distill/models/video2world_model_distill_dmd2.py:421-492 and denoise_edm,
video2world_model_rectified_flow.py:214-346): TrigFlow preconditioning + patchify (HIP) -> one DiT forward at B = 1
-> x0 reconstruction + re-noising (HIP), four times, with no CFG and no solver history.

A "dmd2_stream" model is the causal / self-forcing action student, generated one latent frame at a time over a K/V
cache (StreamingRun, generate_streaming_video; reference: interactive/models/action_video2world_self_forcing.py:170-577).
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _native as N
from . import context_parallel as cpu
from . import trigflow
from .dit import ContextCache, Geometry, MinimalV1LVGDiT
from .net_config import DiTConfig, SamplerConfig
from .scheduler import FlowUniPCMultistepScheduler

NUM_CONDITIONAL_FRAMES_KEY = "num_conditional_frames"


def arch_invariant_rand(shape, dtype, device, seed: Optional[int] = None) -> torch.Tensor:
    """imaginaire/utils/misc.py:158-179: numpy RandomState noise, identical on every host."""
    rng = np.random.RandomState(seed)
    return torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(dtype=dtype, device=device)


def upload_async(t: torch.Tensor, device) -> torch.Tensor:
    """A host tensor on `device`, unchanged in dtype and value, without waiting for the device's earlier work: through
    pinned memory and a stream-ordered copy (a plain .to(device) of pageable memory synchronises the stream first)."""
    device = torch.device(device)
    if t.is_cuda or device.type != "cuda":
        return t.to(device)
    pinned = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    return pinned.copy_(t).to(device, non_blocking=True)


def to_patch_layout(x_C_T_H_W: torch.Tensor) -> torch.Tensor:
    """[C=16, T, H, W] -> [T*(H/2)*(W/2), 64] with feature (p1*2 + p2)*16 + c."""
    C, T, H, W = x_C_T_H_W.shape
    return x_C_T_H_W.reshape(C, T, H // 2, 2, W // 2, 2).permute(1, 2, 4, 3, 5, 0).reshape(-1, 4 * C).contiguous()


def from_patch_layout(xp: torch.Tensor, T: int, H: int, W: int) -> torch.Tensor:
    C = xp.shape[1] // 4
    return xp.view(T, H // 2, W // 2, 2, 2, C).permute(5, 0, 1, 3, 2, 4).reshape(C, T, H, W).contiguous()


class Video2WorldModelRectifiedFlow:
    """Inference model: `generate_samples_from_batch`, `denoise`, `encode`, `decode`."""

    def __init__(self, net_cfg: DiTConfig, sampler_cfg: SamplerConfig, tokenizer=None, device="cuda"):
        self.net_cfg = net_cfg
        self.config = sampler_cfg
        self.device = torch.device(device)
        self.net = MinimalV1LVGDiT(net_cfg, device=self.device)
        self.tokenizer = tokenizer
        self.sample_scheduler = FlowUniPCMultistepScheduler(num_train_timesteps=1000, shift=1)
        self.cp_group = None
        # replay each trajectory's DiT forward from a HIP graph after its first evaluation (SamplingRun; one GPU only):
        # for launch-bound shapes (config 5's 13-frame chunks), where the host's launch rate leaves the device idle
        self.hip_graph = False
        # "device": uint8 conditioning frames go through tokenizer.encode_u8 (Video2WorldInference(pixel_path=...))
        self.pixel_path = "host"

    # ------------------------------------------------------------------ plumbing
    def load_state_dict(self, sd: Dict[str, torch.Tensor], strict: bool = True, lora_alpha: Optional[float] = None,
                        lora_scale: float = 1.0):
        """A plain or peft-LoRA-layout checkpoint dict (MinimalV1LVGDiT.load_state_dict merges the adapters)."""
        self.net.load_state_dict(sd, strict=strict, lora_alpha=lora_alpha, lora_scale=lora_scale)

    def set_context_parallel_group(self, group) -> None:
        self.cp_group = group
        if self.tokenizer is not None and hasattr(self.tokenizer, "set_context_parallel_group"):
            self.tokenizer.set_context_parallel_group(group)
        if group is None:
            self.net.disable_context_parallel()
        else:
            self.net.enable_context_parallel(group)

    @torch.no_grad()
    def encode(self, state: torch.Tensor) -> torch.Tensor:
        return self.tokenizer.encode(state)

    @torch.no_grad()
    def decode(self, latent: torch.Tensor) -> torch.Tensor:
        return self.tokenizer.decode(latent)

    def _normalize_video(self, video: torch.Tensor) -> torch.Tensor:
        # uint8 -> [-1, 1] in bf16 arithmetic (text2world_model_rectified_flow.py:735-736)
        if video.dtype == torch.uint8:
            return video.to(device=self.device, dtype=torch.bfloat16) / 127.5 - 1.0
        return video.to(self.device)

    # ------------------------------------------------------------------ per-frame timesteps
    def _frame_timesteps(self, t: torch.Tensor, frame_mask: torch.Tensor) -> torch.Tensor:
        """denoise :109-122 -> [T] fp32 (cond frames -> conditional_frame_timestep)."""
        tf = t.to(torch.float32).expand(frame_mask.shape[0]).to(frame_mask.device)
        c = self.config.conditional_frame_timestep
        if c >= 0:
            tcond = torch.ones_like(frame_mask) * c
            tf = tcond * frame_mask + t.to(frame_mask.device) * (1 - frame_mask)
        return tf

    # ------------------------------------------------------------------ the sampler
    @torch.no_grad()
    def begin_sampling(self, gt: Optional[torch.Tensor], ctx_cond: torch.Tensor,
                       ctx_uncond: Optional[torch.Tensor], *,
                       state_shape, num_conditional_frames: int, guidance: float, seed: int, num_steps: int,
                       shift: float = 5.0, cfg_mode: Optional[str] = None, net_fn=None,
                       action: Optional[torch.Tensor] = None,
                       view_indices: Optional[torch.Tensor] = None,
                       init_noise: Optional[torch.Tensor] = None) -> "SamplingRun":
        """Set up one trajectory of the sampling loop (text2world_model_rectified_flow.py:556-582):
        noise, schedule, conditioning; SamplingRun.step() then runs one loop iteration (:584-594).
        A model whose config.sampler is "dmd2" returns the distilled student's DistilledSamplingRun instead (same
        interface): ctx_uncond, guidance, shift and cfg_mode are accepted and unused there (teacher guidance is
        distilled into the student: video2world_model_distill_dmd2.py:371), init_noise is that loop's own argument."""
        if self.config.sampler == "dmd2":
            if action is not None or view_indices is not None:
                raise ValueError("the distilled (dmd2) sampler serves the plain video2world student: no `action` "
                                 "and no `view_indices`")
            return DistilledSamplingRun(self, gt, ctx_cond, state_shape=state_shape,
                                        num_conditional_frames=num_conditional_frames, seed=seed,
                                        num_steps=num_steps, net_fn=net_fn, init_noise=init_noise)
        if self.config.sampler == "dmd2_stream":
            raise ValueError("the streaming (dmd2_stream) student generates frame by frame: generate_streaming_video / "
                             "StreamingRun, not the chunk sampler")
        if self.config.sampler != "unipc":
            raise ValueError(f"unknown SamplerConfig.sampler {self.config.sampler!r} ('unipc', 'dmd2' or "
                             "'dmd2_stream')")
        if init_noise is not None:
            raise ValueError("`init_noise` is the distilled (dmd2) sampler's argument")
        return SamplingRun(self, gt, ctx_cond, ctx_uncond, state_shape=state_shape,
                           num_conditional_frames=num_conditional_frames, guidance=guidance, seed=seed,
                           num_steps=num_steps, shift=shift, cfg_mode=cfg_mode, net_fn=net_fn, action=action,
                           view_indices=view_indices)

    @torch.no_grad()
    def sample_latents(self, gt: Optional[torch.Tensor], ctx_cond: torch.Tensor, ctx_uncond: torch.Tensor, *,
                       state_shape, num_conditional_frames: int, guidance: float, seed: int, num_steps: int,
                       shift: float = 5.0, cfg_mode: Optional[str] = None, progress=None,
                       net_fn=None, action: Optional[torch.Tensor] = None,
                       view_indices: Optional[torch.Tensor] = None,
                       init_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Core loop. gt: x0 latent [1, C, T, H, W] fp32 (or None when no frame is conditioned);
        ctx_*: text embeddings [1, Lctx, proj_in]. Returns latents [1, C, T, H, W] fp32.
        net_fn(rows [n,1,72] bf16, t_B_T [2,T] fp32, geo) -> [n,2,64] replaces the DiT (tests only).
        With config.sampler == "dmd2" this runs the distilled student's loop (DistilledSamplingRun: one branch, so
        net_fn sees t_B_T [1,T] and returns [n,1,64]; ctx_uncond may be None)."""
        run = self.begin_sampling(gt, ctx_cond, ctx_uncond, state_shape=state_shape,
                                  num_conditional_frames=num_conditional_frames, guidance=guidance, seed=seed,
                                  num_steps=num_steps, shift=shift, cfg_mode=cfg_mode, net_fn=net_fn,
                                  action=action, view_indices=view_indices, init_noise=init_noise)
        while not run.done:
            i = run.step()
            if progress is not None:
                progress(i, run.num_evals)
        return run.latents()

    @torch.no_grad()
    def generate_streaming_video(self, gt: torch.Tensor, ctx: torch.Tensor, actions: torch.Tensor, *,
                                 init_noise: Optional[torch.Tensor] = None, seed: int = 0, n_steps: int = 4,
                                 cache_frame_size: Optional[int] = None, net_fn=None) -> torch.Tensor:
        """The streaming action student's clip (StreamingRun): gt [1, C, T, H, W] whose frame 0 conditions the clip, ctx
        the text embedding [1, Lctx, proj_in], actions [1, (T - 1) * action_per_latent_frame, action_dim]; noise from
        init_noise [1, C, T, H, W] or arch_invariant_rand(seed); cache_frame_size None = the config's. Returns the
        latents [1, C, T, H, W] bf16 (interactive/models/action_video2world_self_forcing.py:449-577)."""
        if self.config.sampler != "dmd2_stream":
            raise ValueError(f"generate_streaming_video needs a 'dmd2_stream' sampler config, got "
                             f"{self.config.sampler!r}")
        run = StreamingRun(self, gt, ctx, actions, seed=seed, n_steps=n_steps, cache_frame_size=cache_frame_size,
                           net_fn=net_fn, init_noise=init_noise)
        while not run.done:
            run.next_frame()
        return run.latents()

    @torch.no_grad()
    def generate_streaming_video_batch(self, gt: torch.Tensor, ctx, actions: torch.Tensor, *,
                                       init_noise: Optional[torch.Tensor] = None, seed=0, n_steps: int = 4,
                                       cache_frame_size: Optional[int] = None, net_fn=None) -> torch.Tensor:
        """generate_streaming_video for B sessions in lock-step (StreamingBatchRun): gt [B, C, T, H, W], actions
        [B, (T - 1) * action_per_latent_frame, action_dim], one text context [1, Lctx, proj_in] for all, seed an int or B
        ints (or init_noise [B, C, T, H, W]). Returns the latents [B, C, T, H, W] bf16."""
        if self.config.sampler != "dmd2_stream":
            raise ValueError(f"generate_streaming_video_batch needs a 'dmd2_stream' sampler config, got "
                             f"{self.config.sampler!r}")
        run = StreamingBatchRun(self, gt, ctx, actions, seed=seed, n_steps=n_steps, cache_frame_size=cache_frame_size,
                                net_fn=net_fn, init_noise=init_noise)
        while not run.done:
            run.next_frame()
        return run.latents()

    @torch.no_grad()
    def generate_camera_samples(self, ctx_cond: torch.Tensor, ctx_uncond: torch.Tensor, camera: torch.Tensor, *,
                                source_video: Optional[torch.Tensor] = None,
                                source_latent: Optional[torch.Tensor] = None, num_conditional_frames: int = 1,
                                guidance: float = 1.5, seed: int = 1, num_steps: int = 35, shift: float = 5.0,
                                camera_cache: Optional[str] = None, net_fn=None, progress=None):
        """Camera-conditioned Video2World (CameraSamplingRun): the source clip as source_video [1, 3, T_pix, H, W]
        (uint8 or [-1, 1]; encoded whole by the tokenizer, camera_conditioned_video2world_model_rectified_flow.py:
        199-203) or as source_latent [1, C, T_seg, H, W]; camera the per-token features of the three clips in the
        order they arrive in the reference's data batch, [source | target 0 | target 1] along the frame axis
        ([3 T_seg, Hp, Wp, camera_dim], or with a leading batch dimension of 1), reordered here to the latent axis's
        [target 0 | source | target 1] (:186-188). Returns the (target 0, target 1) latents, [1, C, T_seg, H, W] fp32."""
        from .camera import reorder_source_first

        if (source_video is None) == (source_latent is None):
            raise ValueError("give exactly one of source_video / source_latent")
        if source_latent is None:
            if self.pixel_path == "device" and source_video.dtype == torch.uint8:
                source_latent = self.tokenizer.encode_u8(source_video.to(self.device))
            else:
                source_latent = self.encode(self._normalize_video(source_video))
        source_latent = source_latent.contiguous().float()
        _, C, Ts, H, W = source_latent.shape
        cam = camera[0] if camera.dim() == 5 and camera.shape[0] == 1 else camera
        if cam.dim() != 4 or tuple(cam.shape[:3]) != (3 * Ts, H // 2, W // 2):
            raise ValueError(f"camera {tuple(camera.shape)}: expected [{3 * Ts}, {H // 2}, {W // 2}, camera_dim] for "
                             f"three {Ts}-frame segments")
        cam = reorder_source_first(cam, dim=0)
        cache = None
        if net_fn is None:
            geo = Geometry(T=3 * Ts, Hp=H // 2, Wp=W // 2, tok0=0, n_tok=3 * Ts * (H // 2) * (W // 2))
            cache = self.net.prepare_camera(cam.to(self.device), geo, camera_cache)
        run = CameraSamplingRun(self, source_latent, ctx_cond, ctx_uncond, cache,
                                num_conditional_frames=num_conditional_frames, guidance=guidance, seed=seed,
                                num_steps=num_steps, shift=shift, net_fn=net_fn)
        while not run.done:
            i = run.step()
            if progress is not None:
                progress(i, run.num_evals)
        return run.target_latents()

    @torch.no_grad()
    def generate_samples_from_batch(self, data_batch: Dict, guidance: float = 1.5, seed: int = 1,
                                    state_shape=None, n_sample: Optional[int] = None,
                                    is_negative_prompt: bool = False, num_steps: int = 35, shift: float = 5.0,
                                    **kwargs) -> torch.Tensor:
        """text2world_model_rectified_flow.py:516-599 (+ the Video2World velocity_fn)."""
        run = self.begin_sampling_from_batch(data_batch, guidance=guidance, seed=seed, state_shape=state_shape,
                                             is_negative_prompt=is_negative_prompt, num_steps=num_steps, shift=shift)
        while not run.done:
            run.step()
        return run.latents()

    @torch.no_grad()
    def begin_sampling_from_batch(self, data_batch: Dict, guidance: float = 1.5, seed: int = 1, state_shape=None,
                                  is_negative_prompt: bool = False, num_steps: int = 35,
                                  shift: float = 5.0) -> "SamplingRun":
        """generate_samples_from_batch up to its loop: encode the conditioning frames (VAE), build the
        CFG contexts, noise and schedule; returns the steppable SamplingRun."""
        video = data_batch["video"]
        if state_shape is None:
            _T, _H, _W = video.shape[-3:]
            sc = self.tokenizer.spatial_compression_factor
            state_shape = [self.config.state_ch, self.tokenizer.get_latent_num_frames(_T), _H // sc, _W // sc]
        n_cond = data_batch.get(NUM_CONDITIONAL_FRAMES_KEY, 1)
        n_cond = int(n_cond.item()) if isinstance(n_cond, torch.Tensor) else int(n_cond)
        gt = None
        if n_cond > 0:
            gt = self.encode_conditioning(video, n_cond, state_shape[1])
        ctx_c = data_batch["t5_text_embeddings"]
        if self.config.sampler == "dmd2":
            # one branch, no CFG: no unconditional context is built or prepared (get_x0_fn_from_batch,
            # video2world_model_distill_dmd2.py:364-418, uses the condition alone)
            return self.begin_sampling(gt, ctx_c, None, state_shape=state_shape, num_conditional_frames=n_cond,
                                       guidance=guidance, seed=seed, num_steps=num_steps, shift=shift,
                                       action=data_batch.get("action"))
        if is_negative_prompt and isinstance(data_batch.get("neg_t5_text_embeddings"), torch.Tensor):
            ctx_u = data_batch["neg_t5_text_embeddings"]
        else:
            ctx_u = torch.zeros_like(ctx_c)  # TextAttr dropout (rate 0.2 > 0) zeroes the embedding
        # action-conditioned nets: the same action conditions both CFG branches (the conditioner's
        # action ReMapkey has no dropout: action/configs/action_conditioned/conditioner.py:222-233,272-275)
        return self.begin_sampling(gt, ctx_c, ctx_u, state_shape=state_shape, num_conditional_frames=n_cond,
                                   guidance=guidance, seed=seed, num_steps=num_steps, shift=shift,
                                   action=data_batch.get("action"))

    @torch.no_grad()
    def encode_conditioning(self, video: torch.Tensor, n_cond: int, T_lat: int) -> torch.Tensor:
        """x0 latent of the conditioning frames: [1, C, T_lat, H, W] fp32.

        The causal VAE makes latent frame j depend only on pixel frames <= 4j, so encoding the first
        1 + 4 (n_cond - 1) pixel frames yields the reference's first n_cond latent frames bit-for-bit;
        only those frames reach the output (mask-selected in denoise, video2world_model_rectified_flow.py
        :105-107 and :131-136). The remaining latent frames are zero-filled and never read."""
        px = 1 + 4 * (n_cond - 1)
        if self.pixel_path == "device" and video.dtype == torch.uint8:
            # uint8 straight into the encoder's clip (cp25_u8_to_clip): _normalize_video's arithmetic, no bf16 video
            lat = self.tokenizer.encode_u8(video[:, :, :px].to(self.device)).float()
        else:
            lat = self.encode(self._normalize_video(video[:, :, :px])).float()
        B, C, Tc, H, W = lat.shape
        gt = torch.zeros((B, C, T_lat, H, W), dtype=torch.float32, device=self.device)
        gt[:, :, :Tc] = lat
        return gt

    # ------------------------------------------------------------------ reference-compatible pieces
    @torch.no_grad()
    def denoise(self, noise: torch.Tensor, xt_B_C_T_H_W: torch.Tensor, timesteps_B_T: torch.Tensor,
                condition) -> torch.Tensor:
        """Video2WorldModelRectifiedFlow.denoise (:77-138) for one condition (API compatibility;
        the sampler itself runs the fused CFG-batched path). `condition` is a dict with keys
        gt_frames, condition_video_input_mask_B_C_T_H_W, crossattn_emb, padding_mask (optional)."""
        gt = condition["gt_frames"].to(xt_B_C_T_H_W)
        C = xt_B_C_T_H_W.shape[1]
        m = condition["condition_video_input_mask_B_C_T_H_W"].repeat(1, C, 1, 1, 1).type_as(xt_B_C_T_H_W)
        xt = gt * m + xt_B_C_T_H_W * (1 - m)
        if self.config.conditional_frame_timestep >= 0:
            mt = m.mean(dim=[1, 3, 4], keepdim=True)
            tc = torch.ones_like(mt) * self.config.conditional_frame_timestep
            timesteps_B_T = (tc * mt + timesteps_B_T.to(mt.device) * (1 - mt)).squeeze()
            timesteps_B_T = timesteps_B_T.unsqueeze(0) if timesteps_B_T.ndim == 1 else timesteps_B_T
        out = self.net(xt.to(torch.bfloat16), timesteps_B_T, condition["crossattn_emb"],
                       condition_video_input_mask_B_C_T_H_W=condition["condition_video_input_mask_B_C_T_H_W"],
                       padding_mask=condition.get("padding_mask")).float()
        if self.config.denoise_replace_gt_frames:
            out = (noise - gt.type_as(out)) * m + out * (1 - m)
        return out


class _TokenState:
    """What both sampling runs hold per trajectory: the token geometry and this rank's CP shard of it, the noise, the
    conditioning-frame mask and the ground-truth latent in patch layout, and the gather back to [1, C, T, H, W]."""

    def _setup_state(self, model: "Video2WorldModelRectifiedFlow", gt, state_shape, num_conditional_frames: int,
                     seed: int, init_noise: Optional[torch.Tensor] = None,
                     frame_mask: Optional[torch.Tensor] = None) -> None:
        """frame_mask [T]: an explicit conditioning-frame mask (the camera sampler's), instead of the first
        num_conditional_frames frames of every view."""
        self.model = model
        C, T, H, W = state_shape
        self.state_shape = (C, T, H, W)
        dev = model.device
        geo = Geometry(T=T, Hp=H // 2, Wp=W // 2, n_views=model.net.n_views_for(T))
        L = geo.L
        cp = model.cp_group
        rank, world = (0, 1) if cp is None else (torch.distributed.get_rank(cp), torch.distributed.get_world_size(cp))
        if L % world:
            raise ValueError(f"token count {L} not divisible by the context-parallel size {world}")
        if world > 1 and model.net.cfg.cross_view_attn_map:
            # cross-view nets shard by frame: every view's frames [rank Tl, (rank + 1) Tl) (Geometry.frame_shard)
            geo = Geometry.frame_shard(T, H // 2, W // 2, geo.n_views, rank, world)
            sl = geo.token_ids(dev)
        else:
            geo.n_tok = L // world
            geo.tok0 = rank * geo.n_tok
            sl = slice(geo.tok0, geo.tok0 + geo.n_tok)
        self.geo, self.cp, self.world = geo, cp, world

        if init_noise is None:
            noise_full = arch_invariant_rand((1, C, T, H, W), torch.float32, dev, seed)
        else:
            if tuple(init_noise.shape) != (1, C, T, H, W):
                raise ValueError(f"init_noise {tuple(init_noise.shape)} is not the state shape {(1, C, T, H, W)}")
            noise_full = init_noise.to(dev, torch.float32)
        self.noise = to_patch_layout(noise_full[0])[sl].contiguous()
        del noise_full
        explicit = frame_mask is not None
        if explicit:
            if frame_mask.numel() != T:
                raise ValueError(f"frame_mask has {frame_mask.numel()} entries for {T} latent frames")
            frame_mask = frame_mask.reshape(T).to(dev, torch.float32).contiguous()
        else:
            frame_mask = torch.zeros(T, dtype=torch.float32, device=dev)
        if not explicit and geo.T_view > 1 and num_conditional_frames > 0:
            # the first frames of every view (multi-view FIRST_RANDOM_N, predict2_multiview/configs/vid2vid/
            # defaults/conditioner.py:125-260; one view: video2world conditioner.py:45-143)
            for vi in range(geo.n_views):
                frame_mask[vi * geo.T_view: vi * geo.T_view + num_conditional_frames] = 1.0
        self.frame_mask = frame_mask
        # the per-token kernels (patchify, cfg_velocity) index the mask by (tok0 + token) // hw: a frame-sharded rank
        # passes its own frames' entries with tok0 = 0
        self.kmask = frame_mask if geo.frames is None else frame_mask[list(geo.frames)].contiguous()
        self.gtp = None
        if gt is not None and num_conditional_frames > 0:
            self.gtp = to_patch_layout(gt[0].to(dev, torch.float32))[sl].contiguous()

    @torch.no_grad()
    def latents(self) -> torch.Tensor:
        """The current latent state [1, C, T, H, W] fp32 (all-gathered over the CP group)."""
        x = self.x
        if self.world > 1:
            x = cpu.gather_tokens(x, self.cp)
            if self.geo.frames is not None:  # frame-sharded ranks: back to the global (view, frame, h, w) order
                C_, T_, H_, W_ = self.state_shape
                g = self.geo
                ids = torch.cat([Geometry.frame_shard(T_, g.Hp, g.Wp, g.n_views, r, self.world).token_ids(x.device)
                                 for r in range(self.world)])
                xg = torch.empty_like(x)
                xg[ids] = x
                x = xg
        _, T, H, W = self.state_shape
        return from_patch_layout(x, T, H, W).unsqueeze(0)


class SamplingRun(_TokenState):
    """One sampler trajectory of Video2WorldModelRectifiedFlow, advanced one evaluation at a time.

    Setup = text2world_model_rectified_flow.py:556-582 (noise, schedule, conditioning); step() = one
    iteration of the loop at :584-594 (patchify + frame replacement, the CFG-batched DiT forward,
    GT-frame velocity replacement + CFG, fused UniPC update); latents() = :596-599 (CP gather)."""

    def __init__(self, model: "Video2WorldModelRectifiedFlow", gt, ctx_cond, ctx_uncond, *, state_shape,
                 num_conditional_frames: int, guidance: float, seed: int, num_steps: int, shift: float = 5.0,
                 cfg_mode: Optional[str] = None, net_fn=None, action=None, view_indices=None,
                 init_noise: Optional[torch.Tensor] = None, frame_mask: Optional[torch.Tensor] = None, camera=None):
        """init_noise, frame_mask: the initial state and the conditioning-frame mask given explicitly (_setup_state);
        camera: the camera-conditioned net's dit.CameraCache, handed to every forward (CameraSamplingRun sets all
        three)."""
        self._setup_state(model, gt, state_shape, num_conditional_frames, seed, init_noise, frame_mask)
        dev, geo, world = model.device, self.geo, self.world
        if camera is not None and world > 1:
            raise ValueError("a camera-conditioned net combined with context parallelism is not built")
        self.camera = camera

        self.net_fn = net_fn
        self.ctx = None if net_fn is not None else model.net.prepare_context(torch.cat([ctx_cond, ctx_uncond], 0))
        self.mode = 0 if (cfg_mode or model.config.cfg_mode) == "video2world" else 1
        self.guidance = guidance
        # on the device once (a per-evaluation host copy would also be a pageable copy inside a HIP graph capture)
        self.action = None if action is None else action.to(dev)
        self.view_indices = view_indices
        self._sched_args = dict(num_inference_steps=num_steps, device=dev, shift=shift,
                                use_kerras_sigma=model.config.use_kerras_sigma_at_inference)
        # the run's own solver (configured like the model's sample_scheduler): its UniPC history must not be shared
        # with another live run, nor with a sample_latents call made while this run is alive
        base = model.sample_scheduler
        self.sched = FlowUniPCMultistepScheduler(base.num_train_timesteps, base.solver_order, base.config_shift)
        # HIP graph of the DiT forward (model.hip_graph): captured at the second evaluation, after the first one ran
        # eagerly and built every lazily made buffer (RoPE tables, bf16 weight copies), then replayed on static copies
        # of the two inputs that change per evaluation (patch rows, timesteps); the context, the action and every
        # weight stay the tensors the graph recorded. Not with CP (the K/V gathers run on their own streams), nor for a
        # net with sparse blocks (building a neighborhood plan copies host tables and synchronises), nor for camera runs
        # (out of scope).
        self._graphable = (bool(getattr(model, "hip_graph", False)) and net_fn is None and world == 1
                           and not getattr(model.net, "has_sparse_blocks", False) and camera is None)
        self._graph = None
        self.restart()

    def restart(self) -> None:
        """Back to the first timestep from the same noise (bench: more evaluations than one trajectory)."""
        sched = self.sched
        sched.set_timesteps(**self._sched_args)
        self.timesteps = sched.timesteps.cpu()
        self.x = sched.begin(self.noise)
        self.i = 0

    @property
    def num_evals(self) -> int:
        return len(self.timesteps)

    @property
    def done(self) -> bool:
        return self.i >= len(self.timesteps)

    @torch.no_grad()
    def step(self) -> int:
        """One sampler evaluation; returns its index in the schedule."""
        if self.done:
            raise RuntimeError("the trajectory is complete (restart() to run it again)")
        m, geo = self.model, self.geo
        t = self.timesteps[self.i]
        rows = N.patchify(self.x, self.gtp, self.kmask, None, tok0=geo.tok0, hw=geo.hw, ld=128)
        tf = m._frame_timesteps(t, self.frame_mask)  # [T]
        t_B_T = m.net.scale_timesteps(tf[None, :]).expand(2, geo.T).contiguous()
        if self.net_fn is None:
            # one t row expanded over the CFG pair, one action: the entries differ only in the text context
            shared = self.action is None or self.action.shape[0] == 1

            def forward(rows_, t_):
                return m.net.forward_tokens(rows_, t_, self.ctx, geo, action=self.action,
                                            view_indices=self.view_indices, shared_batch=shared, rows_k128=True,
                                            camera=self.camera)
            if self._graphable and self.i >= 1:
                # rows is the [n, 72] view of patchify's zero-padded [n, 128] buffer (rows_k128): the static copy
                # keeps that layout, pad columns included
                padded = torch.as_strided(rows, (rows.shape[0], rows.stride(0)), (rows.stride(0), 1))
                if self._graph is None:
                    self._g_buf, self._g_t = padded.clone(), t_B_T.clone()
                    self._g_rows = self._g_buf[:, :rows.shape[1]].view(geo.n_tok, 1, -1)
                    self._graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(self._graph):
                        self._g_out = forward(self._g_rows, self._g_t)
                self._g_buf.copy_(padded)
                self._g_t.copy_(t_B_T)
                self._graph.replay()
                net_out = self._g_out
            else:
                net_out = forward(rows.view(geo.n_tok, 1, -1), t_B_T)
        else:
            net_out = self.net_fn(rows.view(geo.n_tok, 1, -1), t_B_T, geo)
        v = N.cfg_velocity(net_out, self.noise, self.gtp, self.kmask, self.guidance, self.mode,
                           tok0=geo.tok0, hw=geo.hw)
        del net_out
        self.sched.step_(v, t)
        self.i += 1
        return self.i - 1


def camera_frame_mask(T: int, num_conditional_frames: int) -> torch.Tensor:
    """set_camera_conditioned_video_condition (camera/configs/camera_conditioned/conditioner.py:42-68): ones on
    latent frames [n, 2n) of the whole three-segment time axis, the literal rule for any n (an image batch, T == 1,
    conditions nothing) -> [T] fp32."""
    m = torch.zeros(T, dtype=torch.float32)
    if T > 1:
        n = int(num_conditional_frames)
        m[n: 2 * n] += 1
    return m


class CameraSamplingRun(SamplingRun):
    """One trajectory of the camera-conditioned Video2World model: one source clip and two target camera trajectories
    in, two re-rendered clips out (CameraConditionedVideo2WorldModelRectifiedFlow.generate_samples_from_batch and
    get_velocity_fn_from_batch, camera/models/camera_conditioned_video2world_model_rectified_flow.py:155-327).

    The latent time axis is three equal segments [target 0 | source | target 1] (:296):
        gt = cat(0, source latent, 0) (:205); the mask is 1 on frames [n, 2n), n = num_conditional_frames
        (camera_frame_mask); the initial state and denoise's `noise` are both cat(noise, source latent, noise), the two
        target segments drawing the same seeded noise (:286-296); CFG cond + g (cond - uncond) (:230); timesteps
        set_timesteps(num_steps, shift=shift), no Karras sigmas (:301); the UniPC step runs on all frames (:316-319).
    Everything per evaluation is SamplingRun.step(): the patchify / cfg_velocity / UniPC kernels index the per-frame
    mask as given. camera: the net's CameraCache over the 3 T_seg frames in the segment order above (the same in both
    CFG branches: the conditioner's camera key has dropout 0), or None with a stub net_fn.
    source_latent [1, C, T_seg, H, W]. target_latents() = chunk(latents, 3, dim=2)[0] and [2] (:324-325)."""

    def __init__(self, model: "Video2WorldModelRectifiedFlow", source_latent: torch.Tensor, ctx_cond, ctx_uncond,
                 camera=None, *, num_conditional_frames: int = 1, guidance: float = 1.5, seed: int = 1,
                 num_steps: int = 35, shift: float = 5.0, net_fn=None):
        if model.config.sampler != "unipc":
            raise ValueError(f"the camera sampler runs the rectified-flow UniPC loop, not {model.config.sampler!r}")
        if model.config.use_kerras_sigma_at_inference:
            raise ValueError("the camera sampler's schedule has no Karras sigmas "
                             "(use_kerras_sigma_at_inference must be False)")
        if source_latent.dim() != 5 or source_latent.shape[0] != 1:
            raise ValueError(f"source_latent must be [1, C, T, H, W], got {tuple(source_latent.shape)}")
        if net_fn is None and camera is None:
            raise ValueError("the camera sampler needs `camera` (MinimalV1LVGDiT.prepare_camera)")
        dev = model.device
        _, C, Ts, H, W = source_latent.shape
        x0 = source_latent.to(dev, torch.float32)
        zeros = torch.zeros_like(x0)
        noise = arch_invariant_rand((1, C, Ts, H, W), torch.float32, dev, seed)
        super().__init__(model, torch.cat([zeros, x0, zeros], dim=2), ctx_cond, ctx_uncond,
                         state_shape=(C, 3 * Ts, H, W), num_conditional_frames=num_conditional_frames,
                         guidance=guidance, seed=seed, num_steps=num_steps, shift=shift, cfg_mode="video2world",
                         net_fn=net_fn, init_noise=torch.cat([noise, x0, noise], dim=2),
                         frame_mask=camera_frame_mask(3 * Ts, num_conditional_frames), camera=camera)

    @torch.no_grad()
    def target_latents(self):
        """(target 0, target 1) latents, [1, C, T_seg, H, W] fp32 each."""
        chunks = torch.chunk(self.latents(), 3, dim=2)
        return chunks[0], chunks[2]


class DistilledSamplingRun(_TokenState):
    """One trajectory of the DMD2-distilled few-step student (config.sampler == "dmd2"), SamplingRun's interface.

    Setup and loop = Video2WorldModelDistillDMD2TrigFlow.generate_samples_from_batch (distill/models/
    video2world_model_distill_dmd2.py:421-492) around denoise_edm with net_type "student" (models/
    video2world_model_rectified_flow.py:214-346). The times are selected_sampling_time[:num_steps] + [0] (:482-484),
    so num_steps = 35 runs all four. One step() at time t_cur is
        trig_patchify (HIP): xt * c_in, conditioning frames gt / sigma_data, the net-dtype cast, the patch rows
        -> one DiT forward at B = 1 on the text context alone (no CFG: the teacher's guidance is distilled in, :371)
        -> trig_x0_step (HIP): x0 = c_skip xt + c_out net, GT frames replaced, then the re-noising
           cos(t_next) x0 / sigma_data + sin(t_next) noise, or nan_to_num(x0) once t_next <= 1e-5.
    The reference holds the state in float64 between the steps and enters the denoiser with x.float() (:486); here
    the state is that fp32 tensor and the kernels do the float64 arithmetic. The per-frame float64 tables (trigflow.py)
    are a few numbers per step, made on the host when the run is set up.
    Noise: `init_noise` [1, C, T, H, W] as the reference's argument, else this build's arch_invariant_rand(seed) (the
    reference draws from a device torch.Generator, whose stream is not portable: DESIGN.md §4).
    model.hip_graph is not used: four evaluations are not launch-bound."""

    def __init__(self, model: "Video2WorldModelRectifiedFlow", gt, ctx, *, state_shape, num_conditional_frames: int,
                 seed: int, num_steps: int, net_fn=None, init_noise: Optional[torch.Tensor] = None):
        cfg = model.config
        times = trigflow.step_times(cfg.selected_sampling_time, num_steps)
        self._setup_state(model, gt, state_shape, num_conditional_frames, seed, init_noise)
        dev, geo = model.device, self.geo
        self.net_fn = net_fn
        self.ctx = None if net_fn is not None else model.net.prepare_context(ctx)
        self.replace_gt = bool(cfg.denoise_replace_gt_frames)
        self.sigma_data = float(cfg.sigma_data)
        mask_host = self.frame_mask.cpu()
        own = None if geo.frames is None else list(geo.frames)  # a frame-sharded rank's rows of the tables (kmask)
        self.steps = []
        for t_cur, t_next in zip(times[:-1], times[1:]):
            tf = trigflow.frame_times(t_cur, mask_host, cfg.sigma_conditional, cfg.sigma_data)
            c_skip, c_out, c_in, c_noise = trigflow.trig_scaling(tf, cfg.trig_scaling, cfg.sigma_data)
            if cfg.change_time_embed:
                c_noise = tf
            tabs = [c if own is None else c[own].contiguous() for c in (c_skip, c_out, c_in)]
            cos_next, sin_next, last = trigflow.renoise_scalars(t_next)
            self.steps.append(dict(c_skip=tabs[0].to(dev), c_out=tabs[1].to(dev), c_in=tabs[2].to(dev),
                                   t_B_T=trigflow.net_timesteps(c_noise, model.net_cfg.timestep_scale).to(dev),
                                   cos_next=cos_next, sin_next=sin_next, last=last))
        self.restart()

    def restart(self) -> None:
        """Back to the first time from the same noise."""
        self.x = self.noise.clone()
        self.i = 0

    @property
    def num_evals(self) -> int:
        return len(self.steps)

    @property
    def done(self) -> bool:
        return self.i >= len(self.steps)

    @torch.no_grad()
    def step(self) -> int:
        """One student evaluation and its state update; returns its index."""
        if self.done:
            raise RuntimeError("the trajectory is complete (restart() to run it again)")
        m, geo, s = self.model, self.geo, self.steps[self.i]
        rows = N.trig_patchify(self.x, self.gtp, self.kmask, s["c_in"], self.sigma_data, None, tok0=geo.tok0,
                               hw=geo.hw, ld=128)
        if self.net_fn is None:
            net_out = m.net.forward_tokens(rows.view(geo.n_tok, 1, -1), s["t_B_T"], self.ctx, geo, rows_k128=True)
        else:
            net_out = self.net_fn(rows.view(geo.n_tok, 1, -1), s["t_B_T"], geo)
        N.trig_x0_step(self.x, net_out.contiguous(), self.noise, self.gtp, self.kmask, s["c_skip"], s["c_out"],
                       replace_gt=self.replace_gt, sigma_data=self.sigma_data, cos_next=s["cos_next"],
                       sin_next=s["sin_next"], last=s["last"], tok0=geo.tok0, hw=geo.hw)
        del net_out
        self.i += 1
        return self.i - 1


class StreamingRun:
    """The causal / self-forcing action student, one latent frame at a time over a K/V cache (config.sampler ==
    "dmd2_stream"): ActionVideo2WorldModelRFSelfForcingDMD2.generate_streaming_video / generate_next_frame around
    denoise_edm_seq (interactive/models/action_video2world_self_forcing.py:449-577, 383-447, 170-227).

        prefill(): the start_idx = 1 conditioning frame at t = 0, stored in the cache, no action (:499-527)
        next_frame(): n_steps evaluations at selected_sampling_time[:n_steps] from the frame's noise, not stored
                      (:416-444), then one store pass at t = 0 on the predicted frame with the frame's actions (:546-575)
    One evaluation is stream_patchify (HIP: x * c_in in bf16, the patch rows) -> forward_frame at B = 1 over the cache
    -> stream_x0_step (HIP: x0 = c_skip x + c_out net and the re-noising, bf16 op by op). The state, the noise and the
    latents are bf16, as the reference casts them to the net dtype (:457, inference/action_video2world_streaming.py:256);
    the per-evaluation scalars are a few bf16 values made on the host (trigflow.stream_scaling / stream_renoise).
    The condition mask is all zeros in this loop (:514-516, :558-560), so t_cond never shows; the arithmetic that would
    apply it is kept (stream_scaling).
    actions=None builds a closed-loop run: next_frame(action) then takes each generated frame's [1, per, dim] actions
    when the frame is run, and nothing else changes (a frame never reads a later frame's actions).
    net_fn(rows [hw, 1, 72] bf16, t_B_1 [1, 1] fp32, geo, frame_idx, action [1, per, dim] | None, store) -> [hw, 1, 64]
    fp32 replaces forward_frame (tests only)."""

    def __init__(self, model: "Video2WorldModelRectifiedFlow", gt: torch.Tensor, ctx, actions: Optional[torch.Tensor], *,
                 seed: int = 0, n_steps: int = 4, cache_frame_size: Optional[int] = None, net_fn=None,
                 init_noise: Optional[torch.Tensor] = None):
        cfg, ncfg, dev = model.config, model.net_cfg, model.device
        times = [float(t) for t in cfg.selected_sampling_time]
        if not 1 <= n_steps <= len(times):  # :453-455
            raise ValueError(f"n_steps must be in 1 .. {len(times)} (the student schedule), got {n_steps}")
        if gt.dim() != 5 or gt.shape[0] != 1:
            raise ValueError(f"gt must be the [1, C, T, H, W] conditioning latent, got {tuple(gt.shape)}")
        _, C, T, H, W = gt.shape
        per = ncfg.action_per_latent_frame
        if not per or (actions is not None and (actions.dim() != 3 or actions.shape[1] != (T - 1) * per
                                                or actions.shape[2] != ncfg.action_dim)):
            raise ValueError(f"actions must be [1, {(T - 1) * max(per, 1)}, {ncfg.action_dim}] for {T} latent frames "
                             f"of a per-latent-frame action net, got {None if actions is None else tuple(actions.shape)}")
        self.model, self.net_fn, self.n_steps = model, net_fn, n_steps
        self.B = 1
        self.state_shape = (C, T, H, W)
        self.geo = Geometry(T=T, Hp=H // 2, Wp=W // 2, tok0=0, n_tok=T * (H // 2) * (W // 2))
        hw = self.geo.hw
        if init_noise is None:
            init_noise = arch_invariant_rand((1, C, T, H, W), torch.float32, dev, seed)
        elif tuple(init_noise.shape) != (1, C, T, H, W):
            raise ValueError(f"init_noise {tuple(init_noise.shape)} is not the state shape {(1, C, T, H, W)}")
        bf = torch.bfloat16
        self.noise = to_patch_layout(init_noise[0].to(dev, bf)).view(T, hw, 64)  # init_noise.to(**tensor_kwargs)
        self.out = torch.zeros((T, hw, 64), dtype=bf, device=dev)  # output_latents, patch layout
        self.out[0] = to_patch_layout(gt[0, :, :1].to(dev, bf))
        self.actions = None if actions is None else actions.to(dev).view(actions.shape[0], T - 1, per, ncfg.action_dim)
        self.action_shape = (1, per, ncfg.action_dim)
        F = cfg.cache_frame_size if cache_frame_size is None else cache_frame_size
        if F == 0 or F < -1:
            raise ValueError(f"cache_frame_size must be -1 (the whole clip) or positive, got {F}")
        # a frame attends to at most T - 1 earlier ones, so that many slots serve -1 (the reference sizes T) and above
        self.cache_frames = T - 1 if F == -1 else min(F, T - 1)
        self.cache = None
        self.ctx = None
        if net_fn is None:
            # the text context's per-block K / V: a ContextCache made once by the caller, or made here
            self.ctx = ctx if isinstance(ctx, ContextCache) else model.net.prepare_context(ctx)
            self.cache = model.net.make_kv_cache(1, self.cache_frames, hw)
        sc = lambda t: trigflow.stream_scaling(t, 0.0, cfg.trig_scaling, cfg.sigma_data, cfg.sigma_conditional)  # noqa: E731
        self.sigma_data = float(cfg.sigma_data)
        self.steps = []
        for s in range(n_steps):
            c_skip, c_out, c_in, c_noise = sc(times[s])
            last = s == n_steps - 1
            cos_n, sin_n = (0.0, 0.0) if last else trigflow.stream_renoise(times[s + 1])
            self.steps.append(dict(c_skip=c_skip, c_out=c_out, c_in=c_in, cos_next=cos_n, sin_next=sin_n, last=last,
                                   t_B_1=trigflow.net_timesteps(c_noise, ncfg.timestep_scale).to(dev)))
        _, _, c_in0, c_noise0 = sc(0.0)
        self.store_step = dict(c_in=c_in0, t_B_1=trigflow.net_timesteps(c_noise0, ncfg.timestep_scale).to(dev))
        self.frame = 0  # the next frame to run: 0 = the prefill

    @property
    def done(self) -> bool:
        return self.frame >= self.geo.T

    def _net(self, x: torch.Tensor, step: dict, frame: int, action, store: bool) -> torch.Tensor:
        rows = N.stream_patchify(x, step["c_in"], 0.0, None, ld=128).view(self.geo.hw, 1, -1)
        if self.net_fn is not None:
            return self.net_fn(rows, step["t_B_1"], self.geo, frame, action, store)
        return self.model.net.forward_frame(rows, step["t_B_1"], self.ctx, self.geo, frame, action, store,
                                            cache=self.cache, rows_k128=True)

    @torch.no_grad()
    def next_frame(self, action: Optional[torch.Tensor] = None) -> int:
        """Run the next frame (the first call: the conditioning frame's prefill); returns its index. A run built with
        actions=None takes the frame's [1, per, dim] actions here, for every frame after the prefill."""
        if self.done:
            raise RuntimeError("every frame of the clip has been generated")
        f = self.frame
        action = _frame_action(self, f, action)
        if f == 0:
            self._net(self.out[0], self.store_step, 0, None, True)
        else:
            x = self.noise[f]
            for s in self.steps:
                net_out = self._net(x, s, f, action, False)
                x = N.stream_x0_step(x, net_out.contiguous(), self.noise[f], c_skip=s["c_skip"], c_out=s["c_out"],
                                     cos_next=s["cos_next"], sin_next=s["sin_next"], sigma_data=self.sigma_data,
                                     last=s["last"], out=self.out[f] if s["last"] else None)
            self._net(self.out[f], self.store_step, f, action, True)
        self.frame += 1
        return f

    @torch.no_grad()
    def latents(self) -> torch.Tensor:
        """output_latents [1, C, T, H, W] bf16 (frames not yet generated are zero, as the reference initialises them)."""
        _, T, H, W = self.state_shape
        return from_patch_layout(self.out.view(-1, 64), T, H, W).unsqueeze(0)

    def frame_rows(self, f: int) -> torch.Tensor:
        """The [hw, 1, 64] bf16 state rows of frame f (the prefill's or a generated one), as cp25_stream_latent_clip
        takes them: a view of the run's latents."""
        return _frame_rows(self, f)


def _frame_action(run, f: int, action: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """The actions of frame f of a streaming run: the slice of the run's action array, or, for a run built with
    actions=None, the `action` [B, per, dim] given to next_frame (none for the prefill, f = 0)."""
    if run.actions is not None:
        if action is not None:
            raise ValueError("this run was built with its action array; next_frame() takes no action")
        return run.actions[:, f - 1] if f else None
    if f == 0:
        if action is not None:
            raise ValueError("the prefill (the first next_frame) takes no action")
        return None
    if action is None:
        raise ValueError(f"a run built with actions=None takes frame {f}'s actions {run.action_shape} in next_frame")
    if not isinstance(action, torch.Tensor) or tuple(action.shape) != run.action_shape:
        got = tuple(action.shape) if isinstance(action, torch.Tensor) else type(action).__name__
        raise ValueError(f"frame {f}'s actions must be a {run.action_shape} tensor, got {got}")
    return action.to(run.model.device)


def _frame_rows(run, f: int) -> torch.Tensor:
    if not 0 <= f < run.frame:
        raise ValueError(f"frame {f} has not been run ({run.frame} of {run.geo.T} frames so far)")
    return run.out[f].view(run.geo.hw, run.B, 64)


MAX_STREAM_BATCH = 16


def session_seeds(seed, B: int) -> List[int]:
    """The per-session noise seeds of a batch of B streaming sessions: an int gives every session that seed (each then
    draws what the one-session run draws with it), a sequence must hold B ints."""
    if isinstance(seed, (int, np.integer)):
        return [int(seed)] * B
    seeds = [int(s) for s in seed]
    if len(seeds) != B:
        raise ValueError(f"{len(seeds)} seeds for {B} sessions")
    return seeds


class StreamingBatchRun:
    """B independent sessions of StreamingRun in lock-step: every session is at the same frame, and one forward_frame
    over a K/V ring of batch B serves them all (parallel action rollouts from B conditioning frames under B action
    sequences). gt [B, C, T, H, W], actions [B, (T - 1) * per, dim], one text context for all sessions; seed an int
    (every session draws StreamingRun(seed=seed)'s noise) or B ints (session b draws StreamingRun(seed=seed[b])'s:
    arch_invariant_rand((1, C, T, H, W), ..., seed_b)), or init_noise [B, C, T, H, W].
    The state, the noise and the latents stay token-major, [T, hw, B, 64] bf16: stream_patchify and stream_x0_step are
    elementwise over rows, so they run on the hw * B rows of a frame unchanged, and the patch rows come out as the
    [hw, B, 72] forward_frame takes. The text context's per-block K / V are made once for one entry and replicated B
    times (ContextCache of batch B). Session b computes what StreamingRun computes for its inputs; which launches keep
    its bits at B > 1 is in DESIGN.md §6e.
    actions=None builds a closed-loop run: next_frame(action) then takes each generated frame's [B, per, dim] actions
    when the frame is run (StreamingRun), and frame_rows(f) hands a finished frame to the decoder without a copy.
    net_fn(rows [hw, B, 72], t_B_1 [B, 1], geo, frame_idx, action [B, per, dim] | None, store) -> [hw, B, 64] fp32
    replaces forward_frame (tests only)."""

    def __init__(self, model: "Video2WorldModelRectifiedFlow", gt: torch.Tensor, ctx, actions: Optional[torch.Tensor], *,
                 seed=0, n_steps: int = 4, cache_frame_size: Optional[int] = None, net_fn=None,
                 init_noise: Optional[torch.Tensor] = None):
        cfg, ncfg, dev = model.config, model.net_cfg, model.device
        times = [float(t) for t in cfg.selected_sampling_time]
        if not 1 <= n_steps <= len(times):
            raise ValueError(f"n_steps must be in 1 .. {len(times)} (the student schedule), got {n_steps}")
        if gt.dim() != 5:
            raise ValueError(f"gt must be the [B, C, T, H, W] conditioning latents, got {tuple(gt.shape)}")
        B, C, T, H, W = gt.shape
        if not 1 <= B <= MAX_STREAM_BATCH:
            raise ValueError(f"a batch of {B} sessions: 1 .. {MAX_STREAM_BATCH} run in one forward")
        per = ncfg.action_per_latent_frame
        if not per or (actions is not None and (actions.dim() != 3 or actions.shape[0] != B
                                                or actions.shape[1] != (T - 1) * per
                                                or actions.shape[2] != ncfg.action_dim)):
            raise ValueError(f"actions must be [{B}, {(T - 1) * max(per, 1)}, {ncfg.action_dim}] for {B} sessions of {T} "
                             f"latent frames of a per-latent-frame action net, got "
                             f"{None if actions is None else tuple(actions.shape)}")
        self.model, self.net_fn, self.n_steps, self.B = model, net_fn, n_steps, B
        self.state_shape = (C, T, H, W)
        self.geo = Geometry(T=T, Hp=H // 2, Wp=W // 2, tok0=0, n_tok=T * (H // 2) * (W // 2))
        hw = self.geo.hw
        bf = torch.bfloat16
        if init_noise is None:
            # drawn on the host as arch_invariant_rand draws it, uploaded without a stream synchronise (a closed-loop
            # session builds a run per chunk inside its step)
            noise = [upload_async(arch_invariant_rand((1, C, T, H, W), torch.float32, "cpu", s)[0], dev)
                     for s in session_seeds(seed, B)]
        elif tuple(init_noise.shape) != (B, C, T, H, W):
            raise ValueError(f"init_noise {tuple(init_noise.shape)} is not the state shape {(B, C, T, H, W)}")
        else:
            noise = [init_noise[b] for b in range(B)]
        # [T, hw, B, 64]: session b's rows are StreamingRun's, interleaved per token
        self.noise = torch.stack([to_patch_layout(n.to(dev, bf)).view(T, hw, 64) for n in noise], dim=2).contiguous()
        self.out = torch.zeros((T, hw, B, 64), dtype=bf, device=dev)
        self.out[0] = torch.stack([to_patch_layout(gt[b, :, :1].to(dev, bf)) for b in range(B)], dim=1)
        self.actions = None if actions is None else actions.to(dev).view(B, T - 1, per, ncfg.action_dim)
        self.action_shape = (B, per, ncfg.action_dim)
        F = cfg.cache_frame_size if cache_frame_size is None else cache_frame_size
        if F == 0 or F < -1:
            raise ValueError(f"cache_frame_size must be -1 (the whole clip) or positive, got {F}")
        self.cache_frames = T - 1 if F == -1 else min(F, T - 1)
        self.cache = None
        self.ctx = None
        if net_fn is None:
            self.ctx = self.batch_context(model, ctx, B)
            self.cache = model.net.make_kv_cache(B, self.cache_frames, hw)
        sc = lambda t: trigflow.stream_scaling(t, 0.0, cfg.trig_scaling, cfg.sigma_data, cfg.sigma_conditional)  # noqa: E731
        self.sigma_data = float(cfg.sigma_data)

        def t_rows(c_noise):  # one time for every session
            return upload_async(trigflow.net_timesteps(c_noise, ncfg.timestep_scale), dev).expand(B, 1).contiguous()

        self.steps = []
        for s in range(n_steps):
            c_skip, c_out, c_in, c_noise = sc(times[s])
            last = s == n_steps - 1
            cos_n, sin_n = (0.0, 0.0) if last else trigflow.stream_renoise(times[s + 1])
            self.steps.append(dict(c_skip=c_skip, c_out=c_out, c_in=c_in, cos_next=cos_n, sin_next=sin_n, last=last,
                                   t_B_1=t_rows(c_noise)))
        _, _, c_in0, c_noise0 = sc(0.0)
        self.store_step = dict(c_in=c_in0, t_B_1=t_rows(c_noise0))
        self.frame = 0

    @staticmethod
    def batch_context(model, ctx, B: int) -> ContextCache:
        """The text context of B sessions: one entry's per-block K / V (a [1, Lctx, proj_in] embedding, projected here,
        or a batch-1 ContextCache made once by the caller) replicated B times; a ContextCache of batch B passes."""
        if isinstance(ctx, ContextCache) and ctx.B == B:
            return ctx
        one = ctx if isinstance(ctx, ContextCache) else model.net.prepare_context(ctx)
        if one.B != 1:
            raise ValueError(f"one text context serves every session; got a context of batch {one.B} for {B} sessions")
        return ContextCache(B=B, k=[k.expand(B, -1, -1, -1).contiguous() for k in one.k],
                            v=[v.expand(B, -1, -1, -1).contiguous() for v in one.v])

    @property
    def done(self) -> bool:
        return self.frame >= self.geo.T

    def _net(self, x: torch.Tensor, step: dict, frame: int, action, store: bool) -> torch.Tensor:
        hw, B = self.geo.hw, self.B
        rows = N.stream_patchify(x.view(hw * B, 64), step["c_in"], 0.0, None, ld=128).view(hw, B, -1)
        if self.net_fn is not None:
            return self.net_fn(rows, step["t_B_1"], self.geo, frame, action, store)
        return self.model.net.forward_frame(rows, step["t_B_1"], self.ctx, self.geo, frame, action, store,
                                            cache=self.cache, rows_k128=True)

    @torch.no_grad()
    def next_frame(self, action: Optional[torch.Tensor] = None) -> int:
        """Run every session's next frame (the first call: the conditioning frames' prefill); returns its index. A run
        built with actions=None takes the frame's [B, per, dim] actions here, for every frame after the prefill."""
        if self.done:
            raise RuntimeError("every frame of the clip has been generated")
        f, n = self.frame, self.geo.hw * self.B
        action = _frame_action(self, f, action)
        if f == 0:
            self._net(self.out[0], self.store_step, 0, None, True)
        else:
            noise = self.noise[f].view(n, 64)
            x = noise
            for s in self.steps:
                net_out = self._net(x, s, f, action, False)
                x = N.stream_x0_step(x, net_out.contiguous(), noise, c_skip=s["c_skip"], c_out=s["c_out"],
                                     cos_next=s["cos_next"], sin_next=s["sin_next"], sigma_data=self.sigma_data,
                                     last=s["last"], out=self.out[f].view(n, 64) if s["last"] else None)
            self._net(self.out[f], self.store_step, f, action, True)
        self.frame += 1
        return f

    @torch.no_grad()
    def latents(self) -> torch.Tensor:
        """output_latents [B, C, T, H, W] bf16 (frames not yet generated are zero)."""
        _, T, H, W = self.state_shape
        return torch.stack([from_patch_layout(self.out[:, :, b].reshape(-1, 64), T, H, W) for b in range(self.B)], 0)

    def frame_rows(self, f: int) -> torch.Tensor:
        """The [hw, B, 64] bf16 state rows of frame f (the prefill's or a generated one), as cp25_stream_latent_clip
        takes them: a view of the run's latents."""
        return _frame_rows(self, f)
