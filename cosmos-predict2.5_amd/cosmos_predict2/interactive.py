"""Streaming action-conditioned generation with the causal / self-forcing student on MI355X.

Mirrors the reference's ActionStreamingInference (cosmos_predict2/_src/predict2/interactive/inference/
action_video2world_streaming.py:90-313): an action sequence is cut into chunks of 12; each chunk conditions on one
frame (the input frame, then the previous chunk's last decoded frame re-quantised to uint8), generates the chunk's
T = 4 latent frames one at a time over a K/V cache (model.StreamingRun, a few student steps per frame, no CFG), decodes
them and contributes the 12 frames after the conditioning one. The noise seed is seed + chunk and the cache is rebuilt per
chunk.

Closed-loop use (ActionSession, `open_session`): the same chunk rules driven one latent frame at a time: 4 actions in,
their 4 decoded frames out, so that a policy can pick its next actions from the frames it has just seen.

The text embedding is an input tensor: the reference loads an empty-string embedding file (:130-148).
Differences: the input frame is resized by this build's resize_input, not mediapy's; the frame arrives
as an array or an image path, not as a video file whose frame 0 is read.
"""
from __future__ import annotations

import os
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .model import MAX_STREAM_BATCH, StreamingBatchRun, StreamingRun, session_seeds, upload_async
from .pipeline import _IMAGE_EXTENSIONS, Video2WorldInference, resize_input

MODEL_NAME = "2B/robot/action-cond/streaming"
CHUNK_ACTIONS = 12  # :217-227


def chunk_seeds(seed, B: int, chunk: int) -> List[int]:
    """The noise seeds of chunk `chunk` of B sessions: session b's chunk c draws seed_b + c, the one-session rule (seed
    + chunk) per session. seed: an int (every session's seed_b) or B ints."""
    return [s + int(chunk) for s in session_seeds(seed, B)]


def check_batch_actions(actions_np, B: int, action_dim: int) -> np.ndarray:
    """actions [B, N, action_dim] of B sessions, or ValueError."""
    a = np.asarray(actions_np)
    if a.ndim != 3 or a.shape[0] != B or a.shape[2] != action_dim:
        raise ValueError(f"actions must be [{B}, N, {action_dim}] for {B} sessions, got {a.shape}")
    return a


def check_equal_frames(shapes: Sequence[Tuple[int, ...]]) -> Tuple[int, ...]:
    """The one shape of every session's conditioning frame (after the resize), or ValueError."""
    if not shapes:
        raise ValueError("a batch needs at least one conditioning frame")
    if any(tuple(s) != tuple(shapes[0]) for s in shapes):
        raise ValueError(f"the sessions' conditioning frames differ in size after the resize: {[tuple(s) for s in shapes]} "
                         "(pass resolution_hw)")
    return tuple(shapes[0])


def session_step_plan(k: int, frames_per_chunk: int = CHUNK_ACTIONS // 4) -> Tuple[int, int, bool]:
    """Step k (0, 1, ...) of a closed-loop session -> (chunk, latent frame within the chunk, opens a chunk). A chunk is
    a conditioning frame (latent frame 0) plus frames_per_chunk generated latent frames, one per step; the step that
    generates frame 1 opens the chunk (conditioning frame, encode, fresh cache, prefill) first."""
    k, n = int(k), int(frames_per_chunk)
    if k < 0 or n < 1:
        raise ValueError(f"step {k} of chunks of {n} generated frames")
    return k // n, 1 + k % n, k % n == 0


def check_step_actions(actions, B: int, per: int, action_dim: int) -> torch.Tensor:
    """One step's actions [B, per, action_dim] (numpy or tensor) of B sessions as a float tensor, or ValueError."""
    if actions is None:
        raise ValueError(f"a step takes the actions [{B}, {per}, {action_dim}] of its latent frame, got None")
    a = actions if isinstance(actions, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(actions)))
    if a.dim() != 3 or tuple(a.shape) != (B, per, action_dim):
        raise ValueError(f"a step's actions must be [{B}, {per}, {action_dim}] ({per} actions per latent frame for "
                         f"{B} sessions), got {tuple(a.shape)}")
    return a.float()


class ActionSession:
    """B closed-loop sessions of the streaming student in lock-step: step(actions) takes one latent frame's 4 actions per
    session and returns that frame's 4 decoded pixel frames. The chunk rules are stream_action_chunks_batch's, applied
    as the steps arrive (session_step_plan): the step that opens a chunk builds the conditioning frame (the input frame,
    then the last decoded frame re-quantised to uint8), encodes it, builds a StreamingBatchRun(actions=None) with a
    fresh cache and the seeds seed_b + chunk_b, runs the prefill and pushes latent frame 0 into a fresh DecodeStream
    (whose one pixel frame is dropped); every step then runs next_frame(action), hands the new frame's state rows to
    the decoder (cp25_stream_latent_clip) and pushes them. Fed the same actions, the steps' frames are the chunk entry
    points' frames bit for bit. Made by ActionStreamingInference.open_session."""

    def __init__(self, inf: "ActionStreamingInference", first_frames, resolution_hw=None, num_steps: int = 4, seed=1,
                 cache_frame_size: int = -1, output: str = "float"):
        if output not in ("float", "u8"):
            raise ValueError(f"output must be 'float' or 'u8', got {output!r}")
        model = inf.pipe.model
        ncfg = model.net_cfg
        first_frames = list(first_frames)
        B = len(first_frames)
        if not 1 <= B <= MAX_STREAM_BATCH:
            raise ValueError(f"a batch of {B} sessions: 1 .. {MAX_STREAM_BATCH} run in one forward")
        seeds = session_seeds(seed, B)
        if ncfg.action_per_latent_frame != 4:
            raise ValueError("the chunk loop is written for 4 actions per latent frame (12 actions -> 3 latent frames)")
        K = len(model.config.selected_sampling_time)
        self.inf, self.B, self.output = inf, B, output
        self.n_steps = max(1, min(int(num_steps), K))
        self.cache_frame_size = cache_frame_size
        frames = [inf._first_frame(f, resolution_hw) for f in first_frames]
        _, self.H, self.W = check_equal_frames([tuple(f.shape) for f in frames])
        frame = torch.stack(frames, 0)  # [B, 3, H, W] uint8
        self.first_frames = frame.float()[:, :, None] / 128 - 1
        self.on_device = inf.pipe.pixel_path == "device"
        self._frame = frame.to(inf.pipe.device) if self.on_device else frame  # the next chunk's conditioning frames
        self._seeds = seeds
        self._chunk = [0] * B  # per session: chunks opened since its (re)start
        self._T_lat = model.tokenizer.get_latent_num_frames(1 + CHUNK_ACTIONS)
        self._run: Optional[StreamingBatchRun] = None
        self._dec = None
        self.steps_done = 0

    @property
    def at_chunk_start(self) -> bool:
        """The next step opens a chunk (conditioning frame, fresh cache): where replace() is legal."""
        return session_step_plan(self.steps_done, self._T_lat - 1)[2]

    def replace(self, b: int, frame, seed: Optional[int] = None) -> None:
        """Restart session b (the episode reset of a batched policy evaluation): its next chunk conditions on `frame`
        (an array or image path, brought to the sessions' resolution) and counts as its chunk 0, with `seed` as its seed
        if one is given. The other sessions continue. Only at a chunk start, where every session's cache is rebuilt."""
        if not self.at_chunk_start:
            raise RuntimeError("replace() is legal only at a chunk start (at_chunk_start): inside a chunk the sessions "
                               "share one cache position")
        if not 0 <= int(b) < self.B:
            raise ValueError(f"session {b} of {self.B}")
        t = self.inf._first_frame(frame, (self.H, self.W))
        self._frame[int(b)] = t.to(self._frame.device)
        self._chunk[int(b)] = 0
        if seed is not None:
            self._seeds[int(b)] = int(seed)

    def _open_chunk(self) -> None:
        inf = self.inf
        model, B = inf.pipe.model, self.B
        gt = model.encode_conditioning(self._frame[:, :, None], 1, self._T_lat)  # [B, C, T_lat, h, w]
        if inf._ctx is None:
            inf._ctx = model.net.prepare_context(inf.text_embeddings)
        if inf._ctx_batch is None or inf._ctx_batch.B != B:
            inf._ctx_batch = StreamingBatchRun.batch_context(model, inf._ctx, B)
        seeds = [s + c for s, c in zip(self._seeds, self._chunk)]
        self._run = StreamingBatchRun(model, gt, inf._ctx_batch, None, seed=seeds, n_steps=self.n_steps,
                                      cache_frame_size=self.cache_frame_size)  # a fresh cache per chunk
        self._run.next_frame()  # the prefill
        self._dec = model.tokenizer.decode_stream(B)
        geo = self._run.geo
        self._dec.push_rows(self._run.frame_rows(0), geo.Hp, geo.Wp)  # the conditioning frame's pixel frame: dropped
        self._chunk = [c + 1 for c in self._chunk]

    @torch.no_grad()
    def step(self, actions) -> torch.Tensor:
        """actions [B, 4, action_dim] (numpy or tensor) -> the 4 frames they generate: [B, 3, 4, H, W] fp32 in [-1, 1]
        on the host (output="float", a piece of stream_action_chunks_batch) or [B, 4, H, W, 3] uint8 on the device
        (output="u8", decode_u8's quantisation; with pixel_path="device" no pixel leaves the device and the step does
        not wait for it)."""
        pipe = self.inf.pipe
        ncfg = pipe.model.net_cfg
        a = check_step_actions(actions, self.B, ncfg.action_per_latent_frame, ncfg.action_dim)
        a = upload_async(a, pipe.device).to(torch.bfloat16)  # host actions: no wait for the device's earlier work
        if self.at_chunk_start:
            self._open_chunk()
        run, B = self._run, self.B
        f = run.next_frame(a)
        clips = self._dec.push_rows(run.frame_rows(f), run.geo.Hp, run.geo.Wp)  # [B * 4, H, W, 3] bf16
        per_clip = clips.unflatten(0, (B, -1))
        self.steps_done += 1
        if self.at_chunk_start:  # the chunk's last frame
            # the next chunk's conditioning frames, re-quantised in the video's bf16 as the chunk loop does
            video = per_clip[:, -1:].permute(0, 4, 1, 2, 3).clip(min=-1, max=1)  # [B, 3, 1, H, W]
            frame = ((1.0 + video[:, :, -1]) / 2 * 255.0).to(torch.uint8)
            self._frame = frame if self.on_device else frame.cpu()
        if self.output == "u8":
            u8 = pipe.model.tokenizer.model._clips_u8(clips, B, "THWC")
            return u8 if B > 1 else u8[None]
        return per_clip.permute(0, 4, 1, 2, 3).contiguous().clip(min=-1, max=1).float().cpu()


class ActionStreamingInference:
    """`generate_action_streaming` (the whole video) and `stream_action_chunks` (a generator: each chunk's frames as soon
    as they are decoded) over one pipeline object (the tokenizer and the streaming student)."""

    def __init__(self, text_embeddings: torch.Tensor, pipe: Optional[Video2WorldInference] = None,
                 stream_gemm: Optional[str] = None, **pipe_kwargs):
        """text_embeddings: [Lctx, dim] or [1, Lctx, dim], what the net's text context takes (the empty-string
        embedding in the reference). pipe_kwargs go to Video2WorldInference (ckpt_path, tokenizer_path, pixel_path,
        lora_path / lora_alpha / lora_scale for a LoRA post-trained student, net_cfg / sampler_cfg overrides, ...).
        stream_gemm: "tile256" (the default of a pipeline made here), "small" or "small_splitk": the GEMM family of the
        per-frame forward (Video2WorldInference(stream_gemm=...)); None leaves a given `pipe` as it is."""
        self.pipe = pipe or Video2WorldInference(MODEL_NAME, **pipe_kwargs)
        if stream_gemm is not None:
            self.pipe.model.net.set_stream_gemm(stream_gemm)
        if self.pipe.model.config.sampler != "dmd2_stream":
            raise ValueError("ActionStreamingInference needs a streaming ('dmd2_stream') model")
        emb = text_embeddings
        if emb.dim() == 2:  # :141-142
            emb = emb.unsqueeze(0)
        if emb.dim() != 3 or emb.shape[0] != 1:
            raise ValueError(f"text embeddings must be [Lctx, dim] or [1, Lctx, dim], got {tuple(text_embeddings.shape)}")
        self.text_embeddings = emb.to(self.pipe.device, torch.bfloat16)  # :238
        self._ctx = None  # the net's text context (projection + every block's cross-attention K / V), made once
        self._ctx_batch = None  # ... replicated for the sessions of the batch entry points

    # ------------------------------------------------------------------ the input frame
    def _first_frame(self, first_frame_or_path, resolution_hw) -> torch.Tensor:
        """uint8 [3, H, W] at the target resolution, on the host."""
        if isinstance(first_frame_or_path, (str, os.PathLike)):
            path = os.fspath(first_frame_or_path)
            if os.path.splitext(path)[1].lower() not in _IMAGE_EXTENSIONS:
                raise ValueError(f"the conditioning frame must be an image file ({_IMAGE_EXTENSIONS}), got {path}")
            from PIL import Image

            frame = np.asarray(Image.open(path).convert("RGB")).copy()
        else:
            frame = np.asarray(first_frame_or_path)
        if frame.ndim != 3 or frame.shape[2] != 3:
            raise ValueError(f"the conditioning frame must be [H, W, 3], got {frame.shape}")
        if frame.dtype != np.uint8:
            frame = np.clip(np.round(frame), 0, 255).astype(np.uint8)  # :209
        t = torch.from_numpy(np.ascontiguousarray(frame)).permute(2, 0, 1)
        if resolution_hw is not None and tuple(t.shape[1:]) != tuple(int(v) for v in resolution_hw):
            t = resize_input(t[None], (int(resolution_hw[0]), int(resolution_hw[1])))[0]
        H, W = t.shape[1:]
        if H % 16 or W % 16:
            raise ValueError(f"resolution {(H, W)}: both sides must be multiples of 16 (8x VAE, 2x2 patches)")
        return t.contiguous()

    # ------------------------------------------------------------------ generation
    @torch.no_grad()
    def stream_action_chunks(self, first_frame_or_path, actions_np: np.ndarray,
                             resolution_hw: Optional[Tuple[int, int]] = None, num_steps: int = 4, seed: int = 1,
                             cache_frame_size: int = -1) -> Iterator[torch.Tensor]:
        """Yields the video piece by piece, each [3, t, H, W] fp32 in [-1, 1] on the host: first the input frame
        (scaled / 128 - 1, :215), then per chunk of 12 actions its 12 decoded frames, as soon as that chunk is decoded.
        Concatenated along t they are generate_action_streaming's result."""
        pipe = self.pipe
        model, dev = pipe.model, pipe.device
        ncfg = model.net_cfg
        actions_np = np.asarray(actions_np)
        if actions_np.ndim != 2 or actions_np.shape[1] != ncfg.action_dim:
            raise ValueError(f"actions must be [N, {ncfg.action_dim}], got {actions_np.shape}")
        if ncfg.action_per_latent_frame != 4:
            raise ValueError("the chunk loop is written for 4 actions per latent frame (12 actions -> 3 latent frames)")
        K = len(model.config.selected_sampling_time)
        n_steps = max(1, min(int(num_steps), K))  # :284-292
        frame = self._first_frame(first_frame_or_path, resolution_hw)  # uint8 [3, H, W]
        _, H, W = frame.shape
        yield frame.float()[:, None] / 128 - 1  # :215
        on_device = pipe.pixel_path == "device"
        if on_device:
            frame = frame.to(dev)
        T_lat = model.tokenizer.get_latent_num_frames(1 + CHUNK_ACTIONS)
        for ar_idx in range(actions_np.shape[0] // CHUNK_ACTIONS):
            # the chunk's 13-frame video is the conditioning frame + 12 zero frames (:219-222); the causal VAE's latent
            # frame 0 depends on pixel frame 0 alone, and the loop reads no other frame of x0 (encode_conditioning)
            gt = model.encode_conditioning(frame[None, :, None], 1, T_lat)
            a = torch.from_numpy(np.ascontiguousarray(actions_np[ar_idx * CHUNK_ACTIONS:(ar_idx + 1) * CHUNK_ACTIONS]))
            a = a.float().unsqueeze(0).to(dev, torch.bfloat16)  # :168, :177
            if self._ctx is None:  # the same text for every chunk (the reference re-projects it in every forward)
                self._ctx = model.net.prepare_context(self.text_embeddings)
            run = StreamingRun(model, gt, self._ctx, a, seed=seed + ar_idx, n_steps=n_steps,
                               cache_frame_size=cache_frame_size)  # a fresh cache per chunk (:475-480)
            while not run.done:
                run.next_frame()
            video = model.decode(run.latents()).clip(min=-1, max=1)  # bf16, as the latents (:302-303)
            # the next chunk's conditioning frame, re-quantised in the video's bf16 (:310)
            frame = ((1.0 + video[0:1, :, -1]) / 2 * 255.0).to(torch.uint8)[0]
            if not on_device:
                frame = frame.cpu()
            yield video[0, :, 1:].float().cpu()  # :307

    @torch.no_grad()
    def generate_action_streaming(self, first_frame_or_path, actions_np: np.ndarray,
                                  resolution_hw: Optional[Tuple[int, int]] = None, num_steps: int = 4, seed: int = 1,
                                  cache_frame_size: int = -1) -> torch.Tensor:
        """-> video [3, 1 + 12 (len(actions) // 12), H, W] fp32 in [-1, 1] (action_video2world_streaming.py:183-313)."""
        return torch.cat(list(self.stream_action_chunks(first_frame_or_path, actions_np, resolution_hw, num_steps, seed,
                                                        cache_frame_size)), dim=1)

    # ------------------------------------------------------------------ B sessions in lock-step
    @torch.no_grad()
    def stream_action_chunks_batch(self, first_frames, actions_np: np.ndarray,
                                   resolution_hw: Optional[Tuple[int, int]] = None, num_steps: int = 4, seed=1,
                                   cache_frame_size: int = -1) -> Iterator[torch.Tensor]:
        """stream_action_chunks for B independent sessions (parallel rollouts) through one sequence of launches: the VAE
        encodes and decodes the B clips in lock-step and one per-frame forward serves all sessions
        (model.StreamingBatchRun). first_frames: B arrays or image paths, of one size after the resize; actions_np
        [B, N, action_dim]; seed an int or B ints, session b's chunk c drawing seed_b + c. Yields [B, 3, t, H, W] fp32
        pieces: the input frames, then each chunk's 12 frames. The chunk rules are the one-session ones."""
        pipe = self.pipe
        model, dev = pipe.model, pipe.device
        ncfg = model.net_cfg
        first_frames = list(first_frames)
        B = len(first_frames)
        actions_np = check_batch_actions(actions_np, B, ncfg.action_dim)
        session_seeds(seed, B)  # a seed list of the wrong length fails before any work
        if ncfg.action_per_latent_frame != 4:
            raise ValueError("the chunk loop is written for 4 actions per latent frame (12 actions -> 3 latent frames)")
        K = len(model.config.selected_sampling_time)
        n_steps = max(1, min(int(num_steps), K))
        frames = [self._first_frame(f, resolution_hw) for f in first_frames]  # uint8 [3, H, W] each
        check_equal_frames([tuple(f.shape) for f in frames])
        frame = torch.stack(frames, 0)  # [B, 3, H, W]
        yield frame.float()[:, :, None] / 128 - 1
        on_device = pipe.pixel_path == "device"
        if on_device:
            frame = frame.to(dev)
        T_lat = model.tokenizer.get_latent_num_frames(1 + CHUNK_ACTIONS)
        for ar_idx in range(actions_np.shape[1] // CHUNK_ACTIONS):
            gt = model.encode_conditioning(frame[:, :, None], 1, T_lat)  # [B, C, T_lat, h, w]
            a = torch.from_numpy(np.ascontiguousarray(
                actions_np[:, ar_idx * CHUNK_ACTIONS:(ar_idx + 1) * CHUNK_ACTIONS]))
            a = a.float().to(dev, torch.bfloat16)
            if self._ctx is None:
                self._ctx = model.net.prepare_context(self.text_embeddings)
            if self._ctx_batch is None or self._ctx_batch.B != B:
                self._ctx_batch = StreamingBatchRun.batch_context(model, self._ctx, B)
            run = StreamingBatchRun(model, gt, self._ctx_batch, a, seed=chunk_seeds(seed, B, ar_idx), n_steps=n_steps,
                                    cache_frame_size=cache_frame_size)  # a fresh cache per chunk
            while not run.done:
                run.next_frame()
            video = model.decode(run.latents()).clip(min=-1, max=1)  # [B, 3, 13, H, W] bf16
            frame = ((1.0 + video[:, :, -1]) / 2 * 255.0).to(torch.uint8)
            if not on_device:
                frame = frame.cpu()
            yield video[:, :, 1:].float().cpu()

    @torch.no_grad()
    def generate_action_streaming_batch(self, first_frames, actions_np: np.ndarray,
                                        resolution_hw: Optional[Tuple[int, int]] = None, num_steps: int = 4, seed=1,
                                        cache_frame_size: int = -1) -> torch.Tensor:
        """-> videos [B, 3, 1 + 12 (N // 12), H, W] fp32 in [-1, 1]: session b is generate_action_streaming of
        first_frames[b], actions_np[b] and seed_b."""
        return torch.cat(list(self.stream_action_chunks_batch(first_frames, actions_np, resolution_hw, num_steps, seed,
                                                              cache_frame_size)), dim=2)

    # ------------------------------------------------------------------ closed loop
    def open_session(self, first_frames, resolution_hw: Optional[Tuple[int, int]] = None, num_steps: int = 4, seed=1,
                     cache_frame_size: int = -1, output: str = "float") -> ActionSession:
        """B closed-loop sessions (ActionSession) from B conditioning frames (arrays or image paths, B = 1 .. 16):
        `sess.first_frames` is the first piece of stream_action_chunks_batch, `sess.step(actions [B, 4, action_dim])`
        returns the 4 frames those actions generate, and `sess.replace(b, frame, seed)` restarts one session at a chunk
        start. Fed the actions of generate_action_streaming_batch, the steps reproduce its video bit for bit."""
        return ActionSession(self, first_frames, resolution_hw, num_steps, seed, cache_frame_size, output)
