"""CPU restatement of the streaming (causal, KV-cached) action student -- TEST INFRASTRUCTURE.

Restated from the reference as text (paths under cosmos_predict2/_src/predict2/):
  interactive/networks/dit_causal.py:1062-1159        KVContextConfig, AttenOpWithKV with its rolling cache (RollingKV)
  interactive/networks/dit_causal.py:1162-1190        VideoSeqPos (the frame's rows of the clip's RoPE table)
  interactive/networks/dit_action_causal.py:324-472   forward_seq; :591-638 its condition-mask channel
  interactive/models/action_video2world_self_forcing.py:170-227   denoise_edm_seq
  interactive/models/action_video2world_self_forcing.py:383-577   generate_next_frame, generate_streaming_video
  modules/denoiser_scaling.py:28-67                   the sCM wrappers: float64 inside, cast back to the time's dtype
  interactive/inference/action_video2world_streaming.py:183-313   the chunk loop (chunk_plan)
built from oracle.dit's helpers, in chronological key order and with concatenation, as the reference is written.

Arithmetic. The student runs in bf16 op by op: x, the noise, the latents, the times and the coefficients are bf16
tensors (init_noise.to(**tensor_kwargs) :457, t_tensor dtype=bfloat16 :420, scaling_from_time's cast back), so every
torch op of the loop is a bf16 elementwise op, which PyTorch evaluates in fp32 and rounds once. `_ew` writes exactly
that, so that nothing depends on how the CPU's own bf16 kernels are written. Operand by operand (:226, :442-444):
  c_skip * x, c_out * net, x * c_in       bf16 [B,1,1,1,1] tensor x bf16 tensor: fp32 product (exact), one rounding
  cos(t_next) * x0, sin(t_next) * noise   t_next is a 0-dim bf16 tensor, so cos / sin are 0-dim bf16 tensors (the cosine
                                          is rounded to bf16 before the product, unlike round 8's Python-float sine)
  ... / self.sigma_data                   a device tensor divided by a Python float: PyTorch's div kernel multiplies by
                                          the reciprocal, computed in the op's math type: x * (1.0f / float(sigma_data)),
                                          one rounding (BinaryDivTrueKernel.cu, "a * reciprocal(b)"). The CPU kernel
                                          divides; the reference runs on the GPU. (For sigma_data 1, 0.5 and 0.8 the two
                                          agree on every bf16 input: 1 / float(0.8) is exactly 1.25 in fp32.)
  a + b                                   fp32 sum of two bf16 values, one rounding
Inside `oracle.dit.fp32_truth()` the same loop keeps every activation in fp32 (the bf16-valued inputs and times, no
intermediate rounding): the truth both the bf16 restatement and the HIP path are measured against.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional

import torch
import torch.nn.functional as F

from oracle import dit as odit

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


# ----------------------------------------------------------------------------- AttenOpWithKV
@dataclass
class KVContextConfig:  # dit_causal.py:1061-1066
    run_with_kv: bool = False
    store_kv: bool = False
    start_idx: int = 0


class RollingKV:
    """AttenOpWithKV (dit_causal.py:1069-1159) without the wrapped op: forward returns the (k_out, v_out) it attends."""

    def __init__(self, batch: int, seq_len: int, tail_shape, dtype):
        self.k_cache = torch.zeros(batch, seq_len, *tail_shape, dtype=dtype)
        self.v_cache = torch.zeros(batch, seq_len, *tail_shape, dtype=dtype)
        self.start_pointer = 0
        self.cache_size = seq_len

    def forward(self, k: torch.Tensor, v: torch.Tensor, cfg: KVContextConfig):
        if cfg.run_with_kv and cfg.start_idx > 0:
            history_k = self.k_cache[:, : cfg.start_idx - self.start_pointer]
            history_v = self.v_cache[:, : cfg.start_idx - self.start_pointer]
            k_out = torch.cat([history_k, k], dim=1)
            v_out = torch.cat([history_v, v], dim=1)
        else:
            k_out, v_out = k, v
        if cfg.store_kv:
            start = int(cfg.start_idx)
            end = start + int(k.shape[1])
            if end > self.start_pointer + self.cache_size:  # rolling kv cache
                old_start = end - self.cache_size
                sp = self.start_pointer
                self.k_cache = torch.cat([self.k_cache[:, old_start - sp: start - sp], k], dim=1)
                self.v_cache = torch.cat([self.v_cache[:, old_start - sp: start - sp], v], dim=1)
                self.start_pointer = old_start
            else:
                self.k_cache[:, start - self.start_pointer: end - self.start_pointer] = k
                self.v_cache[:, start - self.start_pointer: end - self.start_pointer] = v
        return k_out, v_out


def cache_tokens(T: int, hw: int, cache_frame_size: int) -> int:
    """full_cache_size (action_video2world_self_forcing.py:470-473)."""
    return T * hw if cache_frame_size == -1 else cache_frame_size * hw


def pass_schedule(T: int, n_steps: int):
    """(frame, store) of every net pass of generate_streaming_video, in order (:499-575)."""
    out = [(0, True)]
    for t in range(1, T):
        out += [(t, False)] * n_steps + [(t, True)]
    return out


def attended_frames(T: int, hw: int, cache_frame_size: int, n_steps: int = 2) -> List[List[int]]:
    """The frames whose keys each pass of the loop attends to, in key order, from running RollingKV on keys that hold
    their frame index."""
    kv = RollingKV(1, cache_tokens(T, hw, cache_frame_size), (1, 1), F32)
    seen = []
    for frame, store in pass_schedule(T, n_steps):
        k = torch.full((1, hw, 1, 1), float(frame))
        k_out, _ = kv.forward(k, k, KVContextConfig(run_with_kv=True, store_kv=store, start_idx=frame * hw))
        ids = k_out[0, :, 0, 0].view(-1, hw)
        assert bool((ids == ids[:, :1]).all())  # whole frames
        seen.append([int(i) for i in ids[:, 0]])
    return seen


def chunk_plan(n_actions: int, seed: int):
    """The chunk loop's bookkeeping (action_video2world_streaming.py:217-313): per chunk its action rows, its noise
    seed and the pixel frames it contributes (12, after dropping the decoded frame 0); plus the total frame count."""
    chunks = [dict(actions=(i * 12, (i + 1) * 12), seed=seed + i, frames=12) for i in range(n_actions // 12)]
    return chunks, 1 + 12 * len(chunks)


# ----------------------------------------------------------------------------- elementwise bf16 ops, written out
def _act():
    return odit.act_dtype()


def _ew(fn, *xs) -> torch.Tensor:
    """One elementwise torch op on tensors of the activation dtype: fp32 math, one rounding."""
    return fn(*[x.float() for x in xs]).to(_act())


def mul(a, b):
    return _ew(torch.mul, a, b)


def add(a, b):
    return _ew(torch.add, a, b)


def div_scalar(a: torch.Tensor, s: float) -> torch.Tensor:
    """tensor / python_float on the GPU: a * (1.0f / float(s)) (module docstring)."""
    inv = torch.tensor(1.0, dtype=F32) / torch.tensor(float(s), dtype=F32)
    return (a.float() * inv).to(_act())


def scaling_from_time(t: torch.Tensor, scaling: str, sigma_data: float):
    """denoiser_scaling.py:28-67: float64 inside, the coefficients cast back to t's dtype."""
    dtype = t.dtype
    t = t.to(F64)
    sd = sigma_data
    if scaling == "rectified_flow":
        c_skip = sd / (torch.cos(t) + sd * torch.sin(t))
        c_out = -sd * torch.sin(t) / (torch.cos(t) + sd * torch.sin(t))
        c_in = sd / (torch.cos(t) + sd * torch.sin(t))
        c_noise = sd * torch.sin(t) / (torch.cos(t) + sd * torch.sin(t))
    else:
        sigma = torch.tan(t) * sd
        c_skip = sd * torch.cos(t)
        c_out = sd * torch.sin(t)
        c_in = torch.ones_like(t)
        c_noise = 0.25 * sigma.log()
    return c_skip.to(dtype), c_out.to(dtype), c_in.to(dtype), c_noise.to(dtype)


def edm_coefficients(t_bf16: torch.Tensor, mask_mean: torch.Tensor, scaling: str, sigma_data: float,
                     sigma_conditional: float):
    """denoise_edm_seq :196-203 on the [B,1,T,1,1] time (bf16 values; kept in the activation dtype)."""
    time = t_bf16.to(_act())
    m = mask_mean.to(_act())
    ones_s = _ew(lambda o: o * (sigma_conditional / sigma_data), torch.ones_like(time))
    t_cond = _ew(torch.atan, ones_s)
    time = add(mul(t_cond, m), mul(time, _ew(lambda x: 1 - x, m)))
    return scaling_from_time(time, scaling, sigma_data)


def x0_from_net(x, net_out, c_skip, c_out):
    """:226: c_skip * x + c_out * net_output."""
    return add(mul(c_skip, x), mul(c_out, net_out))


def renoise(x0, noise, t_next: float, sigma_data: float):
    """:441-444: cos(t_next_tensor) * x0 / sigma_data + sin(t_next_tensor) * noise, t_next a 0-dim bf16 tensor (its
    value stays bf16 under the fp32 truth too: an input of the loop)."""
    tn = torch.tensor(float(t_next), dtype=BF16).to(_act())
    c, s = _ew(torch.cos, tn), _ew(torch.sin, tn)
    return add(div_scalar(mul(c, x0), sigma_data), mul(s, noise))


# ----------------------------------------------------------------------------- forward_seq
def project_context(cfg: dict, sd: dict, crossattn_emb: torch.Tensor) -> torch.Tensor:
    ctx = crossattn_emb.to(_act())
    if cfg["use_crossattn_projection"]:
        ctx = F.gelu(odit._lin(ctx, odit._w(sd, "crossattn_proj.0.weight"), odit._w(sd, "crossattn_proj.0.bias")))
    return ctx


def _block(cfg, sd, i, x, emb, lora, ctx, freqs, kv: RollingKV, kv_cfg: KVContextConfig):
    """CausalBlock.forward (dit_causal.py:490-566; Block.forward's body, oracle.dit.block_forward) with the
    self-attention's K / V passed through AttenOpWithKV."""
    p = f"blocks.{i}."
    nh, hd = cfg["num_heads"], cfg["model_channels"] // cfg["num_heads"]
    mods = []
    for m in ("self_attn", "cross_attn", "mlp"):
        mods += [t[:, :, None, None, :].to(_act()) for t in odit.adaln(sd, p + "adaln_modulation_" + m, emb, lora)]
    sh_sa, sc_sa, g_sa, sh_ca, sc_ca, g_ca, sh_ml, sc_ml, g_ml = mods
    B, T, H, W, D = x.shape
    lin, w = odit._lin, odit._w

    h = odit.ln_mod(x, sh_sa, sc_sa).reshape(B, T * H * W, D)
    q = lin(h, w(sd, p + "self_attn.q_proj.weight")).reshape(B, -1, nh, hd)
    k = lin(h, w(sd, p + "self_attn.k_proj.weight")).reshape(B, -1, nh, hd)
    v = lin(h, w(sd, p + "self_attn.v_proj.weight")).reshape(B, -1, nh, hd)
    q = odit.apply_rope(odit.te_rmsnorm(q, w(sd, p + "self_attn.q_norm.weight")).float(), freqs).to(_act())
    k = odit.apply_rope(odit.te_rmsnorm(k, w(sd, p + "self_attn.k_norm.weight")).float(), freqs).to(_act())
    k_out, v_out = kv.forward(k, v.to(_act()), kv_cfg)
    o = odit.sdpa(q, k_out, v_out)
    o = lin(o, w(sd, p + "self_attn.output_proj.weight")).reshape(B, T, H, W, D)
    x = x + g_sa * o

    h = odit.ln_mod(x, sh_ca, sc_ca).reshape(B, T * H * W, D)
    q = odit.te_rmsnorm(lin(h, w(sd, p + "cross_attn.q_proj.weight")).reshape(B, -1, nh, hd),
                        w(sd, p + "cross_attn.q_norm.weight"))
    k = odit.te_rmsnorm(lin(ctx, w(sd, p + "cross_attn.k_proj.weight")).reshape(B, -1, nh, hd),
                        w(sd, p + "cross_attn.k_norm.weight"))
    v = lin(ctx, w(sd, p + "cross_attn.v_proj.weight")).reshape(B, -1, nh, hd)
    o = lin(odit.sdpa(q, k, v), w(sd, p + "cross_attn.output_proj.weight")).reshape(B, T, H, W, D)
    x = o * g_ca + x

    h = odit.ln_mod(x, sh_ml, sc_ml)
    y = lin(F.gelu(lin(h, w(sd, p + "mlp.layer1.weight"))), w(sd, p + "mlp.layer2.weight"))
    return x + g_ml * y


class StreamNet:
    """The causal action net with its per-block rolling caches: make_it_kv_cache + forward_seq."""

    def __init__(self, cfg: dict, sd: dict, crossattn_emb: torch.Tensor):
        self.cfg, self.sd = cfg, sd
        self.ctx = project_context(cfg, sd, crossattn_emb)
        self.kv: List[RollingKV] = []

    def make_it_kv_cache(self, batch: int, seq_len: int) -> None:
        nh, hd = self.cfg["num_heads"], self.cfg["model_channels"] // self.cfg["num_heads"]
        self.kv = [RollingKV(batch, seq_len, (nh, hd), _act()) for _ in range(self.cfg["num_blocks"])]

    def forward_seq(self, x_B_C_1_H_W, mask_B_1_1_H_W, t_B_1, frame: int, kv_cfg: KVContextConfig,
                    action: Optional[torch.Tensor]) -> torch.Tensor:
        cfg, sd = self.cfg, self.sd
        x = torch.cat([x_B_C_1_H_W, mask_B_1_1_H_W.type_as(x_B_C_1_H_W)], dim=1)  # :625
        B, _, T1, Hl, Wl = x.shape
        if cfg["concat_padding_mask"]:  # prepare_embedded_sequence, dit_causal.py:780-786 (a zero padding mask)
            x = torch.cat([x, torch.zeros(B, 1, T1, Hl, Wl, dtype=x.dtype)], dim=1)
        ps = cfg["patch_spatial"]
        Hp, Wp = Hl // ps, Wl // ps
        xp = x.reshape(B, x.shape[1], 1, 1, Hp, ps, Wp, ps).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B, 1, Hp, Wp, -1)
        x = odit._lin(xp, odit._w(sd, "x_embedder.proj.1.weight"))
        t = t_B_1.to(BF16)  # timesteps arrive in the net dtype (:216); the truth takes the same bf16 values
        t = t * cfg["timestep_scale"] if _act() == BF16 else t.float() * cfg["timestep_scale"]  # :360
        # the per-frame action embedding "b t d -> b 1 (t d)" with no zero row (:385-407): the per-chunk form of the
        # oracle's embedders on this frame's actions
        emb, lora = odit.timestep_embedding(dict(cfg, action_per_latent_frame=0), sd, t, action)
        hw = Hp * Wp
        freqs = odit.rope_freqs(cfg, frame + 1, Hp, Wp)[frame * hw: (frame + 1) * hw]  # :412-421
        for i in range(cfg["num_blocks"]):
            x = _block(cfg, sd, i, x, emb, lora, self.ctx, freqs, self.kv[i], kv_cfg)
        D = cfg["model_channels"]
        cd = odit.cond_dtype(cfg)
        sh, sc = odit.adaln(sd, "final_layer.adaln_modulation", emb, lora[..., : 2 * D], n_chunks=2)
        xf = F.layer_norm(x.to(cd), (D,), eps=1e-6)
        xf = xf * (1 + sc[:, :, None, None, :]) + sh[:, :, None, None, :]
        out = odit._lin(xf, odit._w(sd, "final_layer.linear.weight").to(cd))
        C = cfg["out_channels"]
        out = out.reshape(B, 1, Hp, Wp, ps, ps, 1, C).permute(0, 7, 1, 6, 2, 4, 3, 5).reshape(B, C, 1, Hl, Wl)
        return out.to(_act())  # .type_as(x_B_C_T_H_W)


# ----------------------------------------------------------------------------- the loop
def denoise_edm_seq(net_call, x, t_B_T, smp: dict, mask=None):
    """:170-227. net_call(net_state_in, mask, c_noise_B_T) -> net output [B, C, 1, H, W]."""
    B, C, _, H, W = x.shape
    time = t_B_T.reshape(B, 1, -1, 1, 1)
    if mask is None:
        mask = torch.zeros((B, 1, 1, H, W), dtype=x.dtype)
    cm = mask.repeat(1, C, 1, 1, 1).type_as(x)
    cm_mean = cm.float().mean(dim=[1, 3, 4], keepdim=True).to(x.dtype)
    c_skip, c_out, c_in, c_noise = edm_coefficients(time, cm_mean, smp["trig_scaling"], smp["sigma_data"],
                                                    smp["sigma_conditional"])
    net_in = mul(x, c_in)
    net_out = net_call(net_in, mask, c_noise.reshape(B, -1)).float().to(x.dtype)
    return x0_from_net(x, net_out, c_skip, c_out)


def generate_streaming_video(smp: dict, gt, actions, init_noise, n_steps: int, cache_frame_size: int, *,
                             net: Optional[StreamNet] = None, net_fn=None, per_frame: int = 4):
    """generate_streaming_video (:449-577) -> latents [B, C, T, H, W] in the activation dtype. gt's frame 0 conditions;
    net: a StreamNet (the real net), or net_fn(net_in [B,C,1,H,W], mask, c_noise [B,1], frame, action, store) stands in."""
    act = _act()
    t_steps = [float(t) for t in smp["selected_sampling_time"]]
    assert 1 <= n_steps <= len(t_steps)
    init_noise = init_noise.to(BF16).to(act)  # :457 (the truth keeps the bf16-valued noise)
    gt = gt.to(BF16).to(act)                  # action_video2world_streaming.py:256
    B, C, T, H, W = init_noise.shape
    out = torch.zeros(B, C, T, H, W, dtype=act)
    out[:, :, :1] = gt[:, :, :1]
    hw = (H // 2) * (W // 2)
    if net is not None:
        net.make_it_kv_cache(B, cache_tokens(T, hw, cache_frame_size))

    def call(frame, store, action):
        kv_cfg = KVContextConfig(run_with_kv=True, store_kv=store, start_idx=frame * hw)

        def f(net_in, mask, c_noise):
            if net_fn is not None:
                return net_fn(net_in, mask, c_noise, frame, action, store)
            return net.forward_seq(net_in, mask, c_noise, frame, kv_cfg, action)
        return f

    zeros_t = torch.zeros(B, 1, dtype=BF16)
    denoise_edm_seq(call(0, True, None), out[:, :, :1], zeros_t, smp)  # prefill (:499-527)
    for t_idx in range(1, T):
        noise = init_noise[:, :, t_idx: t_idx + 1]
        action = actions[:, (t_idx - 1) * per_frame: t_idx * per_frame]
        x = noise
        for s in range(n_steps):
            t_tensor = torch.full((B, 1), t_steps[s], dtype=BF16)
            x0 = denoise_edm_seq(call(t_idx, False, action), x, t_tensor, smp)
            if s < n_steps - 1:
                x = renoise(x0, noise, t_steps[s + 1], smp["sigma_data"])
        out[:, :, t_idx: t_idx + 1] = x0
        denoise_edm_seq(call(t_idx, True, action), x0, zeros_t, smp)  # store pass (:546-575)
    return out


def to_patch(x_C_T_H_W: torch.Tensor) -> torch.Tensor:
    """[C, T, H, W] -> [T * H/2 * W/2, 64], feature (p1 * 2 + p2) * 16 + c (the sampler's patch layout)."""
    C, T, H, W = x_C_T_H_W.shape
    return x_C_T_H_W.reshape(C, T, H // 2, 2, W // 2, 2).permute(1, 2, 4, 3, 5, 0).reshape(-1, 4 * C).contiguous()


def from_patch(xp: torch.Tensor, T: int, H: int, W: int) -> torch.Tensor:
    C = xp.shape[1] // 4
    return xp.view(T, H // 2, W // 2, 2, 2, C).permute(5, 0, 1, 3, 2, 4).reshape(C, T, H, W).contiguous()


def patch_rows(net_in_C_1_H_W: torch.Tensor, mask_value: float = 0.0) -> torch.Tensor:
    """The x_embedder's [hw, 72] rows of one frame: feature c * 4 + p for the 16 latent channels, the mask channel and
    the zero padding-mask channel (cp25_patchify's layout)."""
    C, _, H, W = net_in_C_1_H_W.shape
    x = torch.cat([net_in_C_1_H_W, torch.full((1, 1, H, W), mask_value, dtype=net_in_C_1_H_W.dtype),
                   torch.zeros(1, 1, H, W, dtype=net_in_C_1_H_W.dtype)], 0)
    return x.reshape(C + 2, H // 2, 2, W // 2, 2).permute(1, 3, 0, 2, 4).reshape(-1, (C + 2) * 4).contiguous()


STUDENT_TIMES = (math.pi / 2, math.atan(15), math.atan(5), math.atan(5 / 3))
