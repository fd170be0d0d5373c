"""Wan2.1 causal video VAE (the Cosmos-Predict2.5 tokenizer) for MI355X.

Same weights (tokenizer.pth keys encoder.* / conv1.* / conv2.* / decoder.*), same chunking and
causal feature-cache semantics as the reference (cosmos_predict2/_src/predict2/tokenizers/wan2pt1.py:
Encoder3d :264-359, Decoder3d :362-458, WanVAE_.encode/decode :504-570, Wan2pt1VAEInterface :961-1060),
re-laid-out for the GPU:
* activations are channels-last clips [T][H][W][C] bf16, so every convolution is an implicit GEMM
  over (kt, kh, kw, cin) with contiguous channel vectors (cp25_conv3d, bf16 MFMA);
* the causal padding / feat_cache of every CausalConv3d is a table of frame pointers handed to the
  kernel (zero frames are NULL), never a concatenated copy;
* nearest-2x upsampling is fused into the conv's input gather, the upsample3d frame interleave into
  its epilogue, bias + residual adds into the conv epilogue; RMS_norm + SiLU is one HIP kernel.
The single-head AttentionBlock core (C = 384 at h/8 x w/8) is the flash kernel cp25_vae_attn reading q / k / v
straight out of the to_qkv output (no score matrix in HBM); its 1x1 projections and norm are the HIP conv /
norm kernels.

Context parallel decode (set_context_parallel_group): the reference replicates the VAE on every rank;
here each rank decodes a band of h/N latent rows (8h/N output rows) of every frame. A 3x3 conv needs
one input row beyond its band on each side: `_halo` fetches the neighbours' edge rows (RCCL
all-gather of the bands' first/last rows; zero rows at the image edge = the conv's zero padding)
and the conv runs unpadded in h over the haloed band (causal caches keep the haloed frames, so the
cached frames carry their halos too); the nearest-2x upsample conv reads the haloed low-res band with
pads (-1, -1), the (3,1,1) time_conv and 1x1 convs need no halo, RMS_norm is per pixel, and the
middle AttentionBlock gathers K/V of the whole frame. Bands are gathered into the full video at the
end. Every output pixel is computed from the same inputs in the same order as the unbanded decode.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn.functional as F

from . import _native as N
from . import context_parallel as cpx

BF16 = torch.bfloat16
CACHE_T = 2
MAX_FRAMES = 24  # frame-table size of cp25_conv3d

_MEAN = [-0.7571, -0.7089, -0.9113, 0.1075, -0.1745, 0.9653, -0.1517, 1.5508,
         0.4134, -0.0715, 0.5517, -0.3632, -0.1922, -0.9497, 0.2503, -0.2921]
_STD = [2.8184, 1.4541, 2.3275, 2.6558, 1.2196, 1.7708, 2.6052, 2.0743,
        3.2687, 2.1526, 2.8652, 1.5579, 1.6382, 1.1253, 2.8251, 1.9160]


# ----------------------------------------------------------------------------- layout
def encoder_layers(dim=96, dim_mult=(1, 2, 4, 4), nres=2, tdown=(False, True, True)):
    dims = [dim * u for u in (1,) + tuple(dim_mult)]
    out = []
    for i, (cin, cout) in enumerate(zip(dims[:-1], dims[1:])):
        for _ in range(nres):
            out.append(("res", cin, cout))
            cin = cout
        if i != len(dim_mult) - 1:
            out.append(("downsample3d" if tdown[i] else "downsample2d", cout, cout))
    return out


def decoder_layers(dim=96, dim_mult=(1, 2, 4, 4), nres=2, tup=(True, True, False)):
    dims = [dim * u for u in (dim_mult[-1],) + tuple(dim_mult[::-1])]
    out = []
    for i, (cin, cout) in enumerate(zip(dims[:-1], dims[1:])):
        if i in (1, 2, 3):
            cin //= 2
        for _ in range(nres + 1):
            out.append(("res", cin, cout))
            cin = cout
        if i != len(dim_mult) - 1:
            out.append(("upsample3d" if tup[i] else "upsample2d", cout, cout))
    return out


def vae_state_dict_shapes(dim=96, z_dim=16) -> Dict[str, tuple]:
    s: Dict[str, tuple] = {}

    def conv(name, cout, cin, k):
        s[name + ".weight"] = (cout, cin) + k
        s[name + ".bias"] = (cout,)

    def res(p, cin, cout):
        s[p + ".residual.0.gamma"] = (cin, 1, 1, 1)
        conv(p + ".residual.2", cout, cin, (3, 3, 3))
        s[p + ".residual.3.gamma"] = (cout, 1, 1, 1)
        conv(p + ".residual.6", cout, cout, (3, 3, 3))
        if cin != cout:
            conv(p + ".shortcut", cout, cin, (1, 1, 1))

    def attn(p, c):
        s[p + ".norm.gamma"] = (c, 1, 1)
        conv(p + ".to_qkv", 3 * c, c, (1, 1))
        conv(p + ".proj", c, c, (1, 1))

    def resample(p, kind, c):
        if kind.startswith("upsample"):
            conv(p + ".resample.1", c // 2, c, (3, 3))
            if kind == "upsample3d":
                conv(p + ".time_conv", 2 * c, c, (3, 1, 1))
        else:
            conv(p + ".resample.1", c, c, (3, 3))
            if kind == "downsample3d":
                conv(p + ".time_conv", c, c, (3, 1, 1))

    conv("encoder.conv1", dim, 3, (3, 3, 3))
    for i, (k, ci, co) in enumerate(encoder_layers(dim)):
        (res if k == "res" else (lambda p, a, b, kk=k: resample(p, kk, a)))(f"encoder.downsamples.{i}", ci, co)
    top = 4 * dim
    res("encoder.middle.0", top, top)
    attn("encoder.middle.1", top)
    res("encoder.middle.2", top, top)
    s["encoder.head.0.gamma"] = (top, 1, 1, 1)
    conv("encoder.head.2", 2 * z_dim, top, (3, 3, 3))
    conv("conv1", 2 * z_dim, 2 * z_dim, (1, 1, 1))
    conv("conv2", z_dim, z_dim, (1, 1, 1))
    conv("decoder.conv1", top, z_dim, (3, 3, 3))
    res("decoder.middle.0", top, top)
    attn("decoder.middle.1", top)
    res("decoder.middle.2", top, top)
    for i, (k, ci, co) in enumerate(decoder_layers(dim)):
        (res if k == "res" else (lambda p, a, b, kk=k: resample(p, kk, a)))(f"decoder.upsamples.{i}", ci, co)
    s["decoder.head.0.gamma"] = (dim, 1, 1, 1)
    conv("decoder.head.2", 3, dim, (3, 3, 3))
    return s


def init_vae_state_dict(seed: int = 0, device="cpu") -> Dict[str, torch.Tensor]:
    """Seeded synthetic weights (kaiming-uniform convs as nn.Conv default; gammas ~1)."""
    g = torch.Generator(device=device).manual_seed(seed)
    out = {}
    for k, shp in vae_state_dict_shapes().items():
        if k.endswith("gamma"):
            out[k] = (1 + 0.1 * torch.randn(shp, generator=g, device=device)).to(BF16)
        elif k.endswith("bias"):
            out[k] = (0.02 * torch.randn(shp, generator=g, device=device)).to(BF16)
        else:
            fan_in = math.prod(shp[1:])
            bound = 1.0 / math.sqrt(fan_in)
            out[k] = ((torch.rand(shp, generator=g, device=device) * 2 - 1) * bound * math.sqrt(3)).to(BF16)
    return out


# ----------------------------------------------------------------------------- frame tables of several clips
def clip_table_layout(Tc: int, stride_t: int, kt: int, n_clips: int, max_frames: int = MAX_FRAMES):
    """The frame table of cp25_conv3d_clips for n_clips clips of Tc output frames each -> (Fc, launches).
    Fc = (Tc - 1) * stride_t + kt entries per clip; clip c's run starts at entry c * Fc. launches: the clip ranges
    (c0, c1) of the launches, in order, each of at most max_frames // Fc clips so that its table ((c1 - c0) * Fc entries,
    clip c0's run first) fits. A single clip whose run alone overflows the table (Fc > max_frames) gets a launch range of
    its own; the caller runs it on the one-clip path, which chunks over output frames."""
    if Tc < 1 or stride_t < 1 or kt < 1 or n_clips < 1:
        raise ValueError(f"clip_table_layout: Tc {Tc}, stride_t {stride_t}, kt {kt}, n_clips {n_clips}")
    Fc = (Tc - 1) * stride_t + kt
    per = max(1, max_frames // Fc)
    return Fc, [(c0, min(n_clips, c0 + per)) for c0 in range(0, n_clips, per)]


def clip_table_entry(clip: int, frame: int, tap: int, Fc: int, stride_t: int) -> int:
    """The table entry output frame `frame` of clip `clip` reads at time tap `tap` (clip counted within its launch)."""
    return clip * Fc + frame * stride_t + tap


# ----------------------------------------------------------------------------- conv helpers
class _Conv:
    """One convolution with device weights repacked [Cout][KT][KH][KW][Cin_pad]."""

    def __init__(self, w: torch.Tensor, b: Optional[torch.Tensor], device, out_rows: Optional[int] = None):
        if w.dim() == 4:
            w = w.unsqueeze(2)  # Conv2d -> KT = 1
        if out_rows is not None:
            w = w[:out_rows]
            b = b[:out_rows] if b is not None else None
        cout, cin, kt, kh, kw = w.shape
        cin_p = ((cin + 15) // 16) * 16
        wp = torch.zeros((cout, kt, kh, kw, cin_p), dtype=BF16, device=device)
        wp[..., :cin] = w.to(device=device, dtype=BF16).permute(0, 2, 3, 4, 1)
        self.w = wp.contiguous()
        self.b = b.to(device=device, dtype=BF16).contiguous() if b is not None else None
        self.cout, self.cin, self.cin_p, self.kt, self.kh, self.kw = cout, cin, cin_p, kt, kh, kw

    def __call__(self, frames: List[Optional[torch.Tensor]], Tout: int, H: int, W: int, *, stride_t=1, stride_hw=1,
                 pad=(0, 0, 0, 0), upsample=False, out_split=0, residual=None, n_clips=1, out=None) -> torch.Tensor:
        """frames: the frame table; Tout output frames. n_clips > 1: `frames` is n_clips equal runs (each clip's causal
        history, then its frames) and Tout counts every clip's output frames, clip-major (cp25_conv3d_clips)."""
        dev = self.w.device
        Hu, Wu = (2 * H, 2 * W) if upsample else (H, W)
        Ho = (Hu + pad[0] + pad[2] - self.kh) // stride_hw + 1
        Wo = (Wu + pad[1] + pad[3] - self.kw) // stride_hw + 1
        if out is not None:
            pass  # (a slice of a batch's output)
        elif out_split:
            out = torch.empty((2 * Tout, Ho, Wo, out_split), dtype=BF16, device=dev)
        else:
            out = torch.empty((Tout, Ho, Wo, self.cout), dtype=BF16, device=dev)
        f = 2 if out_split else 1
        if n_clips > 1:
            kw = dict(Hin=H, Win=W, Cin=self.cin_p, Cout=self.cout, KT=self.kt, KH=self.kh, KW=self.kw,
                      stride_t=stride_t, stride_hw=stride_hw, pad=pad, upsample=upsample, out_split=out_split)
            if Tout % n_clips or len(frames) % n_clips:
                raise ValueError(f"{Tout} output frames / {len(frames)} table entries do not split into {n_clips} clips")
            Tc, L = Tout // n_clips, len(frames) // n_clips
            Fc, launches = clip_table_layout(Tc, stride_t, self.kt, n_clips)
            if L < Fc:
                raise ValueError(f"a clip brings {L} frames, {Tc} output frames read {Fc}")
            for c0, c1 in launches:
                o = out[f * c0 * Tc: f * c1 * Tc]
                r = None if residual is None else residual[f * c0 * Tc: f * c1 * Tc]
                if Fc > MAX_FRAMES:  # (c1 = c0 + 1) one clip overflows the table: the one-clip path chunks its frames
                    self(frames[c0 * L: c0 * L + Fc], Tc, H, W, stride_t=stride_t, stride_hw=stride_hw, pad=pad,
                         upsample=upsample, out_split=out_split, residual=r, out=o)
                    continue
                tab = [fr for c in range(c0, c1) for fr in frames[c * L: c * L + Fc]]
                N.conv3d_clips(tab, c1 - c0, self.w, self.b, o, Tout=(c1 - c0) * Tc, residual=r, **kw)
            return out
        # the kernel takes at most MAX_FRAMES input frames per launch: chunk the output frames
        per = max(1, (MAX_FRAMES - self.kt) // stride_t + 1)
        for t0 in range(0, Tout, per):
            t1 = min(Tout, t0 + per)
            fr = frames[t0 * stride_t: (t1 - 1) * stride_t + self.kt]
            N.conv3d(fr, self.w, self.b, out[f * t0: f * t1], Hin=H, Win=W, Cin=self.cin_p, Cout=self.cout,
                     Tout=t1 - t0, KT=self.kt, KH=self.kh, KW=self.kw, stride_t=stride_t, stride_hw=stride_hw,
                     pad=pad, upsample=upsample, out_split=out_split,
                     residual=None if residual is None else residual[f * t0: f * t1])
        return out


def _frames(x: torch.Tensor) -> List[torch.Tensor]:
    return [x[i] for i in range(x.shape[0])]


class _FeatCache:
    def __init__(self):
        self.slots: Dict[int, object] = {}
        self.idx = 0


class WanVAE:
    """Encoder/decoder over channels-last clips. B clips of one size run in lock-step through one sequence of launches:
    an activation is [B * T, H, W, C], clip-major (clip b's T frames at rows b T .. b T + T - 1), so the per-pixel and
    per-frame kernels (rms_norm_silu, vae_attn) see B * T frames, and every convolution gets a frame table of B runs,
    clip b's causal history followed by clip b's frames (cp25_conv3d_clips; _Conv splits the clips over several launches
    where the runs overflow one table). The feature cache holds B * k frames per slot the same way. B = 1 is the one-clip
    path: the same launches as before the batch existed."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", dim=96, z_dim=16,
                 temporal_window: int = 16):
        self.device = torch.device(device)
        self.dim, self.z_dim, self.temporal_window = dim, z_dim, temporal_window
        sd = {k: v for k, v in state_dict.items()}
        self.convs: Dict[str, _Conv] = {}
        self.gammas: Dict[str, torch.Tensor] = {}
        for k, v in sd.items():
            if k.endswith(".weight"):
                name = k[: -len(".weight")]
                if name == "conv1":  # only mu = the first z_dim output channels is ever used
                    self.convs[name] = _Conv(v, sd.get(name + ".bias"), self.device, out_rows=z_dim)
                else:
                    self.convs[name] = _Conv(v, sd.get(name + ".bias"), self.device)
            elif k.endswith(".gamma"):
                self.gammas[k[: -len(".gamma")]] = v.to(self.device, BF16).reshape(-1).contiguous()
        mean = torch.tensor(_MEAN, dtype=BF16, device=self.device)
        std = torch.tensor(_STD, dtype=BF16, device=self.device)
        self.mean, self.inv_std = mean, 1.0 / std
        self.cp_group = None  # decode shards latent rows over this group (see module docstring)
        self._band = None  # (group, rank, world) while a banded decode runs
        self._nb = 1  # clips in flight (set by encode / decode for the call)

    # ---------------------------------------------------------------- context-parallel bands
    def _halo(self, x: torch.Tensor) -> torch.Tensor:
        """[T, R, W, C] band -> [T, R + 2, W, C] with the neighbouring bands' edge rows (zeros at the
        image's top and bottom edge)."""
        group, r, n = self._band
        T, R, W, C = x.shape
        xh = torch.empty((T, R + 2, W, C), dtype=x.dtype, device=x.device)
        xh[:, 1:R + 1] = x
        edge = torch.stack([x[:, 0], x[:, R - 1]], 0)  # [2, T, W, C]
        allv = torch.empty((n,) + tuple(edge.shape), dtype=x.dtype, device=x.device)
        cpx.all_gather_into(allv, edge, group)
        if r > 0:
            xh[:, 0] = allv[r - 1, 1]
        else:
            xh[:, 0].zero_()
        if r < n - 1:
            xh[:, R + 1] = allv[r + 1, 0]
        else:
            xh[:, R + 1].zero_()
        return xh

    # ---------------------------------------------------------------- clip-major helpers
    def _tail(self, x: torch.Tensor, k: int) -> torch.Tensor:
        """A copy of the last k frames of every clip (all of them where a clip has fewer), clip-major."""
        if self._nb == 1:
            return x[-k:].clone()
        return x.unflatten(0, (self._nb, -1))[:, -k:].clone(memory_format=torch.contiguous_format).flatten(0, 1)

    def _last(self, x: torch.Tensor) -> torch.Tensor:
        """Every clip's last frame, [B, H, W, C]."""
        if self._nb == 1:
            return x[-1:]
        return x.unflatten(0, (self._nb, -1))[:, -1]

    def _cat_t(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """Per clip: a's frames, then b's."""
        if self._nb == 1:
            return torch.cat([a, b], 0)
        return torch.cat([a.unflatten(0, (self._nb, -1)), b.unflatten(0, (self._nb, -1))], 1).flatten(0, 1)

    def _cat_clips(self, parts: List[torch.Tensor]) -> torch.Tensor:
        """Clip-major pieces [nb * k_i, ...] of consecutive time ranges -> [nb * sum k_i, ...], clip-major."""
        if self._nb == 1:
            return torch.cat(parts, 0)
        return torch.cat([p.unflatten(0, (self._nb, -1)) for p in parts], 1).flatten(0, 1)

    def _table(self, prev: Optional[torch.Tensor], x: torch.Tensor, n_pre: int = 2) -> List[Optional[torch.Tensor]]:
        """The frame table of a causal conv: per clip n_pre history entries (the clip's cached frames `prev`, zero
        frames = None in front where it has fewer) and then the clip's frames of x."""
        nb = self._nb
        if nb == 1:
            if prev is None:
                return [None] * n_pre + _frames(x)
            return [None] * (n_pre - prev.shape[0]) + _frames(prev) + _frames(x)
        T = x.shape[0] // nb
        kp = 0 if prev is None else prev.shape[0] // nb
        tab: List[Optional[torch.Tensor]] = []
        for b in range(nb):
            tab += [None] * (n_pre - kp)
            tab += [prev[b * kp + j] for j in range(kp)]
            tab += [x[b * T + j] for j in range(T)]
        return tab

    def _push(self, cache: _FeatCache, x: torch.Tensor):
        """The feat_cache rule of a CausalConv3d (wan2pt1.py:206-219): the slot takes every clip's last CACHE_T frames
        (topped up with the previous entry's last frame); returns the previous entry."""
        i = cache.idx
        prev = cache.slots.get(i)
        if self._nb == 1:
            cache_x = x[-CACHE_T:].clone()
            if cache_x.shape[0] < 2 and prev is not None:
                cache_x = torch.cat([prev[-1:], cache_x], 0)
        else:
            cache_x = self._tail(x, CACHE_T)
            if cache_x.shape[0] // self._nb < 2 and prev is not None:
                cache_x = self._cat_t(self._last(prev), cache_x)
        cache.slots[i] = cache_x
        cache.idx += 1
        return prev

    # ---------------------------------------------------------------- building blocks
    def _causal(self, name, x, cache: Optional[_FeatCache], H, W):
        """CausalConv3d 3x3x3 (pad 1) with the feat_cache rule (wan2pt1.py:206-219)."""
        conv = self.convs[name]
        pad = (1, 1, 1, 1)
        if self._band is not None:
            x = self._halo(x)
            H, pad = H + 2, (0, 1, 0, 1)
        prev = self._push(cache, x) if cache is not None else None
        return conv(self._table(prev, x), x.shape[0], H, W, pad=pad, n_clips=self._nb)

    def _res(self, p, x, cache, H, W, cin, cout):
        if cin != cout:
            h = self.convs[p + ".shortcut"](_frames(x), x.shape[0], H, W, n_clips=self._nb)
        else:
            h = x
        y = N.rms_norm_silu(x, self.gammas[p + ".residual.0"], silu=True)
        y = self._causal_res(p + ".residual.2", y, cache, H, W)
        y = N.rms_norm_silu(y, self.gammas[p + ".residual.3"], silu=True)
        return self._causal_res(p + ".residual.6", y, cache, H, W, residual=h)

    def _causal_res(self, name, x, cache, H, W, residual=None):
        conv = self.convs[name]
        pad = (1, 1, 1, 1)
        if self._band is not None:
            x = self._halo(x)
            H, pad = H + 2, (0, 1, 0, 1)
        prev = self._push(cache, x)
        return conv(self._table(prev, x), x.shape[0], H, W, pad=pad, residual=residual, n_clips=self._nb)

    def _attn(self, p, x, H, W):
        C = x.shape[-1]
        T = x.shape[0]
        y = N.rms_norm_silu(x, self.gammas[p + ".norm"], silu=False)
        qkv = self.convs[p + ".to_qkv"](_frames(y), T, H, W, n_clips=self._nb)  # [T, H, W, 3C]
        qkv = qkv.view(T, H * W, 3 * C)
        q, k, v = qkv[:, :, :C], qkv[:, :, C:2 * C], qkv[:, :, 2 * C:]
        if self._band is not None:  # K/V of the whole frame: every band's rows, in row order
            group, _, n = self._band
            kv = qkv[:, :, C:].contiguous()
            kv_all = torch.empty((n,) + tuple(kv.shape), dtype=BF16, device=self.device)
            cpx.all_gather_into(kv_all, kv, group)
            kv_all = kv_all.permute(1, 0, 2, 3).reshape(T, n * H * W, 2 * C)  # [T, all rows, 2C]
            k, v = kv_all[:, :, :C], kv_all[:, :, C:]
        # F.scaled_dot_product_attention(q, k, v) on bf16, one head (wan2pt1.py:251-254): the flash kernel
        # cp25_vae_attn (fp32 scores, bf16 P), no score matrix in HBM
        o = N.vae_attn(q, k, v)
        o = o.view(T, H, W, C)
        return self.convs[p + ".proj"](_frames(o), T, H, W, residual=x, n_clips=self._nb)

    def _resample(self, p, kind, x, cache, H, W):
        T = x.shape[0]
        if kind == "upsample3d" and cache is not None:
            i = cache.idx
            prev = cache.slots.get(i)
            if prev is None:
                cache.slots[i] = "Rep"
                cache.idx += 1
            else:
                nb = self._nb
                cache_x = self._tail(x, CACHE_T)
                if cache_x.shape[0] // nb < 2 and not isinstance(prev, str):
                    cache_x = self._cat_t(self._last(prev), cache_x)
                if cache_x.shape[0] // nb < 2 and isinstance(prev, str):
                    cache_x = self._cat_t(torch.zeros_like(cache_x), cache_x)
                tab = self._table(None if isinstance(prev, str) else prev, x)
                x = self.convs[p + ".time_conv"](tab, T, H, W, out_split=x.shape[-1], n_clips=nb)
                cache.slots[i] = cache_x
                cache.idx += 1
        T = x.shape[0]
        conv = self.convs[p + ".resample.1"]
        if kind.startswith("upsample") and self._band is not None:
            # haloed low-res band; in upsampled coordinates the output rows start one row in: pads -1
            xh = self._halo(x)
            y = conv(_frames(xh), T, H + 2, W, pad=(-1, 1, -1, 1), upsample=True)
            H, W = 2 * H, 2 * W
        elif kind.startswith("upsample"):
            y = conv(_frames(x), T, H, W, pad=(1, 1, 1, 1), upsample=True, n_clips=self._nb)
            H, W = 2 * H, 2 * W
        else:
            y = conv(_frames(x), T, H, W, stride_hw=2, pad=(0, 0, 1, 1), n_clips=self._nb)
            H, W = H // 2, W // 2
        if kind == "downsample3d" and cache is not None:
            i = cache.idx
            prev = cache.slots.get(i)
            if prev is None:
                cache.slots[i] = y.clone()
                cache.idx += 1
            else:
                nb = self._nb
                cache_x = self._tail(y, 1)
                fr = self._table(self._last(prev), y, n_pre=1)
                tout = (len(fr) // nb - 3) // 2 + 1  # per clip
                y = self.convs[p + ".time_conv"](fr, nb * tout, H, W, stride_t=2, n_clips=nb)
                cache.slots[i] = cache_x
                cache.idx += 1
        return y, H, W

    # ---------------------------------------------------------------- encoder / decoder
    def _encoder(self, x, cache, H, W):
        x = self._causal("encoder.conv1", x, cache, H, W)
        for i, (kind, ci, co) in enumerate(encoder_layers(self.dim)):
            p = f"encoder.downsamples.{i}"
            if kind == "res":
                x = self._res(p, x, cache, H, W, ci, co)
            else:
                x, H, W = self._resample(p, kind, x, cache, H, W)
        top = 4 * self.dim
        x = self._res("encoder.middle.0", x, cache, H, W, top, top)
        x = self._attn("encoder.middle.1", x, H, W)
        x = self._res("encoder.middle.2", x, cache, H, W, top, top)
        x = N.rms_norm_silu(x, self.gammas["encoder.head.0"], silu=True)
        return self._causal("encoder.head.2", x, cache, H, W), H, W

    def _decoder(self, x, cache, H, W):
        x = self._causal("decoder.conv1", x, cache, H, W)
        top = 4 * self.dim
        x = self._res("decoder.middle.0", x, cache, H, W, top, top)
        x = self._attn("decoder.middle.1", x, H, W)
        x = self._res("decoder.middle.2", x, cache, H, W, top, top)
        for i, (kind, ci, co) in enumerate(decoder_layers(self.dim)):
            p = f"decoder.upsamples.{i}"
            if kind == "res":
                x = self._res(p, x, cache, H, W, ci, co)
            else:
                x, H, W = self._resample(p, kind, x, cache, H, W)
        x = N.rms_norm_silu(x, self.gammas["decoder.head.0"], silu=True)
        return self._causal("decoder.head.2", x, cache, H, W), H, W

    @torch.no_grad()
    def encode(self, video: torch.Tensor) -> torch.Tensor:
        """video [B, 3, T, H, W] (bf16 in [-1, 1]) -> mu [B, 16, 1 + (T-1)//4, H/8, W/8] bf16; the B clips run in
        lock-step (class docstring), each with the bits of its own B = 1 call."""
        if video.dim() != 5 or video.shape[0] < 1:
            raise ValueError(f"encode takes a [B, C, T, H, W] video, got {tuple(video.shape)}")
        B, C, T, H, W = video.shape
        x = torch.zeros((B * T, H, W, 16), dtype=BF16, device=self.device)  # channels padded 3 -> 16
        x.view(B, T, H, W, 16)[..., :C] = video.to(self.device, BF16).permute(0, 2, 3, 4, 1)
        return self._encode_clip(x, B)

    @torch.no_grad()
    def encode_u8(self, video_u8: torch.Tensor) -> torch.Tensor:
        """uint8 device video [B, 3, T, H, W] (any strides) -> mu, as encode(video.to(bf16) / 127.5 - 1.0): the
        normalisation, the channels-last permute and the 3 -> 16 channel pad are one kernel (cp25_u8_to_clip) per clip
        writing the encoder's input clip."""
        if video_u8.dim() != 5 or video_u8.shape[0] < 1 or video_u8.dtype != torch.uint8:
            raise ValueError(f"encode_u8 takes a uint8 [B, C, T, H, W] video, got {video_u8.dtype} {tuple(video_u8.shape)}")
        B = video_u8.shape[0]
        if B == 1:
            return self._encode_clip(N.u8_to_clip(video_u8[0].to(self.device)))
        _, _, T, H, W = video_u8.shape
        x = torch.empty((B * T, H, W, 16), dtype=BF16, device=self.device)
        for b in range(B):
            N.u8_to_clip(video_u8[b].to(self.device), out=x[b * T:(b + 1) * T])
        return self._encode_clip(x, B)

    def _encode_clip(self, x: torch.Tensor, nb: int = 1) -> torch.Tensor:
        """x [nb * T, H, W, 16] bf16 channels-last clips (clip-major) -> mu [nb, 16, Tl, H/8, W/8]."""
        _, H, W, _ = x.shape
        T = x.shape[0] // nb
        x5 = x.view(nb, T, H, W, 16)
        cache = _FeatCache()
        tw = self.temporal_window
        chunks = [x5[:, :1]]
        n_iter = 1 + (T - 1) // tw
        for i in range(1, n_iter):
            chunks.append(x5[:, 1 + tw * (i - 1): 1 + tw * i])
        if (T - 1) % tw:
            chunks.append(x5[:, 1 + tw * (n_iter - 1):])
        outs = []
        self._nb = nb
        try:
            for ch in chunks:
                cache.idx = 0
                o, h, w = self._encoder(ch.contiguous().flatten(0, 1), cache, H, W)
                outs.append(o)
            out = self._cat_clips(outs)
            mu = self.convs["conv1"](_frames(out), out.shape[0], h, w, n_clips=nb)  # [nb * Tl, h, w, 16]
        finally:
            self._nb = 1
        mu = (mu - self.mean) * self.inv_std
        return mu.unflatten(0, (nb, -1)).permute(0, 4, 1, 2, 3).contiguous()

    @torch.no_grad()
    def decode(self, z: torch.Tensor) -> torch.Tensor:
        """latent [B, 16, T, h, w] -> video [B, 3, 1 + 4 (T-1), 8h, 8w] bf16; the B clips run in lock-step (class
        docstring), each with the bits of its own B = 1 call. The banded (context-parallel) decode takes B = 1."""
        return self._decode_clip(z).unflatten(0, (z.shape[0], -1)).permute(0, 4, 1, 2, 3).contiguous()

    @torch.no_grad()
    def decode_u8(self, z: torch.Tensor, layout: str = "THWC") -> torch.Tensor:
        """latent -> uint8 video, [T, H, W, 3] ("THWC") or [1, 3, T, H, W] ("NCTHW"): decode's channels-last
        result quantised by cp25_clip_to_u8 (trunc(clamp((v + 1) / 2, 0, 1) * 255)), with no NCTHW or fp32 copy.
        B > 1 latents give [B, T, H, W, 3] or [B, 3, T, H, W], clip b as its own B = 1 call."""
        if layout not in ("THWC", "NCTHW"):
            raise ValueError(f"layout must be 'THWC' or 'NCTHW', got {layout!r}")
        return self._clips_u8(self._decode_clip(z), z.shape[0], layout)

    @staticmethod
    def _clips_u8(clips: torch.Tensor, B: int, layout: str) -> torch.Tensor:
        """decode_u8's quantisation of the channels-last clips [B * t, H, W, 3] (clip-major)."""
        from .pixels import clip_to_uint8

        if B == 1:
            return clip_to_uint8(clips, layout)
        outs = [clip_to_uint8(c, layout) for c in clips.unflatten(0, (B, -1))]
        return torch.stack(outs, 0) if layout == "THWC" else torch.cat(outs, 0)

    def _unnormalised(self, z: torch.Tensor) -> torch.Tensor:
        """latent [nb, 16, T, h, w] -> the decoder's channels-last clips [nb * T, h, w, 16] bf16, z / inv_std + mean."""
        zl = z.to(self.device, BF16).permute(0, 2, 3, 4, 1).contiguous().flatten(0, 1)
        return zl / self.inv_std + self.mean

    def _conv2(self, zl: torch.Tensor, h: int, w: int) -> torch.Tensor:
        """The decoder's 1x1x1 conv2 over every frame of the self._nb clips zl [nb * T, h, w, 16] (clip-major)."""
        return self.convs["conv2"](_frames(zl), zl.shape[0], h, w, n_clips=self._nb)

    def decode_stream(self, n_clips: int = 1) -> "DecodeStream":
        """A decoder of n_clips clips in lock-step that takes one latent frame per push (DecodeStream)."""
        return DecodeStream(self, n_clips)

    def _decode_clip(self, z: torch.Tensor) -> torch.Tensor:
        """latent [B, 16, T, h, w] -> channels-last video [B * Tp, H, W, 3] bf16, clip-major (bands gathered under CP)."""
        if z.dim() != 5 or z.shape[0] < 1:
            raise ValueError(f"decode takes a [B, 16, T, h, w] latent, got {tuple(z.shape)}")
        nb, C, T, h, w = z.shape
        zl = self._unnormalised(z)
        group = self.cp_group
        r, n = cpx.cp_rank_world(group)
        if n > 1 and h % n == 0:
            if nb > 1:
                raise ValueError(f"the banded (context-parallel) decode takes one clip, got a batch of {nb}")
            self._band = (group, r, n)
            zl = zl[:, r * (h // n):(r + 1) * (h // n)]
            h = h // n
        self._nb = nb
        try:
            x = self._conv2(zl.contiguous(), h, w)
            x5 = x.unflatten(0, (nb, T))
            cache = _FeatCache()
            outs = []
            for i in range(T):
                cache.idx = 0
                o, H, W = self._decoder(x5[:, i: i + 1].contiguous().flatten(0, 1), cache, h, w)
                outs.append(o)
            video = self._cat_clips(outs)  # [nb * Tp, H, W, 3] (this rank's band of H rows when banded)
            if self._band is not None:
                allv = torch.empty((n,) + tuple(video.shape), dtype=video.dtype, device=video.device)
                cpx.all_gather_into(allv, video, group)
                video = allv.permute(1, 0, 2, 3, 4).reshape(video.shape[0], n * video.shape[1], *video.shape[2:])
        finally:
            self._band = None
            self._nb = 1
        return video


class DecodeStream:
    """WanVAE.decode one latent frame at a time: the decoder is causal and _decode_clip already runs it frame by frame
    over a feature cache, so a stream that owns that cache between calls gives decode's frames as the latents arrive.
    push(z) takes the next latent frame of the n_clips clips, z [B, 16, 1, h, w] (a normalised latent, as decode takes)
    or [B, h, w, 16] bf16 channels-last and already un-normalised (cp25_stream_latent_clip's output), and returns the
    decoder's frames of it, [B * t, H, W, 3] bf16 clip-major: t = 1 for the first push, 4 for every later one. The pushes
    of the frames of z [B, 16, T, h, w] concatenated per clip are decode(z) bit for bit. The VAE's clip count is set per
    push, so decode, encode and other streams of the same WanVAE may run between two pushes. One clip size per stream;
    not under a context-parallel group (the banded decode gathers whole clips)."""

    def __init__(self, vae: "WanVAE", n_clips: int = 1):
        if int(n_clips) < 1:
            raise ValueError(f"a decode stream takes at least one clip, got {n_clips}")
        self.vae, self.n_clips = vae, int(n_clips)
        self._check_cp()
        self.cache = _FeatCache()
        self.frames = 0  # latent frames pushed
        self.hw: Optional[Tuple[int, int]] = None

    def _check_cp(self) -> None:
        if self.vae.cp_group is not None:
            raise ValueError("decode_stream does not run under a context-parallel group (the banded decode takes a "
                             "whole clip)")

    @torch.no_grad()
    def push(self, z: torch.Tensor) -> torch.Tensor:
        vae, nb = self.vae, self.n_clips
        self._check_cp()
        if z.dim() == 5 and z.shape[0] == nb and z.shape[1] == vae.z_dim and z.shape[2] == 1:
            zl = vae._unnormalised(z)
        elif z.dim() == 4 and z.shape[0] == nb and z.shape[3] == vae.z_dim and z.dtype == BF16:
            zl = z.to(vae.device)
        else:
            raise ValueError(f"push takes one latent frame of {nb} clips, [{nb}, {vae.z_dim}, 1, h, w] or un-normalised "
                             f"bf16 [{nb}, h, w, {vae.z_dim}], got {z.dtype} {tuple(z.shape)}")
        h, w = zl.shape[1:3]
        if self.hw is None:
            self.hw = (h, w)
        elif self.hw != (h, w):
            raise ValueError(f"this stream decodes {self.hw} latents, got {(h, w)}")
        vae._nb = nb
        try:
            x = vae._conv2(zl.contiguous(), h, w)  # [nb, h, w, 16]
            self.cache.idx = 0
            o, _, _ = vae._decoder(x, self.cache, h, w)
        finally:
            vae._nb = 1
        self.frames += 1
        return o

    def push_rows(self, rows: torch.Tensor, Hp: int, Wp: int) -> torch.Tensor:
        """push of one frame of the streaming student's token-major state, rows [Hp * Wp, B, 64] bf16
        (StreamingBatchRun.frame_rows): the rows go to the decoder's un-normalised frame in one kernel
        (cp25_stream_latent_clip), with no NCTHW latent in between."""
        if rows.dim() != 3 or rows.shape[1] != self.n_clips:
            raise ValueError(f"rows must be [hw, {self.n_clips}, 64], got {tuple(rows.shape)}")
        return self.push(N.stream_latent_clip(rows, self.vae.inv_std, self.vae.mean, Hp, Wp))

    def push_video(self, z: torch.Tensor) -> torch.Tensor:
        """push in decode's layout: [B, 3, t, H, W] bf16."""
        return self.push(z).unflatten(0, (self.n_clips, -1)).permute(0, 4, 1, 2, 3).contiguous()

    def push_u8(self, z: torch.Tensor, layout: str = "THWC") -> torch.Tensor:
        """push quantised as decode_u8 does: [t, H, W, 3] / [1, 3, t, H, W] for one clip, [B, t, H, W, 3] /
        [B, 3, t, H, W] for more."""
        if layout not in ("THWC", "NCTHW"):
            raise ValueError(f"layout must be 'THWC' or 'NCTHW', got {layout!r}")
        return self.vae._clips_u8(self.push(z), self.n_clips, layout)


class Wan2pt1VAEInterface:
    """VideoTokenizerInterface of the reference (tokenizers/interface.py:25-98, wan2pt1.py:961-1060)."""

    def __init__(self, state_dict: Dict[str, torch.Tensor], device="cuda", temporal_window: int = 16,
                 chunk_duration: int = 81):
        self.model = WanVAE(state_dict, device=device, temporal_window=temporal_window)
        self.chunk_duration = chunk_duration

    def set_context_parallel_group(self, group) -> None:
        """Decode shards latent rows over `group` (WanVAE module docstring); encode stays replicated."""
        self.model.cp_group = group

    def encode(self, state: torch.Tensor) -> torch.Tensor:
        in_dtype = state.dtype
        return self.model.encode(state).to(in_dtype)

    def decode(self, latent: torch.Tensor) -> torch.Tensor:
        in_dtype = latent.dtype
        return self.model.decode(latent).to(in_dtype)

    def encode_u8(self, video_u8: torch.Tensor) -> torch.Tensor:
        """uint8 [B, 3, T, H, W] device video -> bf16 latent (WanVAE.encode_u8)."""
        return self.model.encode_u8(video_u8)

    def decode_u8(self, latent: torch.Tensor, layout: str = "THWC") -> torch.Tensor:
        """latent -> uint8 device video [T, H, W, 3] ("THWC") or [1, 3, T, H, W] ("NCTHW"); [B, ...] latents with
        B > 1 give [B, T, H, W, 3] or [B, 3, T, H, W] (WanVAE.decode_u8)."""
        return self.model.decode_u8(latent, layout)

    def decode_stream(self, n_clips: int = 1) -> DecodeStream:
        """A decoder that takes one latent frame of n_clips clips per push (WanVAE.decode_stream)."""
        return self.model.decode_stream(n_clips)

    def get_latent_num_frames(self, num_pixel_frames: int) -> int:
        return 1 + (num_pixel_frames - 1) // 4

    def get_pixel_num_frames(self, num_latent_frames: int) -> int:
        return (num_latent_frames - 1) * 4 + 1

    @property
    def spatial_compression_factor(self) -> int:
        return 8

    @property
    def temporal_compression_factor(self) -> int:
        return 4

    @property
    def latent_ch(self) -> int:
        return 16

    @property
    def pixel_chunk_duration(self) -> int:
        return self.chunk_duration

    @property
    def latent_chunk_duration(self) -> int:
        return self.get_latent_num_frames(self.chunk_duration)

    @property
    def spatial_resolution(self) -> int:
        return 512

    @property
    def name(self) -> str:
        return "wan2pt1_tokenizer"
