"""Ground truth for the Reason1 text encoder (cosmos_predict2/text_encoder.py): a CPU restatement of the language half
of Qwen2.5-VL as the reference's online encoder runs it (text_encoders/text_encoder.py:131-220,
reason1/networks/qwen2_5_vl.py), written op by op. No GPU, no product code.

Two modes, as stream_truth.py has them:

  rounded=True   every reference op on bf16 tensors is one fp32 evaluation followed by one bf16 rounding, in the
                 reference's order: what the HIP encoder computes, up to the fp32 summation order of its GEMMs, norms
                 and attention (the "bf16 truth");
  rounded=False  no rounding at all, every op in `dtype` (float32 or float64): the architecture itself, which
                 test_text_encoder_cpu.py holds against transformers' Qwen2_5_VLTextModel.

State dict: transformers' bare key layout (embed_tokens.weight, layers.N.self_attn.q_proj.weight / .bias, ...,
norm.weight), any float dtype.
"""
import math

import torch

BF16 = torch.bfloat16
EPS = 1e-6
ROPE_THETA = 1e6
HEAD_DIM = 128


def rb(t):
    """Round an fp32 tensor to bf16 values (kept in fp32): one bf16 tensor op's result."""
    return t.to(BF16).float()


def rope_tables(L, theta=ROPE_THETA, dtype=torch.float32):
    """cos / sin [L, 128] of Qwen2_5_VLRotaryEmbedding for position ids arange(L) on all three mrope rows: fp32
    inv_freq, fp32 angles, cat(freqs, freqs)."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.int64).to(dtype) / HEAD_DIM))
    freqs = torch.arange(L, dtype=dtype)[:, None] * inv_freq[None, :]
    emb = torch.cat([freqs, freqs], -1)
    return emb.cos(), emb.sin()


def rotate_half(x):
    return torch.cat([-x[..., 64:], x[..., :64]], -1)


def rmsnorm(x, w, rounded, eps=EPS):
    """Qwen2RMSNorm: statistics in the working precision; rounded: the normalised row goes to bf16 before the weight
    multiply, whose result is bf16 again. 1 / sqrt, not rsqrt (IEEE operations only)."""
    rstd = 1.0 / torch.sqrt((x * x).sum(-1, keepdim=True) / x.shape[-1] + eps)
    if rounded:
        return rb(w * rb(x * rstd))
    return w * (x * rstd)


def rope(x, cos, sin, rounded):
    """x [B, L, H, 128]; cos / sin [L, 128] (bf16 values in the rounded mode)."""
    c, s = cos[None, :, None, :], sin[None, :, None, :]
    if rounded:
        return rb(rb(x * c) + rb(rotate_half(x) * s))
    return x * c + rotate_half(x) * s


def causal_attention(q, k, v, scale, rounded):
    """q [B, L, Hq, 128], k / v [B, L, Hkv, 128] -> [B, L, Hq, 128]. rounded: the flash-style bf16-P form (fp32 scores
    and row sum of the unrounded weights, P rounded to bf16 for P V, one output rounding); else plain softmax."""
    B, L, Hq, D = q.shape
    g = Hq // k.shape[2]
    kk = k.repeat_interleave(g, dim=2)
    vv = v.repeat_interleave(g, dim=2)
    s = torch.einsum("bqhd,bkhd->bhqk", q, kk) * scale
    mask = torch.ones(L, L, dtype=torch.bool).tril()
    s = s.masked_fill(~mask, -math.inf)
    if not rounded:
        return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), vv)
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    o = torch.einsum("bhqk,bkhd->bqhd", rb(p), vv) / p.sum(-1).permute(0, 2, 1)[..., None]
    return rb(o)


def silu(x):
    return x / (1.0 + torch.exp(-x))


def swiglu(g, u, rounded):
    return rb(rb(silu(g)) * u) if rounded else silu(g) * u


def mean_normalize(t, rounded):
    """TextEncoder.mean_normalize. rounded: on a bf16 tensor, op by op: mean, difference, unbiased std (an fp32
    reduction about the fp32 mean), + 1e-8, quotient, each rounded to bf16."""
    if not rounded:
        return (t - t.mean(-1, keepdim=True)) / (t.std(-1, keepdim=True) + 1e-8)
    D = t.shape[-1]
    mean = t.sum(-1, keepdim=True) / D
    d = t - mean
    std = rb(torch.sqrt((d * d).sum(-1, keepdim=True) / (D - 1)))
    den = rb(std + torch.tensor(1e-8, dtype=torch.float32))
    return rb(rb(t - rb(mean)) / den)


def _linear(x, w, b, rounded):
    """x w^T (+ b): the rounded mode accumulates in float64 and rounds the sum once to bf16 (the GEMM's fp32
    accumulator with the bias inside, up to its summation order)."""
    if not rounded:
        y = x @ w.T
        return y if b is None else y + b
    y = x.double() @ w.double().T
    if b is not None:
        y = y + b.double()
    return rb(y.float())


def hidden_states(sd, ids, n_heads, n_kv_heads, rounded=True, dtype=torch.float32):
    """hidden_states[1:] of the text model for ids [B, L] (long): the residual stream after each layer, the last one
    through the final norm. A list of [B, L, D] tensors in `dtype` (fp32 holding bf16 values in the rounded mode)."""
    if rounded:
        dtype = torch.float32
        W = {k: rb(v.float()) for k, v in sd.items()}
    else:
        W = {k: v.to(dtype) for k, v in sd.items()}
    n_layers = 1 + max(int(k.split(".")[1]) for k in W if k.startswith("layers."))
    B, L = ids.shape
    cos, sin = rope_tables(L, dtype=torch.float32 if rounded else dtype)
    if rounded:
        cos, sin = rb(cos), rb(sin)
    x = W["embed_tokens.weight"][ids]
    scale = HEAD_DIM ** -0.5
    out = []
    y = None
    for i in range(n_layers):
        p = f"layers.{i}."
        if y is not None:
            x = rb(x + y) if rounded else x + y
            out.append(x)
        h = rmsnorm(x, W[p + "input_layernorm.weight"], rounded)
        q = _linear(h, W[p + "self_attn.q_proj.weight"], W[p + "self_attn.q_proj.bias"], rounded)
        k = _linear(h, W[p + "self_attn.k_proj.weight"], W[p + "self_attn.k_proj.bias"], rounded)
        v = _linear(h, W[p + "self_attn.v_proj.weight"], W[p + "self_attn.v_proj.bias"], rounded)
        q = rope(q.view(B, L, n_heads, HEAD_DIM), cos, sin, rounded)
        k = rope(k.view(B, L, n_kv_heads, HEAD_DIM), cos, sin, rounded)
        a = causal_attention(q, k, v.view(B, L, n_kv_heads, HEAD_DIM), scale, rounded)
        o = _linear(a.reshape(B, L, n_heads * HEAD_DIM), W[p + "self_attn.o_proj.weight"], None, rounded)
        x = rb(x + o) if rounded else x + o
        h = rmsnorm(x, W[p + "post_attention_layernorm.weight"], rounded)
        g = _linear(h, W[p + "mlp.gate_proj.weight"], None, rounded)
        u = _linear(h, W[p + "mlp.up_proj.weight"], None, rounded)
        y = _linear(swiglu(g, u, rounded), W[p + "mlp.down_proj.weight"], None, rounded)
    x = rb(x + y) if rounded else x + y
    out.append(rmsnorm(x, W["norm.weight"], rounded))
    return out


def encode(sd, ids, n_heads, n_kv_heads, rounded=True, dtype=torch.float32):
    """The full_concat embedding [B, L, n_layers * D]: every hidden state mean-normalised, concatenated."""
    hs = hidden_states(sd, ids, n_heads, n_kv_heads, rounded, dtype)
    return torch.cat([mean_normalize(h, rounded) for h in hs], -1)


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


# ---------------------------------------------------------------- exact inputs of the row-kernel tests
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def integer_rows(n, D, seed, lo=-8, hi=8, zero_mean=False):
    """Integer-valued bf16 rows [n, D] (|x| <= 8): every sum of the x, of their squares and of squared differences from
    an integer mean is an integer below 2^24, so it is exact in fp32 in any order. zero_mean: the second half of a row is
    the negated first half, so the row mean is exactly 0."""
    g = _gen(seed)
    x = torch.randint(lo, hi + 1, (n, D), generator=g).float()
    if zero_mean:
        x[:, D // 2:] = -x[:, :D // 2]
    return x.to(BF16)


def integer_mean_rows(n, D, seed, mean=3):
    """integer_rows(zero_mean=True) + an integer: the row mean is exactly `mean`, a bf16 value."""
    return (integer_rows(n, D, seed, -5, 5, zero_mean=True).float() + float(mean)).to(BF16)


def sums_exact(x, centered=False):
    """The premise of the exact tests: the fp32 sums a row kernel takes of these rows (x and x^2; centered: the row
    mean is a bf16 value and (x - mean)^2 as well), in ascending, descending and torch's own order, all equal the
    float64 sums."""
    xf, xd = x.float(), x.double()
    terms = [(xf, xd), (xf * xf, xd * xd)]
    ok = True
    if centered:
        mean = xd.mean(-1, keepdim=True)
        ok = torch.equal(mean.to(BF16).double(), mean)
        terms.append(((xf - mean.float()) ** 2, (xd - mean) ** 2))
    for tf, td in terms:
        want = td.sum(-1)
        asc = torch.zeros(tf.shape[0])
        for c in range(tf.shape[1]):
            asc = asc + tf[:, c]
        desc = torch.zeros(tf.shape[0])
        for c in reversed(range(tf.shape[1])):
            desc = desc + tf[:, c]
        ok = ok and torch.equal(asc.double(), want) and torch.equal(desc.double(), want)
        ok = ok and torch.equal(tf.sum(-1).double(), want)
    return ok


def bf16_order(t):
    """bf16 values as integers in value order (adjacent representable values differ by 1; +-0 coincide)."""
    i = t.to(BF16).view(torch.int16).int()
    return torch.where(i < 0, -(i & 0x7FFF), i)


def ulp_distance(a, b):
    """Per element, how many bf16 values apart a and b are (both finite bf16 tensors)."""
    return (bf16_order(a) - bf16_order(b)).abs()
