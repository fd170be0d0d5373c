"""Truths for the LoRA merge (cp25_lora_merge, MinimalV1LVGDiT.merge_lora): CPU only, no package code.

merge_restated  the kernel's arithmetic as separate fp32 torch ops (torch CPU elementwise ops never contract): the
                exact tests compare bits against it.
merge_truth64   an independent formula in float64, W + (lora_scale * alpha / r) * (B @ A): tests/test_lora_cpu.py holds
                the restatement to it, so a transposed operand or a wrong scale in the restatement cannot hide.
"""
import math

import torch

BF16 = torch.bfloat16
F32 = torch.float32

# name -> (N, K, ldw, r, scale): the kernel test's shapes (tests/test_lora_merge_gpu.py)
SHAPES = {
    "rank1": (256, 64, 64, 1, 1.0),
    "ragged": (130, 72, 72, 5, 8.0 / 12.0),
    "guard_cols": (96, 64, 192, 33, 0.5),
    "recipe_xattn_kv": (512, 1024, 1024, 32, 1.0),
    "rank256": (64, 2048, 2048, 256, 2.0),
    "qkv_slice": (512, 512, 512, 32, 1.0),  # the middle 512 rows of a 1536 x 512 buffer
}


def fp32_scale(lora_scale: float, alpha: float, r: int) -> float:
    """fp32(lora_scale * alpha / r), the product and quotient taken in double."""
    return torch.tensor(float(lora_scale) * float(alpha) / r, dtype=torch.float64).to(F32).item()


def make_case(N: int, K: int, r: int, seed: int):
    """W bf16 [N, K] truncated normal (std 1 / sqrt(K), +-3 std: init_state_dict's), A fp32 [r, K] uniform
    +-1 / sqrt(K) (peft's Kaiming-uniform init of lora_A), B fp32 [N, r] N(0, 0.02), non-zero (a trained adapter; peft
    initialises it to zero)."""
    g = torch.Generator().manual_seed(seed)
    std = 1.0 / math.sqrt(K)
    w = torch.empty(N, K, dtype=F32)
    torch.nn.init.trunc_normal_(w, std=std, a=-3 * std, b=3 * std, generator=g)
    a = (torch.rand(r, K, generator=g, dtype=F32) * 2 - 1) * std
    b = torch.randn(N, r, generator=g, dtype=F32) * 0.02
    assert b.abs().max() > 0
    return w.to(BF16), a, b


def cases():
    """name -> (W, A, B, scale) for every entry of SHAPES, fixed seeds."""
    out = {}
    for i, (name, (N, K, _, r, scale)) in enumerate(SHAPES.items()):
        w, a, b = make_case(N, K, r, seed=100 + i)
        out[name] = (w, a, b, scale)
    return out


def merge_restated(w_bf16: torch.Tensor, a: torch.Tensor, b: torch.Tensor, scale: float, pre_rounding: bool = False):
    """acc = 0; for j ascending: acc = acc + (B[:, j] * A[j, :]) in fp32, product and sum rounded separately; then
    bf16(float(W) + acc * fp32(scale)). pre_rounding=True returns the fp32 value ahead of the bf16 rounding."""
    assert w_bf16.dtype == BF16 and a.dtype == F32 and b.dtype == F32
    assert a.shape[0] == b.shape[1] and a.shape[1] == w_bf16.shape[1] and b.shape[0] == w_bf16.shape[0]
    acc = torch.zeros(w_bf16.shape, dtype=F32)
    for j in range(a.shape[0]):
        prod = b[:, j:j + 1] * a[j:j + 1, :]
        acc = acc + prod
    delta = acc * torch.tensor(scale, dtype=F32)
    assert delta.dtype == F32
    out = w_bf16.float() + delta
    return out if pre_rounding else out.to(BF16)


def merge_truth64(w: torch.Tensor, a: torch.Tensor, b: torch.Tensor, alpha: float, r: int, lora_scale: float = 1.0):
    """W + (lora_scale * alpha / r) * (B @ A) in float64."""
    assert a.shape[0] == r
    return w.double() + (lora_scale * alpha / r) * (b.double() @ a.double())


def bf16_half_ulp(x: torch.Tensor) -> torch.Tensor:
    """Half the bf16 spacing at |x| (float64): 2^(floor(log2 |x|) - 8); bf16's smallest normal binade below it."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 8)
