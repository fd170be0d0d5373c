#!/usr/bin/env python3
"""The Reason1 text encoder (cosmos_predict2/text_encoder.py) at the 7B size, synthetic weights drawn on the device.

    python tools/bench_text_encoder.py [--out profiles/r15/text_encoder] [--layers 28] [--passes 5] [--tokens 512]

One prompt = 512 ids through 28 layers. Reports

  * ms per prompt between device events (one untimed pass first: code load; then --passes timed passes), the spread
    of the passes, and the same with the weights parked in host memory (offload: the upload is then part of a prompt);
  * the split into GEMMs / causal attention / row kernels (gather, add + RMSNorm, rotary, SwiGLU, mean-normalise)
    from one further pass with a device event around every launch (the events add host time, so the parts are given
    as they were measured and as shares, not as a sum that must equal the untimed-launch total);
  * the operations and bytes a prompt needs, computed from the shapes: 2 n N K per projection, 4 L^2 / 2 x 128 per head
    for the causal attention, and the weight bytes every prompt streams once (n = 512 rows reuse each weight tile, so
    a prompt is bound by whichever is larger: FLOPs over the 2.5 PFLOP/s dense bf16 peak or weight bytes over the
    8 TB/s HBM peak), hence TFLOP/s and weight bytes per second.

Writes <out>/text_encoder.jsonl and <out>/SUMMARY.md. Reported, not gated: there is no parent number to compare with,
and bench.py stays the metric.
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "cosmos-predict2.5_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

HBM_PEAK = 8.0e12      # B/s, spec
BF16_PEAK = 2.5e15     # FLOP/s dense bf16 MFMA, spec
GROUPS = {"gemm": ("gemm_epi", "gemm_sm_epi"), "attention": ("attn_causal",),
          "rows": ("embed_gather", "add_rmsnorm", "rope_qk", "swiglu", "mean_normalize")}


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "text_encoder"))
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--tokens", type=int, default=512)
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-offload", action="store_true", help="skip the offload=True timing")
    return ap.parse_args()


def counts(cfg, n_tok):
    """(projection FLOPs, attention FLOPs, weight bytes streamed) of one prompt of n_tok ids."""
    D, I, q = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads * 128
    per_layer_w = cfg.qkv_dim * (D + 64) + D * q + 2 * I * D + D * I
    gemm = 2 * n_tok * per_layer_w * cfg.num_hidden_layers
    attn = cfg.num_hidden_layers * cfg.num_attention_heads * 4 * 128 * n_tok * (n_tok + 64) // 2  # 64-key tiles
    return gemm, attn, 2 * per_layer_w * cfg.num_hidden_layers


def timed(fn, passes):
    out = []
    for _ in range(passes):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def split_pass(TE, enc, ids):
    """One encode with an event pair around every launch: {group: ms}, {group: launches}."""
    N = TE.N
    marks = []
    saved = {}

    def wrap(name, group):
        fn = getattr(N, name)
        saved[name] = fn

        def inner(*a, **k):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **k)
            e1.record()
            marks.append((group, e0, e1))
            return r

        setattr(N, name, inner)

    for group, names in GROUPS.items():
        for name in names:
            wrap(name, group)
    try:
        enc.encode_ids(ids)
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(N, name, fn)
    ms = {g: 0.0 for g in GROUPS}
    launches = {g: 0 for g in GROUPS}
    for group, e0, e1 in marks:
        ms[group] += e0.elapsed_time(e1)
        launches[group] += 1
    return ms, launches


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("bench_text_encoder needs an MI355X: there is no CPU path")
    from cosmos_predict2 import text_encoder as TE

    dev = torch.device("cuda:0")
    cfg = dataclasses.replace(TE.REASON1_7B, num_hidden_layers=a.layers, num_tokens=a.tokens)
    enc = TE.Reason1TextEncoder.synthetic(cfg, device=dev, seed=0)
    ids = torch.randint(0, cfg.vocab_size, (1, a.tokens), generator=torch.Generator().manual_seed(0))
    gemm_flop, attn_flop, w_bytes = counts(cfg, a.tokens)
    out = enc.encode_ids(ids)  # untimed: code load
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    t = timed(lambda: enc.encode_ids(ids), a.passes)
    best, med = min(t), sorted(t)[len(t) // 2]
    parts, launches = split_pass(TE, enc, ids)
    rec = {"layers": a.layers, "tokens": a.tokens, "device": torch.cuda.get_device_name(0), "ms_passes": t, "ms_median": med,
           "ms_best": best, "split_ms": parts, "launches": launches, "gemm_flop": gemm_flop, "attn_flop": attn_flop,
           "weight_bytes": w_bytes, "tflops_median": (gemm_flop + attn_flop) / med / 1e9,
           "weight_gbps_median": w_bytes / med / 1e6,
           "gemm_tflops_in_split": gemm_flop / parts["gemm"] / 1e9, "attn_tflops_in_split": attn_flop / parts["attention"] / 1e9,
           "bound_ms": {"flops": (gemm_flop + attn_flop) / BF16_PEAK * 1e3, "weight_bytes": w_bytes / HBM_PEAK * 1e3}}
    if not a.no_offload:
        # offload: the same device weights copied to pinned-less host memory once, then uploaded by every encode
        enc._host = {k: v.cpu() for k, v in enc._dev.items()}
        enc.offload = True
        enc._park()
        torch.cuda.synchronize()
        enc.encode_ids(ids)
        rec["ms_offload_passes"] = timed(lambda: enc.encode_ids(ids), min(2, a.passes))
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "text_encoder.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    tot = sum(parts.values())
    lines = [
        "# Reason1 text encoder, synthetic 7B weights", "",
        f"`python tools/bench_text_encoder.py --layers {a.layers} --tokens {a.tokens} --passes {a.passes}` on one "
        f"{rec['device']}. Reported, not gated.", "",
        f"- one prompt ({a.tokens} ids, {a.layers} layers): median {med:.2f} ms, best {best:.2f} ms over {a.passes} passes "
        f"({', '.join(f'{x:.2f}' for x in t)})",
        f"- work per prompt: {gemm_flop / 1e12:.2f} TFLOP of projections, {attn_flop / 1e9:.1f} GFLOP of causal attention, "
        f"{w_bytes / 1e9:.2f} GB of weights streamed once",
        f"- whole-prompt rates at the median: {rec['tflops_median']:.0f} TFLOP/s, {rec['weight_gbps_median']:.0f} GB/s of "
        f"weight bytes (least possible time: {rec['bound_ms']['flops']:.2f} ms by FLOPs at 2.5 PFLOP/s, "
        f"{rec['bound_ms']['weight_bytes']:.2f} ms by weight bytes at 8 TB/s)",
        f"- split (one pass with an event pair around each of the {sum(launches.values())} launches; sum {tot:.2f} ms): "
        + "; ".join(f"{g} {parts[g]:.2f} ms ({100 * parts[g] / tot:.1f} %, {launches[g]} launches)" for g in GROUPS),
        f"- inside the split: GEMMs {rec['gemm_tflops_in_split']:.0f} TFLOP/s, attention {rec['attn_tflops_in_split']:.1f} TFLOP/s",
    ]
    if "ms_offload_passes" in rec:
        lines.append("- offload=True (weights parked in pageable host memory, uploaded by every encode): "
                     + ", ".join(f"{x:.0f}" for x in rec["ms_offload_passes"]) + " ms per prompt")
    with open(os.path.join(a.out, "SUMMARY.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
