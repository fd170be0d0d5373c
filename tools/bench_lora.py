#!/usr/bin/env python3
"""cp25_lora_merge over the recipe's targets of a whole net, at the 2B and 14B widths, synthetic weights.

    python tools/bench_lora.py [--out profiles/r12/lora] [--rank 32] [--nets 2B,14B] [--blocks 0]

Per net: one bf16 weight per recipe target (q_proj, k_proj, v_proj, output_proj of self_attn and cross_attn,
mlp.layer1, mlp.layer2) of every block, each with its own fp32 adapter of the given rank, all allocated up front
(2B: ~3.5 GB, 14B: ~27 GB of weights), then merged one launch per target, which is what load_state_dict of a
peft-layout checkpoint and merge_lora do. A pass touches every weight once, so nothing is re-read from a cache: the
time is the cold, HBM-to-HBM time of a real merge. One untimed pass (code load), then --passes timed passes between
device events (merging again into merged weights costs the same).

Reports ms per pass, GB/s over the bytes a merge must move (2 B read + 2 B written per weight element, plus the fp32
adapters once), that rate's share of the 8.0 TB/s HBM peak, and beside it the kernel's other bound: it spends 2 r + 2
unfused fp32 operations per element (FP contraction is off by contract), against a vector rate of 78.6 T op/s for
unfused packed fp32 (half the 157.3 TFLOPS FMA peak). Writes <out>/lora.jsonl and <out>/SUMMARY.md. Reported, not
gated; bench.py stays the metric.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "cosmos-predict2.5_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

BF16 = torch.bfloat16
HBM_PEAK = 8.0e12  # B/s, spec
VECTOR_UNFUSED = 157.3e12 / 2  # op/s: the FP32 vector peak counts an FMA as two


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "lora"))
    ap.add_argument("--rank", type=int, default=32)
    ap.add_argument("--nets", default="2B,14B")
    ap.add_argument("--blocks", type=int, default=0, help="blocks to build per net (0 = all)")
    ap.add_argument("--passes", type=int, default=3)
    return ap.parse_args()


def target_shapes(cfg, blocks):
    """[N, K] of every recipe target of `blocks` blocks, in checkpoint order."""
    D, ctx, hid = cfg.model_channels, cfg.crossattn_emb_channels, cfg.mlp_hidden
    per_block = [(D, D)] * 4 + [(D, D), (D, ctx), (D, ctx), (D, D)] + [(hid, D), (D, hid)]
    return per_block * blocks


def main():
    a = parse()
    from cosmos_predict2 import _native as N
    from cosmos_predict2.net_config import DIT_2B, DIT_14B

    if not torch.cuda.is_available():
        raise SystemExit("bench_lora.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    rows = []
    r = a.rank
    for name in a.nets.split(","):
        cfg = {"2B": DIT_2B, "14B": DIT_14B}[name]
        nb = a.blocks or cfg.num_blocks
        shapes = target_shapes(cfg, nb)
        g = torch.Generator(device=dev).manual_seed(0)
        ws, ads = [], []
        for n, k in shapes:
            ws.append((torch.randn((n, k), generator=g, device=dev) * k ** -0.5).to(BF16))
            ads.append(((torch.rand((r, k), generator=g, device=dev) * 2 - 1) * k ** -0.5,
                        torch.randn((n, r), generator=g, device=dev) * 0.02))
        elems = sum(n * k for n, k in shapes)
        nbytes = 4 * elems + sum(4 * r * (n + k) for n, k in shapes)
        ops = (2 * r + 2) * elems

        def one_pass():
            for w, (la, lb) in zip(ws, ads):
                N.lora_merge(w, la, lb, 1.0)

        one_pass()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.passes):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            one_pass()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        ms = min(times)
        row = dict(net=name, blocks=nb, rank=r, targets=len(shapes), weight_elements=elems, bytes=nbytes, ops=ops,
                   ms_passes=times, ms=ms, GBps=nbytes / (ms * 1e-3) / 1e9,
                   hbm_share=nbytes / (ms * 1e-3) / HBM_PEAK, hbm_bound_ms=nbytes / HBM_PEAK * 1e3,
                   vector_bound_ms=ops / VECTOR_UNFUSED * 1e3, device=torch.cuda.get_device_name(0))
        rows.append(row)
        print(json.dumps(row), flush=True)
        del ws, ads
        torch.cuda.empty_cache()
    with open(os.path.join(a.out, "lora.jsonl"), "w") as f:
        for row in rows:
            f.write(json.dumps(row) + "\n")
    lines = [f"# cp25_lora_merge over a whole net's recipe targets, rank {r}", "",
             f"Synthetic weights, one {rows[0]['device']}, device events, best of {a.passes} passes after one untimed pass; "
             "every pass touches each weight once (cold). Produced by `tools/bench_lora.py`. Reported, not gated.", "",
             "| net | blocks | targets | weight elements | bytes moved | ms | GB/s | share of 8.0 TB/s | HBM bound ms | "
             "vector bound ms | passes ms |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for row in rows:
        lines.append(f"| {row['net']} | {row['blocks']} | {row['targets']} | {row['weight_elements'] / 1e9:.2f} G | "
                     f"{row['bytes'] / 1e9:.2f} GB | {row['ms']:.2f} | {row['GBps']:.0f} | {row['hbm_share']:.3f} | "
                     f"{row['hbm_bound_ms']:.2f} | {row['vector_bound_ms']:.2f} | "
                     f"{', '.join('%.2f' % t for t in row['ms_passes'])} |")
    lines += ["", "HBM bound: bytes over the 8.0 TB/s spec peak. Vector bound: (2 r + 2) unfused fp32 operations per "
              "element over 78.6 T op/s (packed, unfused: half the 157.3 TFLOPS FMA peak). The larger of the two is the "
              "least time the hardware could take; at rank 32 that is the vector bound, because the contract forbids "
              "the fused multiply-add."]
    with open(os.path.join(a.out, "SUMMARY.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
