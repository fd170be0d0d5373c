#!/usr/bin/env python3
"""Sparse (3D neighborhood) attention against dense attention, in one process on one MI355X.

    python tools/bench_sparse_attn.py [--out profiles/r10/sparse] [--grid 31,44,80] [--rounds 3] [--skip-eval]

(a) Attention launches at the metric shape (patch grid 31 x 44 x 80 = 109 120 tokens, 16 heads, B = 1), q / k / v as
    the DiT passes them (column views of one token-major [n, B, 3 H D] buffer, q RMS-normed and pre-scaled, unit norm
    weights): the dense N.attn_fwd in the DiT's default prescaled form with its weight norm bounds, and N.attn_na3d
    with windows (-1, 12, 24) and (-1, 28, 56), stride (1, 4, 8). Every launch is timed by device events, in the
    order dense / sparse / sparse / dense per round after an untimed round of each; the ratio is stated beside the key
    density that bounds it, and FLOP/s count 4 L keys 128 per head.
(b) One sampler evaluation (the CFG pair) of `2B/post-trained` against `2B/sparse-7dense` at the same shape, synthetic
    seeded weights, device events around each evaluation, same interleaving.
Writes <out>/sparse.jsonl (one JSON object per measurement) and <out>/SUMMARY.md. bench.py stays the metric
(`bench.py --model 2B/sparse-7dense` runs the sparse net through it; the recorded SUMMARY.md's section (c) was added
by hand from two such runs).
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "cosmos-predict2.5_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

LOG2E = 1.4426950408889634
WINDOWS = ((-1, 12, 24), (-1, 28, 56))
STRIDE = (1, 4, 8)


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "sparse"))
    ap.add_argument("--grid", default="31,44,80", help="patch grid T,H,W")
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3, help="timed dense / sparse / sparse / dense rounds")
    ap.add_argument("--eval-rounds", type=int, default=1)
    ap.add_argument("--skip-eval", action="store_true", help="attention launches only")
    return ap.parse_args()


def timed(fn):
    """Milliseconds of fn() on the current stream, by device events."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def abba(a_fn, b_fn, rounds):
    """([a ms], [b ms]) over `rounds` of a / b / b / a, after one untimed call of each."""
    a_fn()
    b_fn()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(rounds):
        ta.append(timed(a_fn))
        tb.append(timed(b_fn))
        tb.append(timed(b_fn))
        ta.append(timed(a_fn))
    return ta, tb


def bench_attention(a, dev, emit):
    from cosmos_predict2 import _native as N
    from cosmos_predict2 import sparse_attn as SA

    T, Hg, Wg = (int(x) for x in a.grid.split(","))
    L, H, D, B = T * Hg * Wg, a.heads, 128, 1
    g = torch.Generator(device=dev).manual_seed(0)
    qkv = torch.randn(L, B, 3 * H * D, device=dev, generator=g, dtype=torch.float32)
    rows = qkv.view(L, B, 3 * H, D)
    rows[:, :, :2 * H] *= torch.rsqrt(rows[:, :, :2 * H].pow(2).mean(-1, keepdim=True) + 1e-6)  # unit-weight RMSNorm
    c = D ** -0.5 * LOG2E
    rows[:, :, :H] *= c
    qkv = qkv.to(torch.bfloat16)
    q, k, v = (qkv[:, :, i * H * D:(i + 1) * H * D].view(L, B, H, D).transpose(0, 1) for i in range(3))
    o = torch.empty(L, B, H * D, dtype=torch.bfloat16, device=dev)
    ov = o.view(L, B, H, D).transpose(0, 1)
    bounds = (D ** 0.5 * c * 1.01, D ** 0.5 * 1.01)
    dense = lambda: N.attn_fwd(q, k, v, out=ov, prescaled=True, norm_bounds=bounds)  # noqa: E731
    dense_name = N.attn_kernel_name(L, norm_bounds=bounds, prescaled=True)
    out = []
    for win in WINDOWS:
        plan = SA.build_plan((T, Hg, Wg), dict(window_size=win, stride=STRIDE), dev)
        sparse = lambda: N.attn_na3d(q, k, v, plan, out=ov, prescaled=True)  # noqa: E731
        td, ts = abba(dense, sparse, a.rounds)
        md, ms = statistics.median(td), statistics.median(ts)
        rec = dict(kind="attention", grid=[T, Hg, Wg], tokens=L, heads=H, batch=B, window=list(plan.window),
                   stride=list(plan.stride), keys_per_query=plan.keys_per_query, key_density=plan.density,
                   tiles=plan.n_tiles, tile_fill=float((plan.q_tok >= 0).float().mean().item()),
                   dense_kernel=dense_name, dense_ms=td, sparse_ms=ts, dense_ms_median=md, sparse_ms_median=ms,
                   ratio=ms / md, dense_tflops=4.0 * B * H * L * L * D / md / 1e9,
                   sparse_tflops=4.0 * B * H * L * plan.keys_per_query * D / ms / 1e9)
        emit(rec)
        out.append(rec)
    return out


def bench_evaluation(a, dev, emit):
    from cosmos_predict2.dit import init_state_dict
    from cosmos_predict2.model import Video2WorldModelRectifiedFlow
    from cosmos_predict2.net_config import MODELS

    T, Hg, Wg = (int(x) for x in a.grid.split(","))
    runs = {}
    g = torch.Generator(device=dev).manual_seed(1)
    state_shape = (16, T, 2 * Hg, 2 * Wg)
    gt = torch.randn(1, *state_shape, device=dev, generator=g)
    for name in ("2B/post-trained", "2B/sparse-7dense"):
        ncfg, scfg = MODELS[name]
        model = Video2WorldModelRectifiedFlow(ncfg, scfg, device=dev)
        model.load_state_dict(init_state_dict(ncfg, seed=0, device=dev))
        ctx = [torch.randn(1, 512, ncfg.crossattn_proj_in_channels, device=dev, generator=g).to(torch.bfloat16)
               for _ in range(2)]
        run = model.begin_sampling(gt, ctx[0], ctx[1], state_shape=state_shape, num_conditional_frames=1, guidance=7,
                                   seed=0, num_steps=35)
        runs[name] = (model, run)

    def step(name):
        run = runs[name][1]
        if run.done:
            run.restart()
        run.step()

    td, ts = abba(lambda: step("2B/post-trained"), lambda: step("2B/sparse-7dense"), a.eval_rounds)
    net = runs["2B/sparse-7dense"][0].net
    rec = dict(kind="evaluation", grid=[T, Hg, Wg], tokens=T * Hg * Wg, dense_model="2B/post-trained",
               sparse_model="2B/sparse-7dense", sparse_blocks=sum(p is not None for p in net.sparse_params),
               blocks=net.cfg.num_blocks, kernels=net.attention_kernels(T * Hg * Wg), dense_ms=td, sparse_ms=ts,
               dense_ms_median=statistics.median(td), sparse_ms_median=statistics.median(ts),
               ratio=statistics.median(ts) / statistics.median(td))
    emit(rec)
    return rec


def summary(att, ev, path):
    lines = ["# Sparse (3D neighborhood) attention against dense attention", "",
             "Measured by `tools/bench_sparse_attn.py` in one process on one MI355X: device events around every launch /",
             "evaluation, one untimed call of each first, timed in the order dense / sparse / sparse / dense; medians",
             "below, every sample in `sparse.jsonl`. Synthetic seeded inputs and weights.", "",
             "## (a) Attention launches", "",
             f"Patch grid {att[0]['grid']} = {att[0]['tokens']} tokens, {att[0]['heads']} heads, B = 1, head dim 128, "
             "stride (1, 4, 8).", f"Dense kernel: `{att[0]['dense_kernel']}`.", "",
             "| window | keys / query | key density (bound of the ratio) | dense ms | sparse ms | sparse / dense | "
             "dense TFLOP/s | sparse TFLOP/s | tiles (fill) |", "|---|---|---|---|---|---|---|---|---|"]
    for r in att:
        lines.append(f"| {tuple(r['window'])} | {r['keys_per_query']} | {r['key_density']:.3f} | "
                     f"{r['dense_ms_median']:.2f} | {r['sparse_ms_median']:.2f} | {r['ratio']:.3f} | "
                     f"{r['dense_tflops']:.0f} | {r['sparse_tflops']:.0f} | {r['tiles']} ({r['tile_fill']:.3f}) |")
    lines += ["", "The ratio cannot fall below the key density; its distance from it is the box kernel's lower MFMA rate "
              "(gathered K / V rows, a 128-row tile against the dense kernel's 256, no softmax-shift shortcut).", ""]
    if ev is not None:
        lines += ["## (b) One 2B sampler evaluation (CFG pair)", "",
                  f"`{ev['dense_model']}` against `{ev['sparse_model']}` ({ev['sparse_blocks']} of {ev['blocks']} blocks "
                  "sparse, window (-1, 12, 24)), same grid.", "",
                  "| model | ms / evaluation |", "|---|---|",
                  f"| {ev['dense_model']} | {ev['dense_ms_median']:.1f} |",
                  f"| {ev['sparse_model']} | {ev['sparse_ms_median']:.1f} |", "",
                  f"sparse / dense = {ev['ratio']:.3f}. Kernels: `{json.dumps(ev['kernels'])}`.", ""]
    with open(path, "w") as f:
        f.write("\n".join(lines))


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sparse_attn.py measures on the GPU; none found")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    os.makedirs(a.out, exist_ok=True)
    log = open(os.path.join(a.out, "sparse.jsonl"), "w")

    def emit(rec):
        log.write(json.dumps(rec) + "\n")
        log.flush()
        print(json.dumps({k: v for k, v in rec.items() if not isinstance(v, list) or len(v) <= 4}), flush=True)

    with torch.no_grad():
        att = bench_attention(a, dev, emit)
        ev = None if a.skip_eval else bench_evaluation(a, dev, emit)
    summary(att, ev, os.path.join(a.out, "SUMMARY.md"))
    log.close()


if __name__ == "__main__":
    main()
