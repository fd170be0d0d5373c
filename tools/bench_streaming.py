#!/usr/bin/env python3
"""The streaming action student (2B/robot/action-cond/streaming) on one MI355X: time per latent frame and its anatomy.

    python tools/bench_streaming.py --resolution 256,320 [--num-steps 4] [--cache-frame-size -1] [--out DIR]
                                    [--stream-gemm tile256|small|small_splitk]

One process per run (one resolution). Seeded synthetic weights: the arithmetic, not the picture, is timed. It runs the
chunk loop of ActionStreamingInference on one 13-frame chunk (T = 4 latent frames: the conditioning frame's prefill, then
three generated frames of num_steps evaluations + one store pass each) and reports
  * ms per generated latent frame and ms per student evaluation (one stream_patchify + forward_frame [+ x0 step]), from
    device events around every evaluation of --repeats timed chunks after one untimed chunk;
  * frames/s: 12 pixel frames per chunk over the chunk's whole device time (prefill included; VAE encode / decode are
    reported beside it and included in frames_per_s_end_to_end);
  * the split of the device's busy time between attention, GEMM and all other kernels, from the kernel records of one
    more chunk run under torch.profiler, and the idle share between kernels: 1 - (that chunk's summed kernel time) /
    (an unprofiled chunk's event-timed duration); the profiler stretches the host side, not the kernels;
  * the tile count of each block GEMM launch at this frame's row count against the CU count: every launch with fewer
    256 x 256 output tiles than CUs leaves CUs without work (the persistent GEMM runs one tile per workgroup round).
--stream-gemm: the GEMM family of the per-frame forward (Video2WorldInference(stream_gemm=...)); the mode is written into
the JSON line, with the spread of the timed chunks' latent-frame times (max - min) as the noise two modes are compared
against.
Prints one JSON line; with --out also appends it to <out>/streaming.jsonl.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "cosmos-predict2.5_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cosmos_predict2.interactive import MODEL_NAME  # noqa: E402
from cosmos_predict2.model import StreamingRun  # noqa: E402
from cosmos_predict2.pipeline import Video2WorldInference  # noqa: E402


def kernel_class(name: str) -> str:
    n = name.lower()
    if "attn" in n:
        return "attention"
    if "gemm" in n or "cijk" in n or "mfma" in n:
        return "gemm"
    return "other"


def run_chunk(model, gt, emb, actions, a, events=None):
    run = StreamingRun(model, gt, emb, actions, seed=1, n_steps=a.num_steps, cache_frame_size=a.cache_frame_size)
    if events is not None:
        inner = run._net

        def timed(*args):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = inner(*args)
            e1.record()
            events.append((args[2], args[4], e0, e1))  # frame, store
            return out
        run._net = timed
    while not run.done:
        run.next_frame()
    return run.latents()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolution", default="256,320")
    ap.add_argument("--num-steps", type=int, default=4)
    ap.add_argument("--cache-frame-size", type=int, default=-1)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--stream-gemm", default="tile256", choices=("tile256", "small", "small_splitk"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    h, w = (int(x) for x in a.resolution.split(","))
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    pipe = Video2WorldInference(MODEL_NAME, device=dev, pixel_path="device", stream_gemm=a.stream_gemm)
    model, ncfg = pipe.model, pipe.model.net_cfg
    rng = np.random.RandomState(0)
    frame = torch.from_numpy(rng.randint(0, 256, size=(3, h, w), dtype=np.uint8)).to(dev)
    actions = torch.from_numpy((rng.standard_normal((1, 12, ncfg.action_dim)) * 0.1).astype(np.float32)).to(dev)
    emb = torch.from_numpy(rng.standard_normal((1, 512, ncfg.crossattn_proj_in_channels)).astype(np.float32))
    emb = emb.to(dev, torch.bfloat16)
    emb = model.net.prepare_context(emb)  # the text context once, as ActionStreamingInference holds it
    hw = (h // 16) * (w // 16)

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    gt, _ = sync_time(lambda: model.encode_conditioning(frame[None, :, None], 1, 4))
    lat = run_chunk(model, gt, emb, actions, a)  # untimed: code objects, RoPE tables, padded weights
    sync_time(lambda: model.decode(lat))
    _, enc_ms = sync_time(lambda: model.encode_conditioning(frame[None, :, None], 1, 4))
    chunks = []
    for _ in range(a.repeats):
        ev = []
        c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        c0.record()
        lat = run_chunk(model, gt, emb, actions, a, ev)
        c1.record()
        torch.cuda.synchronize()
        evals = [(f, s, e0.elapsed_time(e1)) for f, s, e0, e1 in ev]
        chunks.append(dict(chunk_ms=c0.elapsed_time(c1), evals=evals))
    _, dec_ms = sync_time(lambda: model.decode(lat))
    best = min(chunks, key=lambda c: c["chunk_ms"])
    denoise = [ms for c in chunks for f, s, ms in c["evals"] if not s]
    store = [ms for c in chunks for f, s, ms in c["evals"] if s and f > 0]
    per_frame = [sum(ms for f, s, ms in c["evals"] if f == fr) for c in chunks for fr in (1, 2, 3)]

    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        run_chunk(model, gt, emb, actions, a)
        torch.cuda.synchronize()
    busy = {"attention": 0.0, "gemm": 0.0, "other": 0.0}
    top = {}
    for e in prof.events():
        if e.device_type is not None and "cuda" in str(e.device_type).lower() and e.device_time_total > 0:
            busy[kernel_class(e.name)] += e.device_time_total / 1e3
            top[e.name] = top.get(e.name, 0.0) + e.device_time_total / 1e3
    total_busy = sum(busy.values())
    if total_busy <= 0:
        raise RuntimeError("the profiler recorded no device kernels")
    n_cu = torch.cuda.get_device_properties(dev).multi_processor_count
    D = ncfg.model_channels
    tiles = {name: -(-hw // 256) * (n // 256) for name, n in (("qkv", 3 * D), ("out / cross-q / cross-out / mlp2", D),
                                                               ("mlp1", ncfg.mlp_hidden))}
    res = dict(workload=f"streaming action student, one 13-frame chunk at {h}x{w} ({hw} tokens per latent frame), "
                        f"{a.num_steps} steps, cache_frame_size {a.cache_frame_size}, bf16, synthetic weights",
               stream_gemm=a.stream_gemm, ms_per_latent_frame=float(np.median(per_frame)),
               ms_per_latent_frame_all=per_frame, ms_per_latent_frame_spread=float(max(per_frame) - min(per_frame)),
               ms_per_denoise_eval=float(np.median(denoise)),
               ms_per_store_eval=float(np.median(store)), chunk_ms_best=best["chunk_ms"],
               chunk_ms_all=[c["chunk_ms"] for c in chunks], frames_per_s_dit=12e3 / best["chunk_ms"],
               vae_encode_ms=enc_ms, vae_decode_ms=dec_ms,
               frames_per_s_end_to_end=12e3 / (best["chunk_ms"] + enc_ms + dec_ms),
               busy_ms_profiled_chunk=total_busy, busy_share={k: v / total_busy for k, v in busy.items()},
               share_of_chunk_time={k: v / best["chunk_ms"] for k, v in busy.items()},
               idle_share=max(0.0, 1.0 - total_busy / best["chunk_ms"]), compute_units=n_cu,
               gemm_tiles_per_launch=tiles, gemm_launches_under_filled=[k for k, v in tiles.items() if v < n_cu],
               top_kernels_ms=dict(sorted(top.items(), key=lambda kv: -kv[1])[:8]))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "streaming.jsonl"), "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
