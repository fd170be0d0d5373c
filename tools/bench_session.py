#!/usr/bin/env python3
"""Closed-loop action sessions (ActionStreamingInference.open_session) on one MI355X against the chunk entry point
(stream_action_chunks_batch), in one process, the two alternated.

    python tools/bench_session.py [--resolutions 256,320:480,640] [--batches 1,4] [--modes tile256,small]
                                  [--num-steps 4] [--chunks 12] [--rounds 3] [--out DIR]

Seeded synthetic 2B weights: the arithmetic, not the picture, is timed. A configuration is (resolution, stream_gemm, B).
After one untimed chunk of each API (code objects, RoPE tables, padded weights), per configuration:

  latency     --chunks chunks (3 steps each, so 12 chunks = 36 steps), per chunk first the session's 3 steps, then the
              same chunk through the generator of stream_action_chunks_batch. A step's time is a host clock around
              sess.step(actions) with output="float" (the 4 frames as fp32 on the host, what the chunk API yields)
              followed by a synchronise; the chunk API's time is a host clock from asking the generator for the chunk
              until its 12 frames are on the host, which is when its first 4 frames become available. Steps that open a
              chunk (conditioning frame, encode, fresh cache, prefill, latent frame 0 into the decoder) are listed apart
              from the other steps. Median and spread (max - min) of each.
  throughput  --rounds rounds of 6 chunks, alternating: a session with output="u8" (18 steps, one synchronise at the
              end) and the chunk API (6 chunks, each timed for the chunk-to-chunk spread). Session-frames/s = 72 B
              pixel frames over the wall time; the two are "level" when the per-chunk difference is within twice the
              chunk API's chunk-to-chunk spread.

Per configuration one JSON line; with --out the lines go to <out>/session.jsonl and a table to <out>/SUMMARY.md.
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

from cosmos_predict2.interactive import (CHUNK_ACTIONS, MODEL_NAME, ActionStreamingInference,  # noqa: E402
                                         session_step_plan)

STEPS_PER_CHUNK = CHUNK_ACTIONS // 4
THROUGHPUT_CHUNKS = 6


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolutions", default="256,320:480,640")
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--modes", default="tile256,small")
    ap.add_argument("--num-steps", type=int, default=4)
    ap.add_argument("--cache-frame-size", type=int, default=-1)
    ap.add_argument("--chunks", type=int, default=12, help="timed chunks of the latency part (3 steps each)")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of the throughput part (6 chunks of each API)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    a.res = [tuple(int(x) for x in r.split(",")) for r in a.resolutions.split(":")]
    a.bs = [int(b) for b in a.batches.split(",")]
    a.ms = a.modes.split(",")
    if any(len(r) != 2 or r[0] % 16 or r[1] % 16 for r in a.res) or min(a.bs) < 1 or a.rounds < 1 or a.chunks < 1:
        ap.error("resolutions are H,W pairs of multiples of 16, batches >= 1, rounds >= 1, chunks >= 1")
    return a


def split_steps(step_ms):
    """The steps' times in session order -> (times of the steps that open a chunk, times of the others)."""
    opening = [t for k, t in enumerate(step_ms) if session_step_plan(k, STEPS_PER_CHUNK)[2]]
    inside = [t for k, t in enumerate(step_ms) if not session_step_plan(k, STEPS_PER_CHUNK)[2]]
    return opening, inside


def _med_spread(xs):
    return float(np.median(xs)), float(max(xs) - min(xs))


def summarize(cfg, step_ms, chunk_ms, sess_total_ms, api_total_ms, api_chunk_ms):
    """One configuration's result line. step_ms: the latency part's step times in session order; chunk_ms: the chunk
    API's times for the same chunks; sess_total_ms / api_total_ms: per throughput round, the wall time of the 6 chunks;
    api_chunk_ms: every chunk time of the chunk API's throughput rounds."""
    B = cfg["B"]
    opening, inside = split_steps(step_ms)
    o_med, o_spread = _med_spread(opening)
    c_med, c_spread = _med_spread(chunk_ms)
    line = dict(cfg, steps_timed=len(step_ms), open_step_ms=o_med, open_step_ms_spread=o_spread,
                open_step_ms_all=list(opening), chunk_api_ms=c_med, chunk_api_ms_spread=c_spread,
                chunk_api_ms_all=list(chunk_ms))
    if inside:
        i_med, i_spread = _med_spread(inside)
        line.update(step_ms=i_med, step_ms_spread=i_spread, steps_inside=len(inside),
                    session_chunk_ms=o_med + (STEPS_PER_CHUNK - 1) * i_med)
    # the first 4 frames of a chunk: after the opening step in a session, after the whole chunk through the chunk API
    line["first_frames_speedup"] = c_med / o_med
    frames = 4 * STEPS_PER_CHUNK * THROUGHPUT_CHUNKS * B
    s_med, a_med = float(np.median(sess_total_ms)), float(np.median(api_total_ms))
    spread = float(max(api_chunk_ms) - min(api_chunk_ms))
    diff = (s_med - a_med) / THROUGHPUT_CHUNKS
    line.update(session_frames_per_s_u8=frames * 1e3 / s_med, chunk_api_frames_per_s=frames * 1e3 / a_med,
                session_total_ms_all=list(sess_total_ms), chunk_api_total_ms_all=list(api_total_ms),
                chunk_to_chunk_spread_ms=spread, per_chunk_difference_ms=diff, level=bool(abs(diff) <= 2 * spread),
                session_not_slower=bool(diff <= 2 * spread))
    return line


def write_summary(lines, path, title="Closed-loop sessions against the chunk entry point"):
    """The result lines as a markdown table."""
    head = ("| resolution | B | stream_gemm | step ms (spread) | chunk-opening step ms (spread) | chunk API ms (spread) | "
            "first 4 frames: chunk API / opening step | session u8 frames/s | chunk API frames/s | per-chunk "
            "difference ms | chunk-to-chunk spread ms | within 2x spread |")
    rows = [f"# {title}", "", head, "|" + "---|" * 12]
    for l in lines:
        step = f"{l['step_ms']:.2f} ({l['step_ms_spread']:.2f})" if "step_ms" in l else "-"
        rows.append(f"| {l['resolution']} | {l['B']} | {l['stream_gemm']} | {step} | "
                    f"{l['open_step_ms']:.2f} ({l['open_step_ms_spread']:.2f}) | "
                    f"{l['chunk_api_ms']:.2f} ({l['chunk_api_ms_spread']:.2f}) | {l['first_frames_speedup']:.2f}x | "
                    f"{l['session_frames_per_s_u8']:.1f} | {l['chunk_api_frames_per_s']:.1f} | "
                    f"{l['per_chunk_difference_ms']:+.2f} | {l['chunk_to_chunk_spread_ms']:.2f} | "
                    f"{'yes' if l['level'] else 'no'} |")
    rows += ["", "Times are host clocks around synchronised calls, medians with max - min in brackets; step = a step "
             "inside a chunk, with output=\"float\" (4 frames as fp32 on the host). The chunk API makes a chunk's first 4 "
             "frames available when the whole chunk is decoded.", ""]
    text = "\n".join(rows)
    with open(path, "w") as f:
        f.write(text)
    return text


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("bench_session measures on the GPU; none is visible")
    from cosmos_predict2.pipeline import Video2WorldInference

    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    pipe = Video2WorldInference(MODEL_NAME, device=dev, pixel_path="device")
    ncfg = pipe.model.net_cfg
    rng = np.random.RandomState(0)
    emb = torch.from_numpy(rng.standard_normal((512, ncfg.crossattn_proj_in_channels)).astype(np.float32))
    n_chunks = max(a.chunks, THROUGHPUT_CHUNKS) + 1
    kw = dict(num_steps=a.num_steps, seed=1, cache_frame_size=a.cache_frame_size)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    lines = []
    for (h, w) in a.res:
        for mode in a.ms:
            inf = ActionStreamingInference(emb, pipe, stream_gemm=mode)
            for B in a.bs:
                cfg = dict(resolution=f"{h}x{w}", tokens_per_frame=(h // 16) * (w // 16), stream_gemm=mode, B=B,
                           num_steps=a.num_steps)
                imgs = [rng.randint(0, 256, size=(h, w, 3), dtype=np.uint8) for _ in range(B)]
                acts = (rng.standard_normal((B, n_chunks * CHUNK_ACTIONS, ncfg.action_dim)) * 0.1).astype(np.float32)
                step_acts = lambda k: acts[:, 4 * k: 4 * k + 4]  # noqa: E731
                # ---- latency: the session's 3 steps of a chunk, then the chunk API's same chunk; chunk 0 untimed
                sess = inf.open_session(imgs, (h, w), output="float", **kw)
                gen = inf.stream_action_chunks_batch(imgs, acts, (h, w), **kw)
                next(gen)
                for k in range(STEPS_PER_CHUNK):
                    sess.step(step_acts(k))
                next(gen)
                step_ms, chunk_ms = [], []
                for c in range(1, 1 + a.chunks):
                    for k in range(STEPS_PER_CHUNK * c, STEPS_PER_CHUNK * (c + 1)):
                        step_ms.append(clock(lambda: sess.step(step_acts(k)))[1])
                    chunk_ms.append(clock(lambda: next(gen))[1])
                del sess, gen
                # ---- throughput: 6 chunks of each, alternated
                acts6 = acts[:, :THROUGHPUT_CHUNKS * CHUNK_ACTIONS]
                sess_total, api_total, api_chunk = [], [], []

                def session_run():
                    s = inf.open_session(imgs, (h, w), output="u8", **kw)
                    for k in range(STEPS_PER_CHUNK * THROUGHPUT_CHUNKS):
                        s.step(step_acts(k))

                def api_run():
                    g = inf.stream_action_chunks_batch(imgs, acts6, (h, w), **kw)
                    next(g)
                    for _ in range(THROUGHPUT_CHUNKS):
                        api_chunk.append(clock(lambda: next(g))[1])

                for rnd in range(a.rounds):
                    order = (session_run, api_run) if rnd % 2 == 0 else (api_run, session_run)
                    for fn in order:
                        (sess_total if fn is session_run else api_total).append(clock(fn)[1])
                line = summarize(cfg, step_ms, chunk_ms, sess_total, api_total, api_chunk)
                lines.append(line)
                print(json.dumps(line), flush=True)
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "session.jsonl"), "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")
        print(write_summary(lines, os.path.join(a.out, "SUMMARY.md")), flush=True)


if __name__ == "__main__":
    main()
