#!/usr/bin/env python3
"""Parallel action rollouts on one MI355X: B streaming sessions per forward (model.StreamingBatchRun) and the VAE on B
clips in lock-step, against one session (model.StreamingRun), in one process.

    python tools/bench_stream_batch.py [--resolutions 256,320:480,640] [--batches 1,2,4,8] [--modes tile256,small]
                                       [--num-steps 4] [--rounds 3] [--out DIR]

Seeded synthetic 2B weights: the arithmetic, not the picture, is timed. A configuration is (resolution, stream_gemm,
B); its unit of work is one 13-frame chunk of every session, as ActionStreamingInference runs it: encode the B
conditioning frames, the T = 4 latent frames (prefill + 3 generated frames of num_steps evaluations and one store pass
each), decode the B clips. B = 1 is the one-session path (StreamingRun), so the comparison is against what a user runs
today. Every configuration is warmed once (code objects, RoPE tables, padded weights); then --rounds rounds visit all
configurations of a resolution, in forward order in even rounds and in reverse order in odd ones, so a drift of the
machine does not land on one configuration. Per visit: the chunk's device time (events around the frame loop) and the
encode and decode times (host clock around a synchronised call). After the timed rounds one more chunk per configuration
runs under torch.profiler for the summed kernel time; idle share = 1 - that / the median chunk time.
Per configuration one JSON line:
  chunk_ms (median), chunk_ms_all, chunk_ms_spread (max - min over the rounds),
  ms_per_latent_frame_per_session = chunk_ms / (3 generated frames x B), and its spread,
  session_frames_per_s_dit = 12 B pixel frames / chunk_ms; ..._end_to_end with the VAE encode + decode,
  vae_encode_ms, vae_decode_ms, vae_share_of_chunk = (enc + dec) / (chunk + enc + dec), idle_share.
Last line: the claim, per resolution and mode: ms_per_latent_frame_per_session at B = 4 below B = 1 by more than twice
the larger of the two spreads (true / false, with the figures).
With --out the lines are appended to <out>/stream_batch.jsonl.
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
from cosmos_predict2.model import StreamingBatchRun, StreamingRun  # noqa: E402
from cosmos_predict2.pipeline import Video2WorldInference  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--resolutions", default="256,320:480,640")
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--modes", default="tile256,small")
    ap.add_argument("--num-steps", type=int, default=4)
    ap.add_argument("--cache-frame-size", type=int, default=-1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    a.res = [tuple(int(x) for x in r.split(",")) for r in a.resolutions.split(":")]
    a.bs = [int(b) for b in a.batches.split(",")]
    a.ms = a.modes.split(",")
    if any(len(r) != 2 or r[0] % 16 or r[1] % 16 for r in a.res) or min(a.bs) < 1 or a.rounds < 1:
        ap.error("resolutions are H,W pairs of multiples of 16, batches >= 1, rounds >= 1")
    return a


def visit_order(configs, rnd: int):
    return list(configs) if rnd % 2 == 0 else list(configs)[::-1]


def summarize(cfg, chunk, enc, dec, busy_ms):
    """One configuration's result line from its per-round times (ms)."""
    B = cfg["B"]
    c, e, d = float(np.median(chunk)), float(np.median(enc)), float(np.median(dec))
    spread = float(max(chunk) - min(chunk))
    return dict(cfg, chunk_ms=c, chunk_ms_all=list(chunk), chunk_ms_spread=spread,
                ms_per_latent_frame_per_session=c / (3 * B), ms_per_latent_frame_per_session_spread=spread / (3 * B),
                session_frames_per_s_dit=12e3 * B / c, session_frames_per_s_end_to_end=12e3 * B / (c + e + d),
                vae_encode_ms=e, vae_decode_ms=d, vae_encode_ms_all=list(enc), vae_decode_ms_all=list(dec),
                vae_share_of_chunk=(e + d) / (c + e + d), busy_ms_profiled_chunk=busy_ms,
                idle_share=None if busy_ms is None else max(0.0, 1.0 - busy_ms / c))


def claim(lines, b_lo: int = 1, b_hi: int = 4):
    """Per (resolution, mode): does time per session-frame at b_hi fall below b_lo by more than twice the spread?"""
    out = []
    keyed = {(l["resolution"], l["stream_gemm"], l["B"]): l for l in lines}
    for (res, mode, B) in sorted(keyed):
        if B != b_lo or (res, mode, b_hi) not in keyed:
            continue
        lo, hi = keyed[(res, mode, b_lo)], keyed[(res, mode, b_hi)]
        k = "ms_per_latent_frame_per_session"
        spread = max(lo[k + "_spread"], hi[k + "_spread"])
        out.append(dict(resolution=res, stream_gemm=mode, b_lo=b_lo, b_hi=b_hi, ms_lo=lo[k], ms_hi=hi[k], spread=spread,
                        gain=lo[k] / hi[k], holds=bool(lo[k] - hi[k] > 2 * spread)))
    return out


def main(argv=None):
    a = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("bench_stream_batch measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    pipe = Video2WorldInference(MODEL_NAME, device=dev, pixel_path="device")
    model, ncfg = pipe.model, pipe.model.net_cfg
    rng = np.random.RandomState(0)
    Bmax = max(a.bs)
    emb = torch.from_numpy(rng.standard_normal((1, 512, ncfg.crossattn_proj_in_channels)).astype(np.float32))
    ctx1 = model.net.prepare_context(emb.to(dev, torch.bfloat16))
    ctxs = {B: (ctx1 if B == 1 else StreamingBatchRun.batch_context(model, ctx1, B)) for B in a.bs}
    actions = torch.from_numpy((rng.standard_normal((Bmax, 12, ncfg.action_dim)) * 0.1).astype(np.float32)).to(dev)

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def frames_loop(cfg, gt):
        B = cfg["B"]
        kw = dict(seed=1, n_steps=a.num_steps, cache_frame_size=a.cache_frame_size)
        model.net.set_stream_gemm(cfg["stream_gemm"])
        run = (StreamingRun if B == 1 else StreamingBatchRun)(model, gt, ctxs[B], actions[:B], **kw)
        while not run.done:
            run.next_frame()
        return run.latents()

    lines = []
    for (h, w) in a.res:
        frames = torch.from_numpy(rng.randint(0, 256, size=(Bmax, 3, h, w), dtype=np.uint8)).to(dev)
        configs = [dict(resolution=f"{h}x{w}", tokens_per_frame=(h // 16) * (w // 16), stream_gemm=m, B=B,
                        num_steps=a.num_steps) for m in a.ms for B in a.bs]
        enc = lambda cfg: model.encode_conditioning(frames[:cfg["B"], :, None], 1, 4)  # noqa: E731
        lat = {}
        for i, cfg in enumerate(configs):  # warm-up: every shape of the timed window
            lat[i] = frames_loop(cfg, enc(cfg))
            model.decode(lat[i])
        times = {i: dict(chunk=[], enc=[], dec=[]) for i in range(len(configs))}
        for rnd in range(a.rounds):
            for i in visit_order(range(len(configs)), rnd):
                cfg = configs[i]
                gt, e_ms = sync_time(lambda: enc(cfg))
                c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                c0.record()
                lt = frames_loop(cfg, gt)
                c1.record()
                torch.cuda.synchronize()
                _, d_ms = sync_time(lambda: model.decode(lt))
                t = times[i]
                t["chunk"].append(c0.elapsed_time(c1))
                t["enc"].append(e_ms)
                t["dec"].append(d_ms)
        from torch.profiler import ProfilerActivity, profile

        for i, cfg in enumerate(configs):
            gt = enc(cfg)
            torch.cuda.synchronize()
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                frames_loop(cfg, gt)
                torch.cuda.synchronize()
            busy = sum(e.device_time_total for e in prof.events()
                       if e.device_type is not None and "cuda" in str(e.device_type).lower()) / 1e3
            line = summarize(cfg, times[i]["chunk"], times[i]["enc"], times[i]["dec"], busy if busy > 0 else None)
            lines.append(line)
            print(json.dumps(line), flush=True)
        del frames, lat
        torch.cuda.empty_cache()
    verdict = dict(claim="ms per latent frame per session at B = 4 below B = 1 by more than twice the spread",
                   results=claim(lines))
    print(json.dumps(verdict), flush=True)
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "stream_batch.jsonl"), "a") as f:
            for line in lines + [verdict]:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
