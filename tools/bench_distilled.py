#!/usr/bin/env python3
"""Distilled 4-step student against the 35-step UniPC loop: one whole Image2World video each, in one process.

    python tools/bench_distilled.py [--out profiles/r8/distilled] [--frames 121] [--resolution 704,1280]

For `2B/distilled` (config.sampler "dmd2": 4 single-branch evaluations) and `2B/post-trained` (35 UniPC steps = 36
evaluations x the CFG pair), on one MI355X with seeded synthetic weights (the arithmetic, not the picture, is what
is timed), it times the three stages of a video end to end, a host clock around work that ends in a device
synchronise: VAE encode of the conditioning frame, the sampling loop (set-up, every evaluation, the latent gather),
VAE decode. Every stage is primed once untimed (code objects, lazily built tables). The student's video is timed
--repeats times (the spread is reported); the 35-step video once.
It also times the two TrigFlow kernels alone at the video's token count with device events over --kernel-iters
launches each and reports GB/s against the bytes they must move (computed from the shapes below).
Writes <out>/distilled.jsonl (one JSON object per measurement) and <out>/SUMMARY.md. bench.py stays the metric.
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


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r8", "distilled"))
    ap.add_argument("--frames", type=int, default=121)
    ap.add_argument("--resolution", default="704,1280")
    ap.add_argument("--num-steps", type=int, default=35, help="InferenceArguments.num_steps for both models")
    ap.add_argument("--repeats", type=int, default=3, help="timed whole videos of the distilled student")
    ap.add_argument("--kernel-iters", type=int, default=200)
    ap.add_argument("--skip-teacher", action="store_true", help="time the distilled student only")
    return ap.parse_args()


def _sync(dev):
    torch.cuda.synchronize(dev)
    return time.perf_counter()


def whole_video(pipe, batch, state_shape, num_steps, dev):
    """One video: (encode_s, loop_s, decode_s, evaluations). Each stage ends in a device synchronise."""
    model = pipe.model
    state_t = state_shape[1]
    t0 = _sync(dev)
    gt = model.encode_conditioning(batch["video"], 1, state_t)
    t1 = _sync(dev)
    run = model.begin_sampling(gt, batch["t5_text_embeddings"], batch["neg_t5_text_embeddings"],
                               state_shape=state_shape, num_conditional_frames=1, guidance=7, seed=0,
                               num_steps=num_steps)
    while not run.done:
        run.step()
    lat = run.latents()
    t2 = _sync(dev)
    video = model.decode(lat)
    t3 = _sync(dev)
    assert torch.isfinite(video.float()).all()
    return t1 - t0, t2 - t1, t3 - t2, run.num_evals


def time_model(name, a, dev, emit):
    from cosmos_predict2.pipeline import DEFAULT_NEGATIVE_PROMPT, Video2WorldInference

    h, w = (int(x) for x in a.resolution.split(","))
    state_t = 1 + (a.frames - 1) // 4
    pipe = Video2WorldInference(name, device=dev, state_t=state_t)
    model = pipe.model
    frames = model.tokenizer.get_pixel_num_frames(state_t)
    rng = np.random.RandomState(3)
    vid = torch.zeros(1, 3, frames, h, w, dtype=torch.uint8)
    vid[0, :, 0] = torch.from_numpy(rng.randint(0, 256, size=(3, h, w), dtype=np.uint8))
    batch = pipe._get_data_batch_input(vid, "A robot arm pours coffee into a mug on a kitchen counter.", 1,
                                       DEFAULT_NEGATIVE_PROMPT)
    state_shape = (model.config.state_ch, state_t, h // 8, w // 8)
    with torch.no_grad():
        # prime, untimed: encode, one evaluation, a 2-latent-frame decode
        gt = model.encode_conditioning(batch["video"], 1, state_t)
        run = model.begin_sampling(gt, batch["t5_text_embeddings"], batch["neg_t5_text_embeddings"],
                                   state_shape=state_shape, num_conditional_frames=1, guidance=7, seed=0,
                                   num_steps=a.num_steps)
        run.step()
        model.decode(run.latents()[:, :, :2])
        del run, gt
        reps = a.repeats if model.config.sampler == "dmd2" else 1
        rows = []
        for r in range(reps):
            enc, loop, dec, evals = whole_video(pipe, batch, state_shape, a.num_steps, dev)
            rows.append(dict(kind="video", model=name, sampler=model.config.sampler, repeat=r, frames=frames,
                             resolution=[h, w], latent=list(state_shape), evaluations=evals,
                             dit_forwards=evals * (1 if model.config.sampler == "dmd2" else 2), encode_s=enc,
                             loop_s=loop, decode_s=dec, total_s=enc + loop + dec, frames_per_s=frames / (enc + loop + dec)))
            emit(rows[-1])
    del pipe, model
    torch.cuda.empty_cache()
    return rows


def time_kernels(a, dev, emit):
    """The two TrigFlow kernels alone at the video's token count: device events over kernel_iters launches."""
    from cosmos_predict2 import _native as N

    h, w = (int(x) for x in a.resolution.split(","))
    T = 1 + (a.frames - 1) // 4
    hw = (h // 16) * (w // 16)
    n = T * hw
    g = torch.Generator(device=dev).manual_seed(0)
    xs, gt, net, noise = (torch.randn(n, 64, device=dev, generator=g) for _ in range(4))
    fm = torch.zeros(T, device=dev)
    fm[0] = 1
    tab = torch.full((T,), 0.7, dtype=torch.float64, device=dev)
    out = []

    def timed(fn, bytes_moved, name):
        for _ in range(5):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_iters):
            fn()
        e1.record()
        torch.cuda.synchronize(dev)
        us = e0.elapsed_time(e1) * 1e3 / a.kernel_iters
        row = dict(kind="kernel", kernel=name, tokens=n, iters=a.kernel_iters, us_per_launch=us, bytes=bytes_moved,
                   gb_per_s=bytes_moved / us / 1e3,
                   note="back-to-back launches between two device events: launch gaps included")
        emit(row)
        out.append(row)

    # patchify: reads xs and gt (2 x 256 B per token), writes the 128-column bf16 row (256 B); the wrapper's output
    # allocation (caching allocator) is inside the window
    timed(lambda: N.trig_patchify(xs, gt, fm, tab, 1.0, None, tok0=0, hw=hw, ld=128), n * (256 + 256 + 256),
          "cp25_trig_patchify_ld")
    # x0 step, not last: reads xs, net, noise, gt, writes xs (5 x 256 B per token)
    st = xs.clone()
    timed(lambda: N.trig_x0_step(st, net.view(n, 1, 64), noise, gt, fm, tab, tab, replace_gt=True, sigma_data=1.0,
                                 cos_next=0.6, sin_next=0.8, last=False, tok0=0, hw=hw), n * 5 * 256,
          "cp25_trig_x0_step")
    return out


def main():
    a = parse()
    if not torch.cuda.is_available():
        raise SystemExit("bench_distilled.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    os.makedirs(a.out, exist_ok=True)
    jl = open(os.path.join(a.out, "distilled.jsonl"), "w")

    def emit(row):
        jl.write(json.dumps(row) + "\n")
        jl.flush()
        print(json.dumps(row), flush=True)

    emit(dict(kind="setup", device=torch.cuda.get_device_name(0), torch=torch.__version__, frames=a.frames,
              resolution=a.resolution, num_steps=a.num_steps))
    stu = time_model("2B/distilled", a, dev, emit)
    tea = [] if a.skip_teacher else time_model("2B/post-trained", a, dev, emit)
    ker = time_kernels(a, dev, emit)
    jl.close()

    best = min(stu, key=lambda r: r["total_s"])
    lines = ["# Distilled 4-step student against the 35-step UniPC loop", "",
             f"`tools/bench_distilled.py`, one process on one {torch.cuda.get_device_name(0)}, seeded synthetic weights, "
             f"Image2World (1 conditioning frame), {best['frames']} frames at {a.resolution.replace(',', ' x ')}, latent "
             f"{best['latent']}. A host clock around each stage, each ended by a device synchronise; every stage primed "
             "once untimed. Raw rows: `distilled.jsonl`.", "",
             "| model | sampler | evaluations | DiT forwards | encode s | loop s | decode s | total s | frames/s |",
             "|---|---|---|---|---|---|---|---|---|"]
    for r in stu + tea:
        lines.append(f"| {r['model']} (run {r['repeat']}) | {r['sampler']} | {r['evaluations']} | {r['dit_forwards']} | "
                     f"{r['encode_s']:.3f} | {r['loop_s']:.3f} | {r['decode_s']:.3f} | {r['total_s']:.3f} | "
                     f"{r['frames_per_s']:.3f} |")
    lines.append("")
    tot = [r["total_s"] for r in stu]
    lines.append(f"Student spread over {len(stu)} videos: total {min(tot):.3f} .. {max(tot):.3f} s.")
    if tea:
        t = tea[0]
        lines.append(f"35-step video {t['total_s']:.2f} s against the student's {best['total_s']:.2f} s: "
                     f"{t['total_s'] / best['total_s']:.2f}x end to end; the loops alone {t['loop_s']:.2f} s against "
                     f"{best['loop_s']:.2f} s ({t['loop_s'] / best['loop_s']:.2f}x). The 35-step video was timed once.")
    lines += ["", "## The two TrigFlow kernels alone", "",
              f"{ker[0]['tokens']} tokens, {a.kernel_iters} back-to-back launches between two device events (launch gaps "
              "and, for the patchify wrapper, its output allocation included), against the bytes each must move. The "
              f"launches re-read the same buffers ({ker[0]['bytes'] / 1e6:.0f} and {ker[1]['bytes'] / 1e6:.0f} MB), "
              "which fit the 256-MiB Infinity Cache: a cache-assisted rate, not an HBM-only one.", "",
              "| kernel | bytes | us per launch | GB/s |", "|---|---|---|---|"]
    for r in ker:
        lines.append(f"| {r['kernel']} | {r['bytes']} | {r['us_per_launch']:.1f} | {r['gb_per_s']:.0f} |")
    lines.append("")
    open(os.path.join(a.out, "SUMMARY.md"), "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
