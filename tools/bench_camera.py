#!/usr/bin/env python3
"""Camera-conditioned net against the plain 2B net on the same geometry, in one process, synthetic weights.

    python tools/bench_camera.py [--out profiles/r11/camera] [--t-seg 24] [--hp 44] [--wp 80]

Reports (device events, every timed region primed once untimed):
  * ms per evaluation (one forward_tokens of the CFG pair, B = 2, shared input) of `2B/camera-cond` with
    camera_cache "all" (the 28 cam_encoder outputs held) and "none" (recomputed per evaluation), and of the plain 2B net
    on the same 3 x t_seg x hp x wp token grid;
  * the one-off cost of prepare_camera in either mode and the bytes the cache holds;
  * cp25_ln_mod_cam alone at that token count against cp25_ln_mod: time and GB/s over the bytes each must move
    (x in, h out, and the [n, D] cam rows once per token, shared by the batch).
The defaults are the experiment's size (3 x 24 frames of 44 x 80 patches = 253 440 tokens, ~29 GB of cache); smaller
grids take --t-seg / --hp / --wp. Writes <out>/camera.jsonl and <out>/SUMMARY.md. bench.py stays the metric.
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


def parse():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "camera"))
    ap.add_argument("--t-seg", type=int, default=24, help="latent frames per segment (the axis holds three)")
    ap.add_argument("--hp", type=int, default=44)
    ap.add_argument("--wp", type=int, default=80)
    ap.add_argument("--iters", type=int, default=3, help="timed evaluations per net / mode")
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--blocks", type=int, default=0, help="blocks of the 2B layout to build (0 = all 28)")
    return ap.parse_args()


def timed(fn, iters):
    """Mean ms of fn over iters launches between two device events, after one untimed call."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    a = parse()
    from cosmos_predict2 import _native as N
    from cosmos_predict2.dit import Geometry, MinimalV1LVGDiT, init_state_dict
    from cosmos_predict2.net_config import DIT_2B, DIT_2B_CAMERA

    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    rows_out = []

    def emit(r):
        rows_out.append(r)
        print(json.dumps(r), flush=True)

    T = 3 * a.t_seg
    geo = Geometry(T=T, Hp=a.hp, Wp=a.wp, tok0=0, n_tok=T * a.hp * a.wp)
    n = geo.L
    nb = a.blocks or DIT_2B.num_blocks
    g = torch.Generator(device=dev).manual_seed(0)
    patch_rows = torch.randn((n, 1, 72), generator=g, device=dev).to(BF16)
    cam_rows = torch.randn((n, DIT_2B_CAMERA.camera_dim), generator=g, device=dev).to(BF16)
    results = {}
    with torch.no_grad():
        for name, cfg in (("plain", DIT_2B.replace(num_blocks=nb)), ("camera", DIT_2B_CAMERA.replace(num_blocks=nb))):
            net = MinimalV1LVGDiT(cfg, device=dev)
            net.load_state_dict(init_state_dict(cfg, seed=0, device=dev, zero_adaln_out=False))
            ctx = net.prepare_context(torch.randn((2, 512, cfg.crossattn_proj_in_channels), generator=g,
                                                  device=dev).to(BF16))
            t = net.scale_timesteps(torch.full((2, T), 700.0, device=dev))
            modes = ("all", "none") if cfg.camera_dim else (None,)
            for mode in modes:
                cache, prep_ms, held = None, 0.0, 0
                if mode is not None:
                    torch.cuda.synchronize()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    cache = net.prepare_camera(cam_rows, geo, camera_cache=mode)
                    e1.record()
                    torch.cuda.synchronize()
                    prep_ms = e0.elapsed_time(e1)
                    held = sum(e.numel() * 2 for e in (cache.emb or [cache.buf]))
                ms = timed(lambda: net.forward_tokens(patch_rows, t, ctx, geo, shared_batch=True, camera=cache), a.iters)
                key = name if mode is None else f"camera_{mode}"
                results[key] = ms
                emit(dict(kind="evaluation", net=key, tokens=n, grid=[T, a.hp, a.wp], blocks=nb, batch=2,
                          ms_per_evaluation=ms, prepare_camera_ms=prep_ms, cache_bytes=held))
                del cache
                torch.cuda.empty_cache()
            del net, ctx
            torch.cuda.empty_cache()
        # the LN-mod kernels alone: [n, 2, D] rows, cam shared by the batch
        D, B = DIT_2B.model_channels, 2
        x = torch.randn((n, B, D), generator=g, device=dev).to(BF16)
        mods = (torch.randn((B, T, 3 * D), generator=g, device=dev) * 0.5).to(BF16)
        cam = torch.randn((n, D), generator=g, device=dev).to(BF16)
        h = torch.empty((n, B, D), dtype=BF16, device=dev)
        kw = dict(n_tok=n, B=B, tok0=0, hw=geo.hw, x_st=B * D, x_sb=D, h_out=h)
        for kname, extra, nbytes in (("cp25_ln_mod", {}, 2 * n * B * D * 2),
                                     ("cp25_ln_mod_cam", dict(cam=cam), 2 * n * B * D * 2 + n * D * 2)):
            ms = timed(lambda: N.ln_mod(x, mods[..., :D], mods[..., D:2 * D], **kw, **extra), a.kernel_iters)
            results[kname] = ms
            emit(dict(kind="kernel", kernel=kname, tokens=n, batch=B, D=D, ms=ms, bytes=nbytes,
                      GBps=nbytes / (ms * 1e-3) / 1e9))
    with open(os.path.join(a.out, "camera.jsonl"), "w") as f:
        for r in rows_out:
            f.write(json.dumps(r) + "\n")
    ev = {r["net"]: r for r in rows_out if r["kind"] == "evaluation"}
    kr = {r["kernel"]: r for r in rows_out if r["kind"] == "kernel"}
    lines = [f"# Camera-conditioned net, {n} tokens ({T} x {a.hp} x {a.wp}), {nb} blocks of the 2B layout, B = 2", "",
             "Synthetic weights, one MI355X, device events; produced by `tools/bench_camera.py`. Reported, not gated.", "",
             "| net | ms / evaluation | vs plain | prepare_camera ms | cache held |", "|---|---|---|---|---|"]
    for k in ("plain", "camera_all", "camera_none"):
        r = ev[k]
        lines.append(f"| {k} | {r['ms_per_evaluation']:.1f} | {r['ms_per_evaluation'] / ev['plain']['ms_per_evaluation']:.4f} "
                     f"| {r['prepare_camera_ms']:.1f} | {r['cache_bytes'] / 2 ** 30:.2f} GiB |")
    lines += ["", "| kernel | ms | bytes moved | GB/s |", "|---|---|---|---|"]
    for k in ("cp25_ln_mod", "cp25_ln_mod_cam"):
        r = kr[k]
        lines.append(f"| {k} | {r['ms']:.3f} | {r['bytes'] / 1e9:.3f} GB | {r['GBps']:.0f} |")
    with open(os.path.join(a.out, "SUMMARY.md"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
