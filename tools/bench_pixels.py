"""Host pixel path against the device pixel path (cosmos_predict2/pixels.py, csrc/pixel_ops.hip), one process, the
two legs alternating after a warm-up of each. Times, with a device synchronise inside every window:

  input    a decoded 1080x1920 x 121-frame uint8 video -> the encoder's input clip at 704x1280, n_cond = 2
           (host: process_video_frames + _normalize_video + permute/pad; device: process_video_frames_device +
           u8_to_clip);
  output   the decoder's bf16 [121, 704, 1280, 3] result -> uint8 [T, H, W, 3] on the host
           (host: NCTHW permute, fp32 cast, save_video's quantisation, copy, re-layout to [T, H, W, 3] on the CPU;
           device: clip_to_u8, copy);
  action   the pixel work of one action-conditioned chunk, 13 x 480 x 640 (conditioning video -> clip, decoded clip ->
           uint8 frames on the host);
  kernels  each kernel alone (device events) with its achieved GB/s over the bytes the algorithm must move.

One JSON line per item. Needs the GPU; there is no CPU stand-in for the device leg."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "cosmos-predict2.5_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cosmos_predict2 import _native as N  # noqa: E402
from cosmos_predict2 import pixels  # noqa: E402
from cosmos_predict2.action_conditioned import conditioning_video  # noqa: E402
from cosmos_predict2.pipeline import process_video_frames  # noqa: E402

BF16 = torch.bfloat16


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def ab(name, host_fn, dev_fn, dev, reps, same=None, **info):
    """Warm both legs once, then alternate them `reps` times; report the median of each."""
    _, h0 = timed(host_fn, dev)
    _, d0 = timed(dev_fn, dev)
    if same is not None:
        same(h0, d0)
    del h0, d0
    th, td = [], []
    for _ in range(reps):
        th.append(timed(host_fn, dev)[0])
        td.append(timed(dev_fn, dev)[0])
    rec = {"item": name, "host_ms": 1e3 * float(np.median(th)), "device_ms": 1e3 * float(np.median(td)),
           "host_ms_all": [round(1e3 * t, 2) for t in th], "device_ms_all": [round(1e3 * t, 2) for t in td],
           "reps": reps, **info}
    rec["speedup"] = rec["host_ms"] / rec["device_ms"]
    print(json.dumps(rec), flush=True)


def kernel_rate(name, fn, nbytes, dev, reps=20):
    fn()
    torch.cuda.synchronize(dev)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
    ev[0].record()
    for i in range(reps):
        fn()
        ev[i + 1].record()
    torch.cuda.synchronize(dev)
    ms = float(np.median([ev[i].elapsed_time(ev[i + 1]) for i in range(reps)]))
    print(json.dumps({"item": name, "kernel_ms": ms, "algorithmic_bytes": nbytes, "GB_per_s": nbytes / ms / 1e6,
                      "reps": reps}), flush=True)


def host_clip(video_u8_ncthw, px, dev):
    """model._normalize_video + WanVAE.encode's permute / pad, as the parent commit runs them."""
    v = video_u8_ncthw[:, :, :px].to(device=dev, dtype=BF16) / 127.5 - 1.0
    _, C, T, H, W = v.shape
    x = torch.zeros((T, H, W, 16), dtype=BF16, device=dev)
    x[..., :C] = v[0].permute(1, 2, 3, 0)
    return x


def host_output(clip):
    """WanVAE.decode's tail + the interface's fp32 cast + save_video's quantisation and copy."""
    video = clip.permute(3, 0, 1, 2).unsqueeze(0).contiguous().float()
    frames = ((1.0 + video[0]) / 2 * 255.0).clamp(0, 255).to(torch.uint8).permute(1, 2, 3, 0).cpu().numpy()
    return np.ascontiguousarray(frames)  # save_video hands write_mp4 contiguous frames: the re-layout runs on the CPU


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=121)
    ap.add_argument("--source", default="1080,1920")
    ap.add_argument("--resolution", default="704,1280")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-input", action="store_true", help="skip the (slow, host-bound) input item")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pixels needs the GPU")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    N.load_library()
    sh, sw = (int(x) for x in a.source.split(","))
    th, tw = (int(x) for x in a.resolution.split(","))
    T = a.frames
    g = torch.Generator().manual_seed(0)

    # ---- input
    n_cond, px = 2, 5
    if not a.skip_input:
        frames = torch.randint(0, 256, (T, sh, sw, 3), generator=g, dtype=torch.uint8)

        def host_in():
            return host_clip(process_video_frames(frames, (th, tw), T, n_cond), px, dev)

        def dev_in():
            return pixels.video_to_clip(pixels.process_video_frames_device(frames, (th, tw), T, n_cond, device=dev)[:, :, :px])

        def same(h, d):
            diff = (h.float() - d.float()).abs().max().item()
            assert diff <= 2.0 / 127.5 + 1e-6, diff  # bytes within 1 of each other (tie band), usually equal
        ab("input", host_in, dev_in, dev, a.reps, same, source=[T, sh, sw, 3], target=[th, tw], n_cond=n_cond)
        del frames

    # ---- output
    clip = (torch.rand((T, th, tw, 3), generator=g) * 2.4 - 1.2).to(BF16).to(dev)

    def same_bytes(h, d):
        assert np.array_equal(h, d)
    ab("output", lambda: host_output(clip), lambda: pixels.clip_to_uint8(clip, "THWC").cpu().numpy(), dev, a.reps + 2,
       same_bytes, clip=[T, th, tw, 3])

    # ---- one action chunk
    ah, aw, af = 480, 640, 13
    img = np.random.RandomState(0).randint(0, 256, size=(ah, aw, 3), dtype=np.uint8)
    aclip = clip[:af, :ah, :aw].contiguous()
    img_d = torch.from_numpy(img).to(dev).permute(2, 0, 1)

    def host_action():
        x = host_clip(conditioning_video(img, af), 1, dev)
        v = host_output_action(aclip)
        return x, v

    def host_output_action(c):  # action_conditioned.generate's quantisation
        video = c.permute(3, 0, 1, 2).unsqueeze(0).contiguous().float()
        return (torch.clamp((video + 1) / 2, 0, 1)[0] * 255).to(torch.uint8).permute(1, 2, 3, 0).cpu().numpy()

    def dev_action():
        vid = torch.zeros(1, 3, af, ah, aw, dtype=torch.uint8, device=dev)
        vid[0, :, 0] = img_d
        x = pixels.video_to_clip(vid[:, :, :1])
        v8 = pixels.clip_to_uint8(aclip, "THWC")
        return x, v8.cpu().numpy()

    def same_action(h, d):
        assert torch.equal(h[0], d[0]) and np.array_equal(h[1], d[1])
    ab("action_chunk", host_action, dev_action, dev, 10, same_action, chunk=[af, ah, aw, 3])

    # ---- kernels alone
    src = torch.randint(0, 256, (T, sh, sw, 3), generator=g, dtype=torch.uint8).to(dev)  # channels-last frames
    (rh, rw), (top, left) = pixels.resize_geometry((sh, sw), (th, tw))
    ty, tx = pixels.aa_tables(sh, rh, dev), pixels.aa_tables(sw, rw, dev)
    dst = torch.empty((1, 3, T, th, tw), dtype=torch.uint8, device=dev)
    kernel_rate("resize_crop_u8 THWC -> planar", lambda: N.resize_crop_u8(src.permute(0, 3, 1, 2), dst[0].permute(1, 0, 2, 3),
                                                                         ty, tx, (top, left, th, tw)),
                src.numel() * th * tw // (rh * rw) + dst.numel(), dev)
    planar = src.permute(0, 3, 1, 2).contiguous()
    del src
    kernel_rate("resize_crop_u8 planar -> planar", lambda: N.resize_crop_u8(planar, dst[0].permute(1, 0, 2, 3), ty, tx,
                                                                           (top, left, th, tw)),
                planar.numel() * th * tw // (rh * rw) + dst.numel(), dev)
    del planar
    tc = min(T, 33)
    out16 = torch.empty((tc, th, tw, 16), dtype=BF16, device=dev)
    kernel_rate("u8_to_clip", lambda: N.u8_to_clip(dst[0, :, :tc], out16), 3 * tc * th * tw + out16.numel() * 2, dev)
    del out16
    o8 = torch.empty((T, th, tw, 3), dtype=torch.uint8, device=dev)
    kernel_rate("clip_to_u8 THWC", lambda: N.clip_to_u8(clip, o8), clip.numel() * 3, dev)
    kernel_rate("clip_to_u8 NCTHW", lambda: N.clip_to_u8(clip, dst[0].permute(1, 2, 3, 0)), clip.numel() * 3, dev)


if __name__ == "__main__":
    main()
