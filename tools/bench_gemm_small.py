#!/usr/bin/env python3
"""The streaming per-frame forward's block GEMM launches, one by one: cp25_gemm_* (256 x 256 tiles) against the
small-M family (cp25_gemm_sm_*, csrc/gemm_small.hip) at split 1 and at every split the plan may choose.

    python tools/bench_gemm_small.py [--rows 320,1200] [--rounds 7] [--mode graph|direct] [--stages 3,6] [--out DIR]

Launch shapes of one evaluation of the 2B net at 320 (256 x 320) and 1200 (480 x 640) rows per latent frame:
    qkv    N = 6144, K = 2048, the fused q|k|v projection with the k norm + RoPE epilogue
    proj   N = 2048, K = 2048, output / cross-output projection with the gated residual (cross-q: the same shape)
    mlp1   N = 8192, K = 2048, GELU
    mlp2   N = 2048, K = 8192, gated residual
Per shape and form: microseconds per launch, the weight bytes (N K 2) over that time as GB/s, and its share of the
8.0 TB/s HBM peak (the spec value; a weight streamed once is the least traffic the launch can have).

Method (measuring-on-mi355x): every form of a shape runs in one process, interleaved round by round (form A, B, C, ...,
then again), after a warm-up of every form. A round of one form is one pass over `copies` distinct weight tensors, enough
of them to exceed the 256 MiB Infinity Cache several times, so every launch streams its weight from HBM as a block of
the 28-block net does, not from a cache a repeated launch would have warmed. --mode graph (default) captures the pass
into a HIP graph (one linear chain) and times its replay with device events, so the host's launch cost (tens of
microseconds per Python call, the size of the kernels measured) is not in the number; --mode direct times the same
pass launched call by call: what a Python caller gets. Reported per form: the median over rounds, the minimum, and
the spread (max - min over rounds) as the noise against which two forms are compared. `plan` names the split the
library's plan picks (gemm_sm_plan); `faster_than_tile256` / `faster_than_s1` apply the plan's rule: faster by more
than the spread of the reference form's own rounds.
Prints one JSON line per (rows, shape); with --out also appends them to <out>/gemm_small.jsonl.
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from cosmos_predict2 import _native as N  # noqa: E402

BF16 = torch.bfloat16
HBM_PEAK = 8.0e12  # bytes / s, spec
SHAPES = (("qkv", 6144, 2048, "qkv"), ("proj", 2048, 2048, "res"), ("mlp1", 8192, 2048, "gelu"),
          ("mlp2", 2048, 8192, "res"))
SPLITS = (1, 2, 4, 8)


def with_stages(n, fn):
    """fn under the library's lab switch CP25_GEMM_SM_STAGES = n (K-tile buffers per workgroup; read per launch)."""
    def call(i):
        os.environ["CP25_GEMM_SM_STAGES"] = str(n)
        try:
            fn(i)
        finally:
            del os.environ["CP25_GEMM_SM_STAGES"]
    return call


def make_calls(M, Nn, K, epi, copies, dev, g, stages=()):
    """{form: callable(i)} launching the shape against weight copy i, and the plan's split."""
    a = torch.randn(M, K, generator=g, device=dev).to(BF16)
    ws = [(torch.randn(Nn, K, generator=g, device=dev) * 0.02).to(BF16) for _ in range(copies)]
    out = torch.empty(M, Nn, dtype=BF16, device=dev)
    hw = M
    # one workspace for every split of the shape (the wrappers' shared per-device buffer may be re-allocated when a
    # larger split follows: a captured graph must not hold the old one)
    wsp = torch.empty(N.gemm_sm_workspace_bytes(M, Nn, K, max(S for S in SPLITS if S <= K // 64)), dtype=torch.uint8,
                      device=dev)
    if epi == "res":
        x = torch.randn(M, 1, Nn, generator=g, device=dev).to(BF16)
        gate = torch.randn(1, 1, Nn, generator=g, device=dev).to(BF16)
        big = lambda i: N.gemm_res(a, ws[i], x, Nn, 0, gate, B=1, tok0=0, hw=hw, out=out)  # noqa: E731
        small = lambda S: (lambda i: N.gemm_sm_res(a, ws[i], x, Nn, 0, gate, B=1, tok0=0, hw=hw, out=out, split=S,
                                                   workspace=wsp))  # noqa: E731
        code = N.EPI_RES
    elif epi == "gelu":
        big = lambda i: N.gemm_epi(a, ws[i], epilogue=N.EPI_GELU, out=out)  # noqa: E731
        small = lambda S: (lambda i: N.gemm_sm_epi(a, ws[i], epilogue=N.EPI_GELU, out=out, split=S, workspace=wsp))  # noqa: E731
        code = N.EPI_GELU
    else:
        kw = torch.ones(128, dtype=BF16, device=dev)
        ang = torch.rand(M, 64, generator=g, device=dev) * 6.28
        cos, sin = torch.cos(ang), torch.sin(ang)
        D = Nn // 3
        big = lambda i: N.gemm_qkv(a, ws[i], kw, k_col0=D, k_cols=D, B=1, cos=cos, sin=sin, out=out)  # noqa: E731
        small = lambda S: (lambda i: N.gemm_sm_qkv(a, ws[i], kw, k_col0=D, k_cols=D, B=1, cos=cos, sin=sin, out=out,  # noqa: E731
                                                   split=S, workspace=wsp))
        code = N.EPI_QKV
    forms = {"tile256": big}
    for S in SPLITS:
        if S <= K // 64:
            forms[f"small_s{S}"] = small(S)
            for n in stages:
                forms[f"small_s{S}_st{n}"] = with_stages(n, small(S))
    return forms, N.gemm_sm_plan(M, Nn, K, code)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", default="320,1200")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--mode", choices=("graph", "direct"), default="graph")
    ap.add_argument("--cache-mib", type=int, default=768, help="distinct weight bytes per pass, at least")
    ap.add_argument("--stages", default="", help="also time each split with this many K-tile buffers (3, 4, 6), e.g. 3,6")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError("bench_gemm_small needs the GPU: there is no CPU path")
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    g = torch.Generator(device=dev).manual_seed(0)
    lines = []
    for M in (int(x) for x in a.rows.split(",")):
        for name, Nn, K, epi in SHAPES:
            wbytes = Nn * K * 2
            copies = max(8, -(-a.cache_mib * (1 << 20) // wbytes))
            forms, plan = make_calls(M, Nn, K, epi, copies, dev, g, tuple(int(x) for x in a.stages.split(",") if x))
            side = torch.cuda.Stream(dev)
            runners = {}
            for form, call in forms.items():
                def one_pass(call=call):
                    for i in range(copies):
                        call(i)
                with torch.cuda.stream(side):  # warm-up on the stream the capture uses (workspace, code objects)
                    one_pass()
                    one_pass()
                side.synchronize()
                if a.mode == "graph":
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=side):
                        one_pass()
                    runners[form] = gr.replay
                else:
                    runners[form] = one_pass
            torch.cuda.synchronize()
            for run in runners.values():  # one untimed round
                run()
            torch.cuda.synchronize()
            us = {form: [] for form in runners}
            for _ in range(a.rounds):
                for form, run in runners.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run()
                    e1.record()
                    e1.synchronize()
                    us[form].append(e0.elapsed_time(e1) * 1e3 / copies)
            rep = {}
            for form, v in us.items():
                med = float(np.median(v))
                rep[form] = dict(us_median=med, us_min=float(min(v)), us_spread=float(max(v) - min(v)),
                                 weight_gb_per_s=wbytes / med / 1e3, share_of_hbm_peak=wbytes / (med * 1e-6) / HBM_PEAK)
            ref = rep["tile256"]
            s1 = rep["small_s1"]
            best = min((f for f in rep if f != "tile256"), key=lambda f: rep[f]["us_median"])
            res = dict(rows=M, shape=name, N=Nn, K=K, epilogue=epi, mode=a.mode, weight_copies=copies, rounds=a.rounds,
                       weight_bytes=wbytes, plan=dict(small=plan.small, split=plan.split, tile=[plan.bm, plan.bn]),
                       forms=rep, best_small_form=best,
                       faster_than_tile256={f: ref["us_median"] - r["us_median"] > ref["us_spread"]
                                            for f, r in rep.items() if f != "tile256"},
                       faster_than_s1={f: s1["us_median"] - r["us_median"] > s1["us_spread"]
                                       for f, r in rep.items() if f not in ("tile256", "small_s1")},
                       stages_default=os.environ.get("CP25_GEMM_SM_STAGES", "library default"))
            line = json.dumps(res)
            print(line, flush=True)
            lines.append(line)
            del forms, runners
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "gemm_small.jsonl"), "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
