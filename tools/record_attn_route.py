#!/usr/bin/env python3
"""Records tests/golden/attn_route.json: what a libcp25.so answers, on a machine without a GPU (num_cus() = 256), for
cp25_attn_kernel over a grid of key counts, norm bounds, flags and the two process-wide forms, and for cp25_attn_plan /
cp25_attn_tail_workspace_bytes over a list of shapes under every self form. The table is the behaviour the routing
header (csrc/attn_route.h) has to keep, so it is recorded from a build of the commit BEFORE a change to the routing:

    git worktree add /tmp/parent <commit> && make -C /tmp/parent/cosmos-predict2.5_amd/csrc
    python tools/record_attn_route.py --lib /tmp/parent/cosmos-predict2.5_amd/cosmos_predict2/_lib/libcp25.so \\
        --commit $(git rev-parse <commit>)

tests/test_attn_route_cpu.py replays it against the built library and against the header compiled alone."""
import argparse
import ctypes
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LK = [1, 64, 65, 128, 512, 4096, 4097, 8192, 8193, 109120, 163840]
BOUNDS = [
    (0.0, 0.0), (0.0, 5.0),
    # products on each side of 30 / 1.13, 60, 96, 98 and 110
    (5.0, 5.3), (5.0, 5.31), (5.0, 12.0), (5.0, 12.01), (8.0, 12.0), (8.0, 12.01), (8.0, 12.25), (8.0, 12.26),
    (8.0, 13.75), (8.0, 13.76),
    # the same for an unscaled q at softmax_scale 1 (product x log2 e against 98 and 110)
    (8.0, 8.49), (8.0, 8.5), (8.0, 9.53), (8.0, 9.54),
    # the pairs the GPU tests use
    (1.5, 11.6), (8.5, 12.5), (9.0, 12.5), (4.4, 34.6), (11.0, 11.0), (7.0, 11.6),
]
# (prescaled, fp8, softmax_scale); a prescaled launch's scale is not read
FLAGS = [(0, f, s) for f in (0, 1, 2) for s in (128 ** -0.5, 1.0)] + [(p, f, 1.0) for p in (1, 2) for f in (0, 1, 2)]
SELF_FORMS = [0, 1, 320, 384]
FORMS = [(s, c) for s in SELF_FORMS for c in (0, 1)]
SHAPES = [(2, 16, 109120, 109120), (1, 16, 13664, 13664), (1, 40, 13640, 109120), (1, 16, 864, 6912),
          (1, 1, 256, 109120), (1, 16, 4800, 4800), (1, 16, 256, 64), (1, 1, 1, 1), (7, 16, 23400, 163800)]


def load(path):
    lib = ctypes.CDLL(path)
    lib.cp25_attn_kernel.restype = ctypes.c_char_p
    lib.cp25_attn_kernel.argtypes = [ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_int,
                                     ctypes.c_int]
    lib.cp25_attn_plan.restype = ctypes.c_int
    lib.cp25_attn_plan.argtypes = [ctypes.c_int] * 5
    lib.cp25_attn_tail_workspace_bytes.restype = ctypes.c_size_t
    lib.cp25_attn_tail_workspace_bytes.argtypes = [ctypes.c_int] * 4
    for f in (lib.cp25_attn_self_select, lib.cp25_attn_cross_select):
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int]
    return lib


def record(lib, grid):
    """The library's answers over grid (the axes above, as a dict): names[form][Lk][bound][flag] and
    plans[self form][shape] = [plan, tail bytes]. Restores both forms."""
    self0, cross0 = lib.cp25_attn_self_select(1), lib.cp25_attn_cross_select(1)
    try:
        names = []
        for s, c in grid["forms"]:
            assert lib.cp25_attn_self_select(s) >= 0 and lib.cp25_attn_cross_select(c) >= 0
            names.append([[[lib.cp25_attn_kernel(lk, scale, qb, kb, pre, fp8).decode()
                            for pre, fp8, scale in grid["flags"]] for qb, kb in grid["bounds"]] for lk in grid["Lk"]])
        plans = []
        for s in grid["self_forms"]:
            assert lib.cp25_attn_self_select(s) >= 0
            plans.append([[lib.cp25_attn_plan(*shape, 128), lib.cp25_attn_tail_workspace_bytes(*shape)]
                          for shape in grid["shapes"]])
    finally:
        lib.cp25_attn_self_select(self0)
        lib.cp25_attn_cross_select(cross0)
    return names, plans


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", required=True, help="libcp25.so built at --commit")
    ap.add_argument("--commit", required=True, help="hash of the commit the library was built from")
    ap.add_argument("-o", default=os.path.join(ROOT, "tests", "golden", "attn_route.json"))
    args = ap.parse_args()
    grid = {"forms": FORMS, "Lk": LK, "bounds": BOUNDS, "flags": FLAGS, "self_forms": SELF_FORMS, "shapes": SHAPES}
    names, plans = record(load(args.lib), grid)
    table = sorted({n for a in names for b in a for c in b for n in c})
    idx = {n: i for i, n in enumerate(table)}
    out = {"commit": args.commit, "cus": 256, **grid, "names": table,
           "name_idx": [[[[idx[n] for n in c] for c in b] for b in a] for a in names], "plans": plans}
    with open(args.o, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"{args.o}: {sum(len(c) for a in names for b in a for c in b)} names ({len(table)} distinct), "
          f"{sum(len(p) for p in plans)} plans")
