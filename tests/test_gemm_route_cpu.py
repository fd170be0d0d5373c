"""CPU: the small-M GEMM plan (csrc/gemm_route.h). None of it touches a GPU.
(a) cp25_gemm_sm_plan / cp25_gemm_sm_workspace_bytes of the built library equal the header compiled alone by g++ into a
stand-alone program (tests/host/gemm_route_main.cpp, no HIP in it), over M in 1 .. 4096, the 2B net's (N, K) pairs, the
five epilogues and 104 / 256 CUs; (b) that program is also built with ASan + UBSan, its runtimes linked into the program,
and run directly: clean; (c) every planned launch keeps the split's contract: the runs cover every K-tile exactly once
in ascending order, the first (K / 64) % S one tile longer, S <= K / 64, a workspace of at least S M N 4 bytes for
S > 1 and none for S = 1; (d) the six new symbols are declared in cp25.h and exported by libcp25.so, and gemm_small.hip
and the entry points take the plan from the header."""
import os
import re
import subprocess

import pytest

import __graft_entry__
from cosmos_predict2 import _native

ROOT = __graft_entry__.ROOT
CSRC = os.path.join(ROOT, "cosmos-predict2.5_amd", "csrc")
SYMBOLS = ("cp25_gemm_sm_epi", "cp25_gemm_sm_res", "cp25_gemm_sm_hnorm", "cp25_gemm_sm_qkv", "cp25_gemm_sm_plan",
           "cp25_gemm_sm_workspace_bytes")
# (N, K) of the 2B net's per-frame launches: fused QKV, the 2048-wide projections, MLP layers 1 and 2, the patch embedder
SHAPES = ((6144, 2048), (2048, 2048), (8192, 2048), (2048, 8192), (2048, 128))
MS = sorted(set(range(1, 130)) | set(range(130, 4097, 61)) | {255, 256, 257, 320, 1200, 2047, 2048, 2049, 4096})
CUS = (104, 256)


def _grid():
    return [(M, Nn, K, epi, cus) for cus in CUS for Nn, K in SHAPES for epi in range(5) for M in MS]


def _unpack(v):
    return dict(small=bool(v & 1), split=(v >> 8) & 0xFF, bm=((v >> 16) & 0xFF) * 16, bn=((v >> 24) & 0x7F) * 16)


@pytest.fixture(scope="module")
def library_plans():
    lib = _native.load_library()
    out = []
    for M, Nn, K, epi, cus in _grid():
        v = lib.cp25_gemm_sm_plan(M, Nn, K, epi, cus)
        assert v > 0, (M, Nn, K, epi, cus, v)
        out.append((v, lib.cp25_gemm_sm_workspace_bytes(M, Nn, K, _unpack(v)["split"])))
    return out


def _build(tmp_path, sanitize):
    exe = str(tmp_path / "gemm_route_main")
    # the sanitizers' runtimes linked into the program itself: a host program with its own main, run directly
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
             "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "gemm_route_main.cpp"), "-o", exe], check=True)
    return exe


def _run(exe, stdin):
    r = subprocess.run([exe], input=stdin, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_header_alone_equals_library(library_plans, tmp_path, sanitize):
    exe = _build(tmp_path, sanitize)
    got = _run(exe, "".join("plan %d %d %d %d %d\n" % q for q in _grid()))
    assert got == [f"{v} {ws}" for v, ws in library_plans]


def test_plan_invariants(library_plans, tmp_path):
    exe = _build(tmp_path, False)
    seen = set()
    for (M, Nn, K, epi, cus), (v, ws) in zip(_grid(), library_plans):
        p = _unpack(v)
        nk = K // 64
        assert 1 <= p["split"] <= nk and (p["bm"], p["bn"]) == (64, 128), (M, Nn, K, p)
        assert p["small"] or p["split"] == 1
        assert (ws >= p["split"] * M * Nn * 4) if p["split"] > 1 else ws == 0
        seen.add((nk, p["split"]))
    # every (K-tiles, split) the plan uses, and every split a caller may force: each K-tile in exactly one run
    seen |= {(nk, S) for nk in (1, 2, 3, 8, 32, 128) for S in range(1, min(nk, 64) + 1)}
    queries = sorted(seen)
    for (nk, S), line in zip(queries, _run(exe, "".join(f"runs {nk} {S}\n" for nk, S in queries))):
        runs = [tuple(int(x) for x in r.split(":")) for r in line.split()]
        assert len(runs) == S and runs[0][0] == 0 and runs[-1][0] + runs[-1][1] == nk
        assert all(a[0] + a[1] == b[0] for a, b in zip(runs, runs[1:])) and all(n >= 1 for _, n in runs)
        assert [n for _, n in runs] == [nk // S + (1 if r < nk % S else 0) for r in range(S)]
    assert _run(exe, "runs 32 3\n") == ["0:11 11:11 22:10"]
    # a split past K / 64, or no split, has no workspace to speak of
    assert _run(exe, "ws 320 2048 128 3\nws 320 2048 2048 1\nws 320 2048 2048 4\n") == ["0", "0", str(4 * 320 * 2048 * 4)]


def test_plan_of_the_current_device_and_errors():
    lib = _native.load_library()
    # cus = 0: the current device, or 256 without one; this test runs without a GPU as well as with one
    v = lib.cp25_gemm_sm_plan(320, 2048, 2048, 0, 0)
    assert v > 0 and _unpack(v)["split"] >= 1
    assert lib.cp25_gemm_sm_plan(320, 2040, 2048, 0, 256) == -95 and lib.cp25_gemm_sm_plan(320, 2048, 96, 0, 256) == -95
    assert lib.cp25_gemm_sm_plan(0, 2048, 2048, 0, 256) == -22 and lib.cp25_gemm_sm_plan(320, 2048, 2048, 5, 256) == -22
    p = _native.gemm_sm_plan(320, 2048, 2048, _native.EPI_RES, 256)
    assert (p.bm, p.bn) == (64, 128) and 1 <= p.split <= 32
    assert _native.gemm_sm_workspace_bytes(320, 2048, 2048, 4) == 4 * 320 * 2048 * 4


def test_symbols_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "cp25.h")).read()
    lib = _native.load_library()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in cp25.h"
        assert hasattr(lib, name), f"libcp25.so does not export {name}"
        assert name in _native.SIGNATURES
    # one plan: the kernels' file includes the header and neither restates the thresholds nor the run arithmetic
    small = open(os.path.join(CSRC, "gemm_small.hip")).read()
    assert '#include "gemm_route.h"' in small
    assert re.search(r"\bgemm_plan\s*\(", small) and re.search(r"\brun_begin\s*\(", small)
    assert not re.search(r"\b(kSmBlocksPerCu|kSplitMinRunTiles|kSplitMax)\b", small)
    includes = re.findall(r"#include\s*[<\"]([^>\"]*)", open(os.path.join(CSRC, "gemm_route.h")).read())
    assert sorted(includes) == ["algorithm", "cstddef", "cstdint"]
