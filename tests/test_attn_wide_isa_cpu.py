"""Static ISA checks of attn_fwd_wq (attn_wide.hip; CPU: hipcc cross-compiles gfx950 here), every instantiation.

The kernel is one hand-placed stream: asm MFMAs whose operands the compiler does not pad for hazards, LDS reads from
inline asm retired by counted lgkmcnt waits, LDS-DMA asm that writes M0 undeclared, and a register budget at the
512-per-lane limit of one wave per SIMD. So, per instantiation: no LDS-read race (tools/isa_check.py), no M0 outside
the DMA asm, no VALU write within two wait states of an MFMA that reads it (tools/mfma_hazards.py), no spills and no
scratch instruction anywhere in the kernel, its loop included.
"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import isa_check  # noqa: E402
import mfma_hazards  # noqa: E402

SRC = os.path.join(ROOT, "cosmos-predict2.5_amd", "csrc", "attn_wide.hip")
# <kNQ, kMode, kTail>: 320 and 384 rows, fixed shift, the main grid's symbol and the tail segments'
KERNELS = ["attn_fwd_wqILi%dELi0ELi%dEE" % (nq, tail) for nq in (5, 6) for tail in (0, 1)]

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")


@pytest.fixture(scope="module")
def report():
    rep = isa_check.check(SRC, "attn_fwd_wq")
    asm, _ = isa_check.compile_asm(SRC)
    return rep, asm


def _one(rep, pat):
    hit = [(n, r) for n, r in rep.items() if pat in n]
    assert len(hit) == 1, (pat, list(rep))
    return hit[0]


def test_every_instantiation_is_checked(report):
    rep, _ = report
    assert len(rep) == len(KERNELS), list(rep)
    for pat in KERNELS:
        _one(rep, pat)


@pytest.mark.parametrize("pat", KERNELS)
def test_no_lds_read_races_and_no_compiler_m0(report, pat):
    _, r = _one(report[0], pat)
    assert not r["races"], r["races"][:3]
    assert not r["m0_uses"], r["m0_uses"][:3]


@pytest.mark.parametrize("pat", KERNELS)
def test_no_asm_mfma_operand_hazards(report, pat):
    name, _ = _one(report[0], pat)
    asm = report[1]
    i = asm.index(name + ":")
    body = asm[i:asm.index(".Lfunc_end", i)].split("\n")
    assert sum(l.strip().startswith("v_mfma") for l in body) >= 170  # the loop's stream is in this text
    found = mfma_hazards.check(body)
    assert not found, [(b, a, ws) for _, a, b, ws in found[:3]]


@pytest.mark.parametrize("pat", KERNELS)
def test_no_spills_no_scratch(report, pat):
    name, r = _one(report[0], pat)
    assert r.get("VGPRs Spill") == 0 and r.get("SGPRs Spill") == 0, r
    assert r["inloop_scratch"] == 0
    assert r["inloop_vmcnt0"] == 1, r["inloop_vmcnt0"]  # the drain of the iteration's DMA pieces, nothing else
    asm = report[1]
    i = asm.index(name + ":")
    body = asm[i:asm.index(".Lfunc_end", i)]
    assert not re.search(r"^\s*scratch_", body, re.M)
