"""CPU: the attention launch routing (csrc/attn_route.h) against the table recorded from the commit before the routing
moved into that header (tests/golden/attn_route.json, tools/record_attn_route.py): kernel names over key counts, norm
bounds, flags and the process-wide forms; key-split plans and tail workspace sizes over shapes. None of it touches a
GPU: without one the library plans for 256 CUs, the MI355X's count, as the table's recording did.
(a) the built library reproduces the table; (b) so does the header compiled alone by g++ (no HIP in it); (c) that
program is clean under ASan + UBSan, and every tail plan it walks keeps plan_tail's contract; (d) the launch and
cp25_attn_kernel take their route from the same function, and the three earlier copies of the decision are gone."""
import json
import os
import re
import subprocess
import sys

import pytest

import __graft_entry__
from cosmos_predict2 import _native

ROOT = __graft_entry__.ROOT
CSRC = os.path.join(ROOT, "cosmos-predict2.5_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_attn_route  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "attn_route.json")) as f:
        g = json.load(f)
    assert g["cus"] == 256 and re.fullmatch(r"[0-9a-f]{40}", g["commit"])
    return g


def _expected(g):
    names = [[[[g["names"][i] for i in c] for c in b] for b in a] for a in g["name_idx"]]
    return names, g["plans"]


def test_library_reproduces_golden(golden):
    lib = _native.load_library()
    forms = (lib.cp25_attn_self_select(1), lib.cp25_attn_cross_select(1))
    lib.cp25_attn_self_select(forms[0]), lib.cp25_attn_cross_select(forms[1])
    names, plans = record_attn_route.record(lib, golden)
    assert (lib.cp25_attn_self_select(forms[0]), lib.cp25_attn_cross_select(forms[1])) == forms  # both restored
    want_names, want_plans = _expected(golden)
    assert plans == want_plans
    assert names == want_names
    # the issue's spot values, so a re-recorded table cannot drift unnoticed
    at = {tuple(s): p for s, p in zip(golden["shapes"], plans[golden["self_forms"].index(1)])}
    assert at[(2, 16, 109120, 109120)] == [1, 94613760] and at[(1, 16, 13664, 13664)] == [1, 49354368]
    assert at[(1, 16, 864, 6912)] == [4, 0] and at[(1, 1, 256, 109120)] == [8, 0]


def _queries(g):
    """The table as the stand-alone program's stdin, and the lines it has to print."""
    want_names, want_plans = _expected(g)
    q, want = [], []
    for (s, c), by_lk in zip(g["forms"], want_names):
        for lk, by_bound in zip(g["Lk"], by_lk):
            for (qb, kb), by_flag in zip(g["bounds"], by_bound):
                for (pre, fp8, scale), name in zip(g["flags"], by_flag):
                    q.append(f"name {s} {c} {lk} {float(scale).hex()} {float(qb).hex()} {float(kb).hex()} {pre} {fp8}")
                    want.append(name)
    for s, by_shape in zip(g["self_forms"], want_plans):
        for shape, (plan, tail) in zip(g["shapes"], by_shape):
            q.append("plan %d %d %d %d %d" % (s, *shape))
            want.append(f"{plan} {tail}")
    return "\n".join(q) + "\n", want


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_header_alone_reproduces_golden(golden, tmp_path, sanitize):
    exe = str(tmp_path / "attn_route_main")
    # the sanitizers' runtimes linked into the program itself: a host program with its own main, run directly
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
             "-g"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "attn_route_main.cpp"), "-o", exe], check=True)
    stdin, want = _queries(golden)
    r = subprocess.run([exe], input=stdin, capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    assert r.stdout.splitlines() == want


def _code(path):
    """A C++ source without its comments and string literals (identifiers in prose are not code)."""
    src = open(path).read()
    return re.sub(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\])*"', " ", src, flags=re.S)


def _body(code, name):
    """The braces-matched body of the function defined as name(...) {."""
    m = re.search(r"\b%s\s*\(" % re.escape(name), code)
    assert m, name
    i = code.index("{", code.index(")", m.end()))
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(code[j], 0)
        j += 1
        if depth == 0:
            return code[i:j]


def test_name_and_launch_share_one_route():
    units = {f: _code(os.path.join(CSRC, f)) for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}
    assert "attn_fwd.hip" in units and "attn_route.h" in units
    idents = {f: set(re.findall(r"[A-Za-z_]\w*", c)) for f, c in units.items()}
    for old in ("m16_mode", "m16_gated", "wide_rows", "wq_default_rows", "use_xattn_persistent", "M16"):
        assert not [f for f, ids in idents.items() if old in ids], old
    fwd = units["attn_fwd.hip"]
    for fn in ("attn_launch", "cp25_attn_kernel"):
        body = _body(fwd, fn)
        assert re.search(r"\battn_route\s*\(\s*(route_query\s*\(|query\b)", body), fn
    assert "attn_route_name" in _body(fwd, "cp25_attn_kernel")
    # attn_route is defined once, in the header, and the process-wide forms reach it through route_query alone
    assert len(re.findall(r"\bAttnRoute\s+attn_route\s*\(", "".join(units.values()))) == 1
    assert re.search(r"\bAttnRoute\s+attn_route\s*\(", units["attn_route.h"])
    includes = re.findall(r"#include\s*[<\"]([^>\"]*)", open(os.path.join(CSRC, "attn_route.h")).read())
    assert sorted(includes) == ["algorithm", "cstddef", "cstdint"]
    readers = [fn for fn in ("route_query", "attn_launch", "cp25_attn_kernel", "cp25_attn_plan")
               if re.search(r"\bg_(self|xattn)_form\b", _body(fwd, fn))]
    assert readers == ["route_query"]
