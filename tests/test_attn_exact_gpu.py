"""Every DiT attention route and the key-split merge against known answers, element by element.

The other attention tests hold a whole output tensor to rel-L2 <= 4e-3 against fp32 attention (a correct kernel
measures 2.2e-3) or compare two of our own kernels with torch.equal. Neither pins down which key, row, column, head
or batch entry a kernel read or wrote. Here the inputs are structured (tests/attn_truth.py) so that the answer is known
without running any attention:

  selector   every query row selects one key (winning score 90 log2 units, 58.5 for fp8 Q K^T; the smallest gap to a runner-up over
             all cases is 43.6 and 31.1 log2 units, 33.0 through q_norm): the output must EQUAL v[pi] bit for bit (the winner's bf16 P cancels against the row sum of the same
             P; the quotient is within 2^-22 of a bf16 value and rounds back to it). pi differs per (b, h) and contains
             key 0, 63, 64, 65, the last key, the ragged tile's first and last key, the first and last key of every key
             split, and as rows 0, the last, R - 1, R and every wave slice's first and last row. `tie`: two identical key
             rows in different tiles / splits: those rows get (v[a] + v[b]) / 2, held to the bound.
  far        every row selects one late key while the whole first key split is anti-aligned: the splits' lse differ by
             180 log2 units, so merge weights not formed against the row's largest lse overflow.
  uniform    every key has the same score +-b_row: the float64 mean of v, at the edges of the fixed shift's window (b_row
             33 where floor(min(b + 60, 126 - b)) changes branch, 63, 109.5; anti-aligned at 109.5 every term is 2^-125.5).
  gap        the online form's lazy rescale: a late key 10 .. 60 log2 units above the first tile's max, rows of one wave
             on both sides of kLazy = 24, and the same q row in a wave that rescales and in one that does not (equal bits).
             qngap: the same through the q_norm entry point, the gap set by the direction of the raw row.
  peaked     RMS-normed Gaussian q / k with q scaled until the fp32 score error allowance is used up.

uniform, gap, peaked and the tie rows are held to |out - ref| <= 2^-9 |ref| + 2^-8 A (attn_truth.bound, never
widened); the largest error / bound per case is printed (DESIGN.md section 3 keeps the table). tests/
test_attn_truth_cpu.py checks, without a GPU, every case's premise (score error <= 2^-10 nats or exact scores, the
selector's gap) and that an emulation of the kernels' arithmetic passes every case while eight wrong arithmetics fail.

Every case asserts the kernel name the library reports for its arguments (forms the default routing does not reach
at these shapes are forced with attn_self_select / attn_cross_select and restored), and writes its output into a
strided view of a sentinel-filled token-major buffer [Lq + 3, B, 2, H, 128]: the neighbouring slot and the extra rows
must be untouched.

Shapes: long-key routes B 2, H 2, Lq = 2 R + 33 (R = rows per workgroup: 545 / 673 / 801), Lk 4097 (one key past a
tile; 65 one-tile splits) and 4200 (Lk mod 64 = 40, past attn_fwd_wq's 32-key half stage; 1 and 3 splits); short-key
routes Lq 545, Lk 3, 64, 77, 130, 512 (the persistent form needs two tiles), and one persistent launch with 2 x the CU
count of blocks, so a workgroup walks several. Tail split: 29 query blocks x (CUs // 29 + 1) heads per width.

Not covered, on purpose:
  * attn_fwd_f8<.., fp8 Q K^T + fp8 P.V>: its P is quantised to quarter steps of log2 by an integer conversion, so
    neither the cancellation argument nor the bound's derivation applies; it needs its own.
  * attn_fwd_m16<self, prescaled, zero shift> and attn_fwd_wq<.., zero shift>: attn_route sends every long-key launch
    with usable bounds to the fixed shift, so no argument reaches them (tests/test_attn_truth_cpu.py
    ::test_zero_shift_long_key_names_unreachable).
"""
import functools
import math

import pytest
import torch

import attn_truth as T
from cosmos_predict2 import _native as N

BF16 = torch.bfloat16
SENTINEL = -1.5e30
LN2 = math.log(2.0)
M90 = (15 / 16, 3 / 4)   # 128 mq mk = 90 log2 units
M60 = (13 / 16, 9 / 16)  # 58.5 (bound product <= 60 with the margin); both exactly representable in e4m3
BIG_MQ = 1.25            # 128 x 1.25 x 3/4 = 120 > kGateFixed = 110: that block runs the online max
CUS_CPU = 256            # the CU count host functions assume without a device

M16 = "attn_fwd_m16<{}>"
ROUTES = {
    # key -> (kernel name, rows per workgroup, rows per wave, launch form)
    "self_np_fixed": (M16.format("self, fixed shift"), 256, 32, dict(pre=False, nb="tight")),
    "self_np_online": (M16.format("self, online max"), 256, 32, dict(pre=False, nb=None)),
    "self_fixed": (M16.format("self, prescaled, fixed shift"), 256, 32, dict(pre=True, nb="tight", self_form=0)),
    "self_online": (M16.format("self, prescaled, online max"), 256, 32, dict(pre=True, nb=None)),
    "self_gated": (M16.format("self, prescaled, gated fixed shift | online max"), 256, 32,
                   dict(pre=True, nb="weights", gated=True)),
    "wq320": ("attn_fwd_wq<self, prescaled, 320 rows, fixed shift>", 320, 80, dict(pre=True, nb="tight", self_form=320)),
    "wq384": ("attn_fwd_wq<self, prescaled, 384 rows, fixed shift>", 384, 96, dict(pre=True, nb="tight", self_form=384)),
    "f8_self": ("attn_fwd_f8<self, fp8 Q K^T>", 256, 32, dict(pre=True, nb="tight", fp8=True)),
    "cross_np_fixed": (M16.format("cross, fixed shift"), 256, 32, dict(pre=False, nb="tight", cross_form=0)),
    "cross_np_online": (M16.format("cross, online max"), 256, 32, dict(pre=False, nb=None, cross_form=0)),
    "cross_fixed": (M16.format("cross, prescaled, fixed shift"), 256, 32, dict(pre=True, nb="p97", cross_form=0)),
    "cross_zero": (M16.format("cross, prescaled, zero shift"), 256, 32, dict(pre=True, nb="tight", cross_form=0)),
    "cross_online": (M16.format("cross, prescaled, online max"), 256, 32, dict(pre=True, nb=None, cross_form=0)),
    "cross_gated": (M16.format("cross, prescaled, gated fixed shift | online max"), 256, 32,
                    dict(pre=True, nb="weights", gated=True, cross_form=0)),
    "pers_np_online": (M16.format("cross, online max, persistent"), 256, 32, dict(pre=False, nb=None, cross_form=1)),
    "pers_zero": (M16.format("cross, prescaled, zero shift, persistent"), 256, 32,
                  dict(pre=True, nb="tight", cross_form=1)),
    "pers_online": (M16.format("cross, prescaled, online max, persistent"), 256, 32,
                    dict(pre=True, nb=None, cross_form=1)),
    "f8_cross": ("attn_fwd_f8<cross, fp8 Q K^T>", 256, 32, dict(pre=True, nb="tight", fp8=True)),
}
SELF = ["self_np_fixed", "self_np_online", "self_fixed", "self_online", "self_gated", "wq320", "wq384", "f8_self"]
CROSS = ["cross_np_fixed", "cross_np_online", "cross_fixed", "cross_zero", "cross_online", "cross_gated", "f8_cross"]
PERS = ["pers_np_online", "pers_zero", "pers_online"]
QN_KINDS = ("qnorm", "qngap")  # cases through the q_norm entry point: d["raw"] is launched, d["qn"] the formula's q
ZERO = {"cross_zero", "pers_zero", "f8_self", "f8_cross"}  # (fp8 Q K^T: P = exp2(S) unshifted)


def _lq(route):
    return 2 * ROUTES[route][1] + 33


def _mk_cases():
    c = {}

    def add(name, kind, route, B, H, Lq, Lk, n_split=1, **kw):
        assert name not in c
        c[name] = dict(kind=kind, route=route, B=B, H=H, Lq=Lq, Lk=Lk, n_split=n_split, **kw)

    # case 1: selector, every route
    for r in SELF:
        for Lk, n in ((4097, 65), (4200, 1), (4200, 3)):
            add(f"sel-{r}-{Lk}-s{n}", "selector", r, 2, 2, _lq(r), Lk, n)
    for r in CROSS:
        for Lk in (3, 64, 77, 130, 512):
            add(f"sel-{r}-{Lk}-s1", "selector", r, 2, 2, 545, Lk)
        add(f"sel-{r}-512-s3", "selector", r, 2, 2, 545, 512, 3)
    for r in PERS:
        for Lk in (77, 130, 512):
            add(f"sel-{r}-{Lk}-s1", "selector", r, 2, 2, 545, Lk)
    add("sel-pers_zero-manyblocks", "selector", "pers_zero", 2, None, 545, 130, blocks_per_cu=2)
    # the q_norm entry point: routed (bounds: the library's width, 320 rows up to 8192 keys) and online (no bounds)
    for rope in (True, False):
        add(f"qn-wq320-rope{int(rope)}", "qnorm", "wq320", 2, 2, 673, 4200 if rope else 4097, rope=rope, self_form=1)
        add(f"qn-online-rope{int(rope)}", "qnorm", "self_online", 2, 2, 545, 4200 if rope else 4097, rope=rope)
    # case 2: the tail split of an unsplit launch, per width; a tie across two tail splits
    for r in ("self_fixed", "wq320", "wq384"):
        add(f"tail-{r}", "selector", r, 1, None, None, 4200, None, tail=True)
    # merge weights over a 180 log2 unit spread
    add("far-self_online-s3", "far", "self_online", 1, 2, 545, 4200, 3)
    add("far-wq384-s3", "far", "wq384", 1, 2, 801, 4200, 3)
    add("far-cross_zero-s3", "far", "cross_zero", 1, 2, 545, 512, 3)
    # case 3: uniform rows at the edges of the fixed shift's window
    for al in (True, False):
        add(f"uni-cross_fixed-{'al' if al else 'anti'}", "uniform", "cross_fixed", 1, 2, 545, 130, b_rows=(97.5,),
            aligned=al)
        for r in ("self_fixed", "wq320", "wq384", "self_gated"):
            add(f"uni-{r}-{'al' if al else 'anti'}", "uniform", r, 1, 2, _lq(r), 4200, b_rows=(33.0, 63.0, 109.5),
                aligned=al)
    # case 4: the online forms' lazy rescale
    add("gap-self_online-s1", "gap", "self_online", 1, 2, 545, 4200)
    add("gap-self_online-s3", "gap", "self_online", 1, 2, 545, 4200, 3)
    add("gap-self_np_online-s1", "gap", "self_np_online", 1, 2, 545, 4200)
    add("gap-cross_online-s1", "gap", "cross_online", 1, 2, 545, 500)
    add("gap-cross_online-s3", "gap", "cross_online", 1, 2, 545, 500, 3)
    add("gap-cross_np_online-s1", "gap", "cross_np_online", 1, 2, 545, 500)
    add("gap-pers_online-s1", "gap", "pers_online", 1, 2, 545, 500)
    add("gap-pers_np_online-s1", "gap", "pers_np_online", 1, 2, 545, 500)
    add("gap-self_gated-s1", "gap", "self_gated", 1, 2, 545, 4200)
    add("gap-cross_gated-s1", "gap", "cross_gated", 1, 2, 545, 500)
    for rope in (True, False):  # the q_norm online launch: the gap set through the raw rows' direction
        add(f"qngap-online-rope{int(rope)}", "qngap", "self_online", 1, 2, 545, 4200, rope=rope)
    add("qngap-online-rope1-s3", "qngap", "self_online", 1, 2, 545, 4200, 3, rope=True)
    # case 5: peaked Gaussian data and ties, one per family
    for r, Lq, Lk, splits in (("self_fixed", 545, 4200, (1, 3)), ("pers_zero", 545, 512, (1,)),
                              ("wq384", 801, 4200, (1, 3)), ("f8_self", 545, 4200, (1, 3))):
        for n in splits:
            add(f"peak-{r}-s{n}", "peaked", r, 1, 2, Lq, Lk, n)
            add(f"tie-{r}-s{n}", "selector", r, 1, 2, Lq, Lk, n, tie=(70, Lk - 90))
    return c


CASES = _mk_cases()


def cu_count(device=None):
    return CUS_CPU if device is None else torch.cuda.get_device_properties(device).multi_processor_count


def resolve(name, cus=CUS_CPU):
    """The case with the shape fields that depend on the CU count filled in."""
    c = dict(CASES[name])
    R = ROUTES[c["route"]][1]
    if c.get("blocks_per_cu"):
        nqb = -(-c["Lq"] // R)
        c["H"] = -(-c["blocks_per_cu"] * cus // (nqb * c["B"]))
    if c.get("tail"):
        # tests/test_attn_wide_gpu.py::test_wide_tail_split_one_round's recipe: the last head's last r query blocks
        # run as key-range splits that fit one round
        nqb = 29
        c["H"] = cus // nqb + 1
        c["Lq"] = nqb * R - 100
        r = nqb * c["H"] - cus
        c["t0"] = (nqb - r) * R
        ntiles = -(-c["Lk"] // 64)
        s = 1
        for n in range(2, 9):  # plan_tail: the most splits that still fit one round
            if -(-ntiles // -(-ntiles // n)) == n and r * n <= cus:
                s = n
        c["tail_s"] = s
        # tile 1 and the last tile but one: in the first and the last split of every split count plan_tail can pick
        # (2 .. 8), so the pair spans two tail splits whatever the plan decides; tail_s only feeds the CPU emulation
        a, b = 70, c["Lk"] - 90
        c["tie"] = (a, b)
        c["pin"] = {c["t0"] + 1: a, c["Lq"] - 1: b, c["t0"] - 1: a}
    return c


@functools.lru_cache(maxsize=2)  # a case is used once (the CPU file: twice in a row); the inputs are not kept
def _data_cached(name, cus):
    c = resolve(name, cus)
    route, R, RW, form = ROUTES[c["route"]]
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    seed = sum(map(ord, name))
    mq, mk = M60 if form.get("fp8") else M90
    kind = c["kind"]
    if kind == "selector":
        splits = {1, 3, c["n_split"] or 1, c.get("tail_s", 1)}
        kw = {}
        if form.get("gated") and Lq > 256:
            kw = dict(big_rows=slice(256, 512), big_mq=BIG_MQ)
        d = T.selector(B, H, Lq, Lk, mq, mk, seed, keys=T.key_targets(Lk, sorted(splits)),
                       rows=T.row_targets(Lq, R, RW), tie=c.get("tie"), pin=c.get("pin"), **kw)
        if c.get("tie"):
            d["ref"], d["A"] = _tie_reference(d, c["tie"])
    elif kind == "far":
        n0 = T.split_edges(Lk, c["n_split"])[1] + 1
        d = T.far_split(B, H, Lq, Lk, mq, mk, seed, n_anti=n0, late=Lk - 3)
    elif kind == "uniform":
        d = T.uniform_rows(B, H, Lq, Lk, c["b_rows"], mk, seed, aligned=c["aligned"])
    elif kind == "gap":
        d = T.gap_rows(B, H, Lq, Lk, seed)
    elif kind == "peaked":
        limit = 60.0 if form.get("fp8") else (96.0 if c["route"] in ZERO else 110.0)
        d = T.peaked(B, H, Lq, Lk, seed, limit, fp8=bool(form.get("fp8")))
    elif kind == "qnorm":
        d = T.qnorm_selector(B, H, Lq, Lk, 90.0, seed, c["rope"], keys=T.key_targets(Lk, (1, 3)),
                             rows=T.row_targets(Lq, R, RW))
    elif kind == "qngap":
        d = T.qnorm_gap_rows(B, H, Lq, Lk, seed, c["rope"])
    else:
        raise AssertionError(kind)
    return c, d


def _tie_reference(d, tie):
    """(ref, A) of the tie rows: (v[a] + v[b]) / 2, exact in float64 (the other keys' weight is below 2^-10 / 127 of
    it by the selector's precondition, far inside the bound)."""
    a, b = tie
    va, vb = d["v"][:, a].double(), d["v"][:, b].double()
    ref = ((va + vb) / 2)[:, None].expand_as(d["expected"])
    A = ((va.abs() + vb.abs()) / 2)[:, None].expand_as(d["expected"])
    return ref, A


def case_data(name, cus=CUS_CPU):
    return _data_cached(name, cus)


def launch_bounds(c, d, q=None):
    """(norm_bounds, slots value) of a case's launch: data-tight bounds x 1.0005, a product of 97 / 97.9 (inside the
    prescaled short-key fixed-shift window (96, 98]), or weight-style bounds 1.15 x too loose each (a product past 110
    and 96: the gated pair decides per block from the measured key bound in the slots)."""
    form = ROUTES[c["route"]][3]
    kind = "tight" if c["kind"] == "qnorm" and c["route"] != "self_online" else form["nb"]
    q = d["q"] if q is None else q
    qb, kb = T.norm_bounds(q, d["k"], 1.0005)
    kmax = d["k"].float().norm(dim=-1).max().item()
    if kind is None:
        return None, kmax
    if kind == "p97":
        return ((97.9 if c["kind"] == "uniform" else 97.0) / kb, kb), kmax
    if kind == "weights":
        return (qb * 1.15, kb * 1.15), kmax
    return (qb, kb), kmax


def _forms(c):
    form = ROUTES[c["route"]][3]
    return c.get("self_form", form.get("self_form")), form.get("cross_form")


def _run(device, name):
    c, d = case_data(name, cu_count(device))
    route, R, RW, form = ROUTES[c["route"]]
    B, H, Lq, Lk = c["B"], c["H"], c["Lq"], c["Lk"]
    pre, fp8, gated = form["pre"], bool(form.get("fp8")), bool(form.get("gated"))
    qn = None
    if c["kind"] in QN_KINDS:
        qn = dict(weight=d["weight"].to(device), cos=None if d["cos"] is None else d["cos"].to(device),
                  sin=None if d["sin"] is None else d["sin"].to(device), out_scale=d["out_scale"])
        q_in, nb_q = d["raw"], d["qn"]
    else:
        q_in = nb_q = d["q"]
    nb, kmax = launch_bounds(c, d, nb_q)
    self_form, cross_form = _forms(c)
    prev_s = N.attn_self_select(self_form) if self_form is not None else None
    prev_c = N.attn_cross_select(cross_form) if cross_form is not None else None
    try:
        got = N.attn_kernel_name(Lk, softmax_scale=LN2, norm_bounds=nb, prescaled=2 if gated else pre, fp8=int(fp8))
        assert got == route, (got, route)
        kw = dict(prescaled=pre, norm_bounds=nb, n_split=c["n_split"])
        if not pre:
            kw["softmax_scale"] = LN2  # scale * log2 e = 1: the same inputs serve the unscaled kernels
        if fp8:
            q8 = d["q8"] if "q8" in d else d["q"].float().to(torch.float8_e4m3fn).view(torch.uint8)
            k8 = d["k8"] if "k8" in d else d["k"].float().to(torch.float8_e4m3fn).view(torch.uint8)
            s = 1.0 if "q8" not in d else 4.0  # peaked: q8 = e4m3(4 q), k8 = e4m3(k / 4), a power of two that cancels
            assert torch.equal(q8.view(torch.float8_e4m3fn).float(), d["q"].float() * s)
            assert torch.equal(k8.view(torch.float8_e4m3fn).float(), d["k"].float() / s)
            kw["fp8_qk"] = (q8.to(device), k8.to(device))
        if gated:
            slots = torch.zeros((64, 32), dtype=torch.float32, device=device)
            slots[3, 0] = kmax
            kw["k_norm_slots"] = slots
        if qn is not None:
            kw["q_norm"] = qn
        if c.get("tail"):
            # the plan has a tail here, and its segment (rows t0 .. Lq of the last head) has the split count this
            # file's recipe expects: the workspace is s x rows x 129 floats (under a wide form the library sizes it for
            # attn_fwd_m16's plan of the shape too, hence >=)
            ws = N.load_library().cp25_attn_tail_workspace_bytes(B, H, Lq, Lk)
            need = c["tail_s"] * (Lq - c["t0"]) * 129 * 4
            assert ws == need if R == 256 else ws >= need, (ws, need)
            assert N.attn_plan(B, H, Lq, Lk) == 1
        buf = torch.full((Lq + 3, B, 2, H, 128), SENTINEL, dtype=BF16, device=device)
        out = buf[:Lq, :, 1].transpose(0, 1)
        N.attn_fwd(q_in.to(device), d["k"].to(device), d["v"].to(device), out=out, **kw)
        torch.cuda.synchronize()
    finally:
        if prev_c is not None:
            N.attn_cross_select(prev_c)
        if prev_s is not None:
            N.attn_self_select(prev_s)
    buf = buf.cpu()
    guard = torch.tensor(SENTINEL, dtype=BF16)
    assert (buf[:, :, 0] == guard).all(), "the neighbouring slot was written"
    assert (buf[Lq:] == guard).all(), "rows past Lq were written"
    o = buf[:Lq, :, 1].transpose(0, 1).contiguous()
    return c, d, o


def check(name, c, d, o):
    """The case's check on an output o [B, Lq, H, 128] bf16 (the kernel's or the emulation's): (passed, text)."""
    if not torch.isfinite(o.float()).all():
        return False, f"{name}: {(~torch.isfinite(o.float())).sum().item()} non-finite outputs"
    kind = c["kind"]
    if kind in ("selector", "far", "qnorm"):
        tie_rows = d.get("tie_rows")
        exact = torch.ones(o.shape[:3], dtype=torch.bool) if tie_rows is None else ~tie_rows
        bad = (o != d["expected"]).any(-1) & exact
        text = f"{name}: gap {d['gap']:.1f} log2 units, {int(bad.sum())} of {int(exact.sum())} rows differ from v[pi]"
        ok = not bad.any()
        if bad.any():
            text += f", first (b, row, h) {tuple(bad.nonzero()[0].tolist())}"
        if tie_rows is not None and tie_rows.any():
            r = ((o.double() - d["ref"]).abs() / T.bound(d["ref"], d["A"]))[tie_rows].max().item()
            text += f"; {int(tie_rows.sum())} tie rows: max error / bound {r:.3f}"
            ok = ok and r <= 1.0
        return ok, text
    r = T.ratio(o, d["ref"], d["A"])
    text = f"{name}: max error / bound {r:.3f}"
    ok = r <= 1.0
    if kind in ("gap", "qngap"):
        p = d["probes"]
        even, odd = o[:, p[0::2]], o[:, p[1::2]]
        same = all(torch.equal(even[:, :1].expand_as(x), x) for x in (even, odd))
        text += f"; the d = 22 row in {len(p)} waves: {'equal bits' if same else 'DIFFERENT bits'}"
        ok = ok and same
    return ok, text


pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(CASES))
def test_attn_exact(device, name):
    c, d, o = _run(device, name)
    ok, text = check(name, c, d, o)
    print(text)
    assert ok, text
