"""cp25_attn_na3d (csrc/attn_na.hip) against known answers, element by element, in the manner of
tests/test_attn_exact_gpu.py and tests/test_attn_causal_gpu.py.

tests/test_sparse_attn_gpu.py holds a whole launch to rel-L2 <= 4e-3 (a few wrong rows among thousands pass, and no
score there ever leaves the first key tile's max by kLazy) and checks membership with q = 0 (blind to the score path
and to a K row paired with another key's V row). Here the inputs are structured (tests/na_truth.py) so that every
output element is known without running attention:

  sel      every query selects one key of its own box; the output must EQUAL v[pi] bit for bit. In every group and every
           (b, h), pi covers box positions 0, 63, 64, 65, the last key, every key tile's first and last key and the
           box's eight corners. selln2: the same through the unscaled entry with softmax_scale = ln 2.
  out      the lure: the selector confined to dims 0 .. 63; every key token OUTSIDE a chosen group's box (the first, a
           middle, the last) and that group's queries carry u x 16 in dims 64 .. 127, so an outside key read for such a
           query scores 2^14 log2 units and overflows. The output must not change by a bit.
  uni      equal scores (0, 8, 32, 64 by row) over the box: the float64 mean of v over the box, within attn_truth.bound.
  gap      the lazy rescale: the box's last key (in the ragged key tile) 10 .. 60 log2 units above the first tile's max,
           rows of one wave on both sides of kLazy = 24; the same q row in a wave that rescales and in one that does not
           gives the same bits. On k385_full (tiles 128, 128, 128, 1) and k130_block (tiles 128 + 2 per box).
  stair    every key tile's max 30 above the previous one: a rescale at every tile; stairrev: descending.
  one      a box of one key: Gaussian q / k / v, the output is v bit for bit.

uni, gap and stair are held to |out - ref| <= 2^-9 |ref| + 2^-8 A against float64 masked attention (attn_truth.bound,
never widened); the largest error / bound is printed per case (DESIGN.md section 6f keeps the table). The grids
(na_truth.NA_EXACT_CASES) have boxes of 1, 63, 65, 130, 195, 385 and 24 keys: last key tiles of 1, 2 and 3 live keys,
three and seven key tiles, a group of 130 queries (a full tile and one whose waves 1 - 3 are empty slots), windows of
one key along an axis and dilation along t. (B, H) differ per grid, so n_tiles H B is 4 (below the 8 XCDs), 12 (no
multiple of 8) and multiples of 8. Plans are valid ones from sparse_attn.plan_tables; windows of one key go in as
resolved triples (build_plan would read them as the full extent).

Most launches take q / k / v as column views of one token-major [L, B, 3 H 128] buffer, as the DiT passes them; every
launch writes into a slice of a sentinel-filled buffer: everything outside the slice must be untouched, every element
inside written. tests/test_na_truth_cpu.py checks, without a GPU, every premise and that an emulation of the kernel's
arithmetic passes every case while seven wrong kernels fail."""
import functools
import math

import pytest
import torch

import attn_truth as AT
import na_truth as NT
from cosmos_predict2 import _native as N
from cosmos_predict2 import sparse_attn as SA

BF16 = torch.bfloat16
SENT = -1.5e30
LN2 = math.log(2.0)
D = AT.D

# (B, H) per grid: n_tiles H B = 120, 12, 36, 32, 48, 4, 36
BH = {"one_key": (1, 2), "k63": (1, 3), "k65": (2, 1), "k130_block": (2, 2), "k195": (2, 3), "k385_full": (1, 1),
      "dil_t": (1, 2)}


def _cases():
    c = {}
    for i, g in enumerate(NT.NA_EXACT_CASES):
        c[f"sel-{g}"] = dict(family="sel", grid=g, seed=100 + i, fused=True)
        c[f"selln2-{g}"] = dict(family="sel", grid=g, seed=200 + i, fused=False, ln2=True)
        c[f"uni-{g}"] = dict(family="uni", grid=g, seed=300 + i, fused=True)
        if g != "k385_full":  # its one box holds every token: nothing is outside
            c[f"out-{g}"] = dict(family="out", grid=g, seed=400 + i, fused=False)  # (the lured launches are fused)
    c["gap-k385_full"] = dict(family="gap", grid="k385_full", seed=500, fused=True)
    c["gap-k130_block"] = dict(family="gap", grid="k130_block", seed=501, fused=True)
    c["stair-k385_full"] = dict(family="stair", grid="k385_full", seed=600, fused=True)
    c["stairrev-k385_full"] = dict(family="stair", grid="k385_full", seed=601, fused=False, reverse=True)
    c["one-one_key"] = dict(family="one", grid="one_key", seed=700, fused=True)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def plan_host(grid_name):
    """(q_tok [n_tiles, 128], box [n_tiles, 4]) int32 numpy: the plan sparse_attn.plan_tables makes for the grid."""
    geo = NT.geometry(grid_name)
    return SA.plan_tables(geo["grid"], geo["window"], geo["stride"], geo["dilation"])


@functools.lru_cache(maxsize=None)
def case_data(name):
    """The case's inputs and answer (host tensors): computed once, never modified."""
    c = CASES[name]
    geo = NT.geometry(c["grid"])
    B, H = BH[c["grid"]]
    fam = c["family"]
    if fam == "sel":
        return NT.na_selector(geo, B, H, 1.0, 1.0, c["seed"])
    if fam == "out":
        return NT.na_outsider(geo, B, H, c["seed"])
    if fam == "uni":
        return NT.na_uniform(geo, B, H, c["seed"])
    if fam == "gap":
        return NT.na_gap_rows(geo, B, H, c["seed"])
    if fam == "stair":
        return NT.na_staircase(geo, B, H, c["seed"], reverse=c.get("reverse", False))
    return NT.na_one_key(geo, B, H, c["seed"])


def launches(name):
    """How many launches the case makes as (fused, contiguous)."""
    c = CASES[name]
    if c["family"] == "out":
        return len(case_data(name)["lured"]), 1
    return (1, 0) if c["fused"] else (0, 1)


def _where(grid_name, idx):
    """'(b, token, head) = ..., tile t slot s (wave w), group g rank r' for an index (b, token, head, ...)."""
    b, tok, h = (int(x) for x in idx[:3])
    q_tok, _ = plan_host(grid_name)
    tile, slot = (int(x[0]) for x in (q_tok == tok).nonzero())
    geo = NT.geometry(grid_name)
    return (f"(b, token, head) = ({b}, {tok}, {h}), tile {tile} slot {slot} (wave {slot // 32}), group "
            f"{int(geo['group_of'][tok])} rank {int(geo['pos_of'][tok])}")


def _equal(grid_name, what, o, want):
    """(passed, text) of a bit-for-bit comparison of two [B, L, H, 128] bf16 tensors."""
    if not torch.isfinite(o.float()).all():
        bad = ~torch.isfinite(o.float()).all(-1)
        return False, f"{what}: {int(bad.sum())} rows with non-finite outputs, first {_where(grid_name, bad.nonzero()[0])}"
    bad = (o != want).any(-1)
    if bad.any():
        return False, f"{what}: {int(bad.sum())} of {bad.numel()} rows differ, first {_where(grid_name, bad.nonzero()[0])}"
    return True, f"{what}: all {bad.numel()} rows equal"


def _bounded(grid_name, what, o, ref, A):
    """(passed, text) of the per-element bound; the text carries the worst error / bound and where it is."""
    if not torch.isfinite(o.float()).all():
        bad = ~torch.isfinite(o.float()).all(-1)
        return False, f"{what}: {int(bad.sum())} rows with non-finite outputs, first {_where(grid_name, bad.nonzero()[0])}"
    r = (o.double() - ref).abs() / AT.bound(ref, A)
    worst = r.max().item()
    text = f"{what}: max error / bound {worst:.3f}"
    if worst > 1.0:
        over = (r > 1.0).any(-1)
        text += f", {int(over.sum())} rows over it, first {_where(grid_name, over.nonzero()[0])}"
    return worst <= 1.0, text


def evaluate(name, run):
    """The case's check of run(grid name, q, k, v, fused, ln2) -> out [B, L, H, 128] bf16 on the host (the kernel, or
    the CPU emulation of it): (passed, text)."""
    c, d = CASES[name], case_data(name)
    g, fam = c["grid"], c["family"]
    ln2 = c.get("ln2", False)
    if fam == "out":
        base = d["base"]
        o = run(g, base["q"], base["k"], base["v"], c["fused"], ln2)
        ok, text = _equal(g, f"{name}: gap {base['gap']:.1f} log2 units, selector vs v[pi]", o, base["expected"])
        for lu in d["lured"]:
            ol = run(g, lu["q"], lu["k"], base["v"], True, ln2)
            ok2, t2 = _equal(g, f"lured group {lu['group']} vs the un-lured run", ol, o)
            ok, text = ok and ok2, text + "; " + t2
        return ok, text
    o = run(g, d["q"], d["k"], d["v"], c["fused"], ln2)
    if fam == "sel":
        return _equal(g, f"{name}: gap {d['gap']:.1f} log2 units, vs v[pi]", o, d["expected"])
    if fam == "one":
        return _equal(g, f"{name}: vs v", o, d["expected"])
    ok, text = _bounded(g, name, o, d["ref"], d["A"])
    if fam == "gap":
        same = all(torch.equal(o[:, p[:1]].expand(-1, len(p), -1, -1), o[:, p]) for p in d["probes"])
        text += f"; the d = 22 row in {sum(len(p) for p in d['probes'])} waves: " \
                f"{'equal bits' if same else 'DIFFERENT bits'} per box"
        ok = ok and same
    return ok, text


def _launch(device, grid_name, q, k, v, fused, ln2):
    """One launch of host q / k / v [B, L, H, 128] into a framed output; returns the output on the host."""
    B, L, H, _ = q.shape
    geo = NT.geometry(grid_name)
    q_tok, box = plan_host(grid_name)
    plan = SA.NaPlan(grid=geo["grid"], window=geo["window"], stride=geo["stride"], dilation=geo["dilation"],
                     q_tok=torch.from_numpy(q_tok).to(device), box=torch.from_numpy(box).to(device))
    if fused:  # token-major, batch inner: the DiT's layout
        qkv = torch.empty(L, B, 3 * H * D, dtype=BF16, device=device)
        for i, t in enumerate((q, k, v)):
            qkv[:, :, i * H * D:(i + 1) * H * D] = t.to(device).transpose(0, 1).reshape(L, B, H * D)
        qd, kd, vd = (qkv[:, :, i * H * D:(i + 1) * H * D].view(L, B, H, D).transpose(0, 1) for i in range(3))
        big = torch.full((L + 2, B, H + 1, D), SENT, dtype=BF16, device=device)
        out = big[1:L + 1, :, :H].transpose(0, 1)
    else:
        qd, kd, vd = q.to(device), k.to(device), v.to(device)
        big = torch.full((B, L + 2, H + 1, D), SENT, dtype=BF16, device=device)
        out = big[:, 1:L + 1, :H]
    kw = dict(softmax_scale=LN2) if ln2 else dict(prescaled=True)
    N.attn_na3d(qd, kd, vd, plan, out=out, **kw)
    torch.cuda.synchronize()
    res = out.cpu().contiguous()
    out.fill_(SENT)
    assert torch.equal(big, torch.full_like(big, SENT)), f"{grid_name}: wrote outside the output slice"
    unwritten = (res == torch.full_like(res, SENT)).any(-1)
    assert not unwritten.any(), f"{grid_name}: {int(unwritten.sum())} rows not (fully) written, first " \
                                f"{_where(grid_name, unwritten.nonzero()[0])}"
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_na3d_exact(device, name):
    ok, text = evaluate(name, functools.partial(_launch, device))
    print(text)
    assert ok, text
