"""cp25_gemm_epi / _res / _hnorm / _qkv / _fp8, bit for bit against float64, in every kernel form a shape can take.

Premise: the operands are small integers (a in [-8, 8], w in [-4, 4] as bf16, [-64, 64] x [-4, 4] at K = 64; [-8, 8] as
float8_e4m3fn), some cases with every row scaled by a power of two (still exact). Every product is an integer and every
partial sum stays below 2^24 as long as |a| |w|^T < 2^24 (the largest case, K = 2048, reaches 2.1e4), so fp32
accumulation is exact in any order and the one rounding left is the output's: the kernel must equal a.double() @ w.double().T rounded
once to bf16 under torch.equal, no tolerance. test_premise (no GPU) checks that per case: the abs-sum bound, torch's
fp32 CPU product equal to the fp64 one, and at K >= 2048 a non-zero share of exact bf16 ties. Measured shares (outputs
that round at all / exact ties; the cases of one K lie within half a point of each other, M = 1 within two): K = 64
with the wide a 52 % / 21 %, K = 128 3.7 % / 3.7 %, K = 192 7.3 % / 7.1 %, K = 256 10.6 % / 10.1 %, K = 320 13.7 % /
12.5 %, K = 384 16.2 % / 14.2 %, K = 2048 43 % / 22 %, ph_n8192 3.7 % / 3.6 %; the tail-plan operands 3.7 % / 3.7 %
(K = 128) and 10.6 % / 10.0 % (K = 256). test_premise prints them per case.

Every launch writes into a row / column slice of a larger buffer pre-filled with a sentinel: the rows before and after
and, with ldc > N, the pad columns of every row must be untouched. Operands passed with a stride lie in storage
filled with NaN, so a read outside the view poisons the sum.

What the cases reach (csrc/gemm.hip; grids on 256 CUs, P = min(4 tiles, CUs) for the persistent kernel):
  nt*   gemm_nt_kernel<EPI_NONE> (K / 64 odd: 64, 192, 320), one workgroup per tile, L2 groups of 8 row tiles, XCD remap
        of 1, 2, 3, 4, 5, 9, 13 and 18 workgroups (nwg % 8 != 0); mt = 9 and 13: a ragged last group.
  ph*   gemm_nt_8ph<EPI_NONE, 2> (K / 64 even: 128 = the pipeline's two-K-tile minimum, 256, 384, 2048). M = 1, 100:
        1 (2) tiles -> grid 4 (8), quarter slices, slices 1-3 (2-3) of each tile wholly past M; M = 257, 300: the
        second row tile's slices 1-3 wholly past M; 3 / 9 / 13 tiles -> grids 12 / 36 / 52 (quarter slices only);
        ph_n8192: N = 8192, mt = 17: L2 groups of 16 with a ragged second group, 544 tiles = 2 rounds of 256 + 32
        tiles as 128 quarter slices.
  *_lda / _blk / _ldw / _ldc / _all: lda = K + 8, a as the middle column block of [M, 3 K], ldw = K + 8, ldc = N + 8,
        all four; both kernels (fp8: pads of 16, test_fp8_exact).
  *_pow2: rows of a and w scaled by 2^-20 .. 2^20. *_nan: a[5, 7] = NaN: row 5 all NaN, every other row exact.
  test_tail_plans: gemm_nt_8ph<NONE / GELU / RES, 2> at K = 128, 256 and gemm_nt_8ph<NONE, 1> (fp8) at K = 256 in each
        of the seven plans (slices only, halves only, whole tiles in a partial round, exactly full, full rounds + a
        quarter / half / whole-tile tail; on 256 CUs nt = 16 with mt = 2, 5, 9, 16, 17, 21, 25), each with M ragged by
        37, 100 and 200 rows: at 100 the last quarter, at 200 the second half and quarters 1-3 of the last row tile lie
        wholly past M (round 6's fault geometry; asserted reached).
  test_residual_grid: gemm_nt_kernel<RES>, gemm_nt_8ph<RES, 2>, gemm_nt_8ph<RES, 1> at B in {1, 2, 4, 8, 16},
        hw = 16 / B (the frame lookup's running remainder wraps on every step), 16 / B + 1, 5 * 16 / B + 3, shard offsets
        inside and across frames, M = 304 (48 rows in the second tile: the first-valid-row fallback).
  test_hnorm / test_qkv: gemm_nt_8ph<HNORM / QKV, 2>, 6 tiles -> grid 24, quarter slices; float64 formula of
        test_dit_ops_gpu's test_head_rmsnorm_rope within 1 bf16 ulp, >= 99.9 % identical; q and v columns torch.equal.
  test_gelu_epilogue_nonfinite: gemm_nt_kernel<GELU> (K = 64) and gemm_nt_8ph<GELU, 2> (K = 128), 255 tiles.
-inf through the GELU epilogue gives NaN (-inf * Phi(-inf) = -inf * 0, as cp25_gelu and torch's GELU), +inf gives +inf.
"""
import dataclasses
import functools
import zlib

import pytest
import torch

from cosmos_predict2 import _native as N
from test_dit_ops_gpu import _check_gelu, bf16_ulp_close
from test_gemm_gpu import _tail_plan

BF16, F8 = torch.bfloat16, torch.float8_e4m3fn
SENT = -1.5e30
GR = 3  # sentinel rows before and after the output slice
NAN = float("nan")


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    amax: int = 8
    lay: str = ""       # a: lda = K + 8, b: a is the middle column block of [M, 3 K], w: ldw = K + 8, c: ldc = N + 8
    pow2: bool = False  # rows of a and of w scaled by 2^-20 .. 2^20
    nan: bool = False   # a[5, 7] = NaN on the device

    def __str__(self):
        return self.name


def _c(M, N, K, tag="", **kw):
    name = f"{'nt' if K // 64 % 2 else 'ph'}_m{M}_n{N}_k{K}{tag}"
    return Case(name, M, N, K, amax=64 if K == 64 else 8, **kw)


CASES = (
    [_c(M, Nn, K) for K in (192, 128) for M in (1, 100, 256, 257, 300) for Nn in (256, 512)]
    + [_c(M, Nn, K) for K in (64, 320, 256, 384) for M, Nn in ((1, 512), (300, 512), (257, 256))]
    + [_c(M, Nn, 2048) for M, Nn in ((1, 256), (257, 512), (300, 256))]
    # tile counts 3, 5, 9, 13, 18: odd grids, mt = 9 / 13 with a ragged last L2 group
    + [_c(M, Nn, K) for K in (192, 128) for M, Nn in ((600, 256), (1200, 256), (9 * 256 - 37, 256),
                                                       (13 * 256 - 37, 256), (9 * 256 - 200, 512))]
    + [Case("ph_n8192", 17 * 256 - 37, 8192, 128)]
    + [_c(300, 512, K, "_" + tag, lay=lay) for K in (192, 128)
       for tag, lay in (("lda", "a"), ("blk", "b"), ("ldw", "w"), ("ldc", "c"), ("all", "abwc"))]
    + [_c(300, 512, K, "_pow2", pow2=True) for K in (192, 128, 2048)]
    + [_c(300, 512, K, "_nan", nan=True) for K in (192, 128)]
)


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _ints(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _pow2(g, lo, hi, n):
    return torch.pow(2.0, torch.randint(lo, hi + 1, (n,), generator=g).double())


def _to_bf16(x):
    """float64 -> bf16 in one rounding (torch converts through fp32, which may land on a bf16 tie the fp64 value is not
    on: such values are first moved one fp32 step back towards the fp64 value)."""
    y = x.float()
    tie = (y.view(torch.int32) & 0xFFFF) == 0x8000
    up = torch.nextafter(y, torch.full_like(y, float("inf")))
    dn = torch.nextafter(y, torch.full_like(y, float("-inf")))
    y = torch.where(tie & (x > y.double()), up, torch.where(tie & (x < y.double()), dn, y))
    return y.to(BF16)


def _tie_shares(acc):
    """Shares of outputs that bf16 rounds at all and of exact ties (acc: float64, exact)."""
    r = acc.float().to(BF16).double()
    ulp = torch.pow(2.0, torch.floor(torch.log2(acc.abs().clamp_min(2.0 ** -120))) - 7)
    return (r != acc).double().mean().item(), ((acc - r).abs() * 2 == ulp).double().mean().item()


def _product(a, w):
    """Exact product, its fp32 twin and the abs-sum bound (a, w: CPU tensors holding exact small values)."""
    acc = a.double() @ w.double().t()
    return dict(acc=acc, acc32=a.float() @ w.float().t(), absum=(a.double().abs() @ w.double().abs().t()).max().item())


@functools.lru_cache(maxsize=None)
def _data(c: Case):
    g = _gen(c.name)
    a, w = _ints(g, -c.amax, c.amax, (c.M, c.K)), _ints(g, -4, 4, (c.N, c.K))
    d = _product(a, w)
    if c.pow2:
        ra, rw = _pow2(g, -20, 20, c.M), _pow2(g, -20, 20, c.N)
        a, w = (a.double() * ra[:, None]).float(), (w.double() * rw[:, None]).float()
        d.update(acc=d["acc"] * ra[:, None] * rw[None, :], acc32=a @ w.t())
    d.update(a=a.to(BF16), w=w.to(BF16), a32=a, w32=w, ref=d["acc"].float().to(BF16))
    return d


def _premise(d, K):
    assert d["absum"] < 2 ** 24
    assert torch.equal(d["acc32"].double(), d["acc"])
    assert torch.equal(d["ref"].double(), _to_bf16(d["acc"]).double())
    rounded, ties = _tie_shares(d["acc"])
    if K >= 2048:
        assert ties > 0
    return rounded, ties


@pytest.mark.parametrize("case", CASES, ids=str)
def test_premise(case):
    """No kernel: integer operands make fp32 accumulation exact; the K >= 2048 cases round ties."""
    d = _data(case)
    rounded, ties = _premise(d, case.K)
    for t, t32 in ((d["a"], d["a32"]), (d["w"], d["w32"])):  # the (scaled) operands are exact bf16 normals
        nz = t32.abs()[t32 != 0]
        assert torch.equal(t.float(), t32) and nz.min() >= 2.0 ** -126 and nz.max() < 2.0 ** 127
    tiles = (case.M + 255) // 256 * (case.N // 256)
    print(f"{case.name}: {tiles} tiles, |sum| <= {d['absum']:.0f}, {rounded:.1%} rounded, {ties:.1%} exact bf16 ties")


def test_premise_case_table():
    assert len({c.name for c in CASES}) == len(CASES)
    assert {c.K // 64 % 2 for c in CASES} == {0, 1} and any(c.K >= 2048 for c in CASES)
    assert {(c.M + 255) // 256 * (c.N // 256) for c in CASES} >= {1, 2, 3, 4, 5, 9, 13, 18}


# ------------------------------------------------------------------------------------------------ device plumbing
def _place(t, device, dtype, pad=0, block=False):
    """t [R, K] on the device as a view of NaN-filled storage: row stride K + pad, or 3 K + pad with t as the middle
    column block (its base stays 16-byte aligned: K elements of 1 or 2 bytes, K % 64 == 0)."""
    R, K = t.shape
    if not pad and not block:
        return t.to(dtype).to(device)
    buf = torch.full((R, (3 * K if block else K) + pad), NAN)
    c0 = K if block else 0
    buf[:, c0:c0 + K] = t.float()
    return buf.to(dtype).to(device)[:, c0:c0 + K]


def _out(M, Nn, device, pad=0):
    big = torch.full((M + 2 * GR, Nn + pad), SENT, dtype=BF16, device=device)
    return big, big[GR:GR + M, :Nn]


def _untouched(big, M, Nn):
    chk = big.clone()
    chk[GR:GR + M, :Nn] = SENT
    return torch.equal(chk, torch.full_like(chk, SENT))


def _mismatch(out, ref):
    bad = (out != ref).nonzero()
    first = ", ".join(f"{tuple(i.tolist())}: got {out[tuple(i)].item()} want {ref[tuple(i)].item()}" for i in bad[:6])
    rows, cols = bad[:, 0].unique(), bad[:, 1].unique()
    return (f"{bad.shape[0]} of {ref.numel()} elements differ in {rows.numel()} rows [{rows.min().item()}, "
            f"{rows.max().item()}] and {cols.numel()} columns [{cols.min().item()}, {cols.max().item()}]; {first}")


def _assert_exact(big, out, ref, what):
    assert _untouched(big, *out.shape), f"{what}: wrote outside the output slice"
    assert torch.equal(out, ref), f"{what}: {_mismatch(out, ref)}"


def _cus(device):
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    return cus & ~7 if cus >= 8 else cus


# ------------------------------------------------------------------------------------------------ 1, 3, 4: the product
@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=str)
def test_gemm_exact(device, case):
    d = _data(case)
    a = _place(d["a"], device, BF16, pad=8 if "a" in case.lay else 0, block="b" in case.lay)
    w = _place(d["w"], device, BF16, pad=8 if "w" in case.lay else 0)
    assert a.stride(0) == case.K + (8 if "a" in case.lay else 0) + (2 * case.K if "b" in case.lay else 0)
    if case.nan:
        a[5, 7] = NAN
    big, out = _out(case.M, case.N, device, pad=8 if "c" in case.lay else 0)
    N.gemm_epi(a, w, out=out)
    ref = d["ref"].to(device)
    if case.nan:
        assert torch.isnan(out[5]).all(), "row 5 holds a NaN operand"
        out[5] = ref[5]
    _assert_exact(big, out, ref, case.name)


# ------------------------------------------------------------------------------------------------ 2: tail plans
RAGGED = (37, 100, 200)
PLANS = {"quarter", "half", "whole", "full", "rounds+quarter", "rounds+half", "rounds+whole"}
TAIL_MT, TAIL_NT = 25, 16  # the operands cover every plan's shape up to 25 x 16 tiles


def _plan7(mt, nt, cus):
    """_tail_plan's four plans, split by whether full rounds of whole tiles precede the last round."""
    p = _tail_plan(mt * 256, nt * 256, cus)
    return ("rounds+" if p != "full" and mt * nt > cus else "") + p


def _tail_shapes(cus):
    """One (mt, nt) per plan: the first row-tile count that lands in it, at the column-tile count that gives the CU count
    a full round at mt = 16 (nt = 16 on 256 CUs: mt = 2, 5, 9, 16, 17, 21, 25)."""
    nt = min(TAIL_NT, max(1, cus // 16))
    pick = {}
    for mt in range(2, TAIL_MT + 1):
        pick.setdefault(_plan7(mt, nt, cus), (mt, nt))
    return pick


def _slice_past_m(M, Nn, cus, gm=8):
    """True when the launch's tail plan (gemm.hip plan / tile_at / tile_mn) runs a row slice that starts at or past M."""
    mt, nt = (M + 255) // 256, Nn // 256
    T = mt * nt
    P = min(4 * T, cus)
    F, R = divmod(T, P)
    sd = 4 if 4 * R <= P else (2 if 2 * R <= P else 1)
    for tile in range(F * P, T):
        first_m = tile // (gm * nt) * gm
        m_tile = first_m + (tile % (gm * nt)) % min(mt - first_m, gm)
        if any(m_tile * 256 + j * (256 // sd) >= M for j in range(1, sd)):
            return True
    return False


@functools.lru_cache(maxsize=None)
def _tail_data(K):
    """Operands of every tail-plan launch at one K: integer a, w; a's rows scaled by 1, 2^-3, 2^-6 in turn (the GELU
    inputs reach the table's range); per-row / per-column power-of-two fp8 scales; bf16 reals for x and the gate."""
    g = _gen(f"tail{K}")
    M, Nn = TAIL_MT * 256 - RAGGED[0], TAIL_NT * 256
    a, w = _ints(g, -8, 8, (M, K)), _ints(g, -4, 4, (Nn, K))
    rs = torch.tensor([1.0, 2.0 ** -3, 2.0 ** -6], dtype=torch.float64).repeat(M // 3 + 1)[:M]
    a_s = (a.double() * rs[:, None]).float()
    d = dict(acc_int=a.double() @ w.double().t(), rs=rs, a8=a.to(F8), w8=w.to(F8), a=a_s.to(BF16), w=w.to(BF16))
    d["ref"] = (d["acc_int"] * rs[:, None]).float().to(BF16)
    d["s8"], d["ws8"] = _pow2(g, -6, 6, M).float(), _pow2(g, -6, 6, Nn).float()
    d["ref8"] = (d["acc_int"] * d["s8"].double()[:, None] * d["ws8"].double()[None, :]).float().to(BF16)
    d["hw"] = 64
    d["gate"] = torch.randn(1, (M + 63) // 64, Nn, generator=g).to(BF16)
    d["x"] = torch.randn(M, 1, Nn, generator=g).to(BF16)
    return d


def _res_ref(y, x, gate, B, tok0, hw):
    """bf16(x + bf16(gate * bf16(acc))) in torch fp32 on the CPU (y: the exact bf16 product [M, N]; x [n_tok, 1 or B, N];
    gate [B, T, N]). A bf16 x bf16 product is exact in fp32, so this is the kernel's IEEE sequence."""
    M, Nn = y.shape
    n_tok = M // B
    fr = (tok0 + torch.arange(n_tok)) // hw
    gy = (gate.float()[:B, fr].transpose(0, 1) * y.float().view(n_tok, B, Nn)).to(BF16).float()
    return (x.float().expand(n_tok, B, Nn) + gy).to(BF16).reshape(M, Nn)


@pytest.mark.parametrize("K", [128, 256])
def test_premise_tail(K):
    d = _tail_data(K)
    p = _product(d["a"], d["w"])
    assert torch.equal(p["acc"], d["acc_int"] * d["rs"][:, None])
    rounded, ties = _premise(dict(p, ref=d["ref"]), K)
    assert torch.equal(d["a8"].float() @ d["w8"].float().t(), d["acc_int"].float())
    scaled = d["acc_int"] * d["s8"].double()[:, None] * d["ws8"].double()[None, :]
    assert torch.equal(d["ref8"].double(), _to_bf16(scaled).double())
    assert set(_tail_shapes(256)) == PLANS
    print(f"tail K={K}: |sum| <= {p['absum']:.0f}, {rounded:.1%} rounded, {ties:.1%} exact bf16 ties")


@pytest.mark.gpu
@pytest.mark.parametrize("kind,K", [("bf16", 128), ("bf16", 256), ("fp8", 256)])
def test_tail_plans(device, kind, K):
    """Every tail plan x every ragged M x the plain, GELU and gated-residual epilogues (bf16) or the scaled product
    (fp8): rows and columns are prefixes of one problem, whose float64 reference is computed once. GELU: cp25_gelu (its
    own kernel, pinned against float64 by test_dit_ops_gpu) applied to the exact reference product, bit for bit."""
    cus = _cus(device)
    shapes = _tail_shapes(cus)
    assert set(shapes) == PLANS, shapes
    d = _tail_data(K)
    hw = d["hw"]
    past = set()
    if kind == "fp8":
        a, w = d["a8"].to(device), d["w8"].to(device)
        s, ws, ref = d["s8"].to(device), d["ws8"].to(device), d["ref8"].to(device)
    else:
        a, w, ref = d["a"].to(device), d["w"].to(device), d["ref"].to(device)
        ref_gelu = N.gelu_(ref.clone())
        ref_res = _res_ref(d["ref"], d["x"], d["gate"], 1, 0, hw).to(device)
        x, gate = d["x"].to(device), d["gate"].to(device)
    for plan, (mt, nt) in sorted(shapes.items(), key=lambda kv: kv[1]):
        Nn = nt * 256
        for rag in RAGGED:
            M = mt * 256 - rag
            assert _plan7(mt, nt, cus) == plan
            if _slice_past_m(M, Nn, cus):
                past.add(plan.split("+")[-1])
            what = f"{kind} K={K} plan {plan} M={M} N={Nn}"
            if kind == "fp8":
                big, out = _out(M, Nn, device)
                N.gemm_fp8(a[:M], s[:M].contiguous(), w[:Nn], ws[:Nn].contiguous(), out=out)
                _assert_exact(big, out, ref[:M, :Nn], what)
                continue
            for epi, r in ((N.EPI_NONE, ref), (N.EPI_GELU, ref_gelu)):
                big, out = _out(M, Nn, device)
                N.gemm_epi(a[:M], w[:Nn], epilogue=epi, out=out)
                _assert_exact(big, out, r[:M, :Nn], f"{what} epilogue {epi}")
            big, out = _out(M, Nn, device)
            N.gemm_res(a[:M], w[:Nn], x[:M, :, :Nn], x.stride(0), x.stride(1), gate[..., :Nn], B=1, tok0=0, hw=hw,
                       out=out)
            _assert_exact(big, out, ref_res[:M, :Nn], f"{what} residual")
    assert past == {"quarter", "half"}, f"no slice wholly past M in {({'quarter', 'half'} - past)}"


# ------------------------------------------------------------------------------------------------ 4, 5: GELU
@functools.lru_cache(maxsize=None)
def _gelu_data(K):
    """Integer products with a's rows scaled by 1, 2^-3, 2^-6 in turn: GELU inputs inside and outside the table."""
    g = _gen(f"gelu{K}")
    M, Nn = 300, 512
    a, w = _ints(g, -8, 8, (M, K)), _ints(g, -4, 4, (Nn, K))
    rs = torch.tensor([1.0, 2.0 ** -3, 2.0 ** -6]).repeat(M // 3)
    d = _product(a * rs[:, None], w)
    d.update(a=(a * rs[:, None]).to(BF16), w=w.to(BF16), ref=d["acc"].float().to(BF16))
    return d


@pytest.mark.parametrize("K", [192, 128, 2048])
def test_premise_gelu(K):
    _premise(_gelu_data(K), K)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [192, 128, 2048])
def test_gelu_epilogue_vs_float64(device, K):
    """EPI_GELU against the correctly rounded float64 GELU of the exact bf16 product (test_dit_ops_gpu's criterion)."""
    d = _gelu_data(K)
    big, out = _out(300, 512, device)
    N.gemm_epi(d["a"].to(device), d["w"].to(device), epilogue=N.EPI_GELU, out=out)
    assert _untouched(big, 300, 512)
    x = d["ref"].to(device)
    assert (x.float().abs() < 8).float().mean().item() > 0.1 and (x.float().abs() >= 8).float().mean().item() > 0.1
    _check_gelu(x, out)


@pytest.mark.gpu
@pytest.mark.parametrize("K", [64, 128])
def test_gelu_epilogue_nonfinite(device, K):
    """Every bf16 value, +-inf and NaN included, through the product and the GELU epilogue (the construction of
    test_gemm_gpu's every-bf16-value test): bit-identical to cp25_gelu; NaN gives NaN, +inf gives +inf, -inf gives NaN
    (-inf * Phi(-inf) = -inf * 0)."""
    bits = torch.arange(0, 1 << 16, dtype=torch.int32).to(torch.int16).view(BF16)
    fin = bits[torch.isfinite(bits.float())]
    x = torch.cat([fin, torch.tensor([float("inf"), float("-inf"), NAN], dtype=BF16)]).to(device)
    n = x.numel()
    a = torch.zeros(n, K, dtype=BF16, device=device)
    a[:, 0] = x
    w = torch.zeros(256, K, dtype=BF16, device=device)
    w[:, 0] = 1.0
    plain = N.gemm_epi(a, w)
    assert torch.equal(plain[:n - 1], x[:n - 1, None].expand(-1, 256)) and torch.isnan(plain[n - 1]).all()
    got = N.gemm_epi(a, w, epilogue=N.EPI_GELU)
    ref = N.gelu_(plain.clone())
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))
    assert torch.isnan(got[n - 1]).all() and (got[n - 3] == float("inf")).all()
    assert torch.isnan(got[n - 2]).all()  # -inf


# ------------------------------------------------------------------------------------------------ 5: gated residual
RES_M, RES_N = 304, 256
RES_KERNELS = {"nt": 192, "ph": 128, "fp8": 256}


@functools.lru_cache(maxsize=None)
def _res_data(kernel):
    g = _gen("res" + kernel)
    K = RES_KERNELS[kernel]
    a, w = _ints(g, -8, 8, (RES_M, K)), _ints(g, -4, 4, (RES_N, K))
    d = _product(a, w)
    d.update(a=a, w=w, ref=d["acc"].float().to(BF16), s=torch.ones(RES_M))
    if kernel == "fp8":
        d["s"], d["ws"] = _pow2(g, -6, 6, RES_M).float(), _pow2(g, -6, 6, RES_N).float()
        d["ref"] = (d["acc"] * d["s"].double()[:, None] * d["ws"].double()[None, :]).float().to(BF16)
    return d


@pytest.mark.parametrize("kernel", list(RES_KERNELS))
def test_premise_residual(kernel):
    d = _res_data(kernel)
    _premise(dict(d, ref=d["acc"].float().to(BF16)), RES_KERNELS[kernel])
    if kernel == "fp8":
        scaled = d["acc"] * d["s"].double()[:, None] * d["ws"].double()[None, :]
        assert torch.equal(d["ref"].double(), _to_bf16(scaled).double())


def _res_call(kernel, a, w, s, ws, x, x_st, x_sb, gate, B, tok0, hw, out):
    if kernel == "fp8":
        return N.gemm_fp8(a, s, w, ws, res=(x, x_st, x_sb, gate, B, tok0, hw), out=out)
    return N.gemm_res(a, w, x, x_st, x_sb, gate, B=B, tok0=tok0, hw=hw, out=out)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2, 4, 8, 16])
@pytest.mark.parametrize("kernel", list(RES_KERNELS))
def test_residual_grid(device, kernel, B):
    """x + gate * y against the documented IEEE sequence on the float64 product: hw at the host's limit 16 / B and just
    above, shard offsets, x broadcast (x_sb = 0) and strided, the gate as the last third of a [B, T, 3 N] view."""
    d = _res_data(kernel)
    dt = F8 if kernel == "fp8" else BF16
    a, w = d["a"].to(dt).to(device), d["w"].to(dt).to(device)
    s, ws = (d["s"].to(device), d["ws"].to(device)) if kernel == "fp8" else (None, None)
    n_tok = RES_M // B
    g = _gen(f"resgrid{kernel}{B}")
    for hw in (16 // B, 16 // B + 1, 5 * 16 // B + 3):
        for tok0 in (0, hw - 1, 3 * hw + 1):
            T = (tok0 + n_tok - 1) // hw + 1
            mods = torch.randn(B, T, 3 * RES_N, generator=g).to(BF16)
            for bcast in (True, False):
                xw = torch.randn(n_tok, 1 if bcast else B, 2 * RES_N, generator=g).to(BF16)
                x_cpu = xw[..., RES_N:]  # a strided column view of a wider buffer
                ref = _res_ref(d["ref"], x_cpu, mods[..., 2 * RES_N:], B, tok0, hw).to(device)
                x, gate = xw.to(device)[..., RES_N:], mods.to(device)[..., 2 * RES_N:]
                big, out = _out(RES_M, RES_N, device, pad=8)
                _res_call(kernel, a, w, s, ws, x, x.stride(0), 0 if bcast else x.stride(1), gate, B, tok0, hw, out)
                _assert_exact(big, out, ref, f"{kernel} B={B} hw={hw} tok0={tok0} x_sb={'0' if bcast else 'B'}")
    # refusals: frames past the gate, hw below 16 / B, B not dividing 16
    big, out = _out(RES_M, RES_N, device)
    x = torch.zeros(RES_M, 1, RES_N, dtype=BF16, device=device)
    gate = torch.zeros(16, 4, RES_N, dtype=BF16, device=device)
    with pytest.raises(ValueError):
        _res_call(kernel, a, w, s, ws, x, RES_N, 0, gate, B, 4 * (16 // B), 16 // B, out)
    if B > 1 and 16 // B > 1:
        with pytest.raises(ValueError):
            _res_call(kernel, a, w, s, ws, x, RES_N, 0, gate[:, :1].expand(16, 400, RES_N), B, 0, 16 // B - 1, out)
    if B == 1:
        with pytest.raises(ValueError):
            _res_call(kernel, a[:303], w, None if s is None else s[:303].contiguous(), ws, x, RES_N, 0,
                      gate[:, :1].expand(16, 400, RES_N), 3, 0, 64, out[:303])
    torch.cuda.synchronize()
    assert _untouched(big, 0, 0), "a refused call wrote"


# ------------------------------------------------------------------------------------------------ 5: head norm, QKV
HN_M, HN_N = 300, 768


def _hnorm_rope(p, kw, dtype, *, out_scale=1.0, cos=None, sin=None, B=1, eps=1e-6):
    """test_dit_ops_gpu::test_head_rmsnorm_rope's formula on the bf16 product p [M, H 128]: RMSNorm per head, weight,
    (bf16), rotate-half RoPE by token row // B, out_scale, bf16."""
    M = p.shape[0]
    h = p.to(dtype).view(M, -1, 128)
    kn = (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)) * kw.to(dtype)
    kn = (_to_bf16(kn) if dtype == torch.float64 else kn.to(BF16)).to(dtype)
    if cos is not None:
        tok = torch.arange(M) // B
        c, s = (torch.cat([t, t], -1)[tok][:, None, :].to(dtype) for t in (cos, sin))
        kn = kn * c + torch.cat([-kn[..., 64:], kn[..., :64]], -1) * s
    kn = kn * out_scale
    return (_to_bf16(kn) if dtype == torch.float64 else kn.to(BF16)).view(M, -1)


@functools.lru_cache(maxsize=None)
def _hn_data(K):
    g = _gen(f"hn{K}")
    a, w = _ints(g, -8, 8, (HN_M, K)), _ints(g, -4, 4, (HN_N, K))
    a[17] = 0  # an all-zero row: rstd = rsqrt(eps)
    d = _product(a, w)
    # the RoPE tables hold multiples of 1 / 16, different for every token and column: x cos + rot(x) sin is then (nearly
    # always) exact in fp32, so a cancelling pair cannot put the fp32 kernel many ulps of a tiny result away from float64
    # (with cos / sin of random angles a few elements per case do, in torch's own fp32 evaluation too: test_premise)
    d.update(a=a.to(BF16), w=w.to(BF16), ref=d["acc"].float().to(BF16), cos=_ints(g, -16, 16, (HN_M, 64)) / 16,
             sin=_ints(g, -16, 16, (HN_M, 64)) / 16, kw=(0.5 + 2.5 * torch.rand(128, generator=g)).to(BF16))
    return d


QKV_CASES = [(128, 1, True, 256), (128, 2, True, 256), (128, 2, False, 256), (128, 1, True, 0), (2048, 2, True, 256),
             (2048, 1, False, 0)]  # K, B, RoPE, k_col0
HNORM_CASES = [(128, 1.0), (128, 0.25), (2048, 1.0), (2048, 0.25)]  # K, out_scale


def _qkv_ref(d, B, rope, k0, dtype):
    ref = d["ref"].clone()
    n_tok = (HN_M + B - 1) // B
    cs = dict(cos=d["cos"][:n_tok], sin=d["sin"][:n_tok]) if rope else {}
    ref[:, k0:k0 + 256] = _hnorm_rope(d["ref"][:, k0:k0 + 256], d["kw"], dtype, B=B, **cs)
    return ref


@pytest.mark.parametrize("K", [128, 2048])
def test_premise_hnorm_qkv(K):
    """The float64 formula stays inside the criterion's cap on its own: its fp32 evaluation meets bf16_ulp_close."""
    d = _hn_data(K)
    _premise(d, K)
    for scale in (1.0, 0.25):
        ok, eq = bf16_ulp_close(_hnorm_rope(d["ref"], d["kw"], torch.float32, out_scale=scale),
                                _hnorm_rope(d["ref"], d["kw"], torch.float64, out_scale=scale))
        assert ok, eq
    for _, B, rope, k0 in QKV_CASES:
        ok, eq = bf16_ulp_close(_qkv_ref(d, B, rope, k0, torch.float32), _qkv_ref(d, B, rope, k0, torch.float64))
        assert ok, eq


@pytest.mark.gpu
@pytest.mark.parametrize("K,scale", HNORM_CASES)
def test_hnorm_vs_float64(device, K, scale):
    d = _hn_data(K)
    big, out = _out(HN_M, HN_N, device, pad=8)
    assert N.gemm_hnorm(d["a"].to(device), d["w"].to(device), d["kw"].to(device), out_scale=scale, out=out) is not None
    assert _untouched(big, HN_M, HN_N)
    ref = _hnorm_rope(d["ref"], d["kw"], torch.float64, out_scale=scale)
    assert (out[17] == 0).all()
    ok, eq = bf16_ulp_close(out.cpu(), ref)
    assert ok, eq


@pytest.mark.gpu
@pytest.mark.parametrize("K,B,rope,k0", QKV_CASES)
def test_qkv_vs_float64(device, K, B, rope, k0):
    d = _hn_data(K)
    n_tok = (HN_M + B - 1) // B
    cos, sin = (d["cos"][:n_tok].to(device), d["sin"][:n_tok].to(device)) if rope else (None, None)
    big, out = _out(HN_M, HN_N, device, pad=8)
    got = N.gemm_qkv(d["a"].to(device), d["w"].to(device), d["kw"].to(device), k_col0=k0, k_cols=256, B=B, cos=cos,
                     sin=sin, out=out)
    assert got is not None and _untouched(big, HN_M, HN_N)
    ref = _qkv_ref(d, B, rope, k0, torch.float64)
    out = out.cpu()
    other = [c for c in range(0, HN_N, 256) if c != k0]
    for c in other:  # q and v: the plain exact product
        got_c, ref_c = out[:, c:c + 256], d["ref"][:, c:c + 256]
        assert torch.equal(got_c, ref_c), _mismatch(got_c, ref_c)
    ok, eq = bf16_ulp_close(out[:, k0:k0 + 256], ref[:, k0:k0 + 256])
    assert ok, eq


# ------------------------------------------------------------------------------------------------ 6: fp8
FP8_M, FP8_N = 300, 512


@functools.lru_cache(maxsize=None)
def _fp8_data(K):
    g = _gen(f"fp8{K}")
    q, w = _ints(g, -8, 8, (FP8_M, K)), _ints(g, -8, 8, (FP8_N, K))
    d = _product(q, w)
    s2, ws2 = _pow2(g, -6, 6, FP8_M).float(), _pow2(g, -6, 6, FP8_N).float()
    sr = torch.rand(FP8_M, generator=g) * 0.09 + 0.001
    wsr = torch.rand(FP8_N, generator=g) * 0.03 + 0.0003
    d.update(q=q, w=w, s2=s2, ws2=ws2, sr=sr, wsr=wsr,
             ref2=(d["acc"] * s2.double()[:, None] * ws2.double()[None, :]).float().to(BF16),
             # the epilogue's documented order (gemm.hip, kES == 1): (acc * a_scale[row]) * w_scale[col], fp32
             refr=((d["acc"].float() * sr[:, None]) * wsr[None, :]).to(BF16))
    return d


@pytest.mark.parametrize("K", [256, 512, 768, 2048])
def test_premise_fp8(K):
    d = _fp8_data(K)
    _premise(dict(d, ref=d["acc"].float().to(BF16)), K)
    assert torch.equal(d["q"].to(F8).float(), d["q"]) and torch.equal(d["w"].to(F8).float(), d["w"])
    scaled = d["acc"] * d["s2"].double()[:, None] * d["ws2"].double()[None, :]
    assert torch.equal(d["ref2"].double(), _to_bf16(scaled).double())


FP8_CASES = ([(K, "") for K in (256, 512, 768, 2048)]
             + [(K, lay) for K in (256, 768) for lay in ("a", "b", "w", "c", "abwc")])


@pytest.mark.gpu
@pytest.mark.parametrize("K,lay", FP8_CASES, ids=lambda v: str(v) or "dense")
def test_fp8_exact(device, K, lay):
    """(a) power-of-two row / column scales: exact, torch.equal with float64; (b) arbitrary fp32 scales: torch.equal
    with (acc * a_scale[row]) * w_scale[col] in fp32. M = 300: the second tile's row scales past M read zero. Strides
    (multiples of 16 bytes, at K = 256 and 768) as in the bf16 cases; the residual form on the dense layout."""
    d = _fp8_data(K)
    q = _place(d["q"], device, F8, pad=16 if "a" in lay else 0, block="b" in lay)
    w = _place(d["w"], device, F8, pad=16 if "w" in lay else 0)
    for s, ws, ref, what in ((d["s2"], d["ws2"], d["ref2"], "pow2"), (d["sr"], d["wsr"], d["refr"], "fp32")):
        big, out = _out(FP8_M, FP8_N, device, pad=8 if "c" in lay else 0)
        N.gemm_fp8(q, s.to(device), w, ws.to(device), out=out)
        _assert_exact(big, out, ref.to(device), f"fp8 K={K} {lay or 'dense'} {what} scales")
        if not lay:
            g = _gen(f"fp8res{K}")
            hw = 48
            gate = torch.randn(1, (FP8_M + hw - 1) // hw, FP8_N, generator=g).to(BF16)
            x = torch.randn(FP8_M, 1, FP8_N, generator=g).to(BF16)
            big, out = _out(FP8_M, FP8_N, device, pad=8)
            N.gemm_fp8(q, s.to(device), w, ws.to(device), out=out,
                       res=(x.to(device), FP8_N, 0, gate.to(device), 1, 0, hw))
            _assert_exact(big, out, _res_ref(ref, x, gate, 1, 0, hw).to(device), f"fp8 K={K} {what} scales, residual")


# ------------------------------------------------------------------------------------------------ 8: host refusals
@pytest.mark.gpu
def test_host_refusals(device):
    """Arguments the wrappers refuse before any launch: each is a ValueError and the output keeps its sentinel."""
    M, Nn, K = 300, 256, 128
    z = lambda *shape, dt=BF16: torch.zeros(*shape, dtype=dt, device=device)  # noqa: E731
    a, w, kw = z(M, K), z(Nn, K), z(128)
    big, out = _out(M, Nn, device)
    N.gemm_epi(a, w, out=out)  # the base arguments are accepted
    assert (out == 0).all()
    out.fill_(SENT)
    bad = [
        lambda: N.gemm_epi(z(M, K + 4)[:, :K], w, out=out),                        # lda % 8 != 0
        lambda: N.gemm_epi(z(M * K).as_strided((M, K), (K - 8, 1)), w, out=out),   # lda < K
        lambda: N.gemm_epi(z(M * K + 8)[1:1 + M * K].view(M, K), w, out=out),      # base one element off 16 bytes
        lambda: N.gemm_epi(a, z(264, K), out=_out(M, 264, device)[1]),             # N % 256 != 0
        lambda: N.gemm_epi(z(M, 96), z(Nn, 96), out=out),                          # K % 64 != 0
        lambda: N.gemm_fp8(z(M, 128, dt=F8), z(M, dt=torch.float32), z(Nn, 128, dt=F8), z(Nn, dt=torch.float32),
                           out=out),                                               # fp8 K % 256 != 0
        lambda: N.gemm_fp8(z(M, 264, dt=F8)[:, :256], z(M, dt=torch.float32), z(Nn, 256, dt=F8),
                           z(Nn, dt=torch.float32), out=out),                      # fp8 lda % 16 != 0
        lambda: N.gemm_epi(a, w, epilogue=N.EPI_RES, out=out),
        lambda: N.gemm_epi(a, w, epilogue=N.EPI_HNORM, out=out),
        lambda: N.gemm_epi(a, w, epilogue=N.EPI_QKV, out=out),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            raise AssertionError(f"refusal {i} was accepted")
    big3, out3 = _out(M, 768, device)
    w3 = z(768, K)
    for k0, kc in ((128, 256), (256, 128), (512, 512), (768, 256)):  # k_col0 % 256, k_cols % 256, k_col0 + k_cols > N
        with pytest.raises(ValueError):
            N.gemm_qkv(a, w3, kw, k_col0=k0, k_cols=kc, B=1, out=out3)
    torch.cuda.synchronize()
    assert _untouched(big, 0, 0) and _untouched(big3, 0, 0), "a refused call wrote"
