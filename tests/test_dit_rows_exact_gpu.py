"""cp25_ln_mod, cp25_ln_mod_fp8, cp25_final_ln_mod, cp25_layer_norm and cp25_head_rmsnorm_rope(_nmax), row by row and bit
for bit, in every template instance and at the row tails.

Integer rows. A row of width D is x_i = u (m + k_i): u a power of two in [2^-4, 2^2], m an integer in [-3, 3], k_i
integers in [-16, 16] drawn in +- pairs and shuffled. Then sum x = u m D, every deviation is u k_i and sum d^2 is u^2
times an integer below 2^24: for D a power of two the fp32 mean and variance are exact in any summation order, so the
reference does not depend on how the kernel reduces. D = 5120 uses m = 0 (fl(1 / 5120) is inexact; a zero mean keeps
the deviations integers) and var = fl(q * fl(1 / 5120)) is one fixed rounding. With a residual, x + g y with g in
{0, +-1, +-2} per (batch, frame) and y of the same family and u is again such a row (|k| <= 48); x_out must equal it.
Head RMSNorm: width 128, m = 0, |k| <= 8.

The one operation left that IEEE does not fix is rsqrtf (v_rsq_f32, 1 ulp). a = fl(fl(q * fl(1 / D)) + eps) is computed
here in fp32; r0 is the fp32 nearest to the float64 1 / sqrt(a); the candidates are r0 - 2 ulp .. r0 + 2 ulp (1 ulp
of the instruction from the true value, one for r0's own rounding). For every row (every (row, head) item) the whole
output row must equal, bit for bit, the CPU fp32 evaluation of the kernel's op sequence with one of the five:
  ln_mod        bf16(rbf(rbf(d r) * rbf(1 + scale)) + shift); fp8: max |h| / 448 and e4m3 (the table of
                test_fp8_cast_exact_gpu) of fl(h * fl(448 / max |h|)) over that h
  layer_norm    bf16(fl(fl(fl(d r) * w) + b))
  final_ln_mod  fl(fl(fl(d r) * fl(1 + scale)) + shift), compared as fp32 bits
  head norm     v = rbf(fl(x r) * w); RoPE fmaf(v, cos, fl(fl(sgn * partner) * sin)); bf16(fl(. * out_scale))
test_premise_* (no GPU) assert per case: the sums exact (fp32 == float64), the residual sum in the family, and
  ln_mod        all five candidates and the float64 chain with the true 1 / sqrt give the same bits, so the GPU test is a
                plain torch.equal with the float64 chain;
  the others    at least half of the candidate-dependent rows are told apart by more than one candidate pair (the search
                can fail). Measured at M = 131: layer_norm 3 % (D = 512) to 26 % (D = 5120) of rows depend on the
                candidate; head norm about 0.5 % of items; final_ln_mod every row (all five differ).
final_ln_mod must also stay within twice the error torch's CPU fp32 evaluation (with r0) shows against float64 on the same
rows (max |out - ref64| / max |ref64| per row, the largest row of the case on both sides).

Modulations of the bf16 kernels are multiples of 2^-6 in [-2, 2] (1 + scale and prod + shift round once); final_ln_mod's
are any fp32. RoPE tables are multiples of 1 / 16 in [-1, 1], so the fmaf has one rounding of an exactly known sum.

Cases. ln_mod / ln_mod_fp8 / final_ln_mod: D in {512, 1024, 2048, 4096, 5120} x (n_tok, B) in {(1, 1), (7, 1), (5, 3),
(9, 2)} (1, 7, 15, 18 rows: rows % 4 = 1, 3, 3, 2, the last workgroup's row >= n_rows exit) x residual on / off; hw = 4,
tok0 cycling through 0, 3, 6 (tokens of two frames in one workgroup); shift, scale and gate are views of one [B, T, 3 D]
tensor (final_ln_mod: fp32 [B, T, 2 D] and a bf16 gate of other strides). ln_mod also: x [n, 1, D] broadcast over B = 2
(x_sb = 0) with a residual; constant rows (var = 0: h = shift; with shift = 0 the fp8 scale and codes are 0; with one
2^-133 in a zero shift the scale is sub-normal and the codes 0: max |h| has a floor of 2^-100 in the divisor).
layer_norm: the same D x M in {1, 6, 131}, x.stride(0) = D + 8, out.stride(0) = D + 64.
head norm: H in {1, 3, 16}, B in {1, 2}, n_rows H % 16 in {0, 1, 13}, head_off 0 and D, RoPE on / off, out_scale 1, 0.25
and fl(128^-0.5 log2 e), out2 absent or with stride H 128 + 64; 1 to 130 workgroups; in one case the longest row lies in
the last, partial, group of 16. The nmax variant must write the same bytes and leave in slot j the largest row norm of
workgroups b = j (mod 64).
Gaussian legs (D = 1024, 4096 and the tail shapes): float64 chain with the rounding points, bf16_ulp_close.
Every output is a slice of a sentinel-filled buffer whose guards must be untouched.
"""
import dataclasses
import functools
import math
import zlib

import pytest
import torch

from cosmos_predict2 import _native as N
from test_dit_ops_gpu import bf16_ulp_close
from test_fp8_cast_exact_gpu import FILL8, SENTINEL, e4m3_round, guarded, guards_ok
from test_gemm_exact_gpu import _to_bf16

BF16 = torch.bfloat16
F32 = torch.float32
WIDTHS = (512, 1024, 2048, 4096, 5120)
ROWSETS = ((1, 1), (7, 1), (5, 3), (9, 2))
HW, T_FRAMES = 4, 4
EPS = torch.tensor(1e-6, dtype=F32)  # what the float argument holds
AMAX_FLOOR = 2.0 ** -100


def _rbf(x):
    return x.to(BF16).float()


def _inv(D):
    return torch.tensor(1.0, dtype=F32) / torch.tensor(float(D), dtype=F32)  # the kernel's constant 1.f / D


def _family(g, R, D, kmax, zero_mean):
    """x = u (m + k) as float64 [R, D] and its parts."""
    half = torch.randint(0, kmax + 1, (R, D // 2), generator=g)
    k = torch.cat([half, -half], 1).gather(1, torch.rand(R, D, generator=g).argsort(1)).double()
    m = torch.zeros(R, 1, dtype=torch.float64) if zero_mean else torch.randint(-3, 4, (R, 1), generator=g).double()
    u = torch.pow(2.0, torch.randint(-4, 3, (R, 1), generator=g).double())
    return u * (m + k), u, m


def _mod64(g, shape):
    return torch.randint(-128, 129, shape, generator=g).double() / 64  # multiples of 2^-6 in [-2, 2]


def _stats(xs):
    """The kernel's fp32 statistics of rows xs (float64, exact bf16 values) and their float64 twins."""
    D = xs.shape[-1]
    x32 = xs.float()
    s32, s64 = x32.sum(-1), xs.sum(-1)
    mean32 = s32 * _inv(D)
    d32 = x32 - mean32[..., None]
    q32 = (d32 * d32).sum(-1)
    a32 = q32 * _inv(D) + EPS
    d64 = xs - (s64 / D)[..., None]
    q64 = (d64 * d64).sum(-1)
    r64 = 1 / torch.sqrt(q64 / D + EPS.double())
    return dict(s32=s32, s64=s64, d32=d32, d64=d64, q32=q32, q64=q64, a32=a32, r64=r64)


def _candidates(a32):
    """[5, ...] fp32: r0 - 2 ulp .. r0 + 2 ulp, r0 the fp32 nearest to the float64 1 / sqrt(a)."""
    r0 = (1 / torch.sqrt(a32.double())).float()
    up, dn = torch.full_like(r0, math.inf), torch.full_like(r0, -math.inf)
    m1, p1 = torch.nextafter(r0, dn), torch.nextafter(r0, up)
    return torch.stack([torch.nextafter(m1, dn), m1, r0, p1, torch.nextafter(p1, up)])


def _bits(t):
    return t.view({BF16: torch.int16, F32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


def _match(got, outs):
    """got [R, ...] against outs [5, R, ...]: per row, whether some candidate's whole row has got's bits."""
    return (_bits(got)[None] == _bits(outs)).flatten(2).all(2).any(0)


def _told_apart(outs):
    """Per row: the number of candidate pairs whose output rows differ (0: the row does not depend on the candidate)."""
    b = _bits(outs).flatten(2)
    n = torch.zeros(b.shape[1], dtype=torch.long)
    for i in range(5):
        for j in range(i + 1, 5):
            n += (b[i] != b[j]).any(1)
    return n


def _check_search_can_fail(outs, name):
    n = _told_apart(outs)
    dep = n > 0
    if dep.any():
        assert (n[dep] > 1).float().mean() >= 0.5, name
    return dep.float().mean().item()


def _exact_sums(st, scale_u):
    """The family's premise: fp32 sums equal the float64 ones, sum d^2 / u^2 an integer below 2^24."""
    assert torch.equal(st["s32"].double(), st["s64"]) and torch.equal(st["q32"].double(), st["q64"])
    assert torch.equal(st["d32"].double(), st["d64"])
    qi = st["q64"] / (scale_u * scale_u).squeeze(-1)
    assert torch.equal(qi, qi.round()) and qi.max() < 2 ** 24


# ================================================================================================ ln_mod / final_ln_mod
@dataclasses.dataclass(frozen=True)
class LnCase:
    D: int
    n_tok: int
    B: int
    tok0: int
    res: bool
    bcast: bool = False  # x is [n_tok, 1, D], x_sb = 0
    const: bool = False  # rows 1, 5, 9 constant; frame 0's shift is zero, frame 2's zero but for one TINY
    gauss: bool = False

    def __str__(self):
        tag = "_res" * self.res + "_bcast" * self.bcast + "_const" * self.const + "_gauss" * self.gauss
        return f"d{self.D}_n{self.n_tok}_b{self.B}_t{self.tok0}{tag}"

    @property
    def rows(self):
        return self.n_tok * self.B


LN_CASES = [LnCase(D, n, B, (0, 3, 6)[(i + j + r) % 3], bool(r))
            for i, D in enumerate(WIDTHS) for j, (n, B) in enumerate(ROWSETS) for r in (0, 1)]
LN_EXTRA = [LnCase(1024, 7, 2, 3, True, bcast=True), LnCase(512, 11, 1, 0, False, const=True)]
TINY = 2.0 ** -133  # the smallest bf16 subnormal
LN_GAUSS = [LnCase(D, n, B, 3, True, gauss=True) for D in (1024, 4096) for n, B in ((5, 3), (9, 2))]


def _ln_draw(c: LnCase, final, salt):
    g = torch.Generator().manual_seed(zlib.crc32(f"{c}{final}{salt}".encode()))
    D, R, Bx = c.D, c.rows, 1 if c.bcast else c.B
    row = torch.arange(R)
    tok, b = row // c.B, row % c.B
    fr = (c.tok0 + tok) // HW
    assert fr.max() < T_FRAMES
    d = dict(tok=tok, b=b, fr=fr)
    if c.gauss:
        x = torch.randn(c.n_tok, Bx, D, generator=g).to(BF16).double()
        y = torch.randn(c.n_tok, c.B, D, generator=g).to(BF16).double()
        gate = (torch.randn(c.B, T_FRAMES, D, generator=g) * 0.5).to(BF16).double()
        u = None
    else:
        x, u, m = _family(g, c.n_tok * Bx, D, 16, zero_mean=D == 5120)
        if c.const:
            x[1], x[5], x[9] = u[1] * m[1], u[5] * m[5], u[9] * m[9]
        x = x.view(c.n_tok, Bx, D)
        u = u.view(c.n_tok, Bx, 1).expand(c.n_tok, c.B, 1).reshape(R, 1)
        yk, yu, _ = _family(g, R, D, 16, zero_mean=D == 5120)  # drawn with its own u: rescaled to the row's
        y = (yk / yu * u).view(c.n_tok, c.B, D)
        gate = torch.randint(-2, 3, (c.B, T_FRAMES, 1), generator=g).double().expand(c.B, T_FRAMES, D).contiguous()
    if final:
        sh, sc = torch.randn(2, c.B, T_FRAMES, D, generator=g).double()
    elif c.gauss:
        sh, sc = (torch.randn(2, c.B, T_FRAMES, D, generator=g) * 0.5).to(BF16).double()
    else:
        sh, sc = _mod64(g, (2, c.B, T_FRAMES, D))
        if c.const:
            sh[:, 0], sh[:, 2] = 0, 0
            sh[0, 2, 7] = TINY
    xr = x.expand(c.n_tok, c.B, D).reshape(R, D)
    yr = y.reshape(R, D)
    if c.res:
        gy = gate[b, fr] * yr
        xs = xr + _to_bf16(gy).double()  # exact in the family; Gaussian: the kernel's fp32 sum, rounded to bf16
        xs = _rbf(xr.float() + _to_bf16(gy).float()).double() if c.gauss else xs
    else:
        gy, xs = None, xr
    d.update(x=x, y=y, gate=gate, sh=sh, sc=sc, u=u, xs=xs, gy=gy, shr=sh[b, fr], scr=sc[b, fr])
    return d


@functools.lru_cache(maxsize=None)
def _ln_data(c: LnCase, final=False):
    """Inputs (float64 holding exact bf16 / fp32 values) of one case and the row-major views the reference needs.
    ln_mod's integer rows are redrawn (another seed, on the CPU reference alone) until no element of h sits close
    enough to a bf16 rounding boundary for the five rsqrt candidates to disagree: about one draw in twelve does."""
    for salt in range(8):
        d = _ln_draw(c, final, salt)
        if final or c.gauss:
            return d
        st = _stats(d["xs"])
        h64 = _ln_mod_f64(st, d["scr"], d["shr"])
        if all(torch.equal(_bits(_ln_mod_chain(st["d32"], r, d["scr"], d["shr"])), _bits(h64)) for r in _candidates(st["a32"])):
            return d
    raise AssertionError(f"{c}: no candidate-independent draw")


def _ln_mod_chain(d32, r, scr, shr):
    ln = _rbf(d32 * r[:, None])
    return (_rbf(ln * _rbf(1 + scr.float())) + shr.float()).to(BF16)


def _ln_mod_f64(st, scr, shr):
    ln = _to_bf16(st["d64"] * st["r64"][:, None]).double()
    prod = _to_bf16(ln * _to_bf16(1 + scr).double()).double()
    return _to_bf16(prod + shr)


def _final_chain(d32, r, scr, shr):
    return (d32 * r[:, None]) * (1 + scr.float()) + shr.float()


def _final_f64(st, scr, shr):
    return st["d64"] * st["r64"][:, None] * (1 + scr) + shr


def _row_err(out, ref64):
    return ((out.double() - ref64).abs().amax(1) / ref64.abs().amax(1)).max().item()


def _fp8_of(h):
    """(scale [R] fp32, codes [R, D] uint8) of bf16 rows h: the kernel's fp32 steps, the table's rounding."""
    amax = h.float().abs().amax(1)
    inv = torch.tensor(448.0) / amax.clamp(min=AMAX_FLOOR)
    f = (h.float() * inv[:, None]).clamp(-448, 448)
    return amax / torch.tensor(448.0), e4m3_round(f.double())


def _family_premise(c, d):
    """x (+ g y) is a family row: exact values, exact sums, zero-sum integer deviations."""
    st = _stats(d["xs"])
    assert torch.equal(d["xs"].float().to(BF16).double(), d["xs"])
    for t in (d["x"], d["y"], d["gate"]):
        assert torch.equal(t.float().to(BF16).double(), t)
    if c.res:  # rbf(g y) and rbf(x + .) are exact
        assert torch.equal(_to_bf16(d["gy"]).double(), d["gy"])
    _exact_sums(st, d["u"])
    k = st["d64"] / d["u"]
    assert torch.equal(k, k.round()) and (k.sum(1) == 0).all() and k.abs().max() <= 48
    if c.D == 5120:
        assert (st["s64"] == 0).all()
    else:
        assert torch.equal((st["s32"] * _inv(c.D)).double(), st["s64"] / c.D)
    return st


@pytest.mark.parametrize("case", LN_CASES + LN_EXTRA, ids=str)
def test_premise_ln_mod(case):
    d = _ln_data(case)
    st = _family_premise(case, d)
    for t in (d["sh"], d["sc"]):
        t = torch.where(t == TINY, 0.0, t) if case.const else t
        assert torch.equal(t * 64, (t * 64).round()) and t.abs().max() <= 2
    h64 = _ln_mod_f64(st, d["scr"], d["shr"])
    for r in _candidates(st["a32"]):
        assert torch.equal(_bits(_ln_mod_chain(st["d32"], r, d["scr"], d["shr"])), _bits(h64))
    if case.const:
        assert (st["q64"][[1, 5, 9]] == 0).all() and (h64[1] == 0).all() and torch.equal(h64[5].double(), d["shr"][5])
        assert (h64[5] != 0).any() and _fp8_of(h64)[0][1] == 0 and (_fp8_of(h64)[1][1] == 0).all()
        # row 9: h is zero but for one TINY: a sub-normal scale, and 448 / amax would be infinite: codes 0 by the floor
        assert h64[9].double().abs().sum() == TINY and 0 < _fp8_of(h64)[0][9] < 2.0 ** -126 and (_fp8_of(h64)[1][9] == 0).all()
    scale, _ = _fp8_of(h64)
    amax = h64.float().abs().amax(1)
    assert ((amax == 0) | (amax > 1e-3) | (amax == TINY)).all() and torch.isfinite(scale).all()


@pytest.mark.parametrize("case", LN_CASES, ids=str)
def test_premise_final_ln_mod(case):
    d = _ln_data(case, True)
    st = _family_premise(case, d)
    outs = torch.stack([_final_chain(st["d32"], r, d["scr"], d["shr"]) for r in _candidates(st["a32"])])
    dep = _check_search_can_fail(outs, str(case))
    assert dep == 1.0 and (_told_apart(outs) == 10).all()  # every candidate gives another row
    cpu = _row_err(outs[2], _final_f64(st, d["scr"], d["shr"]))
    assert 0 < cpu < 1e-6
    print(f"{case}: CPU fp32 error {cpu:.3e}")


def _dev_mods(d, device, final):
    """shift / scale / gate on the device as views of shared storage (strides are not D)."""
    B, T, D = d["gate"].shape
    if final:
        f = torch.cat([d["sh"], d["sc"]], -1).float().to(device)          # [B, T, 2 D] fp32
        gm = torch.full((B, T, 3 * D), float("nan"), dtype=BF16)
        gm[..., 2 * D:] = d["gate"].to(BF16)
        return f[..., :D], f[..., D:], gm.to(device)[..., 2 * D:]
    mods = torch.cat([d["sh"], d["sc"], d["gate"]], -1).to(BF16).to(device)
    return mods[..., :D], mods[..., D:2 * D], mods[..., 2 * D:]


def _run_ln_mod(device, c, fp8):
    d = _ln_data(c)
    D, R = c.D, c.rows
    x = d["x"].to(BF16).to(device)
    y = d["y"].to(BF16).to(device) if c.res else None
    sh, sc, gt = _dev_mods(d, device, False)
    xbuf, x_out = guarded(R * D, BF16, device, SENTINEL)
    lib, st = N.load_library(), N._stream(device)
    head = (N._ptr(x), x.stride(0), 0 if c.bcast else x.stride(1), N._ptr(y), N._ptr(gt) if c.res else None, N._ptr(sh),
            N._ptr(sc), sh.stride(0), sh.stride(1), N._ptr(x_out) if c.res else None)
    tail = (c.n_tok, c.B, D, c.tok0, HW, float(EPS), st)
    if fp8:
        qbuf, q = guarded(R * D, torch.uint8, device, FILL8)
        sbuf, s = guarded(R, F32, device, SENTINEL)
        rc = lib.cp25_ln_mod_fp8(*head, N._ptr(q), N._ptr(s), *tail)
    else:
        hbuf, h = guarded(R * D, BF16, device, SENTINEL)
        rc = lib.cp25_ln_mod(*head, N._ptr(h), *tail)
    torch.cuda.synchronize()
    assert rc == 0
    assert guards_ok(xbuf, R * D, SENTINEL)
    xo = x_out.cpu().view(R, D)
    if c.res:
        assert torch.equal(xo, d["xs"].to(BF16)), "x_out is not x + gate * y"
    else:
        assert (xo == SENTINEL).all(), "x_out written without a residual"
    if fp8:
        assert guards_ok(qbuf, R * D, FILL8) and guards_ok(sbuf, R, SENTINEL)
        return q.cpu().view(R, D), s.cpu()
    assert guards_ok(hbuf, R * D, SENTINEL)
    return h.cpu().view(R, D)


def _first_bad(got, ref):
    bad = (_bits(got) != _bits(ref)).nonzero()
    return f"{bad.shape[0]} of {ref.numel()} differ in rows {bad[:, 0].unique().tolist()[:8]}, first {bad[:4].tolist()}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_CASES + LN_EXTRA, ids=str)
def test_ln_mod_exact(device, case):
    d = _ln_data(case)
    ref = _ln_mod_f64(_stats(d["xs"]), d["scr"], d["shr"])
    h = _run_ln_mod(device, case, False)
    assert torch.equal(_bits(h), _bits(ref)), _first_bad(h, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_CASES + LN_EXTRA, ids=str)
def test_ln_mod_fp8_exact(device, case):
    d = _ln_data(case)
    scale, codes = _fp8_of(_ln_mod_f64(_stats(d["xs"]), d["scr"], d["shr"]))
    q, s = _run_ln_mod(device, case, True)
    assert torch.equal(_bits(s), _bits(scale)), (s.tolist(), scale.tolist())
    assert torch.equal(q, codes), _first_bad(q, codes)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_GAUSS, ids=str)
def test_ln_mod_gaussian(device, case):
    d = _ln_data(case)
    ref = _ln_mod_f64(_stats(d["xs"]), d["scr"], d["shr"])
    h = _run_ln_mod(device, case, False)  # asserts x_out = rbf(x + rbf(g y)) exactly
    ok, eq = bf16_ulp_close(h, ref)
    assert ok, eq
    q, s = _run_ln_mod(device, case, True)
    scale, codes = _fp8_of(h)             # of the bf16 kernel's own h: the two variants share every step before
    assert torch.equal(s, scale) and torch.equal(q, codes)


def _run_final(device, c):
    d = _ln_data(c, True)
    D, R = c.D, c.rows
    x = d["x"].to(BF16).to(device)
    y = d["y"].to(BF16).to(device) if c.res else None
    sh, sc, gt = _dev_mods(d, device, True)
    assert (gt.stride(0), gt.stride(1)) != (sh.stride(0), sh.stride(1))
    obuf, out = guarded(R * D, F32, device, SENTINEL)
    rc = N.load_library().cp25_final_ln_mod(
        N._ptr(x), N._ptr(y), N._ptr(gt) if c.res else None, gt.stride(0), gt.stride(1), N._ptr(sh), N._ptr(sc),
        sh.stride(0), sh.stride(1), N._ptr(out), c.n_tok, c.B, D, c.tok0, HW, float(EPS), N._stream(device))
    torch.cuda.synchronize()
    assert rc == 0 and guards_ok(obuf, R * D, SENTINEL)
    out = out.cpu().view(R, D)
    w = N.final_ln_mod(x, sh, sc, n_tok=c.n_tok, B=c.B, tok0=c.tok0, hw=HW, y=y, gate=gt if c.res else None)
    assert torch.equal(_bits(w.cpu().view(R, D)), _bits(out))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_CASES, ids=str)
def test_final_ln_mod_exact(device, case):
    d = _ln_data(case, True)
    st = _stats(d["xs"])
    outs = torch.stack([_final_chain(st["d32"], r, d["scr"], d["shr"]) for r in _candidates(st["a32"])])
    out = _run_final(device, case)
    ok = _match(out, outs)
    assert ok.all(), f"rows {(~ok).nonzero().flatten().tolist()} equal no candidate's row"
    ref64 = _final_f64(st, d["scr"], d["shr"])
    cpu, gpu = _row_err(outs[2], ref64), _row_err(out, ref64)
    print(f"{case}: error vs float64: CPU fp32 {cpu:.3e}, GPU {gpu:.3e}")
    assert gpu <= 2 * cpu, (gpu, cpu)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LN_GAUSS, ids=str)
def test_final_ln_mod_gaussian(device, case):
    d = _ln_data(case, True)
    st = _stats(d["xs"])
    ref64 = _final_f64(st, d["scr"], d["shr"])
    r0 = (1 / torch.sqrt(st["a32"].double())).float()
    cpu = _row_err(_final_chain(st["d32"], r0, d["scr"], d["shr"]), ref64)
    gpu = _row_err(_run_final(device, case), ref64)
    print(f"{case}: error vs float64: CPU fp32 {cpu:.3e}, GPU {gpu:.3e}")
    assert gpu < 1e-5, (gpu, cpu)  # test_dit_ops_gpu.test_final_ln_mod's bound, here per row


# ================================================================================================ layer_norm
LN_M = (1, 6, 131)


@functools.lru_cache(maxsize=None)
def _affine_data(D, M, gauss=False):
    g = torch.Generator().manual_seed(3 * D + M + 100000 * gauss)
    w = (1 + 0.1 * torch.randn(D, generator=g)).to(BF16).double()
    b = (0.1 * torch.randn(D, generator=g)).to(BF16).double()
    if gauss:
        return dict(x=torch.randn(M, D, generator=g).to(BF16).double(), w=w, b=b, u=None)
    x, u, _ = _family(g, M, D, 16, zero_mean=D == 5120)
    return dict(x=x, w=w, b=b, u=u)


def _affine_chain(d32, r, w, b):
    return ((d32 * r[:, None]) * w.float() + b.float()).to(BF16)


def _affine_outs(d):
    st = _stats(d["x"])
    return st, torch.stack([_affine_chain(st["d32"], r, d["w"], d["b"]) for r in _candidates(st["a32"])])


@pytest.mark.parametrize("M", LN_M)
@pytest.mark.parametrize("D", WIDTHS)
def test_premise_layer_norm(D, M):
    d = _affine_data(D, M)
    st, outs = _affine_outs(d)
    assert torch.equal(d["x"].float().to(BF16).double(), d["x"])
    _exact_sums(st, d["u"])
    dep = _check_search_can_fail(outs, f"{D} x {M}")
    print(f"D = {D}, M = {M}: {dep:.1%} of rows depend on the candidate")


def _run_layer_norm(device, d):
    M, D = d["x"].shape
    xs = torch.full((M, D + 8), float("nan"), dtype=BF16)
    xs[:, :D] = d["x"].to(BF16)
    ld = D + 64
    buf, flat = guarded(M * ld, BF16, device, SENTINEL)
    out = flat.view(M, ld)
    N.layer_norm(xs.to(device)[:, :D], d["w"].to(BF16).to(device), d["b"].to(BF16).to(device), out=out[:, :D])
    torch.cuda.synchronize()
    assert guards_ok(buf, M * ld, SENTINEL)
    got = out.cpu()
    assert (got[:, D:] == SENTINEL).all(), "wrote between the rows"
    return got[:, :D].contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("M", LN_M)
@pytest.mark.parametrize("D", WIDTHS)
def test_layer_norm_exact(device, D, M):
    d = _affine_data(D, M)
    _, outs = _affine_outs(d)
    ok = _match(_run_layer_norm(device, d), outs)
    assert ok.all(), f"rows {(~ok).nonzero().flatten().tolist()} equal no candidate's row"


@pytest.mark.gpu
@pytest.mark.parametrize("D,M", [(1024, 6), (4096, 6), (1024, 131), (4096, 1)])
def test_layer_norm_gaussian(device, D, M):
    d = _affine_data(D, M, gauss=True)
    st = _stats(d["x"])
    ref = _to_bf16(st["d64"] * st["r64"][:, None] * d["w"] + d["b"])
    ok, eq = bf16_ulp_close(_run_layer_norm(device, d), ref)
    assert ok, eq


# ================================================================================================ head RMSNorm + RoPE
OUT_SCALES = (1.0, 0.25, float(torch.tensor(128 ** -0.5 * math.log2(math.e), dtype=F32)))


@dataclasses.dataclass(frozen=True)
class HnCase:
    H: int
    B: int
    n_rows: int
    off_d: bool          # head_off = D (the k columns) instead of 0
    rope: bool
    scale: int           # index into OUT_SCALES
    out2: bool
    peak: bool = False   # the longest output row is item n_rows * H - 2, in the last, partial, group of 16
    gauss: bool = False

    def __str__(self):
        tag = "_offD" * self.off_d + "_rope" * self.rope + "_out2" * self.out2 + "_peak" * self.peak + "_gauss" * self.gauss
        return f"h{self.H}_b{self.B}_r{self.n_rows}_s{self.scale}{tag}"

    @property
    def items(self):
        return self.n_rows * self.H


HN_CASES = [
    HnCase(1, 1, 16, False, False, 0, False),
    HnCase(1, 2, 17, True, True, 1, True),
    HnCase(3, 1, 11, True, True, 2, True),
    HnCase(3, 2, 15, False, True, 0, False),
    HnCase(16, 1, 5, True, False, 1, True),
    HnCase(16, 2, 6, False, True, 2, False),
    HnCase(1, 1, 2077, False, True, 0, True),
    HnCase(1, 1, 29, True, False, 2, False, peak=True),
]
HN_GAUSS = [HnCase(3, 2, 15, False, True, 0, False, gauss=True), HnCase(3, 1, 11, True, True, 2, True, gauss=True)]


@functools.lru_cache(maxsize=None)
def _hn_data(c: HnCase):
    g = torch.Generator().manual_seed(zlib.crc32(str(c).encode()))
    w = (1 + 0.1 * torch.randn(128, generator=g)).to(BF16).double()
    n_tok = -(-c.n_rows // c.B)
    if c.gauss:
        x, u = torch.randn(c.items, 128, generator=g).to(BF16).double(), None
        ang = torch.rand(n_tok, 64, generator=g).double() * 50
        cos, sin = torch.cos(ang).float().double(), torch.sin(ang).float().double()
    else:
        x, u, _ = _family(g, c.items, 128, 8, zero_mean=True)
        cos, sin = torch.randint(-16, 17, (2, n_tok, 64), generator=g).double() / 16
    if c.peak:  # all of the row's weight on the two columns of largest |w|
        i1, i2 = w.abs().argsort(descending=True)[:2].tolist()
        x[c.items - 2] = 0
        x[c.items - 2, i1], x[c.items - 2, i2] = 8 * u[c.items - 2], -8 * u[c.items - 2]
    return dict(x=x.view(c.n_rows, c.H, 128), u=u, w=w, cos=cos, sin=sin)


def _hn_stats(x):
    x32 = x.float()
    q32, q64 = (x32 * x32).sum(-1), (x * x).sum(-1)
    a32 = q32 * _inv(128) + EPS
    return dict(q32=q32, q64=q64, a32=a32, r64=1 / torch.sqrt(q64 / 128 + EPS.double()))


def _hn_chain(c, d, r):
    """bf16 [n_rows, H, 128]: the kernel's fp32 sequence with rstd r [n_rows, H]."""
    v = _rbf((d["x"].float() * r[..., None]) * d["w"].float())
    if c.rope:
        tok = torch.arange(c.n_rows) // c.B
        cs = torch.cat([d["cos"][tok]] * 2, -1)[:, None, :]  # [n_rows, 1, 128]
        sn = torch.cat([d["sin"][tok]] * 2, -1)[:, None, :]
        partner = torch.cat([-v[..., 64:], v[..., :64]], -1)  # sgn * partner
        t = partner * sn.float()
        v = (v.double() * cs + t.double()).float()            # fmaf: one rounding of the exact sum
    return (v * torch.tensor(OUT_SCALES[c.scale], dtype=F32)).to(BF16)


def _hn_f64(c, d, st):
    v = _to_bf16(d["x"] * st["r64"][..., None] * d["w"]).double()
    if c.rope:
        tok = torch.arange(c.n_rows) // c.B
        cs = torch.cat([d["cos"][tok]] * 2, -1)[:, None, :]
        sn = torch.cat([d["sin"][tok]] * 2, -1)[:, None, :]
        v = v * cs + torch.cat([-v[..., 64:], v[..., :64]], -1) * sn
    return _to_bf16(v * OUT_SCALES[c.scale])


def _hn_outs(c, d):
    st = _hn_stats(d["x"])
    return st, torch.stack([_hn_chain(c, d, r) for r in _candidates(st["a32"])])


@pytest.mark.parametrize("case", HN_CASES, ids=str)
def test_premise_head_norm(case):
    d = _hn_data(case)
    st, outs = _hn_outs(case, d)
    x = d["x"]
    assert torch.equal(x.float().to(BF16).double(), x) and (x.sum(-1) == 0).all()
    assert torch.equal(st["q32"].double(), st["q64"])
    qi = st["q64"].flatten() / (d["u"] * d["u"]).flatten()
    assert torch.equal(qi, qi.round()) and qi.max() < 2 ** 24 and qi.min() > 0
    for t in (d["cos"], d["sin"]):
        assert torch.equal(t * 16, (t * 16).round()) and t.abs().max() <= 1
    if case.rope:  # the fmaf's two products are exact in fp32, so their float64 sum is the exact sum
        v = _rbf((x.float() * _candidates(st["a32"])[2][..., None]) * d["w"].float())
        cs = torch.cat([d["cos"][torch.arange(case.n_rows) // case.B]] * 2, -1)[:, None, :]
        assert torch.equal((v * cs.float()).double(), v.double() * cs)
    o = outs.view(5, case.items, 128)
    dep = _check_search_can_fail(o, str(case))
    assert case.items % 16 in (0, 1, 13)
    if case.peak:
        nrm = o[2].double().norm(dim=1)
        assert nrm.argmax() == case.items - 2 >= case.items // 16 * 16 and case.items % 16
    print(f"{case}: {-(-case.items // 16)} workgroups, {dep:.2%} of items depend on the candidate")


def test_premise_head_norm_table():
    assert {c.H for c in HN_CASES} == {1, 3, 16} and {c.B for c in HN_CASES} == {1, 2}
    assert {c.items % 16 for c in HN_CASES} == {0, 1, 13}
    assert {c.scale for c in HN_CASES} == {0, 1, 2} and {c.rope for c in HN_CASES} == {False, True}
    assert {c.off_d for c in HN_CASES} == {False, True} and {c.out2 for c in HN_CASES} == {False, True}
    wgs = [-(-c.items // 16) for c in HN_CASES]
    assert min(wgs) < 64 and 130 in wgs and any(c.peak for c in HN_CASES)
    assert {(c.rope, c.scale != 0, c.out2) for c in HN_CASES} >= {(True, True, True)}


def _run_head_norm(device, c, nmax):
    """(rows [n_rows, H, 128] bf16, out2 rows or None, slots [64, 32] or None); asserts everything else untouched."""
    d = _hn_data(c)
    D = c.H * 128
    off, ld, ld2 = (D if c.off_d else 0), 3 * D, D + 64
    big = torch.full((c.n_rows, ld), SENTINEL, dtype=BF16)
    big[:, off:off + D] = d["x"].view(c.n_rows, D).to(BF16)
    buf, flat = guarded(c.n_rows * ld, BF16, device, SENTINEL)
    flat.copy_(big.view(-1).to(device))
    b2, flat2 = guarded(c.n_rows * ld2, BF16, device, SENTINEL)
    slots = torch.zeros(64, 32, dtype=F32, device=device) if nmax else None
    kw = dict(cos=d["cos"].float().to(device), sin=d["sin"].float().to(device)) if c.rope else {}
    if c.out2:
        kw.update(out2=flat2, out2_stride=ld2)
    N.head_rmsnorm_rope(flat.view(c.n_rows, ld), n_rows=c.n_rows, B=c.B, H=c.H, head_off=off,
                        weight=d["w"].to(BF16).to(device), out_scale=OUT_SCALES[c.scale], norm_max=slots, **kw)
    torch.cuda.synchronize()
    assert guards_ok(buf, c.n_rows * ld, SENTINEL) and guards_ok(b2, c.n_rows * ld2, SENTINEL)
    got = flat.cpu().view(c.n_rows, ld)
    rest = got.clone()
    rest[:, off:off + D] = SENTINEL
    assert (rest == SENTINEL).all(), "wrote outside the head columns"
    got2 = flat2.cpu().view(c.n_rows, ld2)
    assert (got2[:, D:] == SENTINEL).all() and (c.out2 or (got2 == SENTINEL).all())
    rows = got[:, off:off + D].reshape(c.n_rows, c.H, 128)
    return rows, (got2[:, :D].reshape(c.n_rows, c.H, 128) if c.out2 else None), (slots.cpu() if nmax else None)


def _check_slots(c, rows, slots):
    items = rows.reshape(c.items, 128)
    n32, n64 = items.float().norm(dim=1), items.double().norm(dim=1)
    wg = torch.arange(c.items) // 16 % 64
    assert (slots[:, 1:] == 0).all()
    for j in range(64):
        mine = wg == j
        if not mine.any():
            assert slots[j, 0] == 0, j
            continue
        want32, want64 = n32[mine].max().item(), n64[mine].max().item()
        got = slots[j, 0].item()
        assert abs(got - want32) <= 1e-5 * want32 and got >= want64 * (1 - 1e-5), (j, got, want32, want64)


@pytest.mark.gpu
@pytest.mark.parametrize("case", HN_CASES, ids=str)
def test_head_norm_exact(device, case):
    d = _hn_data(case)
    _, outs = _hn_outs(case, d)
    rows, rows2, _ = _run_head_norm(device, case, False)
    ok = _match(rows.reshape(case.items, 128), outs.view(5, case.items, 128))
    assert ok.all(), f"items {(~ok).nonzero().flatten().tolist()[:16]} equal no candidate's row"
    if case.out2:
        assert torch.equal(_bits(rows2), _bits(rows))


@pytest.mark.gpu
@pytest.mark.parametrize("case", HN_CASES + HN_GAUSS, ids=str)
def test_head_norm_nmax(device, case):
    """The nmax variant writes the plain variant's bytes (both run here) and the slot maxima."""
    rows, rows2, _ = _run_head_norm(device, case, False)
    nrows, nrows2, slots = _run_head_norm(device, case, True)
    assert torch.equal(_bits(nrows), _bits(rows))
    if case.out2:
        assert torch.equal(_bits(nrows2), _bits(rows2))
    _check_slots(case, nrows, slots)
    if case.peak:
        j = (case.items - 2) // 16 % 64
        assert slots[:, 0].argmax() == j


@pytest.mark.gpu
@pytest.mark.parametrize("case", HN_GAUSS, ids=str)
def test_head_norm_gaussian(device, case):
    d = _hn_data(case)
    ref = _hn_f64(case, d, _hn_stats(d["x"]))
    rows, rows2, _ = _run_head_norm(device, case, False)
    ok, eq = bf16_ulp_close(rows, ref)
    assert ok, eq
    if case.out2:
        assert torch.equal(_bits(rows2), _bits(rows))
