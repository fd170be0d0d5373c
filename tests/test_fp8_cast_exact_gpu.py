"""cp25_cast_fp8_e4m3, cp25_quant_fp8_rows, cp25_gelu_quant_fp8 and cp25_cast_v_fp8t against a table built from the
e4m3fn format's definition, at the inputs where the rounding is hard.

Reference: the 256 code values in float64 (sign, 4 exponent bits with bias 7, 3 mantissa bits; exponent 0 subnormal,
0x7F / 0xFF NaN, largest finite 448); e4m3_round takes exact float64 inputs to the nearest code, ties to the even
code, saturating at +-448, sign kept on zero. test_premise_table checks it against torch's CPU float8_e4m3fn cast on
every finite bf16 value of magnitude <= 448. Nothing here asks torch's GPU cast.

Every input is chosen so that the kernel's one fp32 product before the conversion is exact (power-of-two scales), so the
bytes must equal the table's: no tolerance anywhere but in the GELU leg, which keeps test_fp8_gpu's own assertions.

  cast_fp8       every finite bf16 bit pattern and +-inf (65 282 values, zero-padded to whole rows) at scales 1, 4, 0.25
                 and 2^-10, widths 16 (4081 rows: 4081 threads, 241 in the last workgroup) and 272 (241 rows, 4097
                 threads, one in the last workgroup), source stride width + 8, output stride width + 16.
  quant_fp8_rows all ten K; M leaves the last workgroup partly dead (17 rows at 4 rows per workgroup, 15 at 2) or is 3
                 where a workgroup holds one row. Row i has its maximum 448 * 2^j in a random column, j cycling through
                 -6 .. 6, the rest every e4m3 value and every midpoint between neighbours times 2^j plus random bf16
                 values no larger: scale = 2^j bit for bit, x * 2^-j exact, every code and tie reached (test_premise_rows).
                 One all-zero row (scale 0, codes 0) and one row whose only non-zero is the smallest bf16 subnormal.
  gelu=True      K = 1024, 1536, 4096, 6144 under test_fp8_gpu.test_quant_rows_bit_exact's assertions.
  cast_v_fp8t    (B, H, L) = (1, 1, 1), (1, 2, 63), (2, 1, 64), (1, 3, 65), (1, 2, 1030): one key, a tile short of one
                 key, exactly a tile, a tile and one key, and two v_amax_kernel chunks with the maxima in rows 1027
                 and 3. Head maxima 448 * 2^j; in the three cases between, the last head is all zero (amax 0, bytes 0);
                 keys past L are zero bytes.

A row whose largest magnitude is below 2^-100 is quantised as if it were 2^-100 (the floor cp25_cast_v_fp8t always had):
448 / amax overflows to infinity below 448 / FLT_MAX = 1.3e-36 and would turn the row's zeros into NaN and, through the
clamp, into -448. The sub-normal row here is the case: its scale is fl(2^-133 / 448) and its codes are all zero.
"""
import functools

import pytest
import torch

from cosmos_predict2 import _native as N
import test_fp8_gpu as T8
from test_attn_fp8qk_gpu import _vt_key

BF16 = torch.bfloat16
F8 = torch.float8_e4m3fn
GUARD = 256
SENTINEL = -1.5e30
FILL8 = 0xA5  # the sentinel of byte buffers
AMAX_FLOOR = 2.0 ** -100


# ------------------------------------------------------------------------------------------------ the table
def _e4m3_values():
    c = torch.arange(256)
    e, m = ((c >> 3) & 15).double(), (c & 7).double()
    mag = torch.where(e == 0, m / 8 * 2.0 ** -6, (1 + m / 8) * torch.pow(2.0, e - 7))
    v = torch.where((c >> 7) == 1, -mag, mag)
    v[(c & 0x7F) == 0x7F] = float("nan")
    return v


VALUES = _e4m3_values()                      # float64 [256], indexed by code
MAGS = VALUES[:127].clone()                  # 0 .. 448 ascending, index == code
FINITE = VALUES[~torch.isnan(VALUES)]        # 254 values, both zeros
MIDS = (MAGS[:-1] + MAGS[1:]) / 2            # 126 exact ties


def e4m3_round(x, ties=False):
    """Exact float64 x -> uint8 e4m3fn codes: nearest, ties to even, saturating (+-inf included)."""
    x = x.double()
    a = x.abs().clamp(max=448.0)
    hi = torch.searchsorted(MAGS, a).clamp(max=126)
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = a - MAGS[lo], MAGS[hi] - a
    tie = (dlo == dhi) & (hi != lo)
    code = torch.where((dhi < dlo) | (tie & (hi % 2 == 0)) | (hi == lo), hi, lo)
    code = (code | (torch.signbit(x).long() << 7)).to(torch.uint8)
    return (code, tie) if ties else code


def guarded(n, dtype, device, fill):
    """A flat n-element output inside a fill-valued buffer with GUARD elements either side."""
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=device)
    return buf, buf[GUARD:GUARD + n]


def guards_ok(buf, n, fill):
    b = buf.cpu()
    g = torch.full((GUARD,), fill, dtype=b.dtype)
    return torch.equal(b[:GUARD], g) and torch.equal(b[GUARD + n:], g)


def _mismatch(got, ref):
    bad = (got != ref).nonzero()
    return f"{bad.shape[0]} of {ref.numel()} differ, first {[(tuple(i.tolist()), int(got[tuple(i)]), int(ref[tuple(i)])) for i in bad[:6]]}"


def test_premise_table():
    assert MAGS[0] == 0 and MAGS[1] == 2.0 ** -9 and MAGS[8] == 2.0 ** -6 and MAGS[126] == 448.0
    assert (MAGS[1:] > MAGS[:-1]).all() and FINITE.numel() == 254
    x = torch.arange(1 << 16, dtype=torch.int32).to(torch.int16).view(BF16)
    x = x[torch.isfinite(x.float()) & (x.float().abs() <= 448)]
    assert torch.equal(x.to(F8).view(torch.uint8), e4m3_round(x.double()))
    # and on the table's own points: every code is a fixed point, every midpoint goes to the even neighbour
    c = torch.arange(256)[~torch.isnan(VALUES)]
    assert torch.equal(e4m3_round(FINITE), c.to(torch.uint8))
    code, tie = e4m3_round(MIDS, ties=True)
    assert tie.all() and (code % 2 == 0).all() and ((code.long() - torch.arange(126)).abs() <= 1).all()
    assert e4m3_round(torch.tensor([float("inf"), -float("inf"), 1e9, -0.0])).tolist() == [0x7E, 0xFE, 0x7E, 0x80]


# ------------------------------------------------------------------------------------------------ cast_fp8
SCALES = (1.0, 4.0, 0.25, 2.0 ** -10)


@functools.lru_cache(maxsize=None)
def _all_bf16(width):
    x = torch.arange(1 << 16, dtype=torch.int32).to(torch.int16).view(BF16)
    x = x[~torch.isnan(x.float())]
    rows = -(-x.numel() // width)
    out = torch.zeros(rows * width, dtype=BF16)
    out[:x.numel()] = x
    return out.view(rows, width)


def test_premise_cast():
    for width in (16, 272):
        x = _all_bf16(width)
        assert x.numel() >= 65282 and not torch.isnan(x.float()).any() and torch.isinf(x.float()).sum() == 2
        assert (x.shape[0] * width // 16) % 256 != 0
        for sc in SCALES:  # the fp32 product is the exact one wherever it matters (overflow saturates either way)
            p32, p64 = x.float() * torch.tensor(sc), x.double() * sc
            assert torch.equal(e4m3_round(p32.double()), e4m3_round(p64))
            fin = torch.isfinite(p32)
            assert torch.equal(p32[fin].double(), p64[fin])


@pytest.mark.gpu
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("width", [16, 272])
def test_cast_fp8_every_bf16(device, width, scale):
    x = _all_bf16(width)
    rows = x.shape[0]
    src = torch.full((rows, width + 8), float("nan"), dtype=BF16)
    src[:, :width] = x
    ld = width + 16
    buf, flat = guarded(rows * ld, torch.uint8, device, FILL8)
    out = flat.view(rows, ld)
    N.cast_fp8(src.to(device)[:, :width], scale, out=out[:, :width])
    torch.cuda.synchronize()
    assert guards_ok(buf, rows * ld, FILL8)
    got = out.cpu()
    assert (got[:, width:] == FILL8).all(), "wrote between the rows"
    ref = e4m3_round(x.double() * scale)
    assert torch.equal(got[:, :width], ref), _mismatch(got[:, :width], ref)


# ------------------------------------------------------------------------------------------------ quant_fp8_rows
ALL_K = (512, 1024, 1536, 2048, 3072, 4096, 5120, 6144, 8192, 20480)
ROWS_PER_WG = {512: 4, 1024: 4, 1536: 4, 2048: 4, 3072: 2, 4096: 2, 5120: 2, 6144: 1, 8192: 1, 20480: 1}
TINY = 2.0 ** -133  # the smallest bf16 subnormal


def _rows_m(K):
    return {4: 17, 2: 15, 1: 3}[ROWS_PER_WG[K]]


def _hard_values(g, n, j, cover):
    """n exact bf16 values of magnitude <= 448 * 2^j: 40 % e4m3 values, 20 % midpoints, the rest random, all times
    2^j; cover: the first 506 are every value and every midpoint once."""
    kind = torch.randint(0, 10, (n,), generator=g)
    grid = FINITE[torch.randint(0, 254, (n,), generator=g)]
    mid = MIDS[torch.randint(0, 126, (n,), generator=g)] * (torch.randint(0, 2, (n,), generator=g) * 2 - 1)
    rnd = (torch.randn(n, generator=g) * 100).to(BF16).double().clamp(-448, 448)
    x = torch.where(kind < 4, grid, torch.where(kind < 6, mid, rnd))
    if cover:
        x[:506] = torch.cat([FINITE, MIDS, -MIDS])
    return x[torch.randperm(n, generator=g)] * 2.0 ** j


@functools.lru_cache(maxsize=None)
def _rows_case(K):
    """x [M, K] bf16, expected scale [M] fp32 and codes [M, K], and the exact x / scale the codes come from."""
    M = _rows_m(K)
    g = torch.Generator().manual_seed(K)
    j0 = ALL_K.index(K) * 4
    x = torch.empty(M, K, dtype=torch.float64)
    js = [(j0 + i) % 13 - 6 for i in range(M)]
    for i, j in enumerate(js):
        x[i] = _hard_values(g, K, j, cover=True)
        col = int(torch.randint(0, K, (1,), generator=g))
        x[i, col] = (448.0 if i % 2 else -448.0) * 2.0 ** j
    scale = torch.tensor([2.0 ** j for j in js], dtype=torch.float64)
    zero_row = {6144: 1, 8192: None}.get(K, 1 if M > 3 else None)
    tiny_row = {6144: None, 8192: 1}.get(K, 2 if M > 3 else None)
    scaled = x / scale[:, None]
    if zero_row is not None:
        x[zero_row], scaled[zero_row], scale[zero_row] = 0, 0, 0
    scale32 = scale.float()
    if tiny_row is not None:
        col = int(torch.randint(0, K, (1,), generator=g))
        x[tiny_row] = 0
        x[tiny_row, col] = TINY
        scale32[tiny_row] = torch.tensor(TINY, dtype=torch.float32) / torch.tensor(448.0)  # fp32 division, subnormal
        scaled[tiny_row] = x[tiny_row] * (448.0 / AMAX_FLOOR)
    codes, tie = e4m3_round(scaled, ties=True)
    return dict(x=x.to(BF16), x64=x, scale=scale32, codes=codes, tie=tie, js=js, zero_row=zero_row, tiny_row=tiny_row)


def test_premise_rows():
    seen, ties, total = set(), 0, 0
    for K in ALL_K:
        d = _rows_case(K)
        M = d["x"].shape[0]
        assert M % ROWS_PER_WG[K] != 0 or ROWS_PER_WG[K] == 1
        assert torch.equal(d["x"].double(), d["x64"])  # bf16 holds every input
        for i, j in enumerate(d["js"]):
            if i in (d["zero_row"], d["tiny_row"]):
                continue
            assert d["x64"][i].abs().max() == 448.0 * 2.0 ** j and d["scale"][i] == 2.0 ** j
            # the kernel's fp32 steps are exact: amax / 448 = 2^j, 448 / amax = 2^-j, x * 2^-j
            amax = d["x"][i].float().abs().max()
            assert amax / torch.tensor(448.0) == 2.0 ** j and torch.tensor(448.0) / amax == 2.0 ** -j
            assert torch.equal((d["x"][i].float() * (torch.tensor(448.0) / amax)).double(), d["x64"][i] * 2.0 ** -j)
        seen |= set(d["codes"].flatten().tolist())
        ties += int(d["tie"].sum())
        total += d["tie"].numel()
    assert seen == set(range(256)) - {0x7F, 0xFF}, sorted(set(range(256)) - seen)
    assert ties >= 0.05 * total, ties / total
    assert sum(d is not None for d in (_rows_case(K)["zero_row"] for K in ALL_K)) >= 1
    assert sum(d is not None for d in (_rows_case(K)["tiny_row"] for K in ALL_K)) >= 1
    print(f"{len(seen)} codes, {ties / total:.1%} exact ties")


@pytest.mark.gpu
@pytest.mark.parametrize("K", ALL_K)
def test_quant_rows_table(device, K):
    d = _rows_case(K)
    M = d["x"].shape[0]
    x = d["x"].to(device)
    qbuf, q = guarded(M * K, torch.uint8, device, FILL8)
    sbuf, s = guarded(M, torch.float32, device, SENTINEL)
    rc = N.load_library().cp25_quant_fp8_rows(N._ptr(x), N._ptr(q), N._ptr(s), M, K, N._stream(device))
    torch.cuda.synchronize()
    assert rc == 0
    assert guards_ok(qbuf, M * K, FILL8) and guards_ok(sbuf, M, SENTINEL)
    s, q = s.cpu(), q.cpu().view(M, K)
    assert torch.equal(s.view(torch.int32), d["scale"].view(torch.int32)), (s.tolist(), d["scale"].tolist())
    assert torch.equal(q, d["codes"]), _mismatch(q, d["codes"])
    # the wrapper returns the same bytes
    q2, s2 = N.quant_fp8_rows(x)
    assert torch.equal(q2.view(torch.uint8).cpu(), d["codes"]) and torch.equal(s2.cpu().view(M), s)


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", [(5, 1024), (7, 1536), (3, 4096), (3, 6144)])
def test_gelu_quant_rows_missing_k(device, M, K):
    """The four K test_fp8_gpu never launches, under its assertions (rows 0 and 2.. Gaussian, row 1 zero)."""
    T8.test_quant_rows_bit_exact(device, M, K, True)


# ------------------------------------------------------------------------------------------------ cast_v_fp8t
V_CASES = ((1, 1, 1), (1, 2, 63), (2, 1, 64), (1, 3, 65), (1, 2, 1030))


@functools.lru_cache(maxsize=None)
def _v_case(B, H, L):
    """buf [L, B, 3 H 128] float64 (exact bf16 values), the j of every head (None: all zero) and its maximum's row."""
    g = torch.Generator().manual_seed(1000 * B + 100 * H + L)
    buf = (torch.randn(L, B, 3 * H * 128, generator=g) * 2).to(BF16).double()
    v = buf[:, :, 2 * H * 128:].view(L, B, H, 128)
    heads = {}
    for b in range(B):
        for h in range(H):
            j = (3 * b + 5 * h + L) % 13 - 6
            row = {0: min(1027, L - 1), 1: min(3, L - 1)}.get(h, L // 2)
            if (b, h) == (B - 1, H - 1) and B * H > 1 and L != 1030:
                v[:, b, h] = 0
                heads[b, h] = (None, None)
                continue
            v[:, b, h] = _hard_values(g, L * 128, j, cover=False).view(L, 128)
            v[row, b, h, int(torch.randint(0, 128, (1,), generator=g))] = -448.0 * 2.0 ** j
            heads[b, h] = (j, row)
    return buf, heads


def _v_expected(B, H, L):
    buf, heads = _v_case(B, H, L)
    v = buf[:, :, 2 * H * 128:].view(L, B, H, 128)
    nt = (L + 63) // 64
    amax = torch.zeros(B * H, dtype=torch.float64)
    scaled = torch.zeros(B, nt * 64, H, 128, dtype=torch.float64)
    for (b, h), (j, _) in heads.items():
        if j is not None:
            amax[b * H + h] = 448.0 * 2.0 ** j
            scaled[b, :L, h] = v[:, b, h] * 2.0 ** -j
    perm = torch.tensor([_vt_key(p) for p in range(64)])
    tiles = scaled.view(B, nt, 64, H, 128)[:, :, perm]  # [B, nt, 64 p, H, 128 d]
    return amax.float(), e4m3_round(tiles.permute(0, 3, 1, 4, 2).contiguous())  # [B, H, nt, d, p]


def test_premise_v():
    assert sorted(_vt_key(p) for p in range(64)) == list(range(64))
    for B, H, L in V_CASES:
        buf, heads = _v_case(B, H, L)
        assert torch.equal(buf.to(BF16).double(), buf)
        v = buf[:, :, 2 * H * 128:].view(L, B, H, 128)
        for (b, h), (j, row) in heads.items():
            if j is None:
                assert (v[:, b, h] == 0).all()
                continue
            a = v[:, b, h].abs()
            assert a.max() == 448.0 * 2.0 ** j and a[row].max() == a.max()
            inv = torch.tensor(448.0) / a.max().float()  # the kernel's 448 / max(amax, 2^-100): a power of two
            assert inv == 2.0 ** -j
        assert B * H == 1 or L == 1030 or any(j is None for j, _ in heads.values())
    _, heads = _v_case(1, 2, 1030)  # two v_amax_kernel chunks of 1024 rows: one maximum in each
    assert heads[0, 0][1] == 1027 and heads[0, 1][1] == 3


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,L", V_CASES)
def test_cast_v_fp8t_table(device, B, H, L):
    buf, _ = _v_case(B, H, L)
    ref_amax, ref = _v_expected(B, H, L)
    v = buf.to(BF16).to(device)[:, :, 2 * H * 128:].view(L, B, H, 128).transpose(0, 1)
    lib = N.load_library()
    n = lib.cp25_v_fp8t_bytes(B, H, L)
    assert n == B * H * ((L + 63) // 64) * 8192
    obuf, v8t = guarded(n, torch.uint8, device, FILL8)
    abuf, amax = guarded(B * H, torch.float32, device, SENTINEL)
    rc = lib.cp25_cast_v_fp8t(N._ptr(v), N._i64x3((v.stride(0), v.stride(1), v.stride(2))), B, H, L, 128, N._ptr(v8t),
                              N._ptr(amax), N._stream(device))
    torch.cuda.synchronize()
    assert rc == 0
    assert guards_ok(obuf, n, FILL8) and guards_ok(abuf, B * H, SENTINEL)
    assert torch.equal(amax.cpu(), ref_amax)
    got = v8t.cpu().view(ref.shape)
    assert torch.equal(got, ref), _mismatch(got, ref)
    w8, wa = N.cast_v_fp8t(v)
    assert torch.equal(w8.cpu().view(ref.shape), ref) and torch.equal(wa.cpu(), ref_amax)


# ------------------------------------------------------------------------------------------------ host refusals
@pytest.mark.gpu
def test_cast_refusals(device):
    x = torch.zeros(8, 64, dtype=BF16, device=device)
    with pytest.raises(ValueError):  # width no multiple of 16
        N.cast_fp8(x[:, :24], 1.0)
    for sc in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            N.cast_fp8(x, sc)
    with pytest.raises(ValueError):  # dtype
        N.cast_fp8(x.float(), 1.0)
    with pytest.raises(ValueError):  # source base 8 elements in: 16-byte aligned, fine; 4 elements in: not
        N.cast_fp8(x[:, 4:36], 1.0)
    with pytest.raises(ValueError):  # output stride no multiple of 16
        N.cast_fp8(x[:, :32], 1.0, out=torch.zeros(8, 40, dtype=torch.uint8, device=device)[:, :32])
    with pytest.raises(ValueError):  # output of another shape
        N.cast_fp8(x, 1.0, out=torch.zeros(8, 32, dtype=torch.uint8, device=device))
    for K in (0, 256, 1000, 2560, 16384):
        with pytest.raises(ValueError):
            N.quant_fp8_rows(torch.zeros(4, K, dtype=BF16, device=device))
    with pytest.raises(ValueError):
        N.quant_fp8_rows(torch.zeros(4, 1024, dtype=BF16, device=device)[:, :512])
    with pytest.raises(ValueError):
        N.cast_v_fp8t(torch.zeros(1, 8, 2, 64, dtype=BF16, device=device))  # head dim
    with pytest.raises(ValueError):
        N.cast_v_fp8t(torch.zeros(1, 8, 2, 128, dtype=torch.float16, device=device))
    with pytest.raises(ValueError):  # a key stride of 132 elements is no multiple of 8
        N.cast_v_fp8t(torch.zeros(1, 8, 2, 132, dtype=BF16, device=device)[..., :128])
