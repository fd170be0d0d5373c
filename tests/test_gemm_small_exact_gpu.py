"""cp25_gemm_sm_epi / _res / _hnorm / _qkv (csrc/gemm_small.hip), bit for bit.

Exact product: the integer operands of test_gemm_exact_gpu (a in [-8, 8], w in [-4, 4]) make fp32 accumulation exact in
any order (at K = 8192 the abs-sum bound is 8 * 4 * 8192 = 262 144 < 2^24), so the exact form and every split must equal
the float64 product rounded once to bf16 under torch.equal. test_premise (no GPU) checks the bound, fp32 == fp64 on the
CPU and, at K >= 2048, a non-zero share of exact bf16 ties, per K. One problem per K (320 x 512 x K): the launches are
row / column prefixes of it, M in {1, 15, 16, 17, 64, 65, 320} (one ragged 64-row tile, exactly one, one row more, five
tiles), N in {256, 512}, K in {64, 128, 192, 2048} (both parities of K / 64) and K = 8192 once at M = 65, N = 256,
split in {1, 2, 3, 4, 8} where S <= K / 64 (S = 3 at K = 2048: the ragged runs 11 / 11 / 10; S = 3 at K = 128 is
refused). Every launch writes into a slice of a sentinel-filled buffer with ldc = N + 8; the operand layouts cycle
through test_gemm_exact_gpu's (lda = K + 8, a as the middle column block of [M, 3 K], ldw = K + 8, all of them) in
NaN-filled storage; one case sets a[5, 7] = NaN.

Exact form == today's kernels on any data: standard-normal operands, split = 1, against N.gemm_epi / gemm_epi(GELU) /
gemm_res / gemm_hnorm / gemm_qkv under torch.equal. (The gated residual takes whole tokens, M % B == 0: B = 2 runs at
M = 18 in place of 17.) HNORM / QKV at odd K / 64, which cp25_gemm_hnorm / _qkv refuse and the small family serves:
against N.gemm_epi followed by N.head_rmsnorm_rope, the two ops those kernels are bit-identical to.

Split form's epilogues: on the integer operands the bf16 product is exact whatever the split, so for S in {2, 4} every
epilogue's output must equal the existing kernel's on the same operands.

Split form on real data (320 x 512 x 2048, S in {2, 4, 8}): two runs give the same bits, the first 65 rows equal an
M = 65 run, and the rel-L2 distance to the float64 product is at most 1.1 x N.gemm_epi's on the same data (the
project's truth gate, test_parity_depth_gpu.py; both are dominated by the one bf16 rounding).
"""
import functools

import pytest
import torch

from cosmos_predict2 import _native as N
from test_gemm_exact_gpu import (BF16, NAN, SENT, _assert_exact, _gelu_data, _gen, _hn_data, _ints, _out, _place,
                                 _premise, _product, _res_ref, _untouched)

MS = (1, 15, 16, 17, 64, 65, 320)
NS = (256, 512)
KS = (64, 128, 192, 2048)
SPLITS = (1, 2, 3, 4, 8)
LAYS = ("", "a", "b", "w", "abw")
MAXM, MAXN = 320, 512


def _runs(nk, S):
    """K-tile counts of the S runs (gemm_route.h run_len): the first nk % S runs are one tile longer."""
    return [nk // S + (1 if r < nk % S else 0) for r in range(S)]


@functools.lru_cache(maxsize=None)
def _data(K):
    g = _gen(f"small{K}")
    M, Nn = (65, 256) if K == 8192 else (MAXM, MAXN)
    a, w = _ints(g, -8, 8, (M, K)), _ints(g, -4, 4, (Nn, K))
    d = _product(a, w)
    d.update(a=a.to(BF16), w=w.to(BF16), ref=d["acc"].float().to(BF16))
    return d


@pytest.mark.parametrize("K", KS + (8192,))
def test_premise(K):
    d = _data(K)
    assert d["absum"] <= 8 * 4 * K and 8 * 4 * 8192 == 262144 < 2 ** 24
    rounded, ties = _premise(d, K)
    assert _runs(2048 // 64, 3) == [11, 11, 10] and sum(_runs(K // 64, min(3, K // 64))) == K // 64
    print(f"K={K}: |sum| <= {d['absum']:.0f}, {rounded:.1%} rounded, {ties:.1%} exact bf16 ties")


def _placed(d, device, K):
    """The operands once per layout: a (lda = K, K + 8, middle block of 3 K, ...) and w (ldw = K, K + 8)."""
    av = {lay: _place(d["a"], device, BF16, pad=8 if "a" in lay else 0, block="b" in lay) for lay in ("", "a", "b", "ab")}
    wv = {lay: _place(d["w"], device, BF16, pad=8 if "w" in lay else 0) for lay in ("", "w")}
    return av, wv


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_exact_product(device, K):
    d = _data(K)
    av, wv = _placed(d, device, K)
    ref = d["ref"].to(device)
    i = 0
    for M in MS:
        for Nn in NS:
            for S in SPLITS:
                if S > K // 64:
                    continue
                lay = LAYS[i % len(LAYS)]
                i += 1
                a = av["".join(c for c in lay if c in "ab")][:M]
                w = wv["w" if "w" in lay else ""][:Nn]
                big, out = _out(M, Nn, device, pad=8)
                N.gemm_sm_epi(a, w, out=out, split=S)
                _assert_exact(big, out, ref[:M, :Nn], f"M={M} N={Nn} K={K} S={S} layout '{lay}'")
    assert i >= len(LAYS)


@pytest.mark.gpu
def test_exact_product_k8192(device):
    d = _data(8192)
    a, w, ref = d["a"].to(device), d["w"].to(device), d["ref"].to(device)
    for S in SPLITS:
        big, out = _out(65, 256, device, pad=8)
        N.gemm_sm_epi(a, w, out=out, split=S)
        _assert_exact(big, out, ref, f"K=8192 S={S}")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 2, 3])
def test_nan_row(device, S):
    """a[5, 7] = NaN: row 5 is all NaN and every other row exact (rows do not mix, in the tile or in the reduction)."""
    d = _data(2048)
    a, w, ref = d["a"][:17].to(device), d["w"].to(device), d["ref"][:17].to(device)
    a[5, 7] = NAN
    big, out = _out(17, MAXN, device, pad=8)
    N.gemm_sm_epi(a, w, out=out, split=S)
    assert torch.isnan(out[5]).all()
    out[5] = ref[5]
    _assert_exact(big, out, ref, f"nan S={S}")


@pytest.mark.gpu
def test_ragged_split_refused(device):
    d = _data(128)
    a, w = d["a"][:17].to(device), d["w"][:256].to(device)
    big, out = _out(17, 256, device, pad=8)
    with pytest.raises(ValueError):
        N.gemm_sm_epi(a, w, out=out, split=3)  # K / 64 = 2 K-tiles
    torch.cuda.synchronize()
    assert _untouched(big, 0, 0)


# ------------------------------------------------------------------------------------ exact form == today's kernels
def _randn(name, *shape):
    return torch.randn(*shape, generator=_gen(name)).to(BF16)


def _res_operands(name, M, Nn, B, device):
    """x as a column view of a wider [n_tok, B, 2 N] buffer, the gate as the last third of a [B, T, 3 N] modulation."""
    hw, tok0 = 24, 5
    n_tok = M // B
    T = (tok0 + n_tok - 1) // hw + 1
    x = _randn(name + "x", n_tok, B, 2 * Nn).to(device)[..., Nn:]
    gate = _randn(name + "g", B, T, 3 * Nn).to(device)[..., 2 * Nn:]
    return x, gate, dict(B=B, tok0=tok0, hw=hw)


def _same(got, want, what):
    assert torch.equal(got.view(torch.int16), want.view(torch.int16)), \
        f"{what}: {(got.view(torch.int16) != want.view(torch.int16)).sum().item()} of {want.numel()} elements differ"


@pytest.mark.gpu
@pytest.mark.parametrize("K", [128, 2048])
@pytest.mark.parametrize("M", [17, 320])
def test_exact_form_equals_tile256(device, M, K):
    a = _randn(f"eq_a{M}{K}", 320, K)[:M].to(device)
    w = _randn(f"eq_w{K}", 768, K).to(device)
    w512 = w[:512]
    kw = (0.5 + 2.5 * torch.rand(128, generator=_gen("eq_kw"))).to(BF16).to(device)
    for epi in (N.EPI_NONE, N.EPI_GELU):
        big, out = _out(M, 512, device, pad=8)
        N.gemm_sm_epi(a, w512, epilogue=epi, out=out, split=1)
        assert _untouched(big, M, 512)
        _same(out, N.gemm_epi(a, w512, epilogue=epi), f"epilogue {epi}")
    for B in (1, 2):
        Mb = M if M % B == 0 else M + 1  # whole tokens
        ab = _randn(f"eq_a{M}{K}", 320, K)[:Mb].to(device)
        x, gate, kwargs = _res_operands(f"eq_res{M}{K}{B}", Mb, 512, B, device)
        big, out = _out(Mb, 512, device, pad=8)
        N.gemm_sm_res(ab, w512, x, x.stride(0), x.stride(1), gate, out=out, split=1, **kwargs)
        assert _untouched(big, Mb, 512)
        _same(out, N.gemm_res(ab, w512, x, x.stride(0), x.stride(1), gate, **kwargs), f"residual B={B}")
    for scale in (1.0, 0.25):
        big, out = _out(M, 512, device, pad=8)
        N.gemm_sm_hnorm(a, w512, kw, out_scale=scale, out=out, split=1)
        assert _untouched(big, M, 512)
        _same(out, N.gemm_hnorm(a, w512, kw, out_scale=scale), f"hnorm x {scale}")
    for B in (1, 2):
        n_tok = (M + B - 1) // B
        for rope in (True, False):
            cs = {}
            if rope:
                ang = torch.rand(n_tok, 64, generator=_gen(f"eq_rope{M}{B}")) * 6.28
                cs = dict(cos=torch.cos(ang).to(device), sin=torch.sin(ang).to(device))
            big, out = _out(M, 768, device, pad=8)
            N.gemm_sm_qkv(a, w, kw, k_col0=256, k_cols=256, B=B, out=out, split=1, **cs)
            assert _untouched(big, M, 768)
            want = N.gemm_qkv(a, w, kw, k_col0=256, k_cols=256, B=B, **cs)
            assert want is not None
            _same(out, want, f"qkv B={B} rope={rope}")


@pytest.mark.gpu
@pytest.mark.parametrize("S", [1, 3])
def test_hnorm_qkv_odd_k_tiles(device, S):
    """K / 64 = 3: cp25_gemm_hnorm / _qkv refuse it (None), the small family serves it, with the bits of the plain
    product followed by cp25_head_rmsnorm_rope. Integer operands, so S = 3 (one K-tile per run) has the same product."""
    d = _hn_data(192)
    M, Nn = d["a"].shape[0], d["w"].shape[0]
    a, w, kw = d["a"].to(device), d["w"].to(device), d["kw"].to(device)
    cos, sin = d["cos"].to(device), d["sin"].to(device)
    assert N.gemm_hnorm(a, w, kw) is None and N.gemm_qkv(a, w, kw, k_col0=256, k_cols=256, B=1) is None
    want = N.gemm_epi(a, w)
    N.head_rmsnorm_rope(want, n_rows=M, B=1, H=Nn // 128, head_off=0, weight=kw, out_scale=0.25)
    _same(N.gemm_sm_hnorm(a, w, kw, out_scale=0.25, split=S), want, "hnorm")
    want = N.gemm_epi(a, w)
    N.head_rmsnorm_rope(want, n_rows=M, B=1, H=2, head_off=256, weight=kw, cos=cos, sin=sin)
    _same(N.gemm_sm_qkv(a, w, kw, k_col0=256, k_cols=256, B=1, cos=cos, sin=sin, split=S), want, "qkv")


# ------------------------------------------------------------------------------------ the split form's epilogues
@pytest.mark.gpu
@pytest.mark.parametrize("K,S", [(128, 2), (2048, 2), (2048, 4)])
def test_split_epilogues_on_exact_products(device, K, S):
    d = _gelu_data(K)
    a, w = d["a"].to(device), d["w"].to(device)
    M, Nn = a.shape[0], w.shape[0]
    big, out = _out(M, Nn, device, pad=8)
    N.gemm_sm_epi(a, w, epilogue=N.EPI_GELU, out=out, split=S)
    assert _untouched(big, M, Nn)
    _same(out, N.gemm_epi(a, w, epilogue=N.EPI_GELU), "GELU")

    d = _hn_data(K)
    a, w, kw = d["a"].to(device), d["w"].to(device), d["kw"].to(device)
    M, Nn = a.shape[0], w.shape[0]
    for B in (1, 2):
        x, gate, kwargs = _res_operands(f"split_res{K}{B}", M, Nn, B, device)
        big, out = _out(M, Nn, device, pad=8)
        N.gemm_sm_res(a, w, x, x.stride(0), x.stride(1), gate, out=out, split=S, **kwargs)
        assert _untouched(big, M, Nn)
        _same(out, N.gemm_res(a, w, x, x.stride(0), x.stride(1), gate, **kwargs), f"residual B={B}")
        # and against the documented IEEE sequence on the float64 product
        want = _res_ref(d["ref"], x.cpu(), gate.cpu(), B, kwargs["tok0"], kwargs["hw"]).to(device)
        _same(out, want, f"residual B={B} vs float64")
    big, out = _out(M, Nn, device, pad=8)
    N.gemm_sm_hnorm(a, w, kw, out_scale=0.25, out=out, split=S)
    assert _untouched(big, M, Nn)
    _same(out, N.gemm_hnorm(a, w, kw, out_scale=0.25), "hnorm")
    for B, rope in ((1, True), (2, True), (2, False)):
        n_tok = (M + B - 1) // B
        cs = dict(cos=d["cos"][:n_tok].to(device), sin=d["sin"][:n_tok].to(device)) if rope else {}
        big, out = _out(M, Nn, device, pad=8)
        N.gemm_sm_qkv(a, w, kw, k_col0=256, k_cols=256, B=B, out=out, split=S, **cs)
        assert _untouched(big, M, Nn)
        _same(out, N.gemm_qkv(a, w, kw, k_col0=256, k_cols=256, B=B, **cs), f"qkv B={B} rope={rope}")


# ------------------------------------------------------------------------------------ the split form on real data
@functools.lru_cache(maxsize=None)
def _real():
    a, w = _randn("real_a", 320, 2048), _randn("real_w", 512, 2048)
    return a, w, a.double() @ w.double().t()


def _rel_l2(x, ref):
    return ((x.double().cpu() - ref).norm() / ref.norm()).item()


@pytest.mark.gpu
@pytest.mark.parametrize("S", [2, 4, 8])
def test_split_on_real_data(device, S):
    a_cpu, w_cpu, ref = _real()
    a, w = a_cpu.to(device), w_cpu.to(device)
    one = N.gemm_sm_epi(a, w, split=S)
    two = N.gemm_sm_epi(a, w, split=S)
    _same(one, two, "two runs")
    _same(one[:65], N.gemm_sm_epi(a[:65], w, split=S), "the first 65 rows against an M = 65 run")
    d_split, d_tile = _rel_l2(one, ref), _rel_l2(N.gemm_epi(a, w), ref)
    print(f"S={S}: rel-L2 to float64 {d_split:.6e} (split) {d_tile:.6e} (gemm_epi), ratio {d_split / d_tile:.4f}")
    assert d_split <= 1.1 * d_tile


# ------------------------------------------------------------------------------------ refusals
@pytest.mark.gpu
def test_refusals(device):
    M, Nn, K = 65, 256, 256
    z = lambda *shape, dt=BF16: torch.zeros(*shape, dtype=dt, device=device)  # noqa: E731
    a, w = z(M, K), z(Nn, K)
    big, out = _out(M, Nn, device, pad=8)
    N.gemm_sm_epi(a, w, out=out, split=2)  # the base arguments are accepted
    assert (out == 0).all()
    out.fill_(SENT)
    need = N.gemm_sm_workspace_bytes(M, Nn, K, 2)
    assert need == 2 * M * Nn * 4 and N.gemm_sm_workspace_bytes(M, Nn, K, 1) == 0
    short = torch.empty(need - 16, dtype=torch.uint8, device=device)
    bad = [
        lambda: N.gemm_sm_epi(a.float(), w.float(), out=out, split=1),               # dtype
        lambda: N.gemm_sm_epi(a, z(384, K), out=_out(M, 384, device)[1], split=1),   # N % 256 != 0
        lambda: N.gemm_sm_epi(z(M, 96), z(Nn, 96), out=out, split=1),                # K % 64 != 0
        lambda: N.gemm_sm_epi(a, w, out=out, split=5),                               # S > K / 64
        lambda: N.gemm_sm_epi(a, w, out=out, split=2, workspace=short),              # a short workspace
        lambda: N.gemm_sm_epi(a, w, epilogue=N.EPI_RES, out=out, split=1),           # its operands: gemm_sm_res
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            raise AssertionError(f"refusal {i} was accepted")
    torch.cuda.synchronize()
    assert _untouched(big, 0, 0), "a refused call wrote"
