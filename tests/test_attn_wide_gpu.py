"""attn_fwd_wq (attn_wide.hip: one wave per SIMD, 320 query rows per workgroup) against attn_fwd_m16 on the same
inputs: bit-identical, because both run the same v_mfma_f32_16x16x32_bf16 chains in the same order on the same operands
(attn_wide.hip header). Reference op: networks/attention.py:90-181.

Every case runs the same call under cp25_attn_self_select(0) (attn_fwd_m16 everywhere) and under the forced width and
compares with torch.equal. Covered: the fixed shift (the only mode long-key launches with norm bounds take; both
branches of its rule floor(min(b_row + 60, 126 - b_row)), and rows of one wave on either side of the branch), ragged
query blocks, fewer rows than one wave owns, ragged key tiles on both sides of the 32-key half stage, odd tile counts,
key-range splits down to one tile, the tail split of a partial last round (one round of splits and the wide kernel's
multi-round segments), the in-kernel q RMSNorm with and without RoPE, the DiT's token-major strided views, and the
kernel names the library reports for routed and unrouted launches.
"""
import pytest
import torch

from cosmos_predict2 import _native as N

pytestmark = pytest.mark.gpu

TOL = 4e-3  # tests/test_attn_m16_gpu.py: rel-L2 vs fp32; two roundings of P at different shifts agree within 1.5 x
LOG2E = 1.4426950408889634
C = 128 ** -0.5 * LOG2E
WIDTHS = [320, 384]  # the widths libcp25.so is built with


def rel_l2(a, b):
    a, b = a.float(), b.float()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _rms_rows(t, w):
    tf = t.float()
    return (tf * torch.rsqrt(tf.pow(2).mean(-1, keepdim=True) + 1e-6) * w).to(torch.bfloat16)


def _inputs(device, B, H, Lq, Lk, seed, wlo=0.5, whi=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    w = wlo + (whi - wlo) * torch.rand(128, generator=g)
    q = (_rms_rows(torch.randn(B, Lq, H, 128, generator=g), w).float() * C).to(torch.bfloat16).to(device)
    k = _rms_rows(torch.randn(B, Lk, H, 128, generator=g), w).to(device)
    v = torch.randn(B, Lk, H, 128, generator=g).to(device, torch.bfloat16)
    return q, k, v, w


def _both(fn, width, fn0=None):
    """(fn0 or fn)() under attn_fwd_m16, then fn() under the forced width (the library's form restored afterwards)."""
    prev = N.attn_self_select(0)
    try:
        a = (fn0 or fn)()
        torch.cuda.synchronize()
        N.attn_self_select(width)
        b = fn()
        torch.cuda.synchronize()
    finally:
        N.attn_self_select(prev)
    return a, b


def _modes(q, k):
    """Norm bounds for the fixed shift (every long-key launch with bounds up to a product of 110 runs it). b_row =
    |q_row| x the key bound picks the branch of floor(min(b_row + 60, 126 - b_row)): lo, the data's own norms (b_row
    ~25, below 33: the first branch); mid, the key bound 33 / the median |q_row|, so the rows of one wave straddle 33;
    hi, the key bound 97 / max |q_row|: the longest row has b_row = 97 and every row is past 33 (the second branch)."""
    qr = q.float().norm(dim=-1)
    qn = qr.max().item() * 1.01
    kn = k.float().norm(dim=-1).max().item() * 1.01
    kmid = 33.0 / qr.median().item()
    assert qn * kn < 33.0 and kmid > kn and qn * kmid > 34.0
    return {"lo": (qn, kn), "mid": (qn, kmid), "hi": (qn, 97.0 / qn)}


def _name(width):
    return f"attn_fwd_wq<self, prescaled, {width} rows, fixed shift>"


def _shapes(R):
    return [(1, 2, 513, 4100, 1),       # ragged query block; Lk mod 64 = 4
            (1, 1, 33, 4097 + 40, 1),   # fewer rows than one wave owns; Lk mod 64 = 41
            (2, 2, 1000, 5000, 1),      # odd tile count
            (1, 1, 300, 4097, 65),      # one-tile splits
            (1, 2, 777, 6000, 3),       # key-range splits
            (2, 3, 2 * R, 4160, 2),     # exactly full blocks
            (1, 2, 4800, 4800, 7)]      # config 5's length


CASES = [(R,) + s for R in WIDTHS for s in _shapes(R)]


@pytest.mark.parametrize("R,B,H,Lq,Lk,n_split", CASES)
@pytest.mark.parametrize("mode", ["lo", "mid", "hi"])
def test_wide_bit_identical_to_m16(device, R, B, H, Lq, Lk, n_split, mode):
    q, k, v, _ = _inputs(device, B, H, Lq, Lk, 11 + Lq + Lk + n_split)
    nb = _modes(q, k)[mode]
    prev = N.attn_self_select(R)
    try:
        assert N.attn_kernel_name(Lk, norm_bounds=nb, prescaled=True) == _name(R)
        assert N.attn_kernel_name(Lk, norm_bounds=nb, prescaled=2) == _name(R)  # key slots given, not gated
    finally:
        N.attn_self_select(prev)
    a, b = _both(lambda: N.attn_fwd(q, k, v, prescaled=True, n_split=n_split, norm_bounds=nb), R)
    assert torch.isfinite(b.float()).all()
    assert torch.equal(a, b), (R, B, H, Lq, Lk, n_split, mode, (a.float() - b.float()).abs().max().item())


def test_kernel_names(device):
    """The default routing sends fixed-shift long-key launches to attn_fwd_wq (384 rows; 320 up to 8192 keys);
    online-max, gated, fp8, unscaled and short-key launches stay on attn_fwd_m16 / attn_fwd_f8 under every form."""
    prev = N.attn_self_select(1)
    try:
        # the library's routing: 384 rows past 8192 keys, 320 rows up to there
        assert N.attn_kernel_name(109120, norm_bounds=(1.5, 11.6), prescaled=True) == _name(384)
        assert N.attn_kernel_name(8193, norm_bounds=(1.5, 11.6), prescaled=True) == _name(384)
        assert N.attn_kernel_name(8192, norm_bounds=(1.5, 11.6), prescaled=True) == _name(320)
        assert N.attn_kernel_name(4097, norm_bounds=(8.0, 13.0), prescaled=True) == _name(320)  # product 104
        for form in (1, 320, 384):
            assert N.attn_self_select(form) in (1, 320, 384)
            if form != 1:
                assert N.attn_kernel_name(109120, norm_bounds=(1.5, 11.6), prescaled=True) == _name(form)
                assert N.attn_kernel_name(4097, norm_bounds=(8.0, 13.0), prescaled=True) == _name(form)
            assert N.attn_kernel_name(109120, prescaled=True) == "attn_fwd_m16<self, prescaled, online max>"
            assert N.attn_kernel_name(109120, norm_bounds=(9.0, 12.5), prescaled=True) == \
                "attn_fwd_m16<self, prescaled, online max>"  # bound product 112.5 > 110
            assert N.attn_kernel_name(109120, norm_bounds=(4.4, 34.6), prescaled=2).startswith("attn_fwd_m16<self")
            assert "gated" in N.attn_kernel_name(109120, norm_bounds=(4.4, 34.6), prescaled=2)
            assert N.attn_kernel_name(109120, norm_bounds=(1.5, 11.6)).startswith("attn_fwd_m16<self")  # not prescaled
            assert N.attn_kernel_name(4096, norm_bounds=(1.5, 11.6), prescaled=True).startswith("attn_fwd_m16<cross")
            assert N.attn_kernel_name(109120, norm_bounds=(1.5, 11.6), prescaled=True, fp8=1).startswith("attn_fwd_f8")
        N.attn_self_select(0)
        assert N.attn_kernel_name(109120, norm_bounds=(1.5, 11.6), prescaled=True) == \
            "attn_fwd_m16<self, prescaled, fixed shift>"
        with pytest.raises(Exception):
            N.attn_self_select(2)
        assert N.attn_self_select(1) == 0  # the refused value left the form as it was
    finally:
        N.attn_self_select(prev)


def _tail_case(device, R, B, H, Lq, Lk, t0, mode, seed):
    """The library's plan under the forced width against attn_fwd_m16's whole launch (n_split = 1): rows the plan
    computes whole ((b, h) before the last, and the last one's rows below t0) bit for bit, the tail segment's rows
    (merged key splits, each split with its own rounding of P) within 1.5 TOL and not identical."""
    q, k, v, _ = _inputs(device, B, H, Lq, Lk, seed)
    nb = _modes(q, k)[mode]
    prev = N.attn_self_select(R)
    try:
        assert N.load_library().cp25_attn_tail_workspace_bytes(B, H, Lq, Lk) > 0  # the plan has a tail here
    finally:
        N.attn_self_select(prev)
    whole, tail = _both(lambda: N.attn_fwd(q, k, v, prescaled=True, norm_bounds=nb), R,
                        lambda: N.attn_fwd(q, k, v, prescaled=True, norm_bounds=nb, n_split=1))
    assert torch.equal(tail[:, :, :H - 1], whole[:, :, :H - 1])
    assert torch.equal(tail[-1, :t0, H - 1], whole[-1, :t0, H - 1])
    if B > 1:
        assert torch.equal(tail[:-1, :, H - 1], whole[:-1, :, H - 1])
    e = rel_l2(tail[-1, t0:, H - 1], whole[-1, t0:, H - 1])
    print(f"width {R} {mode}: tail rows {t0}..{Lq} of the last head vs the whole launch: rel-L2 {e:.3e}")
    assert 0 < e <= 1.5 * TOL, e


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("mode", ["lo", "hi"])
def test_wide_tail_split_one_round(device, R, mode):
    """29 query blocks x enough heads to pass the device's CU count (256 CUs: 9 heads, 261 workgroups): the last few
    blocks of the last head run as key-range segments that fit one round (attn_fwd_wq<.., tail>), merged."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    nqb = 29
    H = cus // nqb + 1
    r = nqb * H - cus
    L = nqb * R - 100
    assert N.attn_plan(1, H, L, L, 128) == 1
    _tail_case(device, R, 1, H, L, L, (nqb - r) * R, mode, 5)


@pytest.mark.parametrize("R", WIDTHS)
def test_wide_tail_split_multi_round(device, R):
    """The metric launch's last round in small: 160 workgroups of one (b, h) past whole rounds (2 heads x (CUs + 160) / 2
    query blocks), too many for one round of splits. The wide kernel's plan runs them as 3 key splits in two rounds."""
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    if (cus + 160) % 2:
        pytest.skip("odd CU count")
    nqb = (cus + 160) // 2
    Lq, Lk = nqb * R - 100, 65536
    _tail_case(device, R, 1, 2, Lq, Lk, (nqb - 160) * R, "lo", 6)


@pytest.mark.parametrize("R", WIDTHS)
@pytest.mark.parametrize("rope", [True, False])
def test_wide_in_kernel_qnorm_bit_identical(device, R, rope):
    """cp25_attn_fwd_prescaled_qnorm: q raw, the kernel normalises (RMSNorm + RoPE + prescale) its own fragments. With
    bounds the launch is routed (fixed shift); without it is online and runs on attn_fwd_m16 under every form."""
    B, H, L = 2, 2, 5000
    g = torch.Generator(device="cpu").manual_seed(9)
    w = (0.5 + torch.rand(128, generator=g)).to(torch.bfloat16)
    q = torch.randn(B, L, H, 128, generator=g).to(device, torch.bfloat16)
    k = _rms_rows(torch.randn(B, L, H, 128, generator=g), w.float()).to(device)
    v = torch.randn(B, L, H, 128, generator=g).to(device, torch.bfloat16)
    ang = torch.rand(L, 64, generator=g) * 50.0
    qn = dict(weight=w.to(device), cos=torch.cos(ang).to(device) if rope else None,
              sin=torch.sin(ang).to(device) if rope else None, out_scale=C)
    wb = 128 ** 0.5 * float(w.float().abs().max()) * 1.02
    prev = N.attn_self_select(R)
    try:
        assert N.attn_kernel_name(L, norm_bounds=(wb * C, wb), prescaled=True) == _name(R)
        assert N.attn_kernel_name(L, prescaled=True) == "attn_fwd_m16<self, prescaled, online max>"
    finally:
        N.attn_self_select(prev)
    for nb in ((wb * C, wb), None):
        a, b = _both(lambda: N.attn_fwd(q, k, v, prescaled=True, norm_bounds=nb, q_norm=qn, n_split=1), R)
        assert torch.isfinite(b.float()).all()
        assert torch.equal(a, b)


@pytest.mark.parametrize("R", WIDTHS)
def test_wide_token_major_views(device, R):
    """q / k / v as strided views of the DiT's fused [L, B, 3, H, 128] buffer, the output into a strided view."""
    L, B, H = 4500, 2, 4
    g = torch.Generator(device="cpu").manual_seed(17)
    w = 0.5 + torch.rand(128, generator=g)
    qkv = _rms_rows(torch.randn(L, B, 3, H, 128, generator=g), w)
    qkv[:, :, 0] = (qkv[:, :, 0].float() * C).to(torch.bfloat16)
    qkv = qkv.to(device)
    q, k, v = (qkv[:, :, i].transpose(0, 1) for i in range(3))
    nb = (q.float().norm(dim=-1).max().item() * 1.01, k.float().norm(dim=-1).max().item() * 1.01)
    prev = N.attn_self_select(R)
    try:
        assert N.attn_kernel_name(L, norm_bounds=nb, prescaled=True) == _name(R)
    finally:
        N.attn_self_select(prev)

    def run():
        out = torch.full((L, B, 2, H, 128), 7.0, device=device, dtype=torch.bfloat16)
        N.attn_fwd(q, k, v, out=out[:, :, 1].transpose(0, 1), prescaled=True, norm_bounds=nb, n_split=1)
        return out
    a, b = _both(run, R)
    assert (b[:, :, 0] == 7.0).all()  # nothing written outside the view
    assert torch.equal(a, b)
