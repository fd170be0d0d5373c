"""The streaming student's three kernels (csrc/stream_ops.hip) on the device, bit for bit.

* cp25_stream_patchify_ld / cp25_stream_x0_step against tests/stream_truth.py's bf16 restatement (every torch op of
  denoise_edm_seq / generate_next_frame as fp32 math + one bf16 rounding; the operand-by-operand derivation is in that
  module's docstring): out_ld 72 / 128, both scalings, sigma_data 1 / 0.5 / 0.8, the four student times, the last step
  and t = 0 (the store pass), hw = 24 (4 x 6 patches) and 320, planted NaN / +-inf, and inputs on which a contracted
  multiply-add rounds differently (counted on the CPU below, and asserted to exist).
  NaNs are compared by position: their bf16 bit pattern is not one value across torch's own CPU conversions.
* the same step against PyTorch's own device bf16 ops on 0-dim / 5-dim bf16 tensors and the Python-float divisor: the
  promotion and the reciprocal-multiply division, witnessed rather than derived.
* cp25_kv_put: the slot's rows equal the source columns, every other row of the cache is untouched, D = 512 and 2048.
"""
import pytest
import torch

import __graft_entry__  # noqa: F401
import stream_truth as st
from cosmos_predict2 import _native as N
from cosmos_predict2 import trigflow

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
GRIDS = {24: (8, 12), 320: (32, 40)}  # hw -> latent (H, W)
TIMES = st.STUDENT_TIMES


def same_bf16(a: torch.Tensor, b: torch.Tensor) -> bool:
    a, b = a.cpu(), b.cpu()
    if a.shape != b.shape or not torch.equal(a.isnan(), b.isnan()):
        return False
    return torch.equal(a.nan_to_num(nan=0.0).view(torch.int16), b.nan_to_num(nan=0.0).view(torch.int16))


@pytest.fixture(scope="module")
def data():
    """Per hw: x / noise bf16 and net fp32 [1, 16, 1, H, W] (never modified), with NaN / +-inf planted in each."""
    out = {}
    for hw, (H, W) in GRIDS.items():
        g = torch.Generator().manual_seed(90 + hw)
        x = torch.randn(1, 16, 1, H, W, generator=g).to(BF16)
        noise = torch.randn(1, 16, 1, H, W, generator=g).to(BF16)
        net = torch.randn(1, 16, 1, H, W, generator=g)  # fp32: the kernel rounds it to bf16 first, as the reference
        for t, at in ((x, 0), (net, 1), (noise, 2)):
            flat = t.view(-1)
            flat[at * 7 + 3] = float("nan")
            flat[at * 7 + 50] = float("inf")
            flat[at * 7 + 97] = float("-inf")
        out[hw] = dict(x=x, noise=noise, net=net, H=H, W=W)
    return out


def _coeffs(t, scaling, sd):
    tt = torch.full((1, 1, 1, 1, 1), t, dtype=BF16)
    return st.edm_coefficients(tt, torch.zeros_like(tt), scaling, sd, 1e-4)


def _rows(t_C_1_H_W):
    return st.to_patch(t_C_1_H_W)


@pytest.mark.parametrize("hw", [24, 320])
@pytest.mark.parametrize("sigma_data", [1.0, 0.5, 0.8])
@pytest.mark.parametrize("scaling", ["rectified_flow", "edm"])
def test_stream_patchify_equals_truth(device, data, scaling, sigma_data, hw):
    d = data[hw]
    xp = _rows(d["x"][0]).to(device)
    pad = (torch.arange(hw * 4) % 3 == 0).to(BF16).view(hw, 4)
    times = list(TIMES) + ([0.0] if scaling == "rectified_flow" else [])
    for t in times:
        _, _, c_in, _ = _coeffs(t, scaling, sigma_data)
        assert float(c_in) == trigflow.stream_scaling(t, 0.0, scaling, sigma_data, 1e-4)[2]
        net_in = st.mul(d["x"], c_in)  # x * c_in, bf16
        for mask in (0.0, 1.0):
            ref = st.patch_rows(net_in[0], mask)
            for ld in (72, 128):
                for pm in (None, pad):
                    want = ref.clone()
                    if pm is not None:
                        want[:, 68:72] = pm
                    rows = N.stream_patchify(xp, float(c_in), mask, None if pm is None else pm.to(device), ld=ld)
                    assert rows.shape == (hw, 72) and rows.stride(0) == ld
                    assert same_bf16(rows, want), (t, mask, ld)
                    if ld == 128:
                        full = torch.as_strided(rows, (hw, 128), (128, 1))
                        assert not full[:, 72:].any()


def test_stream_patchify_rejections(device, data):
    xp = _rows(data[24]["x"][0]).to(device)
    with pytest.raises(ValueError):
        N.stream_patchify(xp, 1.0, 0.0, None, ld=96)  # out_ld is 72 or 128
    with pytest.raises(ValueError):
        N.stream_patchify(xp, 0.1, 0.0, None)  # 0.1 is no bf16 value
    with pytest.raises(ValueError):
        N.stream_patchify(xp.float(), 1.0, 0.0, None)


def _x0_truth(d, c_skip, c_out):
    return st.x0_from_net(d["x"], d["net"].to(BF16), c_skip, c_out)


def test_contraction_sensitive_inputs_exist(data):
    """The premise of the exact tests, on the very elements they compare (hw = 320, atan 15 -> atan 5, sigma_data 0.8):
    (a) 7703 of 20480 elements round differently when c_skip x + c_out net is rounded once (what a contracted
    multiply-add chain gives) than under the reference's three separately rounded ops; (b) the reciprocal-multiply
    form of `/ sigma_data` and a true fp32 division agree on all of them: float(0.8)'s fp32 reciprocal is exactly 1.25,
    c * 1.25 is exact in fp32 for a bf16 c, and c / 0.8f lies within a quarter fp32 ulp of it, so both give the same
    fp32 value before the bf16 rounding. The kernel still multiplies by the reciprocal, as the reference's op does;
    the device-torch witness below pins that for every sigma_data."""
    d = data[320]
    c_skip, c_out, _, _ = _coeffs(TIMES[1], "rectified_flow", 0.8)
    x0 = _x0_truth(d, c_skip, c_out)
    fused = (c_skip.double() * d["x"].double() + c_out.double() * d["net"].to(BF16).double()).float().to(BF16)
    ok = ~(x0.isnan() | fused.isnan())
    n_fma = int((x0[ok] != fused[ok]).sum())
    tn = torch.tensor(TIMES[2], dtype=BF16)
    c = st.mul(torch.cos(tn.float()).to(BF16), x0)
    recip, true_div = st.div_scalar(c, 0.8), (c.float() / torch.tensor(0.8, dtype=torch.float32)).to(BF16)
    ok2 = ~(recip.isnan() | true_div.isnan())
    n_div = int((recip[ok2] != true_div[ok2]).sum())
    total = x0.numel()
    print(f"contraction-sensitive: {n_fma} of {total}; division-sensitive (sigma_data 0.8): {n_div} of {total}")
    assert n_fma >= 16 and n_div == 0, (n_fma, n_div, total)


@pytest.mark.parametrize("hw", [24, 320])
@pytest.mark.parametrize("sigma_data", [1.0, 0.5, 0.8])
@pytest.mark.parametrize("scaling", ["rectified_flow", "edm"])
def test_stream_x0_step_equals_truth(device, data, scaling, sigma_data, hw):
    d = data[hw]
    xp, netp, nzp = (_rows(d[k][0]).to(device) for k in ("x", "net", "noise"))
    for s, t in enumerate(TIMES):
        c_skip, c_out, _, _ = _coeffs(t, scaling, sigma_data)
        x0 = _x0_truth(d, c_skip, c_out)
        kw = dict(c_skip=float(c_skip), c_out=float(c_out), sigma_data=sigma_data)
        got = N.stream_x0_step(xp, netp.view(hw, 1, 64), None, cos_next=0.0, sin_next=0.0, last=True, **kw)
        assert got.dtype == BF16 and same_bf16(got, _rows(x0[0])), (t, "last")
        if s + 1 < len(TIMES):
            want = st.renoise(x0, d["noise"], TIMES[s + 1], sigma_data)
            cos_n, sin_n = trigflow.stream_renoise(TIMES[s + 1])
            got = N.stream_x0_step(xp, netp.view(hw, 1, 64), nzp, cos_next=cos_n, sin_next=sin_n, last=False, **kw)
            assert same_bf16(got, _rows(want[0])), (t, "renoise")
            # in place on the state
            buf = xp.clone()
            N.stream_x0_step(buf, netp.view(hw, 1, 64), nzp, cos_next=cos_n, sin_next=sin_n, last=False, out=buf, **kw)
            assert same_bf16(buf, got)
    assert same_bf16(xp, _rows(d["x"][0]))  # the inputs were left alone


@pytest.mark.parametrize("sigma_data", [1.0, 0.5, 0.8])
def test_stream_x0_step_equals_device_torch(device, data, sigma_data):
    """The reference's expressions evaluated by PyTorch's own device kernels on the reference's operand kinds: bf16
    [1,1,1,1,1] coefficient tensors, 0-dim bf16 cos / sin tensors, the Python-float sigma_data."""
    d = data[320]
    x, net, noise = d["x"].to(device), d["net"].to(device).to(BF16), d["noise"].to(device)
    c_skip, c_out, _, _ = _coeffs(TIMES[1], "rectified_flow", sigma_data)
    cos_n, sin_n = trigflow.stream_renoise(TIMES[2])
    x0 = c_skip.to(device) * x + c_out.to(device) * net
    cos_t, sin_t = torch.tensor(cos_n, dtype=BF16, device=device), torch.tensor(sin_n, dtype=BF16, device=device)
    assert cos_t.dim() == 0 and float(cos_t) == cos_n and float(sin_t) == sin_n
    want = cos_t * x0 / sigma_data + sin_t * noise
    assert want.dtype == BF16
    got = N.stream_x0_step(_rows(d["x"][0]).to(device), _rows(d["net"][0]).to(device).view(320, 1, 64),
                           _rows(d["noise"][0]).to(device), c_skip=float(c_skip), c_out=float(c_out), cos_next=cos_n,
                           sin_next=sin_n, sigma_data=sigma_data, last=False)
    assert same_bf16(got, _rows(want[0].cpu()))


@pytest.mark.parametrize("D,H", [(512, 4), (2048, 16)])
@pytest.mark.parametrize("B", [1, 2])
def test_kv_put(device, D, H, B):
    hw, slots = 24, 3
    g = torch.Generator().manual_seed(D + B)
    qkv = torch.randn(hw * B, 3 * D, generator=g).to(BF16).to(device)
    k = torch.full((B, slots * hw, H, D // H), -7.0, dtype=BF16, device=device)
    v = torch.full((B, slots * hw, H, D // H), 9.0, dtype=BF16, device=device)
    N.kv_put(qkv, k, v, B=B, k_col0=D, v_col0=2 * D, row0=hw)  # slot 1
    src = qkv.view(hw, B, 3 * D).transpose(0, 1)  # [B, hw, 3D]
    assert torch.equal(k[:, hw:2 * hw].reshape(B, hw, D), src[:, :, D:2 * D])
    assert torch.equal(v[:, hw:2 * hw].reshape(B, hw, D), src[:, :, 2 * D:])
    for buf, fill in ((k, -7.0), (v, 9.0)):
        assert bool((buf[:, :hw] == fill).all()) and bool((buf[:, 2 * hw:] == fill).all())
    with pytest.raises(ValueError):
        N.kv_put(qkv, k, v, B=B, k_col0=D, v_col0=2 * D, row0=2 * hw + 1)  # past the last slot
    with pytest.raises(ValueError):
        N.kv_put(qkv, k, v, B=B, k_col0=D, v_col0=2 * D + 8, row0=0)  # columns past the row
