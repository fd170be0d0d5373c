"""cp25_patchify(_ld), cp25_cfg_velocity and cp25_copy_rows in every mode, bit for bit, and the host refusals of the DiT
row and pointwise entry points.

The three kernels are plain IEEE fp32 sequences (dit_ops.hip compiles with FP contraction off), so every assertion is
torch.equal against the CPU fp32 evaluation of the kernel's op order:
  patchify      xin = fl(fl(gt * m) + fl(x * fl(1 - m))) (x itself without gt), bf16(xin) at feature c * 4 + p of the
                token's row, bf16(m) at 64..67, pad_mask[tok] (or 0) at 68..71, zeros from 72 to ld.
  cfg_velocity  vb = fl(fl(fl(noise - gt) * m) + fl(net * fl(1 - m))) (net itself without gt);
                v = fl(vb0 + fl(g * fl(vb0 - vb1))) (cfg_mode 0), fl(vb1 + ...) (cfg_mode 1), vb0 (B = 1).
  copy_rows     the bytes.
An independent float64 evaluation, rounded once to the output type, is compared wherever test_premise* finds it equal
to the fp32 chain (everywhere for frame masks 0 and 1; a 0.5 mask adds a second rounding).

Geometry: hw = 6; n_tok 1, 6, 27 (27 % 4 = 3: the last workgroup of patchify holds three tokens; 27 * 64 = 6.75
workgroups of cfg_velocity); tok0 0 and 4 (with 4 the first workgroup crosses a frame boundary); frame mask
(1, 0, 0.5, 0, 1, 0.5). ld 72, 80, 128, 200: at 200 lanes 0..63 zero columns 72..135 and 136..199, the fill loop's second
trip. Outputs lie in sentinel-filled buffers with 256 guard elements either side.
"""
import functools

import pytest
import torch

from cosmos_predict2 import _native as N
from test_fp8_cast_exact_gpu import SENTINEL, guarded, guards_ok
from test_gemm_exact_gpu import _to_bf16

BF16 = torch.bfloat16
HW = 6
FRAME_MASK = (1.0, 0.0, 0.5, 0.0, 1.0, 0.5)
GEOMETRY = [(n, t0) for n in (1, 6, 27) for t0 in (0, 4)]
LDS = (72, 80, 128, 200)
GUIDANCE = (0.0, 7.0, -1.5)


@functools.lru_cache(maxsize=None)
def _latents(n_tok, tok0):
    g = torch.Generator().manual_seed(100 * n_tok + tok0)
    d = {k: torch.randn(n_tok, 64, generator=g) for k in ("xs", "gt", "noise")}
    d["net"] = torch.randn(n_tok, 2, 64, generator=g)
    d["pad"] = torch.randn(n_tok, 4, generator=g).to(BF16)
    d["fm"] = torch.tensor(FRAME_MASK)
    d["m"] = d["fm"][(tok0 + torch.arange(n_tok)) // HW][:, None]  # [n_tok, 1]
    return d


def _rows72(xin_bf16, m, pad, ld):
    n = xin_bf16.shape[0]
    ref = torch.zeros(n, ld, dtype=BF16)
    ref[:, :64] = xin_bf16.view(n, 4, 16).transpose(1, 2).reshape(n, 64)  # [p, c] -> c * 4 + p
    ref[:, 64:68] = m.to(BF16)
    if pad is not None:
        ref[:, 68:72] = pad
    return ref


def _patchify_ref(n_tok, tok0, with_gt, with_pad, ld, f64=False):
    d = _latents(n_tok, tok0)
    pad = d["pad"] if with_pad else None
    if f64:
        x, gt, m = d["xs"].double(), d["gt"].double(), d["m"].double()
        return _rows72(_to_bf16(gt * m + x * (1 - m) if with_gt else x), d["m"], pad, ld)
    x, gt, m = d["xs"], d["gt"], d["m"]
    return _rows72(((gt * m) + (x * (1 - m)) if with_gt else x).to(BF16), m, pad, ld)


def _cfg_ref(n_tok, tok0, B, mode, guidance, with_gt, f64=False):
    d = _latents(n_tok, tok0)
    cast = (lambda t: t.double()) if f64 else (lambda t: t)
    net, m = cast(d["net"][:, :B]), cast(d["m"])
    g = cast(torch.tensor(guidance, dtype=torch.float32))
    if with_gt:
        vb = [(cast(d["noise"]) - cast(d["gt"])) * m + net[:, b] * (1 - m) for b in range(B)]
    else:
        vb = [net[:, b] for b in range(B)]
    if B == 1:
        v = vb[0]
    else:
        v = (vb[0] if mode == 0 else vb[1]) + g * (vb[0] - vb[1])
    return v.float()


def test_premise_patchify():
    for n_tok, tok0 in GEOMETRY:
        d = _latents(n_tok, tok0)
        assert (tok0 + n_tok - 1) // HW < len(FRAME_MASK)
        for with_gt in (False, True):
            r32, r64 = _patchify_ref(n_tok, tok0, with_gt, True, 72), _patchify_ref(n_tok, tok0, with_gt, True, 72, f64=True)
            whole = ((d["m"] == 0) | (d["m"] == 1)).expand(n_tok, 72)
            assert torch.equal(r32[whole], r64[whole])  # one rounding in both
            assert (r32 == r64).float().mean() >= 0.99
    assert {float(_latents(27, 4)["m"][i]) for i in range(27)} == {0.0, 0.5, 1.0}
    assert _latents(27, 4)["m"][0] != _latents(27, 4)["m"][2]  # tokens 4..7: frames 0 and 1 in one workgroup
    assert 72 + 64 + 63 < 200 <= 72 + 2 * 64  # ld = 200: every lane makes two trips of the zero fill and no third


def test_premise_cfg():
    for n_tok, tok0 in GEOMETRY:
        m = _latents(n_tok, tok0)["m"]
        whole = ((m == 0) | (m == 1)).expand(n_tok, 64)
        for B in (1, 2):
            for mode in (0, 1):
                r32, r64 = _cfg_ref(n_tok, tok0, B, mode, 0.0, True), _cfg_ref(n_tok, tok0, B, mode, 0.0, True, f64=True)
                if B == 1 or mode == 0:  # guidance 0 leaves vb0, one rounding; mode 1 adds fl(vb1 + 0 * ...) = vb1
                    assert torch.equal(r32[whole], r64[whole])
                for gd in GUIDANCE:
                    a, b = _cfg_ref(n_tok, tok0, B, mode, gd, False), _cfg_ref(n_tok, tok0, B, mode, gd, False, f64=True)
                    assert torch.equal(a, b) if B == 1 or gd == 0.0 else (a - b).abs().max() <= 2e-6 * b.abs().max()


def _dev(d, device, *keys):
    return [d[k].to(device) for k in keys]


@pytest.mark.gpu
@pytest.mark.parametrize("ld", LDS)
@pytest.mark.parametrize("n_tok,tok0", GEOMETRY)
def test_patchify_modes(device, n_tok, tok0, ld):
    d = _latents(n_tok, tok0)
    xs, gt, fm, pad = _dev(d, device, "xs", "gt", "fm", "pad")
    lib = N.load_library()
    for with_gt in (False, True):
        for with_pad in (False, True):
            buf, flat = guarded(n_tok * ld, BF16, device, SENTINEL)
            args = (N._ptr(xs), N._ptr(gt) if with_gt else None, N._ptr(fm), N._ptr(pad) if with_pad else None, N._ptr(flat))
            if ld == 72:
                rc = lib.cp25_patchify(*args, n_tok, tok0, HW, N._stream(device))
            else:
                rc = lib.cp25_patchify_ld(*args, ld, n_tok, tok0, HW, N._stream(device))
            torch.cuda.synchronize()
            assert rc == 0
            assert guards_ok(buf, n_tok * ld, SENTINEL), "wrote outside the rows"
            got = flat.cpu().view(n_tok, ld)
            ref = _patchify_ref(n_tok, tok0, with_gt, with_pad, ld)
            assert torch.equal(got[:, 72:], torch.zeros(n_tok, ld - 72, dtype=BF16))
            assert torch.equal(got, ref), (with_gt, with_pad, (got != ref).nonzero()[:6].tolist())
            r64 = _patchify_ref(n_tok, tok0, with_gt, with_pad, ld, f64=True)
            assert torch.equal(got[r64 == ref], r64[r64 == ref])
            # the wrapper returns the same rows
            w = N.patchify(xs, gt if with_gt else None, fm, pad if with_pad else None, tok0=tok0, hw=HW, ld=ld)
            assert w.shape == (n_tok, 72) and w.stride(0) == ld and torch.equal(w.cpu(), ref[:, :72])


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("n_tok,tok0", GEOMETRY)
def test_cfg_velocity_modes(device, n_tok, tok0, B):
    d = _latents(n_tok, tok0)
    noise, gt, fm = _dev(d, device, "noise", "gt", "fm")
    net = d["net"][:, :B].contiguous().to(device)
    lib = N.load_library()
    for mode in (0, 1):
        for gd in GUIDANCE:
            for with_gt in (False, True):
                buf, out = guarded(n_tok * 64, torch.float32, device, SENTINEL)
                opt = (N._ptr(noise), N._ptr(gt), N._ptr(fm)) if with_gt else (None, None, None)
                rc = lib.cp25_cfg_velocity(N._ptr(net), B, *opt, gd, mode, N._ptr(out), n_tok, tok0, HW, N._stream(device))
                torch.cuda.synchronize()
                assert rc == 0
                assert guards_ok(buf, n_tok * 64, SENTINEL)
                got = out.cpu().view(n_tok, 64)
                ref = _cfg_ref(n_tok, tok0, B, mode, gd, with_gt)
                assert torch.equal(got, ref), (mode, gd, with_gt, (got != ref).nonzero()[:6].tolist())
                r64 = _cfg_ref(n_tok, tok0, B, mode, gd, with_gt, f64=True)
                assert torch.equal(got[r64 == ref], r64[r64 == ref])
                if with_gt:
                    w = N.cfg_velocity(net, noise, gt, fm, gd, mode, tok0=tok0, hw=HW)
                else:
                    w = N.cfg_velocity(net, None, None, None, gd, mode, tok0=tok0, hw=HW)
                assert torch.equal(w.cpu(), ref)


COPY_CASES = [(8, 300), (1024, 3)]  # 300 and 384 threads: the last workgroup is partly idle


def test_premise_copy():
    for width, n_rows in COPY_CASES:
        assert n_rows * width // 8 % 256 != 0


@pytest.mark.gpu
@pytest.mark.parametrize("offset", ["off0", "offD"])
@pytest.mark.parametrize("width,n_rows", COPY_CASES)
def test_copy_rows(device, width, n_rows, offset):
    off = 0 if offset == "off0" else width
    ss, ds = 2 * width + 8, width + 16
    g = torch.Generator().manual_seed(width)
    src = torch.randint(-2 ** 15, 2 ** 15, (n_rows, ss), generator=g, dtype=torch.int16)  # every bit pattern, NaN too
    buf, flat = guarded(n_rows * ds, BF16, device, SENTINEL)
    N.copy_rows(src.view(BF16).to(device), ss, flat, ds, n_rows, width, src_offset=off)
    torch.cuda.synchronize()
    assert guards_ok(buf, n_rows * ds, SENTINEL)
    got = flat.cpu().view(n_rows, ds)
    assert torch.equal(got[:, :width].view(torch.int16), src[:, off:off + width])
    assert torch.equal(got[:, width:], torch.full((n_rows, ds - width), SENTINEL, dtype=BF16)), "wrote between the rows"


# ------------------------------------------------------------------------------------------------ host refusals
def _refused(fn, *a, **kw):
    with pytest.raises(ValueError):
        fn(*a, **kw)


@pytest.mark.gpu
def test_ln_mod_refusals(device):
    n, B, D, T, hw = 4, 2, 512, 2, 2
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=device)
    x, y, mods = z(n, B, D), z(n, B, D), z(B, T, 3 * D)
    sh, sc, gt = mods[..., :D], mods[..., D:2 * D], mods[..., 2 * D:]
    kw = dict(n_tok=n, B=B, tok0=0, hw=hw, x_st=B * D, x_sb=D)
    for fp8 in (False, True):
        m768 = z(B, T, 3 * 768)
        _refused(N.ln_mod, z(n, B, 768), m768[..., :768], m768[..., 768:1536], fp8=fp8, **dict(kw, x_st=B * 768, x_sb=768))
        _refused(N.ln_mod, x, sh, z(B, T, D), fp8=fp8, **kw)                     # shift / scale strides differ
        _refused(N.ln_mod, x, sh, sc, y=y, gate=z(B, T, D), x_out=z(n, B, D), fp8=fp8, **kw)  # gate strides differ
        _refused(N.ln_mod, x, sh, sc, fp8=fp8, **dict(kw, tok0=1))                # token 4 is in frame 2 of 2
        _refused(N.ln_mod, x, sh, sc, fp8=fp8, **dict(kw, hw=0))
        _refused(N.ln_mod, x, mods[:1, :, :D], mods[:1, :, D:2 * D], fp8=fp8, **kw)  # modulation for one batch of two
        _refused(N.ln_mod, x, sh, sc, y=y, gate=gt, fp8=fp8, **kw)                # a residual needs x_out
        _refused(N.ln_mod, x, sh, sc, fp8=fp8, **dict(kw, n_tok=0))
        # 16-byte accesses: pointers and strides
        big = z(n * B * D + 8)
        _refused(N.ln_mod, big[4:4 + n * B * D].view(n, B, D), sh, sc, fp8=fp8, **kw)
        _refused(N.ln_mod, x, sh, sc, fp8=fp8, **dict(kw, x_st=B * D + 4))
        _refused(N.ln_mod, x, sh, sc, fp8=fp8, **dict(kw, x_sb=D + 4))
        m4 = z(B, T, 3 * D + 4)
        _refused(N.ln_mod, x, m4[..., :D], m4[..., D:2 * D], fp8=fp8, **kw)       # modulation strides 3 D + 4
        m8 = z(B, T, 3 * D + 8)
        _refused(N.ln_mod, x, m8[..., 4:D + 4], m8[..., D + 4:2 * D + 4], fp8=fp8, **kw)  # modulation base 8 bytes in
        _refused(N.ln_mod, x, sh, sc, y=big[4:4 + n * B * D].view(n, B, D), gate=gt, x_out=z(n, B, D), fp8=fp8, **kw)
        _refused(N.ln_mod, x, sh, sc, y=y, gate=gt, x_out=big[4:4 + n * B * D].view(n, B, D), fp8=fp8, **kw)
    _refused(N.ln_mod, x, sh, sc, h_out=z(n * B * D + 8)[4:4 + n * B * D].view(n, B, D), **kw)


@pytest.mark.gpu
def test_final_ln_mod_refusals(device):
    n, B, D, T, hw = 4, 2, 512, 2, 2
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=device)
    x, y, gm = z(n, B, D), z(n, B, D), z(B, T, 3 * D)
    f = z(B, T, 2 * D, dt=torch.float32)
    sh, sc = f[..., :D], f[..., D:]
    kw = dict(n_tok=n, B=B, tok0=0, hw=hw)
    f768 = z(B, T, 2 * 768, dt=torch.float32)
    _refused(N.final_ln_mod, z(n, B, 768), f768[..., :768], f768[..., 768:], **kw)
    _refused(N.final_ln_mod, x, sh, z(B, T, D, dt=torch.float32), **kw)            # shift / scale strides differ
    _refused(N.final_ln_mod, x, sh, sc, **dict(kw, tok0=1))
    _refused(N.final_ln_mod, x, sh, sc, y=y, gate=gm[:, :1, 2 * D:], **kw)         # the gate has one frame of two
    _refused(N.final_ln_mod, x, sh, sc, y=y, **kw)                                  # a residual needs its gate
    _refused(N.final_ln_mod, x, sh, sc, **dict(kw, n_tok=0))
    big = z(n * B * D + 8)
    _refused(N.final_ln_mod, big[4:4 + n * B * D].view(n, B, D), sh, sc, **kw)
    _refused(N.final_ln_mod, x, sh, sc, y=big[4:4 + n * B * D].view(n, B, D), gate=gm[..., 2 * D:], **kw)
    g4 = z(B, T, D + 4)
    _refused(N.final_ln_mod, x, sh, sc, y=y, gate=g4[..., :D], **kw)                # gate strides D + 4
    g8 = z(B, T, D + 8)
    _refused(N.final_ln_mod, x, sh, sc, y=y, gate=g8[..., 4:D + 4], **kw)           # gate base 8 bytes in


@pytest.mark.gpu
def test_layer_norm_refusals(device):
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=device)
    D = 512
    w, b = z(D), z(D)
    _refused(N.layer_norm, z(4, 768), z(768), z(768))
    _refused(N.layer_norm, z(4, D, dt=torch.float32), w, b)
    _refused(N.layer_norm, z(4, D), w.float(), b)
    _refused(N.layer_norm, z(4, D), z(D + 8), b)
    _refused(N.layer_norm, z(4, D), z(2 * D)[::2], b)
    _refused(N.layer_norm, z(4, D + 4)[:, :D], w, b)                  # row stride D + 4
    _refused(N.layer_norm, z(4, D + 8)[:, 4:D + 4], w, b)             # rows 8 bytes in
    _refused(N.layer_norm, z(4, D), w, b, out=z(4, D + 4)[:, :D])
    _refused(N.layer_norm, z(4, D), w, b, out=z(4, D + 8)[:, 4:D + 4])
    _refused(N.layer_norm, z(4, D), z(D + 8)[4:D + 4], b)             # weight 8 bytes in
    _refused(N.layer_norm, z(4, D), w, z(D + 8)[4:D + 4])
    _refused(N.layer_norm, z(0, D), w, b)


@pytest.mark.gpu
def test_head_rmsnorm_rope_refusals(device):
    z = lambda *s, dt=BF16: torch.zeros(*s, dtype=dt, device=device)
    H, n = 2, 6
    buf, w = z(n, H * 128), z(128)
    cos = z(n, 64, dt=torch.float32)
    kw = dict(n_rows=n, B=1, H=H, head_off=0, weight=w)
    _refused(N.head_rmsnorm_rope, z(n, H * 128 + 4)[:, :H * 128], **kw)            # row stride
    _refused(N.head_rmsnorm_rope, z(n, H * 128 + 8), **dict(kw, head_off=4))
    _refused(N.head_rmsnorm_rope, buf, cos=cos, **kw)                              # cos without sin
    _refused(N.head_rmsnorm_rope, buf, sin=cos, **kw)
    _refused(N.head_rmsnorm_rope, buf, **dict(kw, n_rows=0))
    _refused(N.head_rmsnorm_rope, buf, **dict(kw, H=0))
    _refused(N.head_rmsnorm_rope, buf, **dict(kw, B=0))
    _refused(N.head_rmsnorm_rope, buf, norm_max=z(64, 16, dt=torch.float32), **kw)
    _refused(N.head_rmsnorm_rope, buf, norm_max=z(64, 32), **kw)
    _refused(N.head_rmsnorm_rope, buf, norm_max=z(64, 64, dt=torch.float32)[:, :32], **kw)
    slots = z(64, 32, dt=torch.float32)
    for nm in (None, slots):  # 16-byte accesses, with and without the slots
        _refused(N.head_rmsnorm_rope, z(n, H * 128 + 8)[:, 4:H * 128 + 4], norm_max=nm, **kw)  # rows 8 bytes in
        _refused(N.head_rmsnorm_rope, buf, norm_max=nm, **dict(kw, weight=z(136)[4:132]))
        _refused(N.head_rmsnorm_rope, buf, out2=z(n, H * 128 + 4), out2_stride=H * 128 + 4, norm_max=nm, **kw)
        _refused(N.head_rmsnorm_rope, buf, out2=z(n * H * 128 + 8)[4:], out2_stride=H * 128, norm_max=nm, **kw)
    assert (slots == 0).all() and (buf == 0).all()


@pytest.mark.gpu
def test_pointwise_refusals(device):
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=device)
    n = 8
    xs, fm = z(n, 64), z(2)
    for ld in (70, 76, 64, 0):
        _refused(N.patchify, xs, None, fm, None, tok0=0, hw=4, ld=ld)
    _refused(N.patchify, xs, None, fm, None, tok0=1, hw=4)              # token 8 is in frame 2 of 2
    _refused(N.patchify, xs, None, fm, None, tok0=0, hw=0)
    _refused(N.patchify, xs, None, fm, None, tok0=-1, hw=4)
    _refused(N.patchify, z(0, 64), None, fm, None, tok0=0, hw=4)
    _refused(N.cfg_velocity, z(n, 3, 64), None, None, None, 1.0, 0, tok0=0, hw=4)   # B = 3
    _refused(N.cfg_velocity, z(n, 2, 64), None, z(n, 64), fm, 1.0, 0, tok0=0, hw=4)  # gt without noise
    _refused(N.cfg_velocity, z(n, 2, 64), z(n, 64), z(n, 64), None, 1.0, 0, tok0=0, hw=4)
    _refused(N.cfg_velocity, z(n, 2, 64), z(n, 64), z(n, 64), fm, 1.0, 0, tok0=4, hw=4)
    _refused(N.cfg_velocity, z(n, 2, 64), None, None, None, 1.0, 0, tok0=0, hw=0)
    # copy_rows
    src, dst = z(4, 64, dt=BF16), z(4, 64, dt=BF16)
    _refused(N.copy_rows, src, 64, dst, 64, 4, 12)
    _refused(N.copy_rows, src, 60, dst, 64, 4, 8)
    _refused(N.copy_rows, src, 64, dst, 60, 4, 8)
    _refused(N.copy_rows, src, 64, dst, 64, 0, 8)
    _refused(N.copy_rows, src, 64, dst, 64, 4, 0)
    _refused(N.copy_rows, src, 64, dst, 64, 3, 8, src_offset=4)          # source 8 bytes in
    _refused(N.copy_rows, src, 64, dst.view(-1)[4:], 64, 3, 8)           # destination 8 bytes in
    assert (dst == 0).all()
    # gelu
    _refused(N.gelu_, z(16))
    _refused(N.gelu_, z(4, 16, dt=BF16)[:, :8])
    _refused(N.gelu_, z(12, dt=BF16))
    _refused(N.gelu_, z(24, dt=BF16)[4:20])                              # 16 elements, 8 bytes in
    _refused(N.gelu_, z(0, dt=BF16))


@pytest.mark.gpu
def test_unipc_refusals(device):
    x = torch.zeros(64, device=device)
    ok = dict(sigma=0.5, use_corr=1, order_c=1, order_p=1)
    for bad in (dict(order_c=0), dict(order_c=3), dict(order_p=0), dict(order_p=3), dict(order_c=-1, order_p=2)):
        with pytest.raises(ValueError):
            N.unipc_step(x, x.clone(), x.clone(), x.clone(), x.clone(), N.UniPCParams(**dict(ok, **bad)))
    with pytest.raises(ValueError):
        N.unipc_step(x, torch.zeros(65, device=device), x.clone(), x.clone(), x.clone(), N.UniPCParams(**ok))
    with pytest.raises(ValueError):
        N.unipc_step(x, x.clone(), x.clone().double(), x.clone(), x.clone(), N.UniPCParams(**ok))
    assert (x == 0).all()
