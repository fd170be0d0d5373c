"""cp25_ln_mod_cam / cp25_ln_mod_cam_fp8 against cp25_ln_mod, bit for bit.

The camera kernel is ln_mod_kernel with one more operand: h = bf16(h_ln_mod + cam), one IEEE fp32 add of two bf16
values and one rounding on top of a kernel that tests/test_dit_rows_exact_gpu.py already pins to the reference's
op sequence. So for every case
    h_cam  == (N.ln_mod(same args).float() + cam.float()).to(bf16)       (right-hand side computed on the device)
    x_out  == N.ln_mod's x_out
    fp8    == N.quant_fp8_rows of that bf16 h, codes and scales
and the outputs are slices of sentinel-filled buffers whose guards stay untouched.

Cases: every template width D / 512 in {1, 2, 4, 8, 10}; (n_tok, B) in {(1, 1), (7, 1), (5, 3), (9, 2)} (rows % 4 in
{1, 3, 3, 2}: the last workgroup's `row >= n_rows` exit); hw = 4; tok0 in {0, 3, 6}; the residual on and off; cam
shared (cam_sb = 0) and per entry; cam_st D and D + 64 (a column view of a wider buffer); x broadcast over B
(x_sb = 0). Each D x rows x residual cell is one test; the other options rotate with the cell's indices so that each
value meets each width.
"""
import dataclasses
import zlib

import pytest
import torch

from cosmos_predict2 import _native as N
from test_fp8_cast_exact_gpu import FILL8, SENTINEL, guarded, guards_ok

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
HW = 4
T_FRAMES = 4  # (6 + 9 - 1) // 4 + 1
WIDTHS = (512, 1024, 2048, 4096, 5120)
ROWSETS = ((1, 1), (7, 1), (5, 3), (9, 2))


@dataclasses.dataclass(frozen=True)
class Case:
    D: int
    n_tok: int
    B: int
    tok0: int
    res: bool
    per_entry: bool  # cam [n_tok, B, .] with its own row per batch entry, else cam_sb = 0
    wide: bool       # cam_st = D + 64
    bcast: bool      # x [n_tok, 1, D], x_sb = 0

    def __str__(self):
        tag = "_res" * self.res + "_perb" * self.per_entry + "_wide" * self.wide + "_bcast" * self.bcast
        return f"d{self.D}_n{self.n_tok}_b{self.B}_t{self.tok0}{tag}"


CASES = [Case(D, n, B, (0, 3, 6)[(i + j + r) % 3], bool(r), bool((i + j) % 2), bool((i + j // 2 + r) % 2),
              bool((i + r + j // 2 + 1) % 2) and B > 1)
         for i, D in enumerate(WIDTHS) for j, (n, B) in enumerate(ROWSETS) for r in (0, 1)]


def test_cases_cover_every_option():
    for D in WIDTHS:
        cs = [c for c in CASES if c.D == D]
        assert {(c.n_tok, c.B) for c in cs} == set(ROWSETS)
        for field in ("res", "per_entry", "wide"):
            assert {getattr(c, field) for c in cs} == {False, True}, (D, field)
        assert {c.tok0 for c in cs} == {0, 3, 6} and any(c.bcast for c in cs) and any(not c.bcast for c in cs)


def _inputs(c: Case, device):
    g = torch.Generator().manual_seed(zlib.crc32(str(c).encode()))
    D, n, B = c.D, c.n_tok, c.B
    x = torch.randn(n, 1 if c.bcast else B, D, generator=g).to(BF16).to(device)
    y = torch.randn(n, B, D, generator=g).to(BF16).to(device) if c.res else None
    mods = (torch.randn(B, T_FRAMES, 3 * D, generator=g) * 0.5).to(BF16).to(device)
    sh, sc, gate = mods[..., :D], mods[..., D:2 * D], mods[..., 2 * D:]
    ld = D + 64 if c.wide else D
    cam_full = torch.randn(n, B if c.per_entry else 1, ld, generator=g).to(BF16).to(device)
    cam = cam_full[..., :D]  # [n, B | 1, D], row stride (B | 1) * ld
    return x, y, sh, sc, gate, cam


def _run(c: Case, device):
    x, y, sh, sc, gate, cam = _inputs(c, device)
    D, n, B, R = c.D, c.n_tok, c.B, c.n_tok * c.B
    kw = dict(n_tok=n, B=B, tok0=c.tok0, hw=HW, x_st=x.stride(0), x_sb=0 if c.bcast else x.stride(1), y=y,
              gate=gate if c.res else None)
    # the pinned kernel, and the one added op on the device
    x_ref = torch.empty((n, B, D), dtype=BF16, device=device) if c.res else None
    h_base = N.ln_mod(x, sh, sc, x_out=x_ref, **kw)
    want = (h_base.float() + cam.expand(n, B, D).float()).to(BF16)
    cam_st, cam_sb = cam.stride(0), (cam.stride(1) if c.per_entry else 0)
    assert cam_st == (B if c.per_entry else 1) * (D + 64 if c.wide else D)
    # bf16 form, through the wrapper, into guarded buffers
    hbuf, h = guarded(R * D, BF16, device, SENTINEL)
    xbuf, xo = guarded(R * D, BF16, device, SENTINEL)
    N.ln_mod(x, sh, sc, x_out=xo if c.res else None, h_out=h, cam=cam, cam_st=cam_st, cam_sb=cam_sb, **kw)
    # fp8 form, on the C entry point (the wrapper allocates its own outputs), into guarded buffers
    qbuf, q = guarded(R * D, torch.uint8, device, FILL8)
    sbuf, s = guarded(R, F32, device, SENTINEL)
    x2buf, xo2 = guarded(R * D, BF16, device, SENTINEL)
    rc = N.load_library().cp25_ln_mod_cam_fp8(
        N._ptr(x), kw["x_st"], kw["x_sb"], N._ptr(y), N._ptr(gate) if c.res else None, N._ptr(sh), N._ptr(sc),
        sh.stride(0), sh.stride(1), N._ptr(cam), cam_st, cam_sb, N._ptr(xo2) if c.res else None, N._ptr(q), N._ptr(s),
        n, B, D, c.tok0, HW, 1e-6, N._stream(device))
    assert rc == 0
    q_ref, s_ref = N.quant_fp8_rows(want.view(R, D))
    torch.cuda.synchronize()
    return dict(want=want.view(R, D), h=h.view(R, D), hbuf=hbuf, xbuf=xbuf, xo=xo.view(R, D), x2buf=x2buf,
                xo2=xo2.view(R, D), x_ref=None if x_ref is None else x_ref.view(R, D), qbuf=qbuf, q=q.view(R, D),
                sbuf=sbuf, s=s, q_ref=q_ref.view(torch.uint8), s_ref=s_ref.view(R), cam=cam)


def _bits(t):
    return t.view(torch.int16)


@pytest.mark.parametrize("case", CASES, ids=str)
def test_ln_mod_cam_exact(device, case):
    c = case
    r = _run(c, device)
    R, D = c.n_tok * c.B, c.D
    bad = (_bits(r["h"]) != _bits(r["want"])).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} of {R * D} differ, first {bad[:4].tolist()}"
    for buf in ("hbuf", "xbuf", "x2buf"):
        assert guards_ok(r[buf], R * D, SENTINEL), buf
    assert guards_ok(r["qbuf"], R * D, FILL8) and guards_ok(r["sbuf"], R, SENTINEL)
    if c.res:
        assert torch.equal(_bits(r["xo"]), _bits(r["x_ref"])), "x_out differs from cp25_ln_mod's"
        assert torch.equal(_bits(r["xo2"]), _bits(r["x_ref"])), "the fp8 form's x_out differs from cp25_ln_mod's"
    else:
        assert (r["xo"] == SENTINEL).all() and (r["xo2"] == SENTINEL).all(), "x_out written without a residual"
    assert torch.equal(r["s"].view(torch.int32), r["s_ref"].view(torch.int32)), "fp8 row scales"
    badq = (r["q"] != r["q_ref"]).nonzero()
    assert badq.numel() == 0, f"{badq.shape[0]} fp8 codes differ, first {badq[:4].tolist()}"


def test_wrapper_fp8_form(device):
    """N.ln_mod(fp8=True, cam=...) is cp25_ln_mod_cam_fp8 (the path the fp8 net takes)."""
    c = Case(1024, 7, 2, 3, True, False, False, False)
    x, y, sh, sc, gate, cam = _inputs(c, device)
    kw = dict(n_tok=c.n_tok, B=c.B, tok0=c.tok0, hw=HW, x_st=x.stride(0), x_sb=x.stride(1), y=y, gate=gate)
    xo = torch.empty((c.n_tok, c.B, c.D), dtype=BF16, device=device)
    h = N.ln_mod(x, sh, sc, x_out=xo, cam=cam.squeeze(1), **kw)
    q, s = N.ln_mod(x, sh, sc, x_out=torch.empty_like(xo), fp8=True, cam=cam.squeeze(1), **kw)
    q_ref, s_ref = N.quant_fp8_rows(h.view(-1, c.D))
    assert torch.equal(q.view(torch.uint8), q_ref.view(torch.uint8)) and torch.equal(s, s_ref)


def test_cam_validation(device):
    """The wrapper checks that cam covers the rows the kernel reads; the entry point returns -22 (ValueError) for a
    pointer or stride that breaks the 16-byte loads, before any launch."""
    c = Case(512, 5, 3, 0, False, False, False, False)
    x, y, sh, sc, gate, cam = _inputs(c, device)
    kw = dict(n_tok=c.n_tok, B=c.B, tok0=0, hw=HW, x_st=x.stride(0), x_sb=x.stride(1))
    cam2 = cam.squeeze(1)  # [5, 512]
    with pytest.raises(ValueError, match="does not cover"):
        N.ln_mod(x, sh, sc, cam=cam2[:4], **kw)            # one token short
    with pytest.raises(ValueError, match="does not cover"):
        N.ln_mod(x, sh, sc, cam=cam2, cam_sb=512, **kw)    # per-entry rows the tensor does not hold
    with pytest.raises(ValueError, match="cam strides"):
        N.ln_mod(x, sh, sc, cam=cam2, cam_st=256, **kw)    # cam_st < D
    with pytest.raises(ValueError):
        N.ln_mod(x, sh, sc, cam=cam2.float(), **kw)
    lib, st = N.load_library(), N._stream(device)
    h = torch.empty((c.n_tok, c.B, c.D), dtype=BF16, device=device)
    wide = torch.zeros((c.n_tok, 1024 + 8), dtype=BF16, device=device)

    def rc(cam_ptr, cam_st, cam_sb):
        return lib.cp25_ln_mod_cam(N._ptr(x), x.stride(0), x.stride(1), None, None, N._ptr(sh), N._ptr(sc),
                                   sh.stride(0), sh.stride(1), cam_ptr, cam_st, cam_sb, None, N._ptr(h), c.n_tok, c.B,
                                   c.D, 0, HW, 1e-6, st)

    assert rc(N._ptr(wide), 1032, 0) == 0
    assert rc(N._ptr(wide) + 2, 1032, 0) == -22   # pointer not 16-byte aligned
    assert rc(N._ptr(wide), 1028, 0) == -22       # row stride not a multiple of 8 elements
    assert rc(N._ptr(wide), 1032, 4) == -22       # batch stride not a multiple of 8 elements
    assert rc(N._ptr(wide), 504, 0) == -22        # cam_st < D
    assert rc(None, 1032, 0) == -22
    torch.cuda.synchronize()
