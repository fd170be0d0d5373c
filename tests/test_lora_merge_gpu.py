"""cp25_lora_merge against its restatement in fp32 torch CPU ops (tests/lora_truth.py: merge_restated), bit for bit.

The kernel's contract (include/cp25.h) fixes the order and the roundings: acc = acc + (B[n, j] * A[j, k]) for j
ascending in fp32 without contraction, then bf16(float(W) + acc * scale). torch's CPU elementwise ops round each product
and sum on their own, so the two agree exactly or the kernel is wrong; tests/test_lora_cpu.py holds the restatement
itself to a float64 formula. Shapes (lora_truth.SHAPES): rank 1; ragged N with K no multiple of 64 and a scale that
is no power of two; guard columns [K, ldw) with a rank one past the 32-entry staging chunk; the recipe's rank at the
cross-attention k/v width; rank 256; the k rows of a fused q|k|v buffer. Every view sits in a sentinel-filled buffer
(test_fp8_cast_exact_gpu's guarded / guards_ok): guard elements, rows outside the slice and columns past K must keep
their bits."""
import pytest
import torch

import lora_truth as lt
from cosmos_predict2 import _native as N
from test_fp8_cast_exact_gpu import SENTINEL, guarded, guards_ok

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
F32 = torch.float32
CASES = lt.cases()
_REF = {}


def _ref(name):
    """The restated merge of a case, computed once."""
    if name not in _REF:
        w, a, b, scale = CASES[name]
        _REF[name] = lt.merge_restated(w, a, b, scale)
    return _REF[name]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _mismatch(got, ref):
    bad = (_bits(got) != _bits(ref)).nonzero()
    return (f"{bad.shape[0]} of {ref.numel()} differ, first "
            f"{[(tuple(i.tolist()), float(got[tuple(i)]), float(ref[tuple(i)])) for i in bad[:6]]}")


def _place(device, w, ldw, rows_total=None, row0=0):
    """w [N, K] copied into rows row0 .. row0 + N of a sentinel-filled [rows_total, ldw] area inside a guarded buffer;
    returns (buffer, area, view)."""
    n, k = w.shape
    rows_total = rows_total or n
    buf, flat = guarded(rows_total * ldw, BF16, device, SENTINEL)
    area = flat.view(rows_total, ldw)
    view = area[row0:row0 + n, :k]
    view.copy_(w.to(device))
    return buf, area, view


@pytest.mark.parametrize("name", sorted(lt.SHAPES))
def test_lora_merge_exact(device, name):
    n, k, ldw, r, scale = lt.SHAPES[name]
    w, a, b, _ = CASES[name]
    assert tuple(w.shape) == (n, k) and tuple(a.shape) == (r, k) and tuple(b.shape) == (n, r)
    rows_total, row0 = (1536, 512) if name == "qkv_slice" else (n, 0)
    buf, area, view = _place(device, w, ldw, rows_total, row0)
    before = area.clone()
    out = N.lora_merge(view, a.to(device), b.to(device), scale)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr()
    got, ref = view.cpu(), _ref(name)
    assert torch.equal(_bits(got), _bits(ref)), _mismatch(got, ref)
    assert torch.equal(got, ref)
    assert guards_ok(buf, rows_total * ldw, SENTINEL)
    # rows outside the slice and the guard columns [K, ldw) keep their bits
    keep = torch.ones(rows_total, ldw, dtype=torch.bool)
    keep[row0:row0 + n, :k] = False
    assert torch.equal(_bits(area.cpu())[keep], _bits(before.cpu())[keep])
    assert not torch.equal(got, w)


def test_zero_b_leaves_w_equal(device):
    w, a, b, scale = CASES["ragged"]
    w = w.clone()
    w[0, :8] = -0.0  # may come back as +0: equal, not bit-equal
    view = w.to(device)
    N.lora_merge(view, a.to(device), torch.zeros_like(b).to(device), scale)
    torch.cuda.synchronize()
    assert (view.cpu() == w).all()


def test_host_checks(device):
    w, a, b, scale = CASES["rank1"]
    wd, ad, bd = w.to(device), a.to(device), b.to(device)
    keep = wd.clone()
    with pytest.raises(ValueError):  # K % 8 != 0
        N.lora_merge(wd[:, :60], ad[:, :60].contiguous(), bd, 1.0)
    with pytest.raises(ValueError):  # r = 0
        N.lora_merge(wd, ad[:0], bd[:, :0], 1.0)
    a257 = torch.zeros(257, w.shape[1], device=device)
    b257 = torch.zeros(w.shape[0], 257, device=device)
    with pytest.raises(ValueError):  # r = 257
        N.lora_merge(wd, a257, b257, 1.0)
    N.lora_merge(wd, a257[:256], b257[:, :256].contiguous(), 1.0)  # r = 256 is served (and B = 0 changes nothing)
    with pytest.raises((RuntimeError, ValueError)):  # a CPU tensor
        N.lora_merge(w.clone(), a, b, 1.0)
    with pytest.raises((RuntimeError, ValueError)):
        N.lora_merge(wd, a, bd, 1.0)
    with pytest.raises(ValueError):  # A not fp32
        N.lora_merge(wd, ad.to(BF16), bd, 1.0)
    with pytest.raises(ValueError):  # W not bf16
        N.lora_merge(wd.float(), ad, bd, 1.0)
    with pytest.raises(ValueError):  # shapes that do not fit
        N.lora_merge(wd, ad, bd[:-1], 1.0)
    with pytest.raises(ValueError):  # a misaligned view (16-B accesses)
        N.lora_merge(wd.view(-1)[4:4 + 8 * 64].view(8, 64), ad, bd[:8].contiguous(), 1.0)
    torch.cuda.synchronize()
    assert torch.equal(wd, keep)
