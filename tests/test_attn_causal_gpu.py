"""Known-answer tests of the causal grouped-query attention (csrc/attn_causal.hip, cp25_attn_causal), in the manner
of tests/attn_truth.py / test_attn_exact_gpu.py: structured inputs whose answers are known without running attention.

  selector  every query row i selects one key pi(i) <= i: key rows are +-1 codes x mk in the first 64 dims, query row i
            is the code of key pi(i) x mq, so the winning score is 64 mq mk and every other visible score is mq mk x an
            integer far below (the gap is computed from the exact integer products and asserted). The output must equal
            v[pi(i)] bit for bit. pi covers key 0, i itself, 63 / 64 / 65 and each tile's first and last key.
  lure      the same keys and values; query row i additionally carries, in the last 64 dims, the private direction of a
            lure key j > i (one-hot blocks of 8 dims, one per lure key, so no key j <= i sees it): key j then scores far
            above the selected key (2048 log2 units: unmasked it overflows exp2). The output must not change by a bit.
            Lure keys sit at i + 1 for rows 0, 63, 64, 127 (the diagonal tile's mask) and tiles ahead (the loop bound).
  row 0     equals v[0] on any data.
  uniform   equal scores: the float64 mean of v[0..i] within attn_truth.bound.
  gaussian  rel-L2 to the float64 causal truth at most 1.1 x that of the bf16-P flash-style restatement
            (reason1_truth.causal_attention), the project's gate (test_parity_depth_gpu.py).

q / k / v are strided column views of one fused [B L, (Hq + 2 Hkv) 128] buffer, as the encoder passes them; the output
is a slice of a sentinel-filled buffer whose surroundings must stay untouched."""
import math

import pytest
import torch

import attn_truth as AT
import reason1_truth as T
from cosmos_predict2 import _native as N

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SENT = -1.5e30
LS = (64, 128, 192, 512)
HEADS = ((2, 2), (4, 2), (7, 1), (28, 4))
BS = (1, 2)
MQ = MK = 1.5        # selector magnitudes: winner 64 x 2.25 = 144 log2 units
MLQ = MLK = 16.0     # lure magnitudes: 8 dims x 256 = 2048 log2 units
LN2 = math.log(2.0)  # softmax_scale = ln 2: scores are in log2 units


def _run(device, q, k, v, scale=LN2):
    """q [B, L, Hq, 128], k / v [B, L, Hkv, 128] (host) -> out [B, L, Hq, 128] (host), launched on column views of the
    fused QKV rows, into a framed output."""
    B, L, Hq, _ = q.shape
    Hkv = k.shape[2]
    fused = torch.cat([q.reshape(B * L, -1), k.reshape(B * L, -1), v.reshape(B * L, -1)], 1).to(device)
    f4 = fused.view(B, L, Hq + 2 * Hkv, 128)
    big = torch.full((B, L + 2, Hq + 1, 128), SENT, dtype=BF16, device=device)
    out = big[:, 1:L + 1, :Hq]
    N.attn_causal(f4[:, :, :Hq], f4[:, :, Hq:Hq + Hkv], f4[:, :, Hq + Hkv:], out=out, softmax_scale=scale)
    torch.cuda.synchronize()
    chk = big.clone()
    chk[:, 1:L + 1, :Hq] = SENT
    assert torch.equal(chk, torch.full_like(chk, SENT)), "wrote outside the output slice"
    return out.cpu()


def _pi(L, g):
    """pi(i) <= i for every row: eight rules in turn, each falling back to i itself when its key is in the future."""
    i = torch.arange(L)
    tile0 = i // 64 * 64
    rnd = (torch.rand(L, generator=g) * (i + 1).float()).long().clamp(max=L - 1)
    rules = [torch.zeros(L, dtype=torch.long), i, torch.full((L,), 63), torch.full((L,), 64), torch.full((L,), 65),
             tile0, (tile0 - 1).clamp(min=0), rnd]
    pi = torch.stack(rules)[i % 8, i]
    pi = torch.where(pi <= i, pi, i)
    pi[tile0 + 63 == i] = i[tile0 + 63 == i]  # a tile's last row takes its own (the tile's last) key
    return pi


def _lure_positions(L):
    return sorted({p for p in (1, 64, 65, 128, 129, 191, 320, L - 1) if 0 < p < L})[:8]


def selector_case(B, Hq, Hkv, L, seed):
    g = torch.Generator().manual_seed(seed)
    grp = Hq // Hkv
    code = (torch.randint(0, 2, (B, L, Hkv, 64), generator=g) * 2 - 1).float()
    lures = _lure_positions(L)
    k = torch.zeros(B, L, Hkv, 128)
    k[..., :64] = code * MK
    for m, p in enumerate(lures):
        k[:, p, :, 64 + 8 * m:72 + 8 * m] = MLK
    v = AT._int_v(g, (B, L, Hkv, 128))
    pi = torch.stack([torch.stack([_pi(L, g) for _ in range(Hq)]) for _ in range(B)])  # [B, Hq, L]
    bi = torch.arange(B)[:, None, None]
    kv = (torch.arange(Hq) // grp)[None, :, None]
    q = torch.zeros(B, L, Hq, 128)
    q[..., :64] = (code[bi, pi, kv] * MQ).permute(0, 2, 1, 3)
    ql = q.clone()
    nxt = torch.full((L,), -1)
    for m, p in reversed(list(enumerate(lures))):
        nxt[:p] = m
    for i in range(L):
        if nxt[i] >= 0:
            ql[:, i, :, 64 + 8 * nxt[i]:72 + 8 * nxt[i]] = MLQ
    q, ql, k, v = q.to(BF16), ql.to(BF16), k.to(BF16), v.to(BF16)
    expected = v[bi, pi, kv].permute(0, 2, 1, 3).contiguous()
    # premises, from the exact products: the causal winner is pi with a gap; the lure really is the global winner
    kk = k.float().repeat_interleave(grp, dim=2)
    causal = torch.ones(L, L, dtype=torch.bool).tril()
    for name, qq in (("selector", q), ("lure", ql)):
        s = torch.einsum("bqhd,bkhd->bhqk", qq.float(), kk)
        sc = s.masked_fill(~causal, -math.inf)
        win = sc.gather(-1, pi[..., None])[..., 0]
        assert torch.equal(sc.argmax(-1), pi), name
        rest = sc.scatter(-1, pi[..., None], -math.inf).max(-1).values
        gap = (win - rest)[:, :, 1:].min().item() if L > 1 else math.inf
        assert L * 2.0 ** -gap * 127 < AT.PREMISE, (name, gap)
        if name == "lure":
            lured = nxt >= 0
            future = s.masked_fill(causal, -math.inf).max(-1).values
            assert lured.sum() >= L - 1 and (future[:, :, lured] - win[:, :, lured]).min().item() >= 1000.0
    return dict(q=q, ql=ql, k=k, v=v, pi=pi, expected=expected, lures=lures)


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("L", LS)
def test_selector_and_lure(device, L, Hq, Hkv, B):
    c = selector_case(B, Hq, Hkv, L, seed=L + 7 * Hq + B)
    pi = c["pi"]
    for key in (0, 63, 64, 65, L - 1, L - 64):  # the targets are present
        if key < L:
            assert (pi == key).any(), key
    assert (pi == torch.arange(L)).any()
    out = _run(device, c["q"], c["k"], c["v"])
    bad = (out != c["expected"]).any(-1)
    assert not bad.any(), f"selector: {int(bad.sum())} rows differ, first (b, row, head) {bad.nonzero()[0].tolist()}"
    lured = _run(device, c["ql"], c["k"], c["v"])
    bad = (lured != out).any(-1)
    assert not bad.any(), f"lure: {int(bad.sum())} rows changed, first (b, row, head) {bad.nonzero()[0].tolist()}"


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("L", LS)
def test_uniform_is_the_prefix_mean(device, L, Hq, Hkv, B):
    g = torch.Generator().manual_seed(L + Hq + B)
    u = (torch.randint(0, 2, (B, 1, Hkv, 128), generator=g) * 2 - 1).float()
    k = (u * 0.5).expand(B, L, Hkv, 128).contiguous().to(BF16)
    mags = torch.tensor([0.0, 0.125, 0.5, 1.0])[torch.arange(L) % 4]  # scores 0, 8, 32, 64: equal along a row
    q = (u.repeat_interleave(Hq // Hkv, dim=2) * mags[None, :, None, None]).to(BF16)
    v = torch.randn(B, L, Hkv, 128, generator=g).to(BF16)
    out = _run(device, q, k, v)
    vv = v.double().repeat_interleave(Hq // Hkv, dim=2)
    cnt = torch.arange(1, L + 1, dtype=torch.float64)[None, :, None, None]
    ref = vv.cumsum(1) / cnt
    A = vv.abs().cumsum(1) / cnt
    r = AT.ratio(out, ref, A)
    print(f"uniform L={L} H={Hq}/{Hkv} B={B}: max error / bound {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
@pytest.mark.parametrize("L", LS)
def test_gaussian_and_row0(device, L, Hq, Hkv, B):
    g = torch.Generator().manual_seed(3 * L + Hq + B)
    q = (torch.randn(B, L, Hq, 128, generator=g) * 1.5).to(BF16)
    k = (torch.randn(B, L, Hkv, 128, generator=g) * 1.5).to(BF16)
    v = torch.randn(B, L, Hkv, 128, generator=g).to(BF16)
    scale = 128 ** -0.5
    out = _run(device, q, k, v, scale)
    assert torch.equal(out[:, 0], v[:, 0].repeat_interleave(Hq // Hkv, dim=1)), "row 0 is v[0]"
    truth = T.causal_attention(q.double(), k.double(), v.double(), scale, rounded=False)
    flash = T.causal_attention(q.float(), k.float(), v.float(), scale, rounded=True)
    d_hip, d_ref = T.rel_l2(out, truth), T.rel_l2(flash, truth)
    print(f"gaussian L={L} H={Hq}/{Hkv} B={B}: hip-truth {d_hip:.3e}, bf16-P restatement-truth {d_ref:.3e}")
    assert d_hip <= 1.1 * d_ref


def test_refused_shapes_write_nothing(device):
    """L = 96 (not a multiple of 64) and a head dim of 64: -22 from the C entry, a ValueError, nothing written."""
    for L, D in ((96, 128), (128, 64)):
        q = torch.randn(1, L, 2, D).to(BF16).to(device)
        out = torch.full((1, L, 2, D), SENT, dtype=BF16, device=device)
        with pytest.raises(ValueError, match="-22"):
            N.attn_causal(q, q, q, out=out)
        torch.cuda.synchronize()
        assert torch.equal(out, torch.full_like(out, SENT))
    q = torch.randn(1, 64, 3, 128).to(BF16).to(device)
    with pytest.raises(ValueError, match="-22"):
        N.attn_causal(q, q[:, :, :2], q[:, :, :2])  # 3 query heads on 2 key/value heads
