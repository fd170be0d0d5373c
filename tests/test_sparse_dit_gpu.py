"""Sparse-attention DiT (DiTConfig.n_dense_blocks / natten_parameters) against the CPU oracle.

oracle/dit.py has no sparse option, so its `sdpa` is wrapped at run time: the self-attention calls of the sparse blocks
apply tests/na_truth.py's brute-force mask (fp32 softmax over the box, bf16 output, as the oracle's dense sdpa). The
limit is tests/test_dit_gpu.py's: rel-L2 <= 1e-2 of one forward. The masked and the dense oracle outputs differ by more
than 3e-2 at this seed (asserted), so the test cannot pass with the mask ignored.
"""
import dataclasses
import functools

import pytest
import torch

import na_truth as NT
from cosmos_predict2 import _native as N
from cosmos_predict2 import sparse_attn as SA
from cosmos_predict2.dit import Geometry, MinimalV1LVGDiT, init_state_dict
from cosmos_predict2.net_config import tiny_dit
from oracle import dit as odit

pytestmark = pytest.mark.gpu

GRID = (3, 8, 12)  # patch grid; latent 3 x 16 x 24
PARAMS = dict(window_size=(-1, 4, 6), stride=(1, 2, 3))
FULL = dict(window_size=(-1, -1, -1))
SEED = 3


def rel_l2(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def _cfg(**kw):
    return tiny_dit(**dict(dict(num_blocks=3, n_dense_blocks=1, natten_parameters=PARAMS), **kw))


@functools.lru_cache(maxsize=None)
def _problem():
    cfg = _cfg()
    sd = {"net." + k: v for k, v in init_state_dict(cfg, seed=SEED, zero_adaln_out=False).items()}
    g = torch.Generator().manual_seed(SEED)
    T, H, W = GRID[0], 2 * GRID[1], 2 * GRID[2]
    x = torch.randn(1, 16, T, H, W, generator=g)
    mask = torch.zeros(1, 1, T, H, W)
    mask[:, :, :1] = 1
    t = torch.tensor([[0.1] + [877.0] * (T - 1)])
    ctx = torch.randn(1, 512, cfg.crossattn_proj_in_channels, generator=g).to(torch.bfloat16)
    return cfg, sd, x, t, ctx, mask


def _oracle(sparse_blocks, monkeypatch):
    """oracle.dit.dit_forward with the self-attention of `sparse_blocks` masked by na_mask (sdpa is called twice per
    block: self-attention, then the text cross-attention)."""
    cfg, sd, x, t, ctx, mask = _problem()
    L = GRID[0] * GRID[1] * GRID[2]
    na = NT.na_mask(*GRID, PARAMS)
    calls = [0]
    dense = odit.sdpa

    def sdpa(q, k, v, *a, **kw):
        c = calls[0]
        calls[0] += 1
        if c % 2 or (c // 2) not in sparse_blocks:
            return dense(q, k, v, *a, **kw)
        Bq, Lq, Hq, Dq = q.shape
        assert Lq == L and k.shape[1] == L
        s = torch.matmul(q.float().transpose(1, 2), k.float().transpose(1, 2).transpose(-1, -2)) * Dq ** -0.5
        p = torch.softmax(s.masked_fill(~na[None, None], float("-inf")), dim=-1)
        return torch.matmul(p, v.float().transpose(1, 2)).transpose(1, 2).reshape(Bq, Lq, Hq * Dq).to(odit.act_dtype())

    monkeypatch.setattr(odit, "sdpa", sdpa)
    out = odit.dit_forward(dataclasses.asdict(cfg.replace(n_dense_blocks=-1, natten_parameters=())), sd, x, t, ctx, mask)
    monkeypatch.setattr(odit, "sdpa", dense)
    assert calls[0] == 2 * cfg.num_blocks
    return out


def _run(cfg, device):
    _, sd, x, t, ctx, mask = _problem()
    net = MinimalV1LVGDiT(cfg, device=device)
    net.load_state_dict(sd)
    out = net(x.to(device).to(torch.bfloat16), t.to(device), ctx.to(device),
              condition_video_input_mask_B_C_T_H_W=mask.to(device))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return net, out.cpu()


def test_sparse_forward_matches_masked_oracle(device, monkeypatch):
    ref = _oracle({0, 2}, monkeypatch)
    ref_dense = _oracle(set(), monkeypatch)
    gap = rel_l2(ref, ref_dense)
    print(f"masked vs dense oracle: rel-L2 {gap:.3e}")
    assert gap >= 3e-2, gap  # the mask matters at this seed
    net, out = _run(_cfg(), device)
    err = rel_l2(out, ref)
    print(f"sparse dit forward rel-L2 {err:.3e}")
    assert err <= 1e-2, err
    assert [p is None for p in net.sparse_params] == [False, True, False]
    names = net.attention_kernels(GRID[0] * GRID[1] * GRID[2])
    assert "attn_na3d" in names["sparse"] and names["sparse_blocks"] == "0,2" and "self" in names


def test_per_block_list_with_dense_entry(device, monkeypatch):
    """The list form: block 0 dense (None), blocks 1 and 2 sparse; n_dense_blocks is then ignored."""
    ref = _oracle({1, 2}, monkeypatch)
    net, out = _run(_cfg(n_dense_blocks=0, natten_parameters=[None, PARAMS, dict(PARAMS)]), device)
    err = rel_l2(out, ref)
    print(f"sparse dit (list form) rel-L2 {err:.3e}")
    assert err <= 1e-2, err
    assert [p is None for p in net.sparse_params] == [True, False, False]


def test_full_windows_match_dense_net(device):
    _, dense = _run(_cfg(n_dense_blocks=-1, natten_parameters=()), device)
    _, full = _run(_cfg(n_dense_blocks=0, natten_parameters=FULL), device)
    err = rel_l2(full, dense)
    print(f"full-window sparse net vs dense net: rel-L2 {err:.3e}")
    assert err <= 1e-2, err


def test_attn_events_count_the_box(device):
    cfg, sd, x, t, ctx, mask = _problem()
    net = MinimalV1LVGDiT(cfg, device=device)
    net.load_state_dict(sd)
    net.attn_events = []
    net(x.to(device).to(torch.bfloat16), t.to(device), ctx.to(device), condition_video_input_mask_B_C_T_H_W=mask.to(device))
    torch.cuda.synchronize()
    L = GRID[0] * GRID[1] * GRID[2]
    flops = [e[2] for e in net.attn_events]
    per_key = 4.0 * cfg.num_heads * L * cfg.head_dim
    assert flops == [per_key * 3 * 4 * 6, per_key * L, per_key * 3 * 4 * 6]


def test_unsupported_combinations_raise(device):
    cfg, sd, x, t, ctx, mask = _problem()
    with pytest.raises(NotImplementedError):  # multi-view
        MinimalV1LVGDiT(_cfg(n_cameras_emb=2, view_condition_dim=2, state_t=3), device=device)
    with pytest.raises(NotImplementedError):  # cross-view
        MinimalV1LVGDiT(_cfg(n_cameras_emb=2, state_t=3, adaln_view_embedding=True, cross_view_attn_map=((1,), (0,))),
                        device=device)
    net = MinimalV1LVGDiT(cfg, device=device)
    with pytest.raises(NotImplementedError):  # fp8 attention
        net.set_attention_precision("fp8")
    with pytest.raises(NotImplementedError):
        net.set_attention_precision("fp8qk")
    geo = Geometry(T=GRID[0], Hp=GRID[1], Wp=GRID[2], n_tok=GRID[0] * GRID[1] * GRID[2])
    assert net._sparse_plan(1, geo) is None and net._sparse_plan(0, geo) is not None
    with pytest.raises(NotImplementedError):  # context parallel
        net._sparse_plan(0, geo, cp_size=2)
    with pytest.raises(NotImplementedError):  # K/V cache
        net._sparse_plan(0, geo, kv=(None, 0, 1))
    half = Geometry(T=GRID[0], Hp=GRID[1], Wp=GRID[2], tok0=0, n_tok=geo.L // 2)
    with pytest.raises(NotImplementedError):  # a token shard
        net._sparse_plan(0, half)
    stream = MinimalV1LVGDiT(_cfg(use_wan_fp32_strategy=False), device=device)
    with pytest.raises(NotImplementedError):  # forward_frame
        stream.forward_frame(torch.zeros(96, 1, 72, dtype=torch.bfloat16, device=device),
                             torch.zeros(1, 1, device=device), None, geo, 0, cache=None)
    assert net._sparse_plan(0, Geometry(T=1, Hp=8, Wp=12, n_tok=96)) is None  # one frame: dense


def test_neighborhood_attn_op(device):
    grid, params = NT.NA_CASES["b_ragged"]
    L = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(2, L, 2, 128, generator=g).to(torch.bfloat16) for _ in range(3))
    op = SA.NeighborhoodAttnOp(natten_parameters=dict(params, layer_id=0))
    op.set_context_parallel_group(None, None, None)
    out = op(q.to(device), k.to(device), v.to(device), video_size=SA.VideoSize(*grid))
    torch.cuda.synchronize()
    assert out.shape == (2, L, 2 * 128) and out.dtype == torch.bfloat16
    truth = NT.na_attention_truth(q, k, v, NT.na_mask(*grid, params))
    assert rel_l2(out.cpu().view(2, L, 2, 128), truth) <= 4e-3
    with pytest.raises(ValueError):
        op(q.to(device), k.to(device), v.to(device), video_size=SA.VideoSize(grid[0], grid[1], grid[2] + 1))
    # T == 1: dense attention, whatever the window
    L1 = grid[1] * grid[2]
    q1, k1, v1 = (t[:, :L1].contiguous().to(device) for t in (q, k, v))
    out1 = op(q1, k1, v1, video_size=SA.VideoSize(1, grid[1], grid[2]))
    dense = N.attn_fwd(q1, k1, v1)
    torch.cuda.synchronize()
    assert torch.equal(out1.view(2, L1, 2, 128), dense)
