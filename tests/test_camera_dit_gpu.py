"""The camera-conditioned net option (DiTConfig.camera_dim) on the GPU against tests/camera_truth.py's restatement of
the reference's camera Block / net forward, on tiny_dit(camera_dim=1536) with init_state_dict(zero_adaln_out=False)
so the blocks act.

Geometries: T = 6 latent frames (three 2-frame segments) of 4 x 6 patches at B = 2 (the gated residuals ride in the
GEMM epilogues, every LN-mod is the plain or the `_proj_res` one) and of 2 x 3 patches (hw = 6 < 8: the unfused path,
whose LN-mod carries x + gate y and the camera term together). The CPU truth of each is computed once and shared."""
import dataclasses
import functools

import pytest
import torch

import camera_truth as ct
from cosmos_predict2.dit import ContextCache, Geometry, MinimalV1LVGDiT, init_state_dict
from cosmos_predict2.net_config import tiny_dit

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
T = 6
GEOS = {"fused_4x6": (4, 6), "unfused_2x3": (2, 3)}


def rel_l2(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@functools.lru_cache(maxsize=None)
def _weights():
    cfg = tiny_dit(camera_dim=1536)
    sd = init_state_dict(cfg, seed=3, zero_adaln_out=False)
    return cfg, {"net." + k: v for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def _inputs(geo):
    cfg, _ = _weights()
    Hp, Wp = GEOS[geo]
    g = torch.Generator().manual_seed(70 + Hp)
    x = torch.randn(2, 16, T, 2 * Hp, 2 * Wp, generator=g)
    mask = torch.zeros(2, 1, T, 2 * Hp, 2 * Wp)
    mask[:, :, 2:4] = 1
    t = torch.tensor([[877.0, 877.0, 0.1, 0.1, 877.0, 877.0], [500.0, 500.0, 0.1, 0.1, 500.0, 500.0]])
    ctx = torch.randn(2, 512, cfg.crossattn_proj_in_channels, generator=g).to(BF16)
    cam_a = torch.randn(1, T, Hp, Wp, 1536, generator=g).to(BF16)
    cam_b = torch.randn(1, T, Hp, Wp, 1536, generator=g).to(BF16)
    return x, t, ctx, mask, cam_a, cam_b


@functools.lru_cache(maxsize=None)
def _truth(geo, which):
    cfg, sd = _weights()
    x, t, ctx, mask, cam_a, cam_b = _inputs(geo)
    return ct.camera_dit_forward(dataclasses.asdict(cfg), sd, x, t, ctx, mask, cam_a if which == "a" else cam_b)


def _net(device, cfg=None, sd=None):
    c, s = _weights()
    net = MinimalV1LVGDiT(cfg or c, device=device)
    net.load_state_dict(sd or s)
    return net


def _run(net, device, geo, cam, **kw):
    x, t, ctx, mask, _, _ = _inputs(geo)
    out = net(x.to(device).to(BF16), t.to(device), ctx.to(device),
              condition_video_input_mask_B_C_T_H_W=mask.to(device), **({} if cam is None else dict(camera=cam.to(device))),
              **kw)
    torch.cuda.synchronize()
    return out.cpu()


@pytest.mark.parametrize("geo", sorted(GEOS))
def test_zero_encoder_is_the_plain_net(device, geo):
    """(i) With zeroed cam_encoder weights a random camera adds bf16(h + 0) = h: the forward equals the plain
    tiny_dit's on the same weights, bit for bit."""
    cfg, sd = _weights()
    plain_sd = {k: v for k, v in sd.items() if "cam_encoder" not in k}
    zero_sd = {k: (torch.zeros_like(v) if "cam_encoder" in k else v) for k, v in sd.items()}
    want = _run(_net(device, tiny_dit(), plain_sd), device, geo, None)
    got = _run(_net(device, cfg, zero_sd), device, geo, _inputs(geo)[4])
    assert torch.isfinite(got).all() and torch.equal(got, want)


@pytest.mark.parametrize("geo", sorted(GEOS))
def test_matches_truth_and_sees_the_camera(device, geo):
    """(ii) rel-L2 to camera_truth <= 1e-2 (the bound tests/test_dit_gpu.py holds every net variant to), for two
    cameras; (iii) the truth's outputs for the two cameras differ by >= 5e-2 rel-L2 and the device outputs by more than
    half of that, so a forward that ignored the camera could not pass (ii)."""
    net = _net(device)
    cams = dict(a=_inputs(geo)[4], b=_inputs(geo)[5])
    outs = {k: _run(net, device, geo, v) for k, v in cams.items()}
    for k in "ab":
        err = rel_l2(outs[k], _truth(geo, k))
        print(f"camera dit forward {geo} camera {k}: rel-L2 {err:.3e}")
        assert torch.isfinite(outs[k]).all() and err <= 1e-2, (k, err)
    sep_truth = rel_l2(_truth(geo, "a"), _truth(geo, "b"))
    sep_dev = rel_l2(outs["a"], outs["b"])
    print(f"camera sensitivity {geo}: truth {sep_truth:.3e}, device {sep_dev:.3e}")
    assert sep_truth >= 5e-2
    assert sep_dev > 2.5e-2


@pytest.mark.parametrize("geo", sorted(GEOS))
def test_cache_policies_agree(device, geo):
    """(iv) camera_cache "all" (every block's embedding held) and "none" (recomputed into one buffer per evaluation)
    give the same bits; so does a second evaluation on the same cache."""
    net = _net(device)
    cfg = net.cfg
    x, t, ctx, mask, cam_a, _ = _inputs(geo)
    Hp, Wp = GEOS[geo]
    g = Geometry(T=T, Hp=Hp, Wp=Wp, tok0=0, n_tok=T * Hp * Wp)
    rows = torch.randn(g.L, 1, 72, generator=torch.Generator().manual_seed(5)).to(BF16).to(device)
    cc = net.prepare_context(ctx.to(device))
    tt = net.scale_timesteps(t[:1].expand(2, T).contiguous().to(device))
    outs = {}
    for mode in ("all", "none"):
        cache = net.prepare_camera(cam_a[0].to(device), g, camera_cache=mode)
        assert cache.mode == mode and (cache.emb is None) == (mode == "none")
        outs[mode] = [net.forward_tokens(rows, tt, cc, g, shared_batch=True, camera=cache).cpu() for _ in range(2)]
    assert torch.equal(outs["all"][0], outs["none"][0]) and torch.equal(outs["all"][0], outs["all"][1])
    assert torch.equal(outs["none"][0], outs["none"][1])
    # the net's default policy is "all"; the token-major [n, camera_dim] rows are the same input
    net.camera_cache = "none"
    c2 = net.prepare_camera(cam_a[0].reshape(-1, cfg.camera_dim).to(device), g)
    assert c2.mode == "none" and torch.equal(net.forward_tokens(rows, tt, cc, g, shared_batch=True, camera=c2).cpu(),
                                             outs["all"][0])
    # the CFG pair's shared block-0 prefix stays valid with a camera: the same bits as every entry computing it
    net.share_cfg_block0 = False
    c3 = net.prepare_camera(cam_a[0].to(device), g, camera_cache="all")
    assert torch.equal(net.forward_tokens(rows, tt, cc, g, shared_batch=True, camera=c3).cpu(), outs["all"][0])


def test_fp8_linears(device):
    """(v) linear_precision="fp8" runs with a camera (cp25_ln_mod_cam_fp8 feeds the QKV GEMM; the encoder GEMM stays
    bf16), within the bound tests/test_fp8_gpu.py holds the fp8 net to (6e-2 rel-L2 to the bf16 truth), and is the fp8
    path (further from the truth than the bf16 run)."""
    geo = "fused_4x6"
    net = _net(device)
    cam = _inputs(geo)[4]
    e_bf = rel_l2(_run(net, device, geo, cam), _truth(geo, "a"))
    net.set_linear_precision("fp8")
    out8 = _run(net, device, geo, cam)
    e8 = rel_l2(out8, _truth(geo, "a"))
    print(f"camera dit forward fp8 linears: rel-L2 {e8:.3e} (bf16 {e_bf:.3e})")
    assert torch.isfinite(out8).all() and e_bf < e8 <= 6e-2
    caches = [net.prepare_camera(cam[0].to(device), Geometry(T=T, Hp=4, Wp=6, tok0=0, n_tok=T * 24), camera_cache=m)
              for m in ("all", "none")]
    net.set_linear_precision("bf16")
    ref = net.prepare_camera(cam[0].to(device), Geometry(T=T, Hp=4, Wp=6, tok0=0, n_tok=T * 24))
    assert all(torch.equal(a, b) for a, b in zip(caches[0].emb, ref.emb))  # the encoder GEMM is bf16 either way


def test_unsupported_combinations_raise(device):
    """(vi) every unsupported pairing raises ValueError naming it."""
    geo = "unfused_2x3"
    Hp, Wp = GEOS[geo]
    x, t, ctx, mask, cam_a, _ = _inputs(geo)
    net = _net(device)
    with pytest.raises(ValueError, match="needs `camera`"):
        _run(net, device, geo, None)
    cfg, sd = _weights()
    plain = _net(device, tiny_dit(), {k: v for k, v in sd.items() if "cam_encoder" not in k})
    with pytest.raises(ValueError, match="without cam_encoder"):
        _run(plain, device, geo, cam_a)
    g = Geometry(T=T, Hp=Hp, Wp=Wp, tok0=0, n_tok=T * Hp * Wp)
    with pytest.raises(ValueError, match="without cam_encoder"):
        plain.prepare_camera(cam_a[0].to(device), g)
    cache = net.prepare_camera(cam_a[0].to(device), g)
    rows = torch.zeros(g.L, 1, 72, dtype=BF16, device=device)
    cc = net.prepare_context(ctx.to(device))
    tt = net.scale_timesteps(t.to(device))
    net.cp_group = object()  # context parallelism enabled
    with pytest.raises(ValueError, match="context parallelism"):
        net.forward_tokens(rows, tt, cc, g, camera=cache)
    net.cp_group = None
    net.force_lanes = True  # the CP lanes on one GPU
    with pytest.raises(ValueError, match="context parallelism"):
        net.forward_tokens(rows, tt, cc, g, camera=cache)
    net.force_lanes = False
    half = Geometry(T=T, Hp=Hp, Wp=Wp, tok0=g.L // 2, n_tok=g.L // 2)  # a token shard
    with pytest.raises(ValueError, match="context parallelism"):
        net.prepare_camera(cam_a[0].reshape(-1, 1536)[: g.L // 2].to(device), half)
    with pytest.raises(ValueError, match="camera cache holds"):
        net.forward_tokens(rows[: g.L // 2], tt, cc, Geometry(T=T // 2, Hp=Hp, Wp=Wp, tok0=0, n_tok=g.L // 2),
                           camera=cache)
    with pytest.raises(ValueError, match="camera rows"):
        net.prepare_camera(cam_a[0, :, :, :, :1024].to(device), g)
    with pytest.raises(ValueError, match="camera_cache"):
        net.prepare_camera(cam_a[0].to(device), g, camera_cache="some")
    with pytest.raises(ValueError, match="forward_frame"):
        net.forward_frame(rows[: g.hw], tt[:, :1], ContextCache(B=2, k=cc.k, v=cc.v), g, 0,
                          cache=net.make_kv_cache(2, 1, g.hw))
    for kw, what in ((dict(action_dim=7, action_per_latent_frame=4), "action"),
                     (dict(n_cameras_emb=7, view_condition_dim=7, state_t=8), "multi-view"),
                     (dict(n_dense_blocks=0, natten_parameters=dict(window_size=(-1, 4, 4), stride=(1, 1, 1))), "sparse"),
                     (dict(camera_dim=1000), "GEMM")):
        with pytest.raises(ValueError, match=what):
            MinimalV1LVGDiT(tiny_dit(**dict(dict(camera_dim=1536), **kw)), device=device)
