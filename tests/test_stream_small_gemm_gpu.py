"""forward_frame on the small-M GEMM family (MinimalV1LVGDiT.stream_gemm), tiny action net of test_stream_loop_gpu.

* "small" (the exact form wherever the plan takes the shape): every forward_frame output of the clip and every block's
  K / V cache after every frame are bit-identical to the "tile256" run, at the 4 x 6 (24 rows) and 16 x 20 (320 rows)
  patch grids, cache_frame_size -1 and 2.
* "small_splitk" with stream_gemm_force_split = 2 (the tiny net's K = 512 is below what the plan splits): the generated
  latents meet test_stream_loop_gpu's gate, HIP-vs-fp32-truth <= 1.1 x the oracle's own bf16 distance, by that test's
  own function run on a model in this mode; two runs give the same bits; the split kernels did run.
* linear_precision "fp8" with a mode other than "tile256" is refused; forward_tokens gives the same bits under every
  mode; ActionStreamingInference(stream_gemm="small") yields the default's frames on one chunk at 64 x 96.
"""
import dataclasses

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
import test_stream_loop_gpu as loop
from cosmos_predict2 import _native as N
from cosmos_predict2.dit import MinimalV1LVGDiT, init_state_dict
from cosmos_predict2.interactive import MODEL_NAME, ActionStreamingInference
from cosmos_predict2.model import StreamingRun
from cosmos_predict2.net_config import tiny_dit
from cosmos_predict2.pipeline import Video2WorldInference
from test_stream_loop_gpu import CFG, tiny  # noqa: F401  (tiny: the module fixture with the weights and CPU references)

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _run_recorded(device, sd, d, F, mode, force_split=None, n_steps=2):
    """One clip: every forward_frame output, and every block's K / V cache after every frame."""
    m = loop._model(device, sd)
    m.net.stream_gemm = mode
    m.net.stream_gemm_force_split = force_split
    run = StreamingRun(m, d["gt"], d["ctx"], d["actions"], init_noise=d["noise"], n_steps=n_steps, cache_frame_size=F)
    outs, caches = [], []
    inner = run._net

    def recording(*args):
        out = inner(*args)
        outs.append(out.clone())
        return out
    run._net = recording
    while not run.done:
        run.next_frame()
        caches.append([t.clone() for kv in (run.cache.k, run.cache.v) for t in kv])
    return outs, caches, run.latents()


@pytest.mark.parametrize("F", [-1, 2])
@pytest.mark.parametrize("grid", [(4, 6), (16, 20)])
def test_small_equals_tile256(device, tiny, grid, F):  # noqa: F811
    sd, make, _ = tiny
    d = make(*grid)
    hw, D = grid[0] * grid[1], CFG.model_channels
    for epi, (Nn, K) in ((N.EPI_QKV, (3 * D, D)), (N.EPI_RES, (D, D)), (N.EPI_GELU, (CFG.mlp_hidden, D)),
                         (N.EPI_RES, (D, CFG.mlp_hidden)),
                         (N.EPI_NONE, (D, 128))):
        assert N.gemm_sm_plan(hw, Nn, K, epi).small, "the plan leaves this launch to tile256: nothing would be tested"
    outs0, caches0, lat0 = _run_recorded(device, sd, d, F, "tile256")
    outs1, caches1, lat1 = _run_recorded(device, sd, d, F, "small")
    assert len(outs0) == len(outs1) == 1 + (loop.T - 1) * 3 and len(caches0) == loop.T
    for i, (a, b) in enumerate(zip(outs0, outs1)):
        assert torch.isfinite(a).all() and torch.equal(a, b), f"forward_frame call {i}"
    for f, (ca, cb) in enumerate(zip(caches0, caches1)):
        assert len(ca) == 2 * CFG.num_blocks
        for a, b in zip(ca, cb):
            assert torch.equal(a, b), f"K / V cache after frame {f}"
    assert torch.equal(lat0, lat1)


@pytest.mark.parametrize("grid,F", [((4, 6), -1), ((4, 6), 2), ((16, 20), -1)])
def test_splitk_latents_within_the_oracle_distance(device, tiny, grid, F, monkeypatch):  # noqa: F811
    splits = []
    for name in ("gemm_sm_epi", "gemm_sm_res", "gemm_sm_hnorm", "gemm_sm_qkv"):
        def spy(*args, _fn=getattr(N, name), **kw):
            splits.append(kw["split"])
            return _fn(*args, **kw)
        monkeypatch.setattr(N, name, spy)

    def model(dev, sd):
        m = loop_model(dev, sd)
        m.net.stream_gemm = "small_splitk"
        m.net.stream_gemm_force_split = 2
        return m
    loop_model = loop._model
    monkeypatch.setattr(loop, "_model", model)
    # the existing gate, by its own function, on a model in the split mode
    loop.test_tiny_net_latents_within_the_oracle_distance(device, tiny, grid, F)
    assert splits and set(splits) == {2}, "every routed launch ran the split form with S = 2"
    monkeypatch.setattr(loop, "_model", loop_model)
    sd, make, _ = tiny
    d = make(*grid)
    one = _run_recorded(device, sd, d, F, "small_splitk", 2)[2]
    two = _run_recorded(device, sd, d, F, "small_splitk", 2)[2]
    assert torch.equal(one, two)


def test_fp8_refused_and_forward_tokens_ignores_the_mode(device):
    cfg = tiny_dit(num_blocks=2)
    sd = {"net." + k: v for k, v in init_state_dict(cfg, seed=0, zero_adaln_out=False).items()}
    net = MinimalV1LVGDiT(cfg, device=device)
    net.load_state_dict(sd)
    g = torch.Generator().manual_seed(0)
    T, H, W = 3, 16, 16
    x = torch.randn(1, 16, T, H, W, generator=g).to(device).to(BF16)
    mask = torch.zeros(1, 1, T, H, W, device=device)
    mask[:, :, :1] = 1
    t = torch.tensor([[0.1, 877.0, 877.0]], device=device)
    ctx = torch.randn(1, 512, cfg.crossattn_proj_in_channels, generator=g).to(BF16).to(device)
    outs = {}
    for mode in MinimalV1LVGDiT.STREAM_GEMM_MODES:
        net.set_stream_gemm(mode)
        outs[mode] = net(x, t, ctx, condition_video_input_mask_B_C_T_H_W=mask).clone()
    assert torch.equal(outs["small"], outs["tile256"]) and torch.equal(outs["small_splitk"], outs["tile256"])
    with pytest.raises(ValueError):
        net.set_stream_gemm("small256")
    assert net.stream_gemm == "small_splitk"
    # fp8 linears: only "tile256"
    net.set_stream_gemm("tile256")
    net.set_linear_precision("fp8")
    for mode in ("small", "small_splitk"):
        with pytest.raises(ValueError):
            net.set_stream_gemm(mode)
    with pytest.raises(ValueError):
        Video2WorldInference(MODEL_NAME, device=device, net_cfg=loop.CFG, linear_precision="fp8", stream_gemm="small")
    # the attribute set directly: forward_frame itself refuses
    acfg = dataclasses.replace(loop.CFG, num_blocks=1)
    anet = MinimalV1LVGDiT(acfg, device=device)
    anet.load_state_dict({"net." + k: v for k, v in init_state_dict(acfg, seed=1, zero_adaln_out=False).items()})
    anet.set_linear_precision("fp8")
    anet.stream_gemm = "small"
    from cosmos_predict2.dit import Geometry

    geo = Geometry(T=2, Hp=4, Wp=6)
    cache = anet.make_kv_cache(1, 1, geo.hw)
    actx = anet.prepare_context(torch.randn(1, 512, acfg.crossattn_proj_in_channels, generator=g).to(BF16).to(device))
    rows = torch.zeros(geo.hw, 1, 72, dtype=BF16, device=device)
    with pytest.raises(ValueError, match="fp8"):
        anet.forward_frame(rows, torch.ones(1, 1, device=device), actx, geo, 0, None, True, cache=cache)


def test_action_streaming_inference_argument(device):
    rng = np.random.RandomState(4)
    img = rng.randint(0, 256, size=(64, 96, 3), dtype=np.uint8)
    acts = (rng.randn(12, 7) * 0.5).astype(np.float32)
    cfg1 = dataclasses.replace(loop.CFG, num_blocks=1)
    emb = torch.from_numpy(rng.randn(512, cfg1.crossattn_proj_in_channels).astype(np.float32))
    videos = {}
    for mode in (None, "small"):
        kw = {} if mode is None else dict(stream_gemm=mode)
        inf = ActionStreamingInference(emb, device=device, net_cfg=cfg1, **kw)
        assert inf.pipe.model.net.stream_gemm == (mode or "tile256")
        videos[mode] = inf.generate_action_streaming(img, acts, (64, 96), num_steps=2, seed=5, cache_frame_size=2)
        del inf
    assert tuple(videos[None].shape) == (3, 13, 64, 96) and torch.isfinite(videos[None]).all()
    assert torch.equal(videos["small"], videos[None])
    # through the pipeline's own keyword and the setup arguments' field
    pipe = Video2WorldInference(MODEL_NAME, device=device, net_cfg=cfg1, stream_gemm="small_splitk")
    assert pipe.model.net.stream_gemm == "small_splitk"
    from cosmos_predict2.config import SetupArguments

    assert SetupArguments(output_dir="out").stream_gemm == "tile256"
    assert SetupArguments(output_dir="out", stream_gemm="small").stream_gemm == "small"
    with pytest.raises(ValueError):
        SetupArguments(output_dir="out", stream_gemm="other")
