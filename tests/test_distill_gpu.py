"""The distilled (DMD2 / TrigFlow) few-step sampler on the device against tests/distill_truth.py.

* cp25_trig_patchify_ld / cp25_trig_x0_step: bit for bit (torch.equal) against the reference's float64 op sequence
  evaluated with CPU torch, over both scalings, the four student times with 0 / 1 / 2 conditioning frames (whose
  frames sit at t_cond), sigma_data in {1, 0.5, 0.8} (a real fp64 division), whole ranges and a token shard that
  starts and ends inside frames. A contracted multiply-add, an fp32 shortcut or a single float64 -> bf16 rounding
  fails them: the inputs carry elements on which the one-step and two-step roundings differ (premise asserted in
  tests/test_distill_cpu.py and again here).
* the loop's plumbing with a stand-in denoiser: bit for bit, as test_dit_gpu.test_sampler_plumbing_bit_exact does for
  UniPC; CP = 2 over gloo against CP = 1: bit for bit.
* the tiny student end to end against the oracle DiT: rel-L2 <= 1e-2, the project's bound for its unguided sampler on
  this net and geometry (test_dit_gpu.py:112-120); also at a 4 x 6 latent, where every gated residual is unfused and
  the bf16 final layer takes the last MLP residual itself.
"""
import dataclasses
import math
import os
import socket
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import __graft_entry__  # noqa: F401
import distill_truth as DT
from cosmos_predict2 import _native as N
from cosmos_predict2 import trigflow
from cosmos_predict2.model import from_patch_layout, to_patch_layout
from cosmos_predict2.net_config import SAMPLER_2B_DISTILLED, tiny_dit
from oracle import sampler as osamp

pytestmark = pytest.mark.gpu

TIMES = DT.TIMES_4STEP
T, HP, WP = 3, 2, 3
HW, L, H, W = HP * WP, T * HP * WP, 2 * HP, 2 * WP
SHARDS = ((0, L), (5, 8))  # the whole range; a shard that starts inside frame 0 and ends inside frame 2


def rel_l2(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.fixture(scope="module")
def data():
    """Inputs shared by the kernel tests (never modified): x / gt / net / noise [1, 16, T, H, W] fp32. The last frame
    of x (never a conditioning frame here) carries inputs whose product with c_in(atan 5) rounds differently to bf16
    in one step and in two."""
    g = torch.Generator().manual_seed(40)
    d = {k: torch.randn(1, 16, T, H, W, generator=g) for k in ("x", "gt", "net", "noise")}
    c_in = trigflow.trig_scaling(torch.tensor([TIMES[2]], dtype=torch.float64), "rectified_flow", 1.0)[2].item()
    planted = DT.double_rounding_inputs(c_in)
    assert planted.numel() >= 16, planted.numel()
    k = min(planted.numel(), 16 * H * W)
    last = d["x"][0, :, T - 1].clone().flatten()
    last[:k] = planted[:k]
    d["x"][0, :, T - 1] = last.view(16, H, W)
    d["c_in_atan5"], d["n_planted"] = c_in, k
    return d


def _mask(n_cond):
    return osamp.frame_mask(1, T, H, W, n_cond or 0)


def _tables(t, n_cond, scaling, sd, device):
    fm = _mask(n_cond)[0, 0, :, 0, 0].contiguous()
    tf = trigflow.frame_times(t, fm, 1e-4, sd)
    c_skip, c_out, c_in, c_noise = trigflow.trig_scaling(tf, scaling, sd)
    return fm.to(device), c_skip.to(device), c_out.to(device), c_in.to(device)


def _rows_ref(xb, n_cond, pad=None):
    """The x_embedder rows of the truth's bf16 net input [1, 16, T, H, W]: feature c * 4 + p, mask and pad channels."""
    xin = to_patch_layout(xb[0].float()).to(torch.bfloat16)  # [L, (p c)]
    ref = torch.zeros(L, 72, dtype=torch.bfloat16)
    ref[:, :64] = xin.view(L, 4, 16).transpose(1, 2).reshape(L, 64)
    ref[:, 64:68] = _mask(n_cond)[0, 0, :, 0, 0][torch.arange(L) // HW][:, None].to(torch.bfloat16)
    if pad is not None:
        ref[:, 68:72] = pad
    return ref


@pytest.mark.parametrize("sigma_data", [1.0, 0.5, 0.8])
@pytest.mark.parametrize("scaling", ["rectified_flow", "edm"])
def test_trig_patchify_equals_truth(device, data, scaling, sigma_data):
    x5, gt5 = data["x"], data["gt"]
    xp, gtp = to_patch_layout(x5[0]).to(device), to_patch_layout(gt5[0]).to(device)
    pad = (torch.arange(L * 4) % 3 == 0).to(torch.bfloat16).view(L, 4)
    checked = 0
    for t in TIMES:
        for n_cond in (0, 1, 2, None):  # None: no conditioning latent at all (gt == NULL)
            time_B = torch.tensor([t], dtype=torch.float64)
            xb, _, st = DT.net_input(x5, time_B, gt5 if n_cond is not None else torch.zeros_like(gt5), _mask(n_cond),
                                     scaling=scaling, sigma_data=sigma_data)
            fm, _, _, c_in = _tables(t, n_cond, scaling, sigma_data, device)
            assert torch.equal(c_in.cpu(), st["c_in"].flatten().expand(T))  # the product's table = the truth's
            if scaling == "rectified_flow" and sigma_data == 1.0 and t == TIMES[2]:
                # the premise on the very elements compared: a single float64 -> bf16 rounding differs on >= 16 of them
                one_step = DT.bf16_direct(x5[0, :, T - 1].double() * data["c_in_atan5"])
                assert (one_step != xb[0, :, T - 1]).sum().item() >= 16
            for tok0, n in SHARDS:
                for ld in (72, 128):
                    for pm in (None, pad):
                        ref = _rows_ref(xb, n_cond, pm)[tok0:tok0 + n]
                        rows = N.trig_patchify(xp[tok0:tok0 + n], None if n_cond is None else gtp[tok0:tok0 + n], fm,
                                               c_in, sigma_data, None if pm is None else pm[tok0:tok0 + n].to(device),
                                               tok0=tok0, hw=HW, ld=ld)
                        assert rows.shape == (n, 72) and rows.stride(0) == ld
                        assert torch.equal(rows.cpu(), ref), (t, n_cond, tok0, ld)
                        if ld > 72:
                            whole = torch.as_strided(rows, (n, ld), (ld, 1))
                            assert not whole[:, 72:].any()
                        checked += 1
    assert checked == 4 * 4 * 2 * 2 * 2
    assert torch.equal(xp.cpu(), to_patch_layout(x5[0])) and torch.equal(gtp.cpu(), to_patch_layout(gt5[0]))


@pytest.mark.parametrize("sigma_data", [1.0, 0.5, 0.8])
@pytest.mark.parametrize("scaling", ["rectified_flow", "edm"])
def test_trig_x0_step_equals_truth(device, data, scaling, sigma_data):
    x5, gt5, noise5 = data["x"], data["gt"], data["noise"]
    net_bad = data["net"].clone()  # last = 1: non-finite net outputs, in conditioning frames as well
    for j, (f, v) in enumerate(((0, float("nan")), (0, float("inf")), (1, float("-inf")), (2, float("nan")),
                                (2, float("inf")), (2, float("-inf")))):
        net_bad[0, j, f, j % H, j % W] = v
    xp0, gtp, noisep = (to_patch_layout(a[0]).to(device) for a in (x5, gt5, noise5))
    nets = {0: to_patch_layout(data["net"][0]).to(device), 1: to_patch_layout(net_bad[0]).to(device)}
    keep = {k: v.clone() for k, v in (("gt", gtp), ("noise", noisep), ("net0", nets[0]), ("net1", nets[1]))}
    checked = 0
    for i, t in enumerate(TIMES):
        t_next = TIMES[(i + 1) % 4]
        for n_cond in (0, 1, 2, None):
            time_B = torch.tensor([t], dtype=torch.float64)
            gt_truth = gt5 if n_cond is not None else torch.zeros_like(gt5)
            _, _, st = DT.net_input(x5, time_B, gt_truth, _mask(n_cond), scaling=scaling, sigma_data=sigma_data)
            fm, c_skip, c_out, _ = _tables(t, n_cond, scaling, sigma_data, device)
            for last in (0, 1):
                net5 = net_bad if last else data["net"]
                for replace_gt in (0, 1):
                    x0 = DT.x0_from_net(x5, net5, gt_truth, st, replace_gt=bool(replace_gt))
                    if last:
                        want5 = torch.nan_to_num(x0.float())
                        assert not torch.isfinite(x0).all() and torch.isfinite(want5).all()  # the planted values
                    else:
                        want5 = DT.renoise(x0.to(torch.float64), t_next, noise5, sigma_data).float()
                    want = to_patch_layout(want5[0])
                    for tok0, n in SHARDS:
                        xs = xp0[tok0:tok0 + n].clone()
                        out = N.trig_x0_step(xs, nets[last][tok0:tok0 + n].view(n, 1, 64), noisep[tok0:tok0 + n],
                                             None if n_cond is None else gtp[tok0:tok0 + n], fm, c_skip, c_out,
                                             replace_gt=bool(replace_gt), sigma_data=sigma_data,
                                             cos_next=math.cos(t_next), sin_next=math.sin(t_next), last=bool(last),
                                             tok0=tok0, hw=HW)
                        assert out is xs  # in place
                        assert torch.equal(xs.cpu(), want[tok0:tok0 + n]), (t, n_cond, last, replace_gt, tok0)
                        checked += 1
    assert checked == 4 * 4 * 2 * 2 * 2
    for k, v in (("gt", gtp), ("noise", noisep), ("net0", nets[0]), ("net1", nets[1])):
        assert torch.equal(v.view(torch.int32), keep[k].view(torch.int32)), k  # inputs untouched (bits: NaNs too)
    # last = 1 needs no noise
    fm, c_skip, c_out, _ = _tables(TIMES[3], 1, scaling, sigma_data, device)
    a, b = xp0.clone(), xp0.clone()
    kw = dict(replace_gt=True, sigma_data=sigma_data, cos_next=1.0, sin_next=0.0, last=True, tok0=0, hw=HW)
    N.trig_x0_step(a, nets[0].view(L, 1, 64), None, gtp, fm, c_skip, c_out, **kw)
    N.trig_x0_step(b, nets[0].view(L, 1, 64), noisep, gtp, fm, c_skip, c_out, **kw)
    assert torch.equal(a, b)


def test_trig_host_refusals(device):
    n = 8
    lib = N.load_library()
    fm = torch.zeros(T, device=device)
    tab = torch.ones(T, dtype=torch.float64, device=device)
    buf = torch.zeros(n * 64 + 4, device=device)
    good, mis = buf[: n * 64].view(n, 64), buf[1: 1 + n * 64].view(n, 64)  # 4 bytes off a 16-byte boundary
    assert good.data_ptr() % 16 == 0 and mis.data_ptr() % 16 == 4
    out = torch.empty(n, 72, dtype=torch.bfloat16, device=device)
    args = lambda xs: (xs.data_ptr(), None, fm.data_ptr(), tab.data_ptr(), 1.0, None, out.data_ptr(), 72, n, 0, HW,  # noqa: E731
                       torch.cuda.current_stream().cuda_stream)
    assert lib.cp25_trig_patchify_ld(*args(good)) == 0
    assert lib.cp25_trig_patchify_ld(*args(mis)) == -22
    kw = dict(replace_gt=True, sigma_data=1.0, cos_next=0.5, sin_next=0.5, last=False, tok0=0, hw=HW)
    net = torch.zeros(n, 1, 64, device=device)
    noise = torch.zeros(n, 64, device=device)
    with pytest.raises(ValueError, match="-22"):
        N.trig_patchify(mis, None, fm, tab, 1.0, None, tok0=0, hw=HW)
    with pytest.raises(ValueError, match="-22"):
        N.trig_patchify(good, mis, fm, tab, 1.0, None, tok0=0, hw=HW)
    with pytest.raises(ValueError, match="-22"):
        N.trig_x0_step(mis, net, noise, None, fm, tab, tab, **kw)
    with pytest.raises(ValueError, match="-22"):
        N.trig_x0_step(good, net, mis, None, fm, tab, tab, **kw)
    with pytest.raises(ValueError, match="-22"):
        N.trig_x0_step(good, net, noise, mis, fm, tab, tab, **kw)
    with pytest.raises(ValueError, match="-22"):  # sigma_data must be positive
        N.trig_patchify(good, None, fm, tab, 0.0, None, tok0=0, hw=HW)
    with pytest.raises(ValueError, match="-22"):  # rows narrower than the 72 features
        N.trig_patchify(good, None, fm, tab, 1.0, None, tok0=0, hw=HW, ld=64)
    # a mask (and tables) too short for tok0: tokens [16, 24) are frame 2..3 of a 3-frame mask
    with pytest.raises(ValueError, match="mask"):
        N.trig_patchify(good, None, fm, tab, 1.0, None, tok0=16, hw=HW)
    with pytest.raises(ValueError, match="mask"):
        N.trig_x0_step(good, net, noise, None, fm, tab, tab, **dict(kw, tok0=16))
    # tables: float64, one entry per mask frame
    with pytest.raises(ValueError, match="float64"):
        N.trig_patchify(good, None, fm, tab.float(), 1.0, None, tok0=0, hw=HW)
    with pytest.raises(ValueError, match="float64"):
        N.trig_x0_step(good, net, noise, None, fm, tab[:2], tab, **kw)
    with pytest.raises(ValueError):
        N.trig_x0_step(good, net, None, None, fm, tab, tab, **kw)  # not last: the noise is needed
    assert not buf.any()  # nothing was launched on the refused calls


# ---------------------------------------------------------------- the loop
def _fake(xv, tv):
    """Deterministic stand-in denoiser evaluated on the CPU (same bits on both paths)."""
    return torch.sin(xv.float() * 1.25 + tv)


def _truth_fn(timestep_scale):
    def fn(c, s, x, t, ctx, mask):  # x bf16 [1, C, T, H, W], t bf16 [1, T]: the net scales it in its own dtype
        ts = (t * timestep_scale).float()[0]
        return _fake(x, ts[None, None, :, None, None])
    return fn


def _device_fn(rows, t_B_T, geo):
    assert t_B_T.shape == (1, geo.T) and rows.shape == (geo.n_tok, 1, 72)
    r = rows.cpu()[:, 0, :64].view(-1, 16, 4).transpose(1, 2).reshape(-1, 64)  # (c p) -> (p c)
    tok_t = (geo.tok0 + torch.arange(geo.n_tok)) // geo.hw
    return _fake(r, t_B_T.cpu()[0][tok_t][:, None]).view(-1, 1, 64).to(rows.device)


def _model(cfg, scfg, device):
    from cosmos_predict2.model import Video2WorldModelRectifiedFlow

    return Video2WorldModelRectifiedFlow(cfg, scfg, device=device)


@pytest.mark.parametrize("num_steps", [1, 2, 4, 35])
@pytest.mark.parametrize("ncond", [0, 1, 2])
def test_distilled_plumbing_bit_exact(device, ncond, num_steps):
    """DistilledSamplingRun against the truth loop with an identical stand-in denoiser: tables, preconditioning,
    frame replacement, the timesteps' cast, x0, re-noising and the final nan_to_num must agree bit for bit."""
    cfg = tiny_dit(timestep_scale=1.0, use_wan_fp32_strategy=False)
    Ts, Hs, Ws = 3, 8, 12
    gt = torch.randn(1, 16, Ts, Hs, Ws, generator=torch.Generator().manual_seed(21))
    ctx = torch.zeros(1, 4, 8)
    ref = DT.generate(None, None, gt, ctx, num_cond=ncond, seed=3, num_steps=num_steps,
                      dit_fn=_truth_fn(cfg.timestep_scale))
    model = _model(cfg, SAMPLER_2B_DISTILLED, device)
    run = model.begin_sampling(gt.to(device) if ncond else None, ctx, None, state_shape=(16, Ts, Hs, Ws),
                               num_conditional_frames=ncond, guidance=7.0, seed=3, num_steps=num_steps,
                               net_fn=_device_fn)
    assert run.num_evals == min(num_steps, 4) and not run.done
    out = model.sample_latents(gt.to(device) if ncond else None, ctx, None, state_shape=(16, Ts, Hs, Ws),
                               num_conditional_frames=ncond, guidance=7.0, seed=3, num_steps=num_steps,
                               net_fn=_device_fn)
    assert torch.equal(out.cpu(), ref)
    if ncond and num_steps == 4:  # the steppable interface: step / done / restart give the same trajectory
        for rep in range(2):
            idx = []
            while not run.done:
                idx.append(run.step())
            assert idx == [0, 1, 2, 3] and torch.equal(run.latents().cpu(), ref)
            with pytest.raises(RuntimeError):
                run.step()
            run.restart()


@pytest.mark.parametrize("variant", ["change_time_embed", "edm_sigma0.8", "scale0.001_init_noise", "no_replace_gt"])
def test_distilled_plumbing_variants(device, variant):
    cfg = tiny_dit(timestep_scale=1.0, use_wan_fp32_strategy=False)
    scfg, kw, init = SAMPLER_2B_DISTILLED, {}, None
    Ts, Hs, Ws = 3, 8, 12
    if variant == "change_time_embed":
        scfg, kw = dataclasses.replace(scfg, change_time_embed=True), dict(change_time_embed=True)
    elif variant == "edm_sigma0.8":
        scfg = dataclasses.replace(scfg, trig_scaling="edm", sigma_data=0.8, sigma_conditional=0.02)
        kw = dict(scaling="edm", sigma_data=0.8, sigma_conditional=0.02)
    elif variant == "scale0.001_init_noise":  # the rectified-flow nets' timestep scale, and a caller's own noise
        cfg = tiny_dit()
        init = torch.randn(1, 16, Ts, Hs, Ws, generator=torch.Generator().manual_seed(5))
    else:
        scfg, kw = dataclasses.replace(scfg, denoise_replace_gt_frames=False), dict(replace_gt=False)
    gt = torch.randn(1, 16, Ts, Hs, Ws, generator=torch.Generator().manual_seed(22))
    ctx = torch.zeros(1, 4, 8)
    ref = DT.generate(None, None, gt, ctx, num_cond=2, seed=4, num_steps=4, dit_fn=_truth_fn(cfg.timestep_scale),
                      init_noise=init, **kw)
    out = _model(cfg, scfg, device).sample_latents(gt.to(device), ctx, None, state_shape=(16, Ts, Hs, Ws),
                                                   num_conditional_frames=2, guidance=0.0, seed=4, num_steps=4,
                                                   net_fn=_device_fn, init_noise=init)
    assert torch.equal(out.cpu(), ref)


def _student_case(Ts, Hs, Ws, seed=1):
    from cosmos_predict2.dit import init_state_dict

    cfg = tiny_dit(num_blocks=2, timestep_scale=1.0, use_wan_fp32_strategy=False)
    sd = {"net." + k: v for k, v in init_state_dict(cfg, seed=seed, zero_adaln_out=False).items()}
    g = torch.Generator().manual_seed(20)
    gt = torch.randn(1, 16, Ts, Hs, Ws, generator=g)
    ctx = torch.randn(1, 512, cfg.crossattn_proj_in_channels, generator=g).to(torch.bfloat16)
    return cfg, sd, gt, ctx


def _student_vs_truth(device, Ts, Hs, Ws):
    cfg, sd, gt, ctx = _student_case(Ts, Hs, Ws)
    ref = DT.generate(dataclasses.asdict(cfg), sd, gt, ctx, num_cond=1, seed=0, num_steps=4)
    model = _model(cfg, SAMPLER_2B_DISTILLED, device)
    model.load_state_dict(sd)
    model.hip_graph = True  # ignored by the distilled run
    out = model.sample_latents(gt.to(device), ctx.to(device), None, state_shape=(16, Ts, Hs, Ws),
                               num_conditional_frames=1, guidance=7.0, seed=0, num_steps=4)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(out[0, :, 0].cpu(), gt[0, :, 0])  # the conditioning frame comes back as given (replace_gt)
    return rel_l2(out.cpu(), ref)


def test_tiny_student_matches_truth(device):
    err = _student_vs_truth(device, 3, 16, 16)
    print(f"distilled tiny student (4 steps, 1 conditioning frame, 3x16x16) vs truth rel-L2: {err:.3e}")
    assert err <= 1e-2, err


def test_tiny_student_small_frames_unfused_residual(device):
    """A 4 x 6 latent: no gated residual is fused (gemm_res_supported), so the bf16-conditioning final layer's LN-mod
    takes the last MLP residual with a gate and a shift / scale of different layouts (it raised before)."""
    assert not N.gemm_res_supported(512, 512, 1, 6)
    err = _student_vs_truth(device, 3, 4, 6)
    print(f"distilled tiny student at a 4 x 6 latent (unfused residual path) vs truth rel-L2: {err:.3e}")
    assert err <= 1e-2, err


# ---------------------------------------------------------------- CP = 2 over gloo on one device
def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cp_runs(dev):
    """Both CP cases on the current process group (or none): the stand-in loop and the tiny student."""
    cfg = tiny_dit(timestep_scale=1.0, use_wan_fp32_strategy=False)
    gt = torch.randn(1, 16, 3, 8, 12, generator=torch.Generator().manual_seed(23))
    m = _model(cfg, SAMPLER_2B_DISTILLED, dev)
    if dist.is_initialized():
        m.set_context_parallel_group(dist.group.WORLD)
    a = m.sample_latents(gt.to(dev), torch.zeros(1, 4, 8), None, state_shape=(16, 3, 8, 12), num_conditional_frames=1,
                         guidance=7.0, seed=2, num_steps=4, net_fn=_device_fn).cpu()
    del m
    # 768 tokens: 384 per rank, as tests/test_cp_gpu.py's case (every GEMM keeps its kernel at M = 384)
    cfg, sd, gt, ctx = _student_case(3, 16, 64, seed=3)
    m = _model(cfg, SAMPLER_2B_DISTILLED, dev)
    m.load_state_dict(sd)
    if dist.is_initialized():
        m.set_context_parallel_group(dist.group.WORLD)
    b = m.sample_latents(gt.to(dev), ctx.to(dev), None, state_shape=(16, 3, 16, 64), num_conditional_frames=1,
                         guidance=7.0, seed=0, num_steps=4).cpu()
    return a, b


def _cp_worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    N.set_attn_split(1)  # no key-range split: every attention row sees the same keys in the same order
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        a, b = _cp_runs(torch.device("cuda:0"))
        q.put((rank, a.numpy(), b.numpy()))  # by value: a shared-memory fd dies with this process
    finally:
        dist.destroy_process_group()


def test_distilled_cp2_matches_cp1(device, monkeypatch):
    """Two ranks over gloo sharing cuda:0 (launched as tests/test_cp_gpu.py launches its ranks, key-range split
    disabled): rank r owns tokens [r L / 2, (r + 1) L / 2), shards that start and end inside frames; the gathered
    latents equal CP = 1 bit for bit, with the stand-in denoiser and with the tiny student."""
    monkeypatch.setattr(N, "_ATTN_SPLIT", 1)
    ref = _cp_runs(device)
    torch.cuda.empty_cache()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_cp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in ps:
        p.start()
    res = {r: (torch.from_numpy(a), torch.from_numpy(b)) for r, a, b in (q.get(timeout=100) for _ in ps)}
    for p in ps:
        p.join(timeout=120)
    assert all(p.exitcode == 0 for p in ps)
    for k, name in enumerate(("stand-in", "tiny student")):
        assert torch.equal(res[0][k], res[1][k]), name  # every rank ends with the full gathered latent
        assert torch.isfinite(ref[k]).all() and torch.equal(res[0][k], ref[k]), name


# ---------------------------------------------------------------- the user API
def test_inference_api_distilled(device, tmp_path):
    """Inference(SetupArguments(model="2B/distilled")) end to end (mirrors test_inference_gpu.py): an .mp4 of the
    right shape, the same file on a second call, and the same bytes whatever the guidance (accepted and ignored)."""
    from PIL import Image

    from cosmos_predict2.config import InferenceArguments, SetupArguments
    from cosmos_predict2.inference import Inference
    from cosmos_predict2.model import DistilledSamplingRun
    from cosmos_predict2.video_io import read_mp4

    img = np.random.RandomState(0).randint(0, 256, size=(96, 160, 3), dtype=np.uint8)
    Image.fromarray(img).save(tmp_path / "in.png")
    out = tmp_path / "out"
    inf = Inference(SetupArguments(output_dir=out, model="2B/distilled", state_t=2, keep_going=False))
    assert inf.pipe.model.config.sampler == "dmd2"
    run = inf.pipe.model.begin_sampling(None, torch.zeros(1, 4, 100352, dtype=torch.bfloat16, device=device), None,
                                        state_shape=(16, 2, 8, 16), num_conditional_frames=0, guidance=7, seed=0,
                                        num_steps=35, net_fn=_device_fn)
    assert isinstance(run, DistilledSamplingRun) and run.num_evals == 4
    common = dict(prompt="A robot arm stacks two cubes.", resolution="64,128", num_output_frames=5,
                  inference_type="image2world", input_path=tmp_path / "in.png")
    vids = {}
    for name, g in (("g7", 7), ("g7_again", 7), ("g0", 0)):
        paths = inf.generate([InferenceArguments(name=name, guidance=g, **common)], out)
        assert len(paths) == 1 and paths[0].endswith(".mp4")
        vids[name] = Path(paths[0]).read_bytes()
    v = read_mp4(str(out / "g7.mp4"))
    assert v.shape == (5, 64, 128, 3) and v.dtype == np.uint8
    assert (out / "g7.json").exists()
    assert vids["g7"] == vids["g7_again"]
    assert vids["g7"] == vids["g0"]
