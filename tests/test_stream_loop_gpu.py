"""The streaming student's per-frame forward and loop on the device against tests/stream_truth.py.

Exact (torch.equal):
* attention over the ring cache, read in place through its strides, equals the same launch on those rows copied out
  contiguously in slot order (hw = 24 and 320, 1 .. 4 valid frames, wrapped and unwrapped rings);
* the loop with a stand-in net against the truth's loop, n_steps 1 / 2 / 4, T = 4;
* a bounded cache (cache_frame_size = F) leaves frames <= F bit-identical to the unbounded run on the tiny net;
* forward_frame(store=False) twice in a row returns identical output: a denoising pass does not disturb the history.
Toleranced: the tiny action net's latents at the 4 x 6 and 16 x 20 patch grids with cache_frame_size -1 and 2 (a
wrapped ring's key order differs from the truth's chronological one) against the truth in the oracle's bf16 and in
fp32: HIP-vs-truth <= 1.1 x oracle-bf16-vs-truth, the project's gate (tests/test_parity_depth_gpu.py).
"""
import dataclasses

import pytest
import torch

import __graft_entry__  # noqa: F401
import stream_truth as st
from cosmos_predict2 import _native as N
from cosmos_predict2.dit import Geometry, KVCache, init_state_dict
from cosmos_predict2.model import StreamingRun, Video2WorldModelRectifiedFlow
from cosmos_predict2.net_config import SAMPLER_ACTION_STREAMING, tiny_dit
from oracle import dit as odit

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
T = 4
CFG = tiny_dit(action_dim=7, action_per_latent_frame=4, timestep_scale=1.0, use_wan_fp32_strategy=False)
SMP = dataclasses.asdict(SAMPLER_ACTION_STREAMING)


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


# ----------------------------------------------------------------------------- attention over the ring
@pytest.mark.parametrize("hw", [24, 320])
@pytest.mark.parametrize("cache_frames", [3, 2, 1])
def test_ring_attention_equals_contiguous(device, hw, cache_frames):
    """Frames 0 .. 3 through a ring of cache_frames + 1 slots: 3 never wraps (1 .. 4 valid frames), 2 wraps at frame 3,
    1 at frames 2 and 3. Same kernel, same key order: bit-identical to the contiguous copy."""
    H, hd, D = 4, 128, 512
    g = torch.Generator().manual_seed(hw + cache_frames)
    k = torch.zeros((1, (cache_frames + 1) * hw, H, hd), dtype=BF16, device=device)
    ring = KVCache(batch=1, cache_frames=cache_frames, hw=hw, k=[k], v=[torch.zeros_like(k)])
    c = hd ** -0.5 * 1.4426950408889634
    kw = dict(prescaled=True, norm_bounds=(12.0 * c, 12.0))  # the weight-bound form of unit norm weights
    frames = {}
    for f in range(T):
        qkv = torch.randn(hw, 3 * D, generator=g).clamp(-3, 3).to(BF16).to(device)
        qkv[:, :D] *= c
        frames[f] = qkv
        N.kv_put(qkv, ring.k[0], ring.v[0], B=1, k_col0=D, v_col0=2 * D, row0=ring.slot(f) * hw)
        nv = ring.n_valid(f)
        order = ring.frames_attended(f)
        assert len(order) == nv == min(f, cache_frames) + 1
        q = qkv.view(hw, 1, 3 * D)[:, :, :D].view(hw, 1, H, hd).transpose(0, 1)
        kk, vv = ring.k[0][:, : nv * hw], ring.v[0][:, : nv * hw]
        got = N.attn_fwd(q, kk, vv, **kw)
        # the rows the ring should hold, rebuilt from the frames' own projections in slot order
        kc = torch.cat([frames[j][:, D:2 * D] for j in order]).view(1, nv * hw, H, hd).contiguous()
        vc = torch.cat([frames[j][:, 2 * D:] for j in order]).view(1, nv * hw, H, hd).contiguous()
        assert torch.equal(kk, kc) and torch.equal(vv, vc)
        want = N.attn_fwd(q, kc, vc, **kw)
        assert torch.equal(got, want), (f, order)
        assert torch.isfinite(got.float()).all()


# ----------------------------------------------------------------------------- the loop with a stand-in net
def _standin_truth(net_in, mask, c_noise, frame, action, store):
    a = 0.0 if action is None else float(action[0, 0, 0])
    return net_in.float() * 0.5 + (0.25 * frame - float(c_noise) + a + (0.125 if store else 0.0))


def _standin_device(rows, t_B_1, geo, frame, action, store):
    hw = rows.shape[0]
    assert rows.dtype == BF16 and tuple(rows.shape) == (hw, 1, 72) and rows.stride(0) == 128
    assert not rows[:, 0, 64:].any()  # mask and padding-mask channels: zero in this loop
    a = 0.0 if action is None else float(action[0, 0, 0])
    x = rows[:, 0, :64].float().view(hw, 16, 4).transpose(1, 2).reshape(hw, 1, 64)  # (c p) -> patch layout (p c)
    return x * 0.5 + (0.25 * frame - float(t_B_1) + a + (0.125 if store else 0.0))


@pytest.mark.parametrize("n_steps", [1, 2, 4])
def test_loop_with_standin_net_equals_truth(device, n_steps):
    H, W = 8, 12
    g = torch.Generator().manual_seed(5 + n_steps)
    gt = torch.randn(1, 16, T, H, W, generator=g)
    noise = torch.randn(1, 16, T, H, W, generator=g)
    actions = (torch.randn(1, 12, 7, generator=g) * 0.25).to(BF16)
    want = st.generate_streaming_video(SMP, gt, actions, noise, n_steps, -1, net_fn=_standin_truth)
    model = Video2WorldModelRectifiedFlow(CFG, SAMPLER_ACTION_STREAMING, device=device)
    got = model.generate_streaming_video(gt, None, actions, init_noise=noise, n_steps=n_steps, net_fn=_standin_device)
    assert got.dtype == BF16 and tuple(got.shape) == (1, 16, T, H, W)
    assert torch.equal(got.cpu(), want)
    # the seed form draws the sampler's portable noise
    from cosmos_predict2.model import arch_invariant_rand

    got2 = model.generate_streaming_video(gt, None, actions, seed=3, n_steps=n_steps, net_fn=_standin_device)
    want2 = st.generate_streaming_video(SMP, gt, actions, arch_invariant_rand((1, 16, T, H, W), torch.float32, "cpu", 3),
                                        n_steps, -1, net_fn=_standin_truth)
    assert torch.equal(got2.cpu(), want2)


# ----------------------------------------------------------------------------- the tiny net
@pytest.fixture(scope="module")
def tiny():
    """Weights, inputs and the CPU references of the tiny action net, made once per grid and left unchanged."""
    sd = {"net." + k: v for k, v in init_state_dict(CFG, seed=21, zero_adaln_out=False).items()}
    cache = {}

    def make(Hp, Wp):
        if (Hp, Wp) not in cache:
            H, W = 2 * Hp, 2 * Wp
            g = torch.Generator().manual_seed(100 + Hp)
            d = dict(gt=torch.randn(1, 16, T, H, W, generator=g), noise=torch.randn(1, 16, T, H, W, generator=g),
                     actions=(torch.randn(1, 12, 7, generator=g) * 0.5).to(BF16),
                     ctx=torch.randn(1, 512, CFG.crossattn_proj_in_channels, generator=g).to(BF16), refs={})
            cache[(Hp, Wp)] = d
        return cache[(Hp, Wp)]

    def refs(Hp, Wp, F, n_steps):
        d = make(Hp, Wp)
        if (F, n_steps) not in d["refs"]:
            c = dataclasses.asdict(CFG)
            ref = st.generate_streaming_video(SMP, d["gt"], d["actions"], d["noise"], n_steps, F,
                                              net=st.StreamNet(c, sd, d["ctx"]))
            with odit.fp32_truth():
                truth = st.generate_streaming_video(SMP, d["gt"], d["actions"], d["noise"], n_steps, F,
                                                    net=st.StreamNet(c, sd, d["ctx"]))
            d["refs"][(F, n_steps)] = (ref, truth)
        return d["refs"][(F, n_steps)]

    return sd, make, refs


def _model(device, sd):
    m = Video2WorldModelRectifiedFlow(CFG, SAMPLER_ACTION_STREAMING, device=device)
    m.load_state_dict(sd)
    return m


@pytest.mark.parametrize("F", [-1, 2])
@pytest.mark.parametrize("grid", [(4, 6), (16, 20)])
def test_tiny_net_latents_within_the_oracle_distance(device, tiny, grid, F):
    """Measured on MI355X (rel-L2 over the generated frames 1 .. 3, n_steps = 4): see DESIGN.md §6e."""
    sd, make, refs = tiny
    d = make(*grid)
    n_steps = 4
    ref, truth = refs(*grid, F, n_steps)
    assert torch.isfinite(truth).all() and torch.isfinite(ref.float()).all()
    got = _model(device, sd).generate_streaming_video(d["gt"], d["ctx"], d["actions"], init_noise=d["noise"],
                                                      n_steps=n_steps, cache_frame_size=F).cpu()
    assert torch.equal(got[:, :, 0], d["gt"][:, :, 0].to(BF16))
    hip_truth, ref_truth, hip_ref = (rel(a[:, :, 1:], b[:, :, 1:]) for a, b in ((got, truth), (ref, truth), (got, ref)))
    print(f"grid {grid} cache_frame_size {F}: hip-vs-truth {hip_truth:.3e}  bf16ref-vs-truth {ref_truth:.3e}  "
          f"hip-vs-bf16ref {hip_ref:.3e}")
    assert torch.isfinite(got.float()).all()
    assert 1e-4 < ref_truth < 0.5, ref_truth  # the oracle's own distance is finite and not degenerate
    assert hip_truth <= 1.1 * ref_truth, (hip_truth, ref_truth, hip_ref)


def test_bounded_cache_leaves_early_frames_alone(device, tiny):
    """cache_frame_size = F: frames <= F attend to every earlier frame, in the same slots as the unbounded ring, so
    they are bit-identical to it; a later frame has lost history and differs."""
    sd, make, _ = tiny
    d = make(4, 6)
    m = _model(device, sd)
    kw = dict(init_noise=d["noise"], n_steps=2)
    full = m.generate_streaming_video(d["gt"], d["ctx"], d["actions"], cache_frame_size=-1, **kw)
    for F in (1, 2):
        cut = m.generate_streaming_video(d["gt"], d["ctx"], d["actions"], cache_frame_size=F, **kw)
        assert torch.equal(cut[:, :, : F + 1], full[:, :, : F + 1]), F
        assert not torch.equal(cut[:, :, F + 1:], full[:, :, F + 1:]), F
    same = m.generate_streaming_video(d["gt"], d["ctx"], d["actions"], cache_frame_size=7, **kw)  # >= T - 1: unbounded
    assert torch.equal(same, full)


def test_denoising_pass_leaves_the_history_alone(device, tiny):
    sd, make, _ = tiny
    d = make(4, 6)
    m = _model(device, sd)
    run = StreamingRun(m, d["gt"], d["ctx"], d["actions"], init_noise=d["noise"], n_steps=2)
    run.next_frame()
    run.next_frame()  # frames 0 and 1 stored
    net, geo, hw = m.net, run.geo, run.geo.hw
    hist = [(k[:, : 2 * hw].clone(), v[:, : 2 * hw].clone()) for k, v in zip(run.cache.k, run.cache.v)]
    rows = N.stream_patchify(run.noise[2], 1.0, 0.0, None, ld=128).view(hw, 1, -1)
    t = run.steps[0]["t_B_1"]
    a = run.actions[:, 1]
    o1 = net.forward_frame(rows, t, run.ctx, geo, 2, a, False, cache=run.cache, rows_k128=True).clone()
    o2 = net.forward_frame(rows, t, run.ctx, geo, 2, a, False, cache=run.cache, rows_k128=True)
    assert torch.equal(o1, o2) and torch.isfinite(o1).all()
    for (k0, v0), k, v in zip(hist, run.cache.k, run.cache.v):
        assert torch.equal(k[:, : 2 * hw], k0) and torch.equal(v[:, : 2 * hw], v0)
        assert k[:, 2 * hw: 3 * hw].any()  # the frame's own slot was written
    # frames run in order, each once its predecessors are stored
    with pytest.raises(ValueError):
        net.forward_frame(rows, t, run.ctx, geo, 3, a, False, cache=run.cache, rows_k128=True)
    with pytest.raises(ValueError):
        net.forward_frame(rows, t, run.ctx, Geometry(T=T, Hp=geo.Hp, Wp=geo.Wp), 4, a, False, cache=run.cache)
