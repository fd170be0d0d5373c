"""B streaming sessions in lock-step (model.StreamingBatchRun) against the one-session StreamingRun, on the tiny action
net of tests/test_stream_loop_gpu.py with T = 4.

Bit identity, with the attention's key split pinned to 1 (N.set_attn_split(1), restored afterwards; the tail split's
choice of query blocks depends on a launch's workgroup count, so on the batch): session b's latents equal the B = 1 run
of that session's conditioning frame, actions and seed, for stream_gemm "tile256" and "small", B = 2, 3, 4, the 4 x 6
and 16 x 20 patch grids, an unbounded and a bounded (cache_frame_size = 2) cache; permuting the sessions permutes the
outputs.
The library's own plans (no pin, "small_splitk" included): every session of B = 2 and 4 passes the project's truth
gate, rel-L2 to tests/stream_truth.py under fp32_truth() <= 1.1 x the bf16 oracle's own distance.
The one-session runs and the CPU references are made once per module and shared.
"""
import dataclasses

import pytest
import torch

import __graft_entry__  # noqa: F401
import stream_truth as st
from cosmos_predict2 import _native as N
from cosmos_predict2.dit import init_state_dict
from cosmos_predict2.model import (StreamingBatchRun, StreamingRun, Video2WorldModelRectifiedFlow,
                                   arch_invariant_rand)
from cosmos_predict2.net_config import SAMPLER_ACTION_STREAMING, tiny_dit
from oracle import dit as odit

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
T = 4
NS = 4  # sessions made per grid
SEEDS = [11, 12, 13, 14]
CFG = tiny_dit(action_dim=7, action_per_latent_frame=4, timestep_scale=1.0, use_wan_fp32_strategy=False)
SMP = dataclasses.asdict(SAMPLER_ACTION_STREAMING)


def rel(a, b):
    return ((a.float() - b.float()).norm() / b.float().norm()).item()


@pytest.fixture(scope="module")
def tiny(device):
    sd = {"net." + k: v for k, v in init_state_dict(CFG, seed=21, zero_adaln_out=False).items()}
    model = Video2WorldModelRectifiedFlow(CFG, SAMPLER_ACTION_STREAMING, device=device)
    model.load_state_dict(sd)
    data, single, truth = {}, {}, {}

    def make(grid):
        if grid not in data:
            H, W = 2 * grid[0], 2 * grid[1]
            g = torch.Generator().manual_seed(300 + grid[0])
            data[grid] = dict(gt=torch.randn(NS, 16, T, H, W, generator=g),
                              actions=(torch.randn(NS, 12, 7, generator=g) * 0.5).to(BF16),
                              ctx=torch.randn(1, 512, CFG.crossattn_proj_in_channels, generator=g).to(BF16))
        return data[grid]

    def one(mode, grid, F, b):
        """Session b alone (StreamingRun), [1, C, T, H, W] on the device, under the caller's pins."""
        key = (mode, grid, F, b, N.set_attn_split(None))
        N.set_attn_split(key[-1])
        if key not in single:
            d = make(grid)
            model.net.set_stream_gemm(mode)
            single[key] = model.generate_streaming_video(d["gt"][b: b + 1], d["ctx"], d["actions"][b: b + 1],
                                                         seed=SEEDS[b], n_steps=4, cache_frame_size=F)
        return single[key]

    def refs(grid, F, b):
        """(bf16 oracle, fp32 truth) of session b on the CPU."""
        if (grid, F, b) not in truth:
            d = make(grid)
            H, W = 2 * grid[0], 2 * grid[1]
            c = dataclasses.asdict(CFG)
            noise = arch_invariant_rand((1, 16, T, H, W), torch.float32, "cpu", SEEDS[b])
            args = (SMP, d["gt"][b: b + 1], d["actions"][b: b + 1], noise, 4, F)
            ref = st.generate_streaming_video(*args, net=st.StreamNet(c, sd, d["ctx"]))
            with odit.fp32_truth():
                tr = st.generate_streaming_video(*args, net=st.StreamNet(c, sd, d["ctx"]))
            truth[(grid, F, b)] = (ref, tr)
        return truth[(grid, F, b)]

    yield model, make, one, refs
    model.net.set_stream_gemm("tile256")


@pytest.fixture
def no_attn_split():
    prev = N.set_attn_split(1)
    yield
    N.set_attn_split(prev)


def _batch(model, d, mode, sessions, F, seeds=None):
    model.net.set_stream_gemm(mode)
    idx = torch.tensor(sessions)
    return model.generate_streaming_video_batch(d["gt"][idx], d["ctx"], d["actions"][idx],
                                                seed=seeds or [SEEDS[b] for b in sessions], n_steps=4,
                                                cache_frame_size=F)


@pytest.mark.parametrize("grid", [(4, 6), (16, 20)])
@pytest.mark.parametrize("B", [2, 3, 4])
@pytest.mark.parametrize("mode", ["tile256", "small"])
def test_sessions_equal_their_one_session_runs(device, tiny, no_attn_split, mode, B, grid):
    model, make, one, _ = tiny
    d = make(grid)
    got = _batch(model, d, mode, list(range(B)), -1)
    assert got.dtype == BF16 and tuple(got.shape) == (B, 16, T, 2 * grid[0], 2 * grid[1])
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got[:, :, 0].cpu(), d["gt"][:B, :, 0].to(BF16))
    singles = [one(mode, grid, -1, b) for b in range(B)]
    assert not torch.equal(singles[0], singles[1])  # the sessions differ
    for b in range(B):
        diff = rel(got[b: b + 1], singles[b])
        print(f"{mode} B {B} grid {grid} session {b}: rel-L2 to its one-session run {diff:.3e}")
        assert torch.equal(got[b: b + 1], singles[b]), (mode, B, grid, b, diff)


@pytest.mark.parametrize("mode", ["tile256", "small"])
def test_bounded_cache_sessions_equal_their_one_session_runs(device, tiny, no_attn_split, mode):
    model, make, one, _ = tiny
    grid, B = (4, 6), 3
    d = make(grid)
    got = _batch(model, d, mode, list(range(B)), 2)
    for b in range(B):
        assert torch.equal(got[b: b + 1], one(mode, grid, 2, b)), (mode, b)
    assert not torch.equal(got, _batch(model, d, mode, list(range(B)), -1))  # the bound shows in frame 3


@pytest.mark.parametrize("mode", ["tile256", "small"])
def test_permuting_the_sessions_permutes_the_outputs(device, tiny, no_attn_split, mode):
    model, make, _, _ = tiny
    d = make((4, 6))
    base = _batch(model, d, mode, [0, 1, 2], -1)
    perm = [2, 0, 1]
    got = _batch(model, d, mode, perm, -1)
    assert torch.equal(got, base[torch.tensor(perm)])
    # an int seed gives every session the one-session draw of that seed
    same = _batch(model, d, mode, [1, 1], -1, seeds=12)
    assert torch.equal(same[0], same[1]) and torch.equal(same[0], base[1])


def test_run_interface(device, tiny):
    model, make, _, _ = tiny
    d = make((4, 6))
    model.net.set_stream_gemm("tile256")
    run = StreamingBatchRun(model, d["gt"][:2], d["ctx"], d["actions"][:2], seed=[11, 12])
    ref = StreamingRun(model, d["gt"][:1], d["ctx"], d["actions"][:1], seed=11)
    assert torch.equal(run.noise[:, :, 0], ref.noise) and run.cache.batch == 2 and run.ctx.B == 2
    assert [run.next_frame() for _ in range(T)] == list(range(T)) and run.done
    with pytest.raises(RuntimeError):
        run.next_frame()
    assert tuple(run.latents().shape) == (2, 16, T, 8, 12)
    for bad in (dict(gt=d["gt"][0]), dict(actions=d["actions"][:3]), dict(seed=[1, 2, 3]),
                dict(init_noise=torch.zeros(1, 16, T, 8, 12))):
        kw = dict(dict(gt=d["gt"][:2], actions=d["actions"][:2], seed=1), **bad)
        with pytest.raises(ValueError):
            StreamingBatchRun(model, kw.pop("gt"), d["ctx"], kw.pop("actions"), **kw)
    with pytest.raises(ValueError):
        StreamingBatchRun(model, d["gt"][:1].expand(17, -1, -1, -1, -1), d["ctx"], d["actions"][:1].expand(17, -1, -1))


@pytest.mark.parametrize("B", [2, 4])
@pytest.mark.parametrize("mode", ["tile256", "small", "small_splitk"])
def test_own_plans_pass_the_truth_gate(device, tiny, mode, B):
    """No pin: the attention's own split plan and the small-M family's own K split."""
    model, make, _, refs = tiny
    grid = (4, 6)
    d = make(grid)
    got = _batch(model, d, mode, list(range(B)), -1).cpu()
    for b in range(B):
        ref, truth = refs(grid, -1, b)
        hip_truth, ref_truth = rel(got[b: b + 1, :, 1:], truth[:, :, 1:]), rel(ref[:, :, 1:], truth[:, :, 1:])
        print(f"{mode} B {B} session {b}: hip-vs-truth {hip_truth:.3e}  bf16ref-vs-truth {ref_truth:.3e}")
        assert 1e-4 < ref_truth < 0.5, ref_truth
        assert hip_truth <= 1.1 * ref_truth, (mode, B, b, hip_truth, ref_truth)
