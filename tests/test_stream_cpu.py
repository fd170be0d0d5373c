"""CPU: the streaming student's truth (tests/stream_truth.py) checked against itself and against the ring cache's
bookkeeping (cosmos_predict2.dit.KVCache), the chunk loop's counts and seeds, and the host scalars of the loop."""
import math

import pytest
import torch

import stream_truth as st
from cosmos_predict2 import trigflow
from cosmos_predict2.dit import KVCache

BF16 = torch.bfloat16


@pytest.mark.parametrize("cache_frame_size", [-1, 1, 2, 5])
def test_ring_slots_equal_the_reference_roll(cache_frame_size):
    """T = 6: the frames each pass attends to under AttenOpWithKV's roll-by-concatenation are, as a set, the frames in
    the ring's valid slots (itself + the last min(t, F) frames); the truth lists them in chronological order."""
    T, hw, n_steps = 6, 3, 2
    F = T - 1 if cache_frame_size == -1 else min(cache_frame_size, T - 1)
    ring = KVCache(batch=1, cache_frames=F, hw=hw, k=[], v=[])
    seen = st.attended_frames(T, hw, cache_frame_size, n_steps)
    sched = st.pass_schedule(T, n_steps)
    assert len(seen) == len(sched) == 1 + (T - 1) * (n_steps + 1)
    for (frame, store), frames in zip(sched, seen):
        lo = frame - min(frame, F)
        assert frames == list(range(lo, frame + 1))  # chronological, current last
        got = ring.frames_attended(frame)
        assert sorted(got) == frames and len(got) == ring.n_valid(frame)
        # the current frame's slot is none of its history's
        assert all(ring.slot(f) != ring.slot(frame) for f in frames[:-1])
        assert got.index(frame) == ring.slot(frame)
    # F = 2: frame 5 attends to 3, 4, 5 and the ring has wrapped twice
    if cache_frame_size == 2:
        assert seen[-1] == [3, 4, 5] and ring.frames_attended(5) == [3, 4, 5]
        assert ring.frames_attended(4) == [3, 4, 2]


def test_chunk_plan():
    chunks, total = st.chunk_plan(24, seed=7)
    assert total == 1 + 2 * 12 and [c["seed"] for c in chunks] == [7, 8]
    assert [c["actions"] for c in chunks] == [(0, 12), (12, 24)]
    chunks, total = st.chunk_plan(35, seed=0)  # an incomplete last chunk is dropped (len // 12)
    assert len(chunks) == 2 and total == 25
    assert st.chunk_plan(11, seed=0) == ([], 1)


@pytest.mark.parametrize("scaling", ["rectified_flow", "edm"])
@pytest.mark.parametrize("sigma_data", [1.0, 0.5, 0.8])
def test_host_scalars_equal_the_truth(scaling, sigma_data):
    """trigflow.stream_scaling / stream_renoise (the loop's host arithmetic, CPU bf16 torch ops) give the coefficients
    of the truth's written-out fp32-then-round arithmetic, for the student times, t = 0 and a conditioned mask."""
    for t in list(st.STUDENT_TIMES) + [0.0]:
        for mask in (0.0, 1.0):
            if scaling == "edm" and (t == 0.0 or mask == 1.0):
                continue  # c_noise = log(tan t) / 4 is -inf / tiny there; the edm student is not stepped at t = 0
            tt = torch.full((1, 1, 1, 1, 1), t, dtype=BF16)
            want = st.edm_coefficients(tt, torch.full_like(tt, mask), scaling, sigma_data, 1e-4)
            c_skip, c_out, c_in, c_noise = trigflow.stream_scaling(t, mask, scaling, sigma_data, 1e-4)
            assert [c_skip, c_out, c_in, float(c_noise)] == [float(w) for w in want]
            assert all(w.dtype == BF16 for w in want)
    for t in st.STUDENT_TIMES[1:]:
        tn = torch.tensor(t, dtype=BF16)
        assert trigflow.stream_renoise(t) == (float(torch.cos(tn.float()).to(BF16)), float(torch.sin(tn.float()).to(BF16)))


def test_truth_loop_shapes_and_schedule():
    """generate_streaming_video with a stand-in net: the passes arrive in the reference's order with the reference's
    times, actions and store flags, and the output holds the conditioning frame and every last-step x0."""
    T, H, W = 4, 8, 12
    g = torch.Generator().manual_seed(0)
    gt = torch.randn(1, 16, T, H, W, generator=g)
    noise = torch.randn(1, 16, T, H, W, generator=g)
    actions = torch.randn(1, 12, 7, generator=g)
    smp = dict(selected_sampling_time=st.STUDENT_TIMES, trig_scaling="rectified_flow", sigma_data=1.0,
               sigma_conditional=1e-4)
    log = []

    def net_fn(net_in, mask, c_noise, frame, action, store):
        log.append((frame, store, float(c_noise), None if action is None else tuple(action.shape)))
        assert net_in.dtype == BF16 and float(mask.abs().max()) == 0.0
        return torch.tanh(net_in.float() * 0.5 + frame).to(BF16)

    out = st.generate_streaming_video(smp, gt, actions, noise, 2, -1, net_fn=net_fn)
    assert out.dtype == BF16 and tuple(out.shape) == (1, 16, T, H, W)
    assert torch.equal(out[:, :, 0], gt[:, :, 0].to(BF16))
    assert [(f, s) for f, s, _, _ in log] == st.pass_schedule(T, 2)
    assert log[0][2:] == (0.0, None) and all(e[3] == (1, 4, 7) for e in log[1:])
    # rectified-flow c_noise = sin / (cos + sin) of the bf16-rounded time, itself rounded to bf16; 0 at the store pass
    want = [float(st.scaling_from_time(torch.tensor(t, dtype=BF16), "rectified_flow", 1.0)[3])
            for t in st.STUDENT_TIMES[:2]]
    assert want[0] == 1.0 and abs(want[1] - 15 / 16) < 2 ** -7
    assert [e[2] for e in log[1:4]] == want + [0.0]
    assert math.isfinite(float(out.float().abs().sum()))
