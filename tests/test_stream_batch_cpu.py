"""Host logic of the batched streaming path, no GPU: the clips' frame-table layout against a brute-force enumeration, the
argument rejections of the batch entry points and the per-session, per-chunk seed rule."""
import types

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2 import interactive
from cosmos_predict2.interactive import ActionStreamingInference, check_batch_actions, check_equal_frames, chunk_seeds
from cosmos_predict2.model import arch_invariant_rand, session_seeds
from cosmos_predict2.vae import MAX_FRAMES, clip_table_entry, clip_table_layout


# ----------------------------------------------------------------------------- the frame table of several clips
def _kernel_entry(to, kt, Tc, Fc, stride_t):
    """The lookup of the conv kernels (csrc/vae_ops.hip), output frame `to` counted over the launch's clips: to / Tc
    by the host's Tc_inv = 65536 / Tc + 1 and a shift, exact for the at most 24 output frames of a launch."""
    clip = (to * (65536 // Tc + 1)) >> 16
    assert clip == to // Tc
    return clip * Fc + (to - clip * Tc) * stride_t + kt


@pytest.mark.parametrize("stride_t", [1, 2])
@pytest.mark.parametrize("kt", [1, 3])
def test_clip_table_layout_brute_force(kt, stride_t):
    for Tc in range(1, 19):
        for n_clips in range(1, 10):
            Fc, launches = clip_table_layout(Tc, stride_t, kt, n_clips)
            # Fc: one past the largest entry a clip's windows reach, counted by enumeration
            reach = max(f * stride_t + t for f in range(Tc) for t in range(kt)) + 1
            assert Fc == reach == (Tc - 1) * stride_t + kt
            # the launches cover the clips once, in order
            assert launches[0][0] == 0 and launches[-1][1] == n_clips
            assert all(a[1] == b[0] for a, b in zip(launches, launches[1:]))
            assert all(c1 > c0 for c0, c1 in launches)
            for c0, c1 in launches:
                n = c1 - c0
                if Fc > MAX_FRAMES:
                    assert n == 1  # a clip that overflows the table alone: the one-clip path
                    continue
                assert n * Fc <= MAX_FRAMES
                if c1 < n_clips:
                    assert (n + 1) * Fc > MAX_FRAMES  # no launch takes fewer clips than fit
                owner = {}
                for c in range(n):
                    for f in range(Tc):
                        for t in range(kt):
                            e = clip_table_entry(c, f, t, Fc, stride_t)
                            assert e == _kernel_entry(c * Tc + f, t, Tc, Fc, stride_t)
                            assert c * Fc <= e < (c + 1) * Fc <= n * Fc  # inside the clip's own run and the table
                            assert owner.setdefault(e, c) == c  # no entry is read by two clips
                if stride_t == 1 or kt >= stride_t:
                    assert len(owner) == n * Fc  # every entry of the table is read


def test_clip_table_layout_one_clip_is_the_old_index():
    for Tc in (1, 4, 22):
        Fc, launches = clip_table_layout(Tc, 1, 3, 1)
        assert launches == [(0, 1)]
        for f in range(Tc):
            for t in range(3):
                assert clip_table_entry(0, f, t, Fc, 1) == f + t


def test_clip_table_layout_known_values():
    assert clip_table_layout(2, 1, 3, 8) == (4, [(0, 6), (6, 8)])
    assert clip_table_layout(1, 1, 3, 8) == (3, [(0, 8)])
    assert clip_table_layout(8, 2, 3, 3) == (17, [(0, 1), (1, 2), (2, 3)])
    assert clip_table_layout(30, 1, 1, 2) == (30, [(0, 1), (1, 2)])
    with pytest.raises(ValueError):
        clip_table_layout(0, 1, 3, 2)
    with pytest.raises(ValueError):
        clip_table_layout(2, 1, 3, 0)


# ----------------------------------------------------------------------------- seeds
def test_seed_rule():
    assert session_seeds(5, 3) == [5, 5, 5]
    assert session_seeds([4, 9], 2) == [4, 9]
    assert session_seeds(np.int64(2), 2) == [2, 2]
    for bad in ([1, 2], [1, 2, 3, 4], []):
        with pytest.raises(ValueError):
            session_seeds(bad, 3)
    # session b's chunk c draws seed_b + c: the one-session rule (seed + chunk) per session
    assert chunk_seeds(1, 3, 0) == [1, 1, 1] and chunk_seeds(1, 3, 2) == [3, 3, 3]
    assert chunk_seeds([10, 20, 30], 3, 4) == [14, 24, 34]
    with pytest.raises(ValueError):
        chunk_seeds([1, 2], 3, 0)
    # and that seed's noise is the one-session run's draw
    a = arch_invariant_rand((1, 16, 4, 8, 12), torch.float32, "cpu", chunk_seeds([7, 3], 2, 1)[1])
    assert torch.equal(a, arch_invariant_rand((1, 16, 4, 8, 12), torch.float32, "cpu", 3 + 1))


# ----------------------------------------------------------------------------- argument rejections
def test_helper_rejections():
    assert check_batch_actions(np.zeros((2, 24, 7)), 2, 7).shape == (2, 24, 7)
    for bad in (np.zeros((24, 7)), np.zeros((3, 24, 7)), np.zeros((2, 24, 6)), np.zeros((2, 24, 7, 1))):
        with pytest.raises(ValueError):
            check_batch_actions(bad, 2, 7)
    assert check_equal_frames([(3, 64, 96), (3, 64, 96)]) == (3, 64, 96)
    with pytest.raises(ValueError):
        check_equal_frames([(3, 64, 96), (3, 64, 80)])
    with pytest.raises(ValueError):
        check_equal_frames([])


def _stub_inference():
    """ActionStreamingInference over a pipeline stub: the argument checks run before any device work."""
    net = types.SimpleNamespace(set_stream_gemm=lambda mode: None)
    model = types.SimpleNamespace(net=net, config=types.SimpleNamespace(sampler="dmd2_stream",
                                                                         selected_sampling_time=[1.5, 1.2, 0.9, 0.5]),
                                  net_cfg=types.SimpleNamespace(action_dim=7, action_per_latent_frame=4))
    pipe = types.SimpleNamespace(model=model, device=torch.device("cpu"), pixel_path="host")
    return ActionStreamingInference(torch.zeros(8, 16), pipe=pipe)


def test_entry_point_rejections():
    inf = _stub_inference()
    f = np.zeros((64, 96, 3), dtype=np.uint8)
    acts = np.zeros((2, 24, 7), dtype=np.float32)

    def first(*a, **k):
        return next(inf.stream_action_chunks_batch(*a, **k))

    piece = first([f, f], acts)  # the accepted call yields the input frames first
    assert tuple(piece.shape) == (2, 3, 1, 64, 96) and piece.dtype == torch.float32
    assert torch.equal(piece, torch.full_like(piece, -1.0))
    with pytest.raises(ValueError):
        first([f, np.zeros((64, 80, 3), dtype=np.uint8)], acts)  # unequal sizes, no resize
    with pytest.raises(ValueError):
        first([f, f], acts[0])  # [N, dim]
    with pytest.raises(ValueError):
        first([f, f], np.zeros((3, 24, 7)))  # B
    with pytest.raises(ValueError):
        first([f, f], np.zeros((2, 24, 6)))  # dim
    with pytest.raises(ValueError):
        first([f, f], acts, seed=[1, 2, 3])
    with pytest.raises(ValueError):
        first([f, f], acts, seed=[1])
    with pytest.raises(ValueError):
        inf.generate_action_streaming_batch([f, f], acts, seed=[1, 2, 3])
    # frames of unequal size that the resize makes equal are accepted
    piece = first([f, np.zeros((32, 48, 3), dtype=np.uint8)], acts, resolution_hw=(64, 96))
    assert tuple(piece.shape) == (2, 3, 1, 64, 96)
    assert interactive.CHUNK_ACTIONS == 12


# ----------------------------------------------------------------------------- the measuring tool's arithmetic
def test_bench_tool_summary_and_claim():
    import importlib.util
    import os

    path = os.path.join(__graft_entry__.ROOT, "tools", "bench_stream_batch.py")
    spec = importlib.util.spec_from_file_location("bench_stream_batch", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args(["--resolutions", "256,320:480,640", "--batches", "1,4"])
    assert a.res == [(256, 320), (480, 640)] and a.bs == [1, 4] and a.ms == ["tile256", "small"]
    assert tool.visit_order(range(3), 0) == [0, 1, 2] and tool.visit_order(range(3), 1) == [2, 1, 0]
    base = dict(resolution="256x320", stream_gemm="tile256")
    one = tool.summarize(dict(base, B=1), [180.0, 183.0, 181.0], [10.0] * 3, [50.0] * 3, 150.0)
    four = tool.summarize(dict(base, B=4), [300.0, 306.0, 303.0], [20.0] * 3, [160.0] * 3, 290.0)
    assert one["chunk_ms"] == 181.0 and one["chunk_ms_spread"] == 3.0
    assert one["ms_per_latent_frame_per_session"] == pytest.approx(181.0 / 3)
    assert four["ms_per_latent_frame_per_session"] == pytest.approx(303.0 / 12)
    assert four["session_frames_per_s_dit"] == pytest.approx(48e3 / 303.0)
    assert four["vae_share_of_chunk"] == pytest.approx(180.0 / 483.0)
    assert one["idle_share"] == pytest.approx(1 - 150.0 / 181.0)
    (c,) = tool.claim([one, four])
    assert c["holds"] and c["spread"] == pytest.approx(1.0) and c["gain"] == pytest.approx((181 / 3) / (303 / 12))
    slow = tool.summarize(dict(base, B=4), [720.0, 730.0, 725.0], [20.0] * 3, [160.0] * 3, None)
    assert not tool.claim([one, slow])[0]["holds"] and slow["idle_share"] is None
