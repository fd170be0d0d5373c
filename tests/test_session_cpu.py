"""Host logic of the closed-loop sessions, no GPU: the step-to-chunk helper against a brute-force loop, the argument
rejections of open_session / step / replace that run before any device work, and the arithmetic and summary writer of
tools/bench_session.py on canned numbers."""
import importlib.util
import os
import types

import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401
from cosmos_predict2 import interactive
from cosmos_predict2.interactive import (ActionSession, ActionStreamingInference, check_step_actions,
                                         session_step_plan)


# ----------------------------------------------------------------------------- step -> chunk
@pytest.mark.parametrize("n", [1, 3, 5])
def test_step_plan_brute_force(n):
    """Walk the chunk loop: every chunk is its conditioning frame (latent frame 0) and n generated frames."""
    k = 0
    for chunk in range(7):
        for frame in range(n + 1):
            if frame == 0:
                continue  # the conditioning frame: made by the step that generates frame 1
            assert session_step_plan(k, n) == (chunk, frame, frame == 1), (k, n)
            k += 1
    assert k == 7 * n


def test_step_plan_default_is_the_chunk_of_12_actions():
    assert interactive.CHUNK_ACTIONS == 12
    assert [session_step_plan(k) for k in range(5)] == [(0, 1, True), (0, 2, False), (0, 3, False), (1, 1, True),
                                                         (1, 2, False)]
    assert session_step_plan(np.int64(7)) == (2, 2, False)
    for bad in ((-1, 3), (0, 0)):
        with pytest.raises(ValueError):
            session_step_plan(*bad)


# ----------------------------------------------------------------------------- rejections
def test_check_step_actions():
    a = check_step_actions(np.zeros((2, 4, 7)), 2, 4, 7)
    assert a.dtype == torch.float32 and tuple(a.shape) == (2, 4, 7)
    assert check_step_actions(torch.ones(2, 4, 7, dtype=torch.bfloat16), 2, 4, 7).dtype == torch.float32
    assert tuple(check_step_actions(np.zeros((3, 8, 7))[:2, ::2], 2, 4, 7).shape) == (2, 4, 7)  # a strided slice
    for bad in (None, np.zeros((4, 7)), np.zeros((2, 3, 7)), np.zeros((2, 12, 7)), np.zeros((3, 4, 7)),
                np.zeros((2, 4, 6)), torch.zeros(2, 4, 7, 1)):
        with pytest.raises(ValueError):
            check_step_actions(bad, 2, 4, 7)


def _stub_inference(per=4, pixel_path="host"):
    """ActionStreamingInference over a pipeline stub: the argument checks run before any device work."""
    net = types.SimpleNamespace(set_stream_gemm=lambda mode: None)
    tok = types.SimpleNamespace(get_latent_num_frames=lambda n: 1 + (n - 1) // 4)
    model = types.SimpleNamespace(net=net, tokenizer=tok,
                                  config=types.SimpleNamespace(sampler="dmd2_stream",
                                                               selected_sampling_time=[1.5, 1.2, 0.9, 0.5]),
                                  net_cfg=types.SimpleNamespace(action_dim=7, action_per_latent_frame=per))
    pipe = types.SimpleNamespace(model=model, device=torch.device("cpu"), pixel_path=pixel_path)
    return ActionStreamingInference(torch.zeros(8, 16), pipe=pipe)


def test_open_session_and_its_rejections():
    inf = _stub_inference()
    f = np.full((64, 96, 3), 255, dtype=np.uint8)
    sess = inf.open_session([f, f], seed=[3, 4], num_steps=9)
    assert isinstance(sess, ActionSession) and sess.B == 2 and sess.n_steps == 4  # clamped as the chunk loop clamps
    assert sess.at_chunk_start and sess.steps_done == 0
    ff = sess.first_frames  # the first piece of stream_action_chunks_batch
    assert ff.dtype == torch.float32 and tuple(ff.shape) == (2, 3, 1, 64, 96)
    assert torch.equal(ff, next(inf.stream_action_chunks_batch([f, f], np.zeros((2, 12, 7), dtype=np.float32))))
    assert torch.equal(ff, torch.full_like(ff, 255 / 128 - 1))
    # frames of unequal size that the resize makes equal are accepted
    sess = inf.open_session([f, np.zeros((32, 48, 3), dtype=np.uint8)], resolution_hw=(64, 96))
    assert tuple(sess.first_frames.shape) == (2, 3, 1, 64, 96) and (sess.H, sess.W) == (64, 96)
    with pytest.raises(ValueError):
        inf.open_session([f, np.zeros((64, 80, 3), dtype=np.uint8)])  # unequal sizes, no resize
    with pytest.raises(ValueError):
        inf.open_session([])
    with pytest.raises(ValueError):
        inf.open_session([f] * 17)
    with pytest.raises(ValueError):
        inf.open_session([f, f], seed=[1, 2, 3])
    with pytest.raises(ValueError):
        inf.open_session([f, f], output="uint8")
    with pytest.raises(ValueError):
        inf.open_session([np.zeros((60, 96, 3), dtype=np.uint8)])  # not a multiple of 16
    with pytest.raises(ValueError):
        inf.open_session([np.zeros((64, 96), dtype=np.uint8)])
    with pytest.raises(ValueError):
        _stub_inference(per=2).open_session([f])  # the chunk rules are written for 4 actions per latent frame


def test_step_and_replace_rejections():
    inf = _stub_inference()
    f = np.zeros((64, 96, 3), dtype=np.uint8)
    sess = inf.open_session([f, f], seed=[3, 4])
    for bad in (None, np.zeros((2, 12, 7)), np.zeros((2, 4, 6)), np.zeros((1, 4, 7)), np.zeros((4, 7))):
        with pytest.raises(ValueError):
            sess.step(bad)  # before any device work
    assert sess.steps_done == 0
    # replace at a chunk start: the frame, the chunk count and the seed of that session alone
    g = np.full((32, 48, 3), 255, dtype=np.uint8)
    sess._chunk = [2, 2]
    sess.replace(1, g, seed=9)
    assert sess._chunk == [2, 0] and sess._seeds == [3, 9]
    assert int(sess._frame[0].max()) == 0 and int(sess._frame[1].min()) == 255  # resized to the sessions' size
    sess.replace(0, f)
    assert sess._chunk == [0, 0] and sess._seeds == [3, 9]
    for bad_b in (-1, 2):
        with pytest.raises(ValueError):
            sess.replace(bad_b, f)
    with pytest.raises(ValueError):
        sess.replace(0, np.zeros((64, 96), dtype=np.uint8))
    for done in (1, 2, 4, 5):  # inside a chunk
        sess.steps_done = done
        assert not sess.at_chunk_start
        with pytest.raises(RuntimeError):
            sess.replace(0, f)
    sess.steps_done = 6
    assert sess.at_chunk_start
    sess.replace(0, f, seed=1)
    assert sess._seeds == [1, 9]


# ----------------------------------------------------------------------------- the measuring tool's arithmetic
def test_bench_tool_summary(tmp_path):
    path = os.path.join(__graft_entry__.ROOT, "tools", "bench_session.py")
    spec = importlib.util.spec_from_file_location("bench_session", path)
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    a = tool.parse_args([])
    assert a.res == [(256, 320), (480, 640)] and a.bs == [1, 4] and a.ms == ["tile256", "small"]
    assert a.num_steps == 4 and 3 * a.chunks >= 30  # at least 30 timed steps
    steps = [60.0, 20.0, 22.0, 64.0, 21.0, 20.0, 62.0, 20.0, 23.0]  # three chunks: opening step, two inside
    assert tool.split_steps(steps) == ([60.0, 64.0, 62.0], [20.0, 22.0, 21.0, 20.0, 20.0, 23.0])
    cfg = dict(resolution="256x320", stream_gemm="tile256", B=4)
    line = tool.summarize(cfg, steps, [186.0, 190.0, 184.0], [700.0, 690.0, 710.0], [720.0, 716.0, 724.0],
                          [120.0, 119.0, 121.5, 120.0])
    assert line["open_step_ms"] == 62.0 and line["open_step_ms_spread"] == 4.0
    assert line["step_ms"] == 20.5 and line["step_ms_spread"] == 3.0 and line["steps_inside"] == 6
    assert line["session_chunk_ms"] == pytest.approx(62.0 + 2 * 20.5)
    assert line["chunk_api_ms"] == 186.0 and line["chunk_api_ms_spread"] == 6.0
    assert line["first_frames_speedup"] == pytest.approx(3.0)
    assert line["session_frames_per_s_u8"] == pytest.approx(72 * 4 * 1e3 / 700.0)
    assert line["chunk_api_frames_per_s"] == pytest.approx(72 * 4 * 1e3 / 720.0)
    assert line["chunk_to_chunk_spread_ms"] == 2.5
    assert line["per_chunk_difference_ms"] == pytest.approx(-20.0 / 6) and line["level"] and line["session_not_slower"]
    slow = tool.summarize(cfg, steps, [186.0] * 3, [800.0] * 3, [720.0] * 3, [120.0, 121.0])
    assert not slow["level"] and not slow["session_not_slower"]
    fast = tool.summarize(cfg, steps, [186.0] * 3, [600.0] * 3, [720.0] * 3, [120.0, 121.0])
    assert not fast["level"] and fast["session_not_slower"]
    out = tmp_path / "SUMMARY.md"
    text = tool.write_summary([line, slow], str(out))
    assert out.read_text() == text
    rows = [r for r in text.splitlines() if r.startswith("| 256x320")]
    assert len(rows) == 2 and "| 4 | tile256 | 20.50 (3.00) | 62.00 (4.00) | 186.00 (6.00) | 3.00x |" in rows[0]
    assert rows[0].rstrip().endswith("| yes |") and rows[1].rstrip().endswith("| no |")
