"""CPU: bench.py's command line and its output dump (no GPU work: the argument parser and _dump only)."""
import sys

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "3", "--warmup", "1")
    assert (a.gpus, a.steps, a.warmup) == (1, 3, 1)
    assert a.full is False and a.dump_outputs == ""
    a = _parse(monkeypatch, "--full", "--dump-outputs", "d")
    assert a.full is True and a.dump_outputs == "d"


def test_dump_whole_tensor_is_float32_and_exact(tmp_path):
    t = torch.randn(2, 3, 5, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    bench._dump(str(tmp_path), "x", t)
    got = np.load(tmp_path / "x.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 5)
    assert np.array_equal(got, t.float().numpy())


def test_dump_past_the_cap_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * 100)
    t = torch.arange(1000, dtype=torch.float32).reshape(10, 100)
    bench._dump(str(tmp_path), "a", t)
    bench._dump(str(tmp_path), "b", t + 0.0)
    a, b = np.load(tmp_path / "a.npy"), np.load(tmp_path / "b.npy")
    assert a.dtype == np.float32 and a.nbytes <= 400 and a.shape == (100,)
    assert np.array_equal(a, b)  # the same elements in every run
    assert np.all(np.diff(a) >= 0) and set(a.tolist()) <= set(range(1000))  # elements of t, in index order
