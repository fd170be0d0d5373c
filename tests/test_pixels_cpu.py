"""CPU: the host pixel path pinned value by value against the float64 truth of tests/pixel_truth.py, the filter
tables of cosmos_predict2.pixels, and the frame bookkeeping of process_video_frames (no kernel launches)."""
import numpy as np
import pydantic
import pytest
import torch

import pixel_truth as PT
from cosmos_predict2 import pixels
from cosmos_predict2.config import SetupArguments
from cosmos_predict2.pipeline import process_video_frames, resize_input


def _src(hw, seed=0):
    g = torch.Generator().manual_seed(1000 * hw[0] + hw[1] + seed)
    return torch.randint(0, 256, (2, 3) + tuple(hw), generator=g, dtype=torch.uint8)


@pytest.mark.parametrize("n_in,n_out", [(96, 48), (54, 32), (53, 48), (20, 32), (100, 97), (240, 160), (190, 48),
                                        (121, 31), (7, 7), (128, 32)])
def test_aa_tables_match_truth(n_in, n_out):
    start, count, w = pixels.aa_tables(n_in, n_out)
    assert start.dtype == np.int32 and count.dtype == np.int32 and w.dtype == np.float32
    assert start.shape == count.shape == (n_out,) and w.shape[0] == n_out
    taps = w.shape[1]
    assert taps <= 9 and count.max() <= taps and count.min() >= 1
    assert np.abs(w.astype(np.float64).sum(1) - 1.0).max() <= 1e-6
    assert (start >= 0).all() and (start + count <= n_in).all() and (np.diff(start) >= 0).all()
    for i in range(n_out):
        assert not w[i, count[i]:].any()  # nothing beyond count
    # applied in float64 the tables reproduce the truth: within 1e-5 on a unit-range image, and on byte values within
    # what storing a weight as fp32 costs at most (relative 2^-24 per weight, rows sum to 1: 255 * 2^-24 = 1.52e-5;
    # a bound of 1e-5 on byte values is below that and was missed by 2 % on (54, 32) with exact float64 weights)
    u8 = np.random.RandomState(n_in).randint(0, 256, size=(5, n_in)).astype(np.float64)
    for x, bound in ((u8 / 255.0, 1e-5), (u8, 255 * 2.0 ** -24)):
        got = np.stack([(x[:, start[i]: start[i] + count[i]] * w[i, :count[i]].astype(np.float64)).sum(1)
                        for i in range(n_out)], 1)
        assert np.abs(got - x @ PT.axis_matrix(n_in, n_out).T).max() <= bound
    assert pixels.aa_tables(n_in, n_out)[2] is w  # cached


@pytest.mark.parametrize("hw,target", PT.CASES)
def test_host_resize_obeys_truth(hw, target):
    src = _src(hw)
    got = resize_input(src, target)
    assert got.shape == (2, 3) + tuple(target) and got.dtype == torch.uint8
    PT.check_bytes(got.numpy(), PT.resize_crop_truth(src.numpy(), target), f"host {hw} -> {target}")


def test_host_resize_identity_and_constant():
    src = _src((32, 48))
    assert torch.equal(resize_input(src, (32, 48)), src)
    for hw in ((54, 96), (20, 30), (121, 190)):
        const = torch.full((1, 3) + hw, 201, dtype=torch.uint8)
        assert (resize_input(const, (32, 48)) == 201).all()


@pytest.mark.parametrize("hw,resized,left", [((33, 100), (32, 97), 24), ((33, 102), (32, 99), 26)])
def test_crop_offsets_round_half_even(hw, resized, left):
    """Odd differences: round(24.5) = 24 and round(25.5) = 26 (Python's round, as the reference's center_crop)."""
    (rh, rw), (top, lf) = PT.geometry(hw, (32, 48))
    assert (rh, rw) == resized and (top, lf) == (0, left)
    assert pixels.resize_geometry(hw, (32, 48)) == ((rh, rw), (top, lf))
    src = _src(hw)
    full = PT.resize_truth(src.numpy(), rh, rw)  # uncropped
    got = resize_input(src, (32, 48)).numpy().astype(np.float64)
    assert np.abs(got - full[..., :, left: left + 48]).max() <= 0.5 + PT.MARGIN
    for other in (left - 1, left + 1):  # and no neighbouring offset fits
        assert np.abs(got - full[..., :, other: other + 48]).max() > 0.5 + PT.MARGIN


def test_to_tensor_round_trip_is_identity():
    u = torch.arange(256, dtype=torch.uint8)
    assert torch.equal(((u.float() / 255.0) * 255.0).to(torch.uint8), u)


@pytest.mark.parametrize("n", [1, 2])
def test_process_video_frames_keeps_last_and_pads(n):
    T, H, W = 7, 4, 6
    frames = (torch.arange(T, dtype=torch.uint8) * 10 + 3)[:, None, None, None].expand(T, H, W, 3).contiguous()
    out = process_video_frames(frames, (H, W), num_video_frames=9, num_latent_conditional_frames=n)
    assert out.shape == (1, 3, 9, H, W) and out.dtype == torch.uint8
    need = 4 * (n - 1) + 1
    want = [10 * t + 3 for t in range(T - need, T)] + [10 * (T - 1) + 3] * (9 - need)
    assert out[0, 0, :, 0, 0].tolist() == want
    assert (out == out[:, :1, :, :1, :1]).all()


def test_process_video_frames_rejections():
    frames = torch.zeros(3, 4, 6, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="only 3 frames"):
        process_video_frames(frames, (4, 6), 9, num_latent_conditional_frames=2)
    with pytest.raises(ValueError, match="must be 1 or 2"):
        process_video_frames(torch.zeros(9, 4, 6, 3, dtype=torch.uint8), (4, 6), 9, num_latent_conditional_frames=3,
                             validate=True)
    # the device form checks the same before it touches the GPU
    with pytest.raises(ValueError, match="only 3 frames"):
        pixels.process_video_frames_device(frames, (4, 6), 9, num_latent_conditional_frames=2)
    with pytest.raises(ValueError, match="must be 1 or 2"):
        pixels.process_video_frames_device(torch.zeros(9, 4, 6, 3, dtype=torch.uint8), (4, 6), 9, 3, validate=True)


def test_setup_arguments_pixel_path(tmp_path):
    assert SetupArguments(output_dir=tmp_path).pixel_path == "host"
    assert SetupArguments(output_dir=tmp_path, pixel_path="device").pixel_path == "device"
    with pytest.raises(pydantic.ValidationError):
        SetupArguments(output_dir=tmp_path, pixel_path="gpu")
