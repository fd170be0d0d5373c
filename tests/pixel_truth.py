"""float64 truth of the pixel path's resize, shared by tests/test_pixels_cpu.py and tests/test_pixels_gpu.py.

A numpy restatement of the separable triangle filter of `interpolate(mode="bilinear", align_corners=False,
antialias=True)`, horizontal then vertical, every step in float64, nothing rounded. No torch calls.

Acceptance of a resized byte b against its truth t: |b - t| <= 0.5 + MARGIN. MARGIN = 1e-3 is derived, not tuned:
an fp32 dot product over <= 9 + 9 taps of values <= 255 is off by at most a few x 255 x 2^-24 x 18 ~ 3e-4. Outside
the tie band |frac(t) - 0.5| < MARGIN the rule admits one byte only, rint(t), so two implementations that both
pass must agree there byte for byte.
"""
import math

import numpy as np

MARGIN = 1e-3
BAND_CAP = 0.02  # at most this share of a test image's pixels may lie in the tie band

# (H, W) -> target of the resize cases; sources are torch.randint(0, 256, (2, 3, H, W)) from a seeded generator
CASES = [
    ((54, 96), (32, 48)),     # 4 taps
    ((37, 53), (32, 48)),     # odd width
    ((20, 30), (32, 48)),     # upscale, 2 taps
    ((33, 100), (32, 48)),
    ((48, 40), (32, 48)),     # the height decides the ratio
    ((135, 240), (88, 160)),
    ((121, 190), (32, 48)),   # ratio near 4, 9 taps
]


def axis_matrix(n_in: int, n_out: int) -> np.ndarray:
    """[n_out, n_in] float64 weights of one axis."""
    scale = n_in / n_out
    support = scale if scale >= 1.0 else 1.0
    m = np.zeros((n_out, n_in), np.float64)
    for i in range(n_out):
        center = scale * (i + 0.5)
        start = max(int(center - support + 0.5), 0)
        end = min(int(center + support + 0.5), n_in)
        j = np.arange(start, end, dtype=np.float64)
        w = np.maximum(0.0, 1.0 - np.abs((j - center + 0.5) / max(scale, 1.0)))
        m[i, start:end] = w / w.sum()
    return m


def geometry(hw, target):
    """resize_input's sizes: ((rh, rw), (top, left))."""
    (h, w), (th, tw) = hw, target
    r = max(tw / w, th / h)
    rh, rw = int(math.ceil(r * h)), int(math.ceil(r * w))
    return (rh, rw), (int(round((rh - th) / 2.0)), int(round((rw - tw) / 2.0)))


def resize_truth(img: np.ndarray, rh: int, rw: int) -> np.ndarray:
    """img [..., H, W] (any real dtype) -> unrounded float64 [..., rh, rw]: horizontal pass, then vertical."""
    x = np.asarray(img, np.float64)
    h = x @ axis_matrix(x.shape[-1], rw).T              # [..., H, rw]
    return np.swapaxes(np.swapaxes(h, -1, -2) @ axis_matrix(x.shape[-2], rh).T, -1, -2)


def resize_crop_truth(img: np.ndarray, target) -> np.ndarray:
    """resize_input in float64: [..., H, W] -> unrounded [..., th, tw]."""
    (rh, rw), (top, left) = geometry(img.shape[-2:], target)
    th, tw = target
    return resize_truth(img, rh, rw)[..., top: top + th, left: left + tw]


def in_band(truth: np.ndarray) -> np.ndarray:
    return np.abs(truth - np.floor(truth) - 0.5) < MARGIN


def check_bytes(got: np.ndarray, truth: np.ndarray, what: str = "") -> np.ndarray:
    """Assert the band cap (a property of the truth) and the acceptance rule; returns the out-of-band mask."""
    band = in_band(truth)
    share = band.mean()
    err = np.abs(got.astype(np.float64) - truth)
    print(f"{what}: worst |b - t| - 0.5 = {err.max() - 0.5:.3e}, tie-band share {100 * share:.3f} %")
    assert share <= BAND_CAP, f"{what}: {100 * share:.2f} % of the truth lies in the tie band"
    assert err.max() <= 0.5 + MARGIN, f"{what}: |b - t| = {err.max()}"
    assert np.array_equal(got[~band], np.rint(truth[~band]).astype(got.dtype))
    return ~band
