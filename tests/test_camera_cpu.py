"""Camera-conditioned Video2World, the parts that need no GPU: the net option's state dict, the MODELS entry, the
three-segment layout (reorder and mask), argument validation, and the float64 Pluecker truth the GPU test gates
cp25_plucker_tokens against (tests/camera_truth.py), with the premise of that gate."""
import math

import numpy as np
import pydantic
import pytest
import torch

import camera_truth as ct
from cosmos_predict2 import camera as cam
from cosmos_predict2.config import SetupArguments
from cosmos_predict2.dit import MinimalV1LVGDiT, init_state_dict, state_dict_shapes
from cosmos_predict2.model import camera_frame_mask
from cosmos_predict2.net_config import DIT_2B, MODELS, tiny_dit

BF16 = torch.bfloat16


# ----------------------------------------------------------------------------- net option
def test_state_dict_keys_and_shapes():
    cfg = tiny_dit(camera_dim=1536)
    shapes, plain = state_dict_shapes(cfg), state_dict_shapes(tiny_dit())
    extra = sorted(set(shapes) - set(plain))
    assert extra == [f"blocks.{i}.cam_encoder.weight" for i in range(cfg.num_blocks)]
    assert all(shapes[k] == ((cfg.model_channels, 1536), BF16) for k in extra)
    assert all(shapes[k] == plain[k] for k in plain)
    sd = init_state_dict(cfg, seed=0)
    for k in extra:
        w = sd[k].float()
        std = 1.0 / math.sqrt(cfg.model_channels)  # minimal_v4_dit_camera_conditioned.py:1117-1119
        assert tuple(w.shape) == (cfg.model_channels, 1536) and w.abs().max() <= 3 * std * 1.01
        assert abs(w.std().item() / std - 1) < 0.05
    # the loader takes the keys (with and without the `net.` prefix) and misses them loudly
    net = MinimalV1LVGDiT(cfg, device="cpu")
    net.load_state_dict({"net." + k: v for k, v in sd.items()})
    assert all(k in net.sd for k in extra)
    with pytest.raises(KeyError, match="cam_encoder"):
        MinimalV1LVGDiT(cfg, device="cpu").load_state_dict({k: v for k, v in sd.items() if "cam_encoder" not in k})


def test_models_entry():
    net, smp = MODELS["2B/camera-cond"]
    assert net == DIT_2B.replace(camera_dim=1536)
    assert (net.rope_h_extrapolation_ratio, net.rope_w_extrapolation_ratio, net.rope_t_extrapolation_ratio) == (3, 3, 1)
    assert net.timestep_scale == 0.001 and net.use_wan_fp32_strategy and net.use_crossattn_projection
    assert net.crossattn_proj_in_channels == 100352
    assert smp.sampler == "unipc" and not smp.use_kerras_sigma_at_inference and smp.shift == 5.0
    assert smp.cfg_mode == "video2world" and smp.state_t == 24 and smp.conditional_frame_timestep == 0.1
    assert SetupArguments(output_dir="out", model="2B/camera-cond").model == "2B/camera-cond"
    assert cam.MODEL_NAME in MODELS and cam.CAMERA_DIM == net.camera_dim == 6 * 16 * 16


@pytest.mark.parametrize("kw,what", [(dict(action_dim=7, action_per_latent_frame=4), "action"),
                                     (dict(n_cameras_emb=7, view_condition_dim=7, state_t=8), "multi-view"),
                                     (dict(n_dense_blocks=0, natten_parameters=dict(window_size=(-1, 4, 4),
                                                                                    stride=(1, 1, 1))), "sparse"),
                                     (dict(camera_dim=1500), "GEMM")])
def test_unsupported_net_combinations_raise(kw, what):
    with pytest.raises(ValueError, match=what):
        MinimalV1LVGDiT(tiny_dit(**dict(dict(camera_dim=1536), **kw)), device="cpu")


# ----------------------------------------------------------------------------- layout
def test_reorder_source_first():
    x = torch.arange(6).view(1, 6, 1).expand(2, 6, 3)  # segments [source 0 1 | target0 2 3 | target1 4 5]
    want = torch.tensor([2, 3, 0, 1, 4, 5])
    for fn in (cam.reorder_source_first, ct.reorder_source_first):
        y = fn(x, dim=1)
        assert torch.equal(y[0, :, 0], want) and torch.equal(y[1, :, 2], want)
    assert torch.equal(cam.reorder_source_first(torch.arange(6), dim=0), want)
    with pytest.raises(ValueError):
        cam.reorder_source_first(torch.arange(7), dim=0)


@pytest.mark.parametrize("n,frames", [(1, [1]), (2, [2, 3])])
def test_mask_on_n_to_2n(n, frames):
    T = 6
    want = torch.zeros(T)
    want[frames] = 1
    assert torch.equal(camera_frame_mask(T, n), want)
    assert torch.equal(ct.camera_mask(1, T, 2, 3, n)[0, 0, :, 0, 0], want)
    assert camera_frame_mask(1, n).sum() == 0  # an image batch conditions nothing


def test_poses_for_latent_frames():
    p = torch.arange(21).float()
    assert cam.poses_for_latent_frames(p).tolist() == [0, 4, 8, 12, 16, 20]
    assert cam.poses_for_latent_frames(p, 3).tolist() == [0, 4, 8]
    assert cam.poses_for_latent_frames(torch.arange(20).float()).tolist() == [0, 4, 8, 12, 16]
    with pytest.raises(ValueError):
        cam.poses_for_latent_frames(p, 7)


# ----------------------------------------------------------------------------- arguments
def test_argument_validation(tmp_path):
    ok = dict(name="a", prompt="p", input_path=tmp_path / "v.mp4", cameras_path=tmp_path / "c.npz")
    a = cam.CameraInferenceArguments(**ok)
    assert (a.guidance, a.num_steps, a.num_conditional_frames, a.seed, a.resolution) == (1.5, 35, 1, 1, "none")
    assert isinstance(a.guidance, float) and a.negative_prompt is None
    (tmp_path / "p.txt").write_text(" from a file \n")
    assert cam.CameraInferenceArguments(**dict(ok, prompt=None, prompt_path=tmp_path / "p.txt")).prompt == "from a file"
    for bad in (dict(prompt=None), dict(input_path=tmp_path / "v.png"), dict(cameras_path=tmp_path / "c.json"),
                dict(guidance=-1.0), dict(num_steps=0), dict(num_conditional_frames=-1), dict(resolution="100,96"),
                dict(resolution="tall"), dict(unknown_field=1)):
        with pytest.raises(pydantic.ValidationError):
            cam.CameraInferenceArguments(**dict(ok, **bad))
    with pytest.raises(pydantic.ValidationError):
        SetupArguments(output_dir=tmp_path, model="2B/camera")


def test_load_cameras(tmp_path):
    w2c = np.tile(np.eye(3, 4, dtype=np.float64), (3, 5, 1, 1))
    k = np.ones((3, 5, 4), dtype=np.float64)
    np.savez(tmp_path / "c.npz", w2c=w2c, intrinsics=k)
    a, b = cam.load_cameras(tmp_path / "c.npz")
    assert a.dtype == b.dtype == torch.float32 and tuple(a.shape) == (3, 5, 3, 4) and tuple(b.shape) == (3, 5, 4)
    np.savez(tmp_path / "bad.npz", w2c=w2c[:2], intrinsics=k[:2])
    with pytest.raises(ValueError):
        cam.load_cameras(tmp_path / "bad.npz")
    np.savez(tmp_path / "missing.npz", w2c=w2c)
    with pytest.raises(ValueError):
        cam.load_cameras(tmp_path / "missing.npz")


# ----------------------------------------------------------------------------- Pluecker truth
CASES = ct.plucker_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_plucker_truth_properties(name):
    """What the reference's own camera_test.py:170-186 asserts of get_plucker_rays, on the float64 truth: |d| = 1,
    m . d = 0, m = o x d."""
    w2c, intr = CASES[name]
    pl = ct.plucker_rays(w2c, ct.intrinsics_matrix(intr.double()), (32, 48), torch.float64)
    m, d = pl[..., :3], pl[..., 3:]
    assert torch.allclose(d.norm(dim=-1), torch.ones(2, 32 * 48, dtype=torch.float64), atol=1e-12)
    assert (m * d).sum(-1).abs().max() < 1e-12
    R, t = w2c[:, :, :3].double(), w2c[:, :, 3:].double()
    o = (-R.transpose(1, 2) @ t).squeeze(-1)[:, None].expand_as(d)
    assert torch.allclose(m, torch.linalg.cross(o, d), atol=1e-12)
    if name == "identity":
        assert (m == 0).all()  # the camera sits at the origin
    rows = ct.pack_tokens(pl, 2, 3)  # packing keeps every value
    assert tuple(rows.shape) == (12, 1536) and torch.equal(rows.flatten().sort().values, pl.flatten().sort().values)


def test_packing_order():
    """Token (f, hp, wp), feature (c, m, n): element [tok, c * 256 + m * 16 + n] is channel c of pixel
    (16 hp + m, 16 wp + n) of frame f."""
    Fr, Hp, Wp = 2, 2, 3
    pl = torch.arange(Fr * 32 * 48 * 6, dtype=torch.float64).view(Fr, 32 * 48, 6)
    rows = ct.pack_tokens(pl, Hp, Wp)
    for f, hp, wp, c, m, n in ((0, 0, 0, 0, 0, 0), (1, 1, 2, 5, 15, 15), (0, 1, 0, 3, 7, 2), (1, 0, 1, 2, 0, 9)):
        pix = (16 * hp + m) * 48 + 16 * wp + n
        assert rows[(f * Hp + hp) * Wp + wp, c * 256 + m * 16 + n] == pl[f, pix, c]


@pytest.mark.parametrize("name", sorted(CASES))
def test_plucker_gate_premise(name):
    """The gate of tests/test_camera_ops_gpu.py is |out - truth64| <= half_ulp_bf16(truth64) + 2 E_ref, E_ref the
    largest absolute error of the reference's fp32 op sequence against the float64 truth on the case. Premise: the
    reference sequence itself, rounded to bf16, meets it with margin 1 (E_ref once), so the factor 2 is room for another
    equally valid fp32 evaluation order and not for the reference's own error.

    The first term is bf16's half-ulp AT the truth's magnitude, 2^(floor(log2 |x|) - 8), which lies between
    2^-9 |x| and 2^-8 |x|. The constant 2^-9 |x| is its lower end: it is asserted here that the float64 truth rounded
    CORRECTLY to bf16 already misses `2^-9 |x| + 2 E_ref` on a tenth or more of the elements of every case, so no bf16
    output at all could meet that form; the half-ulp it names is what is gated."""
    w2c, intr = CASES[name]
    t64 = ct.plucker_token_rows(w2c, intr, 2, 3, torch.float64)
    r32 = ct.plucker_token_rows(w2c, intr, 2, 3, torch.float32)
    assert r32.dtype == torch.float32
    e_ref = (r32.double() - t64).abs().max().item()
    print(f"{name}: E_ref = {e_ref:.3e}")
    assert 1e-8 < e_ref < 2e-6  # a few fp32 ulps of values up to |t| = 4
    half_ulp = ct.bf16_half_ulp(t64)
    assert (half_ulp <= 2.0 ** -8 * t64.abs()).all() and (half_ulp >= 2.0 ** -9 * t64.abs()).all()
    assert ((r32.to(BF16).double() - t64).abs() <= half_ulp + e_ref).all()
    rounded = t64.to(BF16).double()
    assert ((rounded - t64).abs() <= half_ulp).all()
    assert ((rounded - t64).abs() > 2.0 ** -9 * t64.abs() + 2 * e_ref).double().mean() > 0.1
