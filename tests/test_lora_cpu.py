"""LoRA merge, CPU side: the premise of the exact kernel test and checkpoint.split_lora_state_dict.

Premise. tests/test_lora_merge_gpu.py asks torch.equal(cp25_lora_merge, lora_truth.merge_restated). That only means
something if the restatement is the right arithmetic, so here it is held to an independent float64 formula
(lora_truth.merge_truth64): |restated - truth64| <= half_ulp_bf16(truth64) + E on every element of every case, E the
largest error of the restatement's fp32 value ahead of its bf16 rounding against the truth on that case (computed
here, as tests/test_camera_cpu.py::test_plucker_gate_premise does for its gate). A transposed A or B cannot even be
multiplied at these shapes, and a swapped alpha / r misses the bound, which is asserted too."""
import pytest
import torch

import lora_truth as lt
from cosmos_predict2.checkpoint import split_lora_state_dict

BF16 = torch.bfloat16
CASES = lt.cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_restated_merge_premise(name):
    w, a, b, scale = CASES[name]
    r = a.shape[0]
    alpha = scale * r  # lora_scale 1: scale = alpha / r
    truth = lt.merge_truth64(w, a, b, alpha, r)
    s32 = lt.fp32_scale(1.0, alpha, r)
    pre = lt.merge_restated(w, a, b, s32, pre_rounding=True)
    assert pre.dtype == torch.float32
    e = (pre.double() - truth).abs().max().item()
    got = lt.merge_restated(w, a, b, s32)
    assert got.dtype == BF16 and got.shape == w.shape
    err = (got.double() - truth).abs()
    bound = lt.bf16_half_ulp(truth) + e
    print(f"{name}: E = {e:.3e}, max |restated - truth| = {err.max().item():.3e}, "
          f"max |delta| = {(truth - w.double()).abs().max().item():.3e}")
    # E is fp32 rounding noise: r products and sums of values below 1, far under a bf16 half-ulp of the weights
    assert e < 2.0 ** -18
    assert (err <= bound).all()
    assert not torch.equal(got, w)  # B is non-zero: the merge moves the weights


def test_swapped_alpha_and_rank_fails_the_premise():
    """alpha = 16 at r = 8 is a scale of 2; alpha and r swapped give 0.5, and that restatement misses the bound."""
    w, a, b = lt.make_case(64, 128, 8, seed=7)
    alpha, r = 16.0, 8
    truth = lt.merge_truth64(w, a, b, alpha, r)
    good = lt.merge_restated(w, a, b, lt.fp32_scale(1.0, alpha, r))
    e = (lt.merge_restated(w, a, b, lt.fp32_scale(1.0, alpha, r), pre_rounding=True).double() - truth).abs().max().item()
    bound = lt.bf16_half_ulp(truth) + e
    assert ((good.double() - truth).abs() <= bound).all()
    wrong = lt.merge_restated(w, a, b, float(r) / alpha)
    assert ((wrong.double() - truth).abs() > bound).any()


def test_fp32_scale_is_rounded_once_from_double():
    assert lt.fp32_scale(1.0, 32, 32) == 1.0
    assert lt.fp32_scale(1.0, 8, 12) == torch.tensor(8.0 / 12.0, dtype=torch.float64).float().item()
    assert lt.fp32_scale(0.3, 16, 5) == torch.tensor(0.3 * 16 / 5, dtype=torch.float64).float().item()


# ----------------------------------------------------------------------------- split_lora_state_dict
def _t(*shape):
    return torch.zeros(*shape)


def _peft_dict(prefix="net.", name=".default"):
    m = "blocks.0.self_attn.q_proj"
    return {
        f"{prefix}{m}.base_layer.weight": _t(8, 16),
        f"{prefix}{m}.lora_A{name}.weight": _t(4, 16),
        f"{prefix}{m}.lora_B{name}.weight": _t(8, 4),
        f"{prefix}blocks.0.self_attn.q_norm.weight": _t(8),
        f"{prefix}pos_embedder.seq": _t(3),
    }


@pytest.mark.parametrize("prefix", ["net.", "", "base_model.model.", "base_model.model.net."])
@pytest.mark.parametrize("name", [".default", ""])
def test_split_key_forms(prefix, name):
    sd = _peft_dict(prefix, name)
    base, ad = split_lora_state_dict(sd)
    assert sorted(base) == ["blocks.0.self_attn.q_norm.weight", "blocks.0.self_attn.q_proj.weight", "pos_embedder.seq"]
    assert list(ad) == ["blocks.0.self_attn.q_proj"]
    a, b = ad["blocks.0.self_attn.q_proj"]
    assert a is sd[f"{prefix}blocks.0.self_attn.q_proj.lora_A{name}.weight"] and tuple(a.shape) == (4, 16)
    assert b is sd[f"{prefix}blocks.0.self_attn.q_proj.lora_B{name}.weight"] and tuple(b.shape) == (8, 4)
    assert base["blocks.0.self_attn.q_proj.weight"] is sd[f"{prefix}blocks.0.self_attn.q_proj.base_layer.weight"]


def test_split_plain_dict_and_ema():
    sd = {"net.blocks.0.mlp.layer1.weight": _t(4, 4), "net_ema.blocks.0.mlp.layer1.weight": _t(4, 4),
          "net_ema.blocks.0.mlp.layer1.lora_A.default.weight": _t(2, 4), "net.blocks.0._extra_state": _t(1)}
    base, ad = split_lora_state_dict(sd)
    assert ad == {}
    assert sorted(base) == ["blocks.0._extra_state", "blocks.0.mlp.layer1.weight"]
    assert base["blocks.0.mlp.layer1.weight"] is sd["net.blocks.0.mlp.layer1.weight"]


def test_split_adapter_only_file():
    sd = {"blocks.1.mlp.layer2.lora_A.weight": _t(2, 8), "blocks.1.mlp.layer2.lora_B.weight": _t(4, 2)}
    base, ad = split_lora_state_dict(sd)
    assert base == {} and list(ad) == ["blocks.1.mlp.layer2"]


def test_split_errors():
    m = "net.blocks.0.cross_attn.k_proj"
    with pytest.raises(ValueError, match="lora_A without its lora_B"):
        split_lora_state_dict({m + ".lora_A.default.weight": _t(2, 4)})
    with pytest.raises(ValueError, match="lora_B without its lora_A"):
        split_lora_state_dict({m + ".lora_B.default.weight": _t(4, 2)})
    with pytest.raises(ValueError, match="more than one adapter name"):
        split_lora_state_dict({m + ".lora_A.default.weight": _t(2, 4), m + ".lora_B.default.weight": _t(4, 2),
                               "net.blocks.1.cross_attn.k_proj.lora_A.other.weight": _t(2, 4),
                               "net.blocks.1.cross_attn.k_proj.lora_B.other.weight": _t(4, 2)})
    with pytest.raises(ValueError, match="rank"):
        split_lora_state_dict({m + ".lora_A.weight": _t(2, 4), m + ".lora_B.weight": _t(4, 3)})
    with pytest.raises(ValueError, match="not matrices"):
        split_lora_state_dict({m + ".lora_A.weight": _t(4), m + ".lora_B.weight": _t(4, 1)})
    with pytest.raises(ValueError, match="unsupported LoRA key"):
        split_lora_state_dict({m + ".lora_magnitude_vector.default.weight": _t(4)})
    with pytest.raises(ValueError, match="unrecognised LoRA key"):
        split_lora_state_dict({m + ".lora_A.default.bias": _t(4)})


def test_setup_arguments_lora_fields(tmp_path):
    from cosmos_predict2.config import SetupArguments

    s = SetupArguments(output_dir=tmp_path)
    assert s.lora_path is None and s.lora_alpha is None and s.lora_scale == 1.0
    f = tmp_path / "adapter.pt"
    f.write_bytes(b"")
    s = SetupArguments(output_dir=tmp_path, lora_path=str(f), lora_alpha=16, lora_scale=0.5)
    assert s.lora_path == str(f) and s.lora_alpha == 16.0 and s.lora_scale == 0.5
    with pytest.raises(ValueError, match="does not exist"):
        SetupArguments(output_dir=tmp_path, lora_path=str(tmp_path / "nope.safetensors"))


def test_loader_keywords_default_to_no_adapter():
    import inspect

    from cosmos_predict2.dit import MinimalV1LVGDiT
    from cosmos_predict2.model import Video2WorldModelRectifiedFlow
    from cosmos_predict2.pipeline import Video2WorldInference

    for fn in (MinimalV1LVGDiT.load_state_dict, Video2WorldModelRectifiedFlow.load_state_dict):
        p = inspect.signature(fn).parameters
        assert p["strict"].default is True and p["lora_alpha"].default is None and p["lora_scale"].default == 1.0
    p = inspect.signature(Video2WorldInference.__init__).parameters
    assert p["lora_path"].default is None and p["lora_alpha"].default is None and p["lora_scale"].default == 1.0
    p = inspect.signature(MinimalV1LVGDiT.merge_lora).parameters
    assert p["alpha"].default is None and p["scale"].default == 1.0
