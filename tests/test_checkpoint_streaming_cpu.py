"""CPU: the streaming action student's net / sampler configuration and its state-dict layout
(interactive/configs/net.py:30-130, interactive/configs/experiment/exp_action_self_forcing.py:92-105, 147-163)."""
import math

import pydantic
import pytest
import torch

from cosmos_predict2.config import SetupArguments
from cosmos_predict2.dit import init_state_dict, state_dict_shapes
from cosmos_predict2.net_config import (DIT_2B, DIT_2B_ACTION_STREAMING, MODELS, SAMPLER_ACTION_STREAMING, tiny_dit)

NAME = "2B/robot/action-cond/streaming"


def test_model_entry():
    net, smp = MODELS[NAME]
    assert net is DIT_2B_ACTION_STREAMING and smp is SAMPLER_ACTION_STREAMING
    # the causal net: the 2B layout, bf16 conditioning, unscaled timesteps, per-latent-frame actions
    assert (net.model_channels, net.num_blocks, net.num_heads) == (2048, 28, 16)
    assert (net.action_dim, net.action_per_latent_frame) == (29, 4)
    assert net.timestep_scale == 1.0 and net.use_wan_fp32_strategy is False
    assert (net.rope_h_extrapolation_ratio, net.rope_w_extrapolation_ratio, net.rope_t_extrapolation_ratio) == (3, 3, 1)
    assert net.use_crossattn_projection and net.crossattn_proj_in_channels == 100352
    assert net.concat_padding_mask and net.patch_features == 72
    assert smp.sampler == "dmd2_stream" and smp.cache_frame_size == -1
    assert smp.selected_sampling_time == (math.pi / 2, math.atan(15), math.atan(5), math.atan(5 / 3))
    assert (smp.trig_scaling, smp.sigma_data, smp.sigma_conditional, smp.state_t) == ("rectified_flow", 1.0, 1e-4, 4)
    # no other entry takes the streaming sampler
    assert [n for n, (_, s) in MODELS.items() if s.sampler == "dmd2_stream"] == [NAME]


def test_model_name_validation(tmp_path):
    assert SetupArguments(output_dir=tmp_path, model=NAME).model == NAME
    with pytest.raises((pydantic.ValidationError, ValueError)):
        SetupArguments(output_dir=tmp_path, model="2B/robot/action-cond/stream")


def test_state_dict_shapes():
    """The causal net's parameters carry MiniTrainDIT's names (CausalAttention q/k/v/output_proj + q/k_norm,
    CausalBlock's adaln_modulation_*, dit_causal.py:204-213, 431-447) plus the two action embedders
    (dit_action_causal.py:89-102); no extra_pos_embedder and no image-context keys."""
    cfg = DIT_2B_ACTION_STREAMING
    shapes = state_dict_shapes(cfg)
    base = state_dict_shapes(DIT_2B)
    extra = set(shapes) - set(base)
    assert extra == {f"action_embedder_B_{o}.fc{i}.{p}" for o in ("D", "3D") for i in (1, 2) for p in ("weight", "bias")}
    assert set(base) <= set(shapes) and all(shapes[k] == base[k] for k in base)
    D = cfg.model_channels
    assert shapes["action_embedder_B_D.fc1.weight"][0] == (4 * D, 29 * 4)
    assert shapes["action_embedder_B_D.fc2.weight"][0] == (D, 4 * D)
    assert shapes["action_embedder_B_3D.fc2.weight"][0] == (3 * D, 4 * D)
    assert shapes["x_embedder.proj.1.weight"][0] == (D, 72)  # 16 latent + condition mask + padding mask, 2 x 2 patch
    assert not any("extra_pos" in k or "img" in k for k in shapes)
    # a tiny net of the same layout initialises with exactly these keys
    tiny = tiny_dit(num_blocks=1, action_dim=7, action_per_latent_frame=4, timestep_scale=1.0,
                    use_wan_fp32_strategy=False)
    sd = init_state_dict(tiny, seed=0)
    want = state_dict_shapes(tiny)
    assert set(sd) == set(want)
    assert all(tuple(sd[k].shape) == tuple(want[k][0]) and sd[k].dtype == torch.bfloat16 for k in want)
