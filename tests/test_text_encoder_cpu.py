"""CPU tests of the Reason1 text encoder's host side and of its ground truth (tests/reason1_truth.py): the truth against
transformers' Qwen2_5_VLTextModel, the premises of the GPU tests' exact inputs, prompt and checkpoint handling, and the
shape / strategy errors. No GPU."""
import dataclasses
import os

import pytest
import torch

import reason1_truth as T
from cosmos_predict2 import text_encoder as TE

BF16 = torch.bfloat16


def _hf_model(cfg, sd, dtype):
    from transformers.models.qwen2_5_vl.configuration_qwen2_5_vl import Qwen2_5_VLTextConfig
    from transformers.models.qwen2_5_vl.modeling_qwen2_5_vl import Qwen2_5_VLTextModel

    c = Qwen2_5_VLTextConfig(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size,
                             intermediate_size=cfg.intermediate_size, num_hidden_layers=cfg.num_hidden_layers,
                             num_attention_heads=cfg.num_attention_heads, num_key_value_heads=cfg.num_key_value_heads,
                             rope_theta=cfg.rope_theta, rms_norm_eps=cfg.rms_norm_eps, max_position_embeddings=1024,
                             rope_scaling={"type": "mrope", "mrope_section": [16, 24, 24]},
                             attn_implementation="eager", eos_token_id=None, pad_token_id=None, bos_token_id=None)
    m = Qwen2_5_VLTextModel(c).to(dtype).eval()
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return m


def test_truth_matches_transformers_every_hidden_state():
    """The unrounded truth is the architecture transformers runs: per hidden state, the fp32 truth's rel-L2 from the
    float64 transformers model is at most 4 x the fp32 transformers model's own (its rounding noise; the factor covers an
    equally valid summation order, a structural error is of order 1). Measured here: transformers fp32 3.5e-7 / 4.7e-7,
    fp32 truth 3.6e-7 / 4.7e-7, float64 truth 1.3e-7 / 1.6e-7 (the rotary tables stay fp32 inside transformers)."""
    cfg = TE.tiny_reason1()
    sd = TE.init_reason1_state_dict(cfg, seed=0, dtype=torch.float32)  # non-trivial biases and norm weights
    ids = torch.randint(0, cfg.vocab_size, (1, 128), generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        h64 = _hf_model(cfg, sd, torch.float64)(input_ids=ids, output_hidden_states=True).hidden_states[1:]
        h32 = _hf_model(cfg, sd, torch.float32)(input_ids=ids, output_hidden_states=True).hidden_states[1:]
    t32 = T.hidden_states(sd, ids, cfg.num_attention_heads, cfg.num_key_value_heads, rounded=False)
    t64 = T.hidden_states(sd, ids, cfg.num_attention_heads, cfg.num_key_value_heads, rounded=False,
                          dtype=torch.float64)
    assert len(h64) == len(t32) == cfg.num_hidden_layers
    for i in range(cfg.num_hidden_layers):
        noise = T.rel_l2(h32[i], h64[i])
        d32, d64 = T.rel_l2(t32[i], h64[i]), T.rel_l2(t64[i], h64[i])
        print(f"hidden_states[{i + 1}]: transformers fp32 {noise:.2e}, truth fp32 {d32:.2e}, truth float64 {d64:.2e}")
        assert 0 < noise < 1e-5
        assert d32 <= 4 * noise and d64 <= 4 * noise


def test_rounded_truth_is_close_to_unrounded():
    """The bf16 truth is the same network: a few 1e-3 from the unrounded one, not of order 1."""
    cfg = TE.tiny_reason1()
    sd = TE.init_reason1_state_dict(cfg, seed=0)
    ids = torch.randint(0, cfg.vocab_size, (1, 64), generator=torch.Generator().manual_seed(2))
    a = T.encode(sd, ids, 4, 2, rounded=True)
    b = T.encode(sd, ids, 4, 2, rounded=False)
    assert a.shape == (1, 64, cfg.out_dim)
    assert torch.equal(a, T.rb(a))
    assert 1e-4 < T.rel_l2(a, b) < 3e-2


@pytest.mark.parametrize("D", [512, 3584])
def test_exact_input_premises(D):
    """The exact inputs of the GPU row-kernel tests: fp32 sums in any order equal the float64 sums, and the row means
    are the bf16 values they are meant to be."""
    x = T.integer_rows(5, D, seed=D)
    assert torch.equal(x.float(), x.float().round()) and T.sums_exact(x)
    z = T.integer_rows(5, D, seed=D + 1, zero_mean=True)
    assert T.sums_exact(z, centered=True) and torch.equal(z.double().mean(-1), torch.zeros(5, dtype=torch.float64))
    m = T.integer_mean_rows(5, D, seed=D + 2, mean=3)
    assert T.sums_exact(m, centered=True) and torch.equal(m.double().mean(-1), torch.full((5,), 3.0, dtype=torch.float64))
    # with exact sums the statistics are single IEEE operations: fp32 and float64 agree after the fp32 rounding
    for t in (z, m):
        d = t.double() - t.double().mean(-1, keepdim=True)
        var64 = (d * d).sum(-1) / (D - 1)
        var32 = ((t.float() - t.float().mean(-1, keepdim=True)) ** 2).sum(-1) / (D - 1)
        assert torch.equal(var32, var64.float())


def test_pad_or_truncate():
    assert TE.pad_or_truncate([5, 6, 7], 9, 6) == [5, 6, 7, 9, 9, 9]
    assert TE.pad_or_truncate(list(range(10)), 9, 6) == [0, 1, 2, 3, 4, 5]
    assert TE.pad_or_truncate([1, 2], 0, 2) == [1, 2]


def test_prompt_template_and_padding_with_a_stub_tokenizer():
    seen = []

    def stub(text):
        seen.append(text)
        return [3 + (ord(c) % 50) for c in text]

    tok = TE.PromptTokenizer(stub, pad_id=2)
    ids = tok("a red car", 512)
    want = ("<|im_start|>system\nYou are a helpful assistant who will provide prompts to an image generator.<|im_end|>\n"
            "<|im_start|>user\na red car<|im_end|>\n")
    assert seen == [want]
    assert len(ids) == 512 and ids[:len(want)] == stub(want) and set(ids[len(want):]) == {2}
    long = tok("x" * 2000, 512)
    assert len(long) == 512 and 2 not in long
    with pytest.raises(ValueError):
        TE.PromptTokenizer(stub)  # no pad id
    with pytest.raises(ValueError):
        TE.PromptTokenizer()  # neither
    with pytest.raises(ValueError):
        TE.PromptTokenizer(tokenizer_path="/nonexistent/tokenizer/dir")


def _prefixed(sd, prefix):
    return {prefix + k: v for k, v in sd.items()}


def test_checkpoint_key_layouts():
    cfg = TE.tiny_reason1(num_hidden_layers=1)
    sd = TE.init_reason1_state_dict(cfg, seed=3)
    extra = {"visual.blocks.0.attn.qkv.weight": torch.zeros(2), "lm_head.weight": torch.zeros(2)}
    for prefix in ("model.", "model.language_model.", ""):
        got = TE.normalize_reason1_keys({**_prefixed(sd, prefix), **extra, "model.visual.merger.weight": torch.zeros(1)})
        assert sorted(got) == sorted(sd)
        assert all(got[k] is sd[k] for k in sd)
        TE._check_state_dict(cfg, got)
    with pytest.raises(ValueError):
        TE.normalize_reason1_keys({"model.rotary.weird": torch.zeros(1)})
    assert TE.config_from_state_dict(sd) == cfg


def test_checkpoint_files_and_missing_keys(tmp_path):
    from safetensors.torch import save_file

    cfg = TE.tiny_reason1(num_hidden_layers=1)
    sd = TE.init_reason1_state_dict(cfg, seed=4)
    torch.save(_prefixed(sd, "model."), tmp_path / "enc.pt")
    save_file(_prefixed(sd, "model.language_model."), str(tmp_path / "enc.safetensors"))
    shards = tmp_path / "shards"
    shards.mkdir()
    keys = sorted(sd)
    save_file({"model." + k: sd[k] for k in keys[:5]}, str(shards / "model-00001-of-00002.safetensors"))
    save_file({"model." + k: sd[k] for k in keys[5:]}, str(shards / "model-00002-of-00002.safetensors"))
    for path in (tmp_path / "enc.pt", tmp_path / "enc.safetensors", shards):
        got = TE.load_reason1_checkpoint(str(path))
        assert sorted(got) == keys and all(torch.equal(got[k], sd[k]) for k in keys)
    short = dict(sd)
    del short["layers.0.self_attn.k_proj.bias"]
    with pytest.raises(KeyError, match="k_proj.bias"):
        TE._check_state_dict(cfg, short)
    with pytest.raises(KeyError):
        TE.Reason1TextEncoder(cfg, state_dict=short, device="cpu", offload=True)
    bad = dict(sd)
    bad["norm.weight"] = torch.zeros(7, dtype=BF16)
    with pytest.raises(ValueError, match="norm.weight"):
        TE._check_state_dict(cfg, bad)
    empty = tmp_path / "empty"
    empty.mkdir()
    with pytest.raises(ValueError):
        TE.load_reason1_checkpoint(str(empty))


def test_config_values_and_shapes():
    c = TE.REASON1_7B
    assert (c.hidden_size, c.intermediate_size, c.num_hidden_layers, c.num_attention_heads, c.num_key_value_heads,
            c.vocab_size, c.num_tokens) == (3584, 18944, 28, 28, 4, 152064, 512)
    assert c.out_dim == 100352 and c.qkv_dim == 4608 and c.embedding_concat_strategy == "full_concat"
    shapes = TE.reason1_state_dict_shapes(c)
    assert len(shapes) == 2 + 28 * 12
    assert shapes["layers.27.self_attn.k_proj.weight"] == (512, 3584)
    assert shapes["layers.0.mlp.down_proj.weight"] == (3584, 18944)
    sd = TE.init_reason1_state_dict(TE.tiny_reason1(), seed=0)
    assert {k: tuple(v.shape) for k, v in sd.items()} == TE.reason1_state_dict_shapes(TE.tiny_reason1())
    assert sd["layers.0.self_attn.q_proj.bias"].float().abs().max() > 0.1


def test_fused_weights_layout():
    """q | k | v rows fused with the bias as column D of a [*, D + 64] weight, gate | up fused (host side only)."""
    cfg = TE.tiny_reason1(num_hidden_layers=1)
    sd = TE.init_reason1_state_dict(cfg, seed=5)
    enc = TE.Reason1TextEncoder(cfg, state_dict=sd, device="cpu", offload=True)
    w = enc._host["0.qkv"]
    D = cfg.hidden_size
    assert w.shape == (cfg.qkv_dim, D + 64) and w.dtype == BF16
    assert torch.equal(w[:512, :D], sd["layers.0.self_attn.q_proj.weight"])
    assert torch.equal(w[512:768, D], sd["layers.0.self_attn.k_proj.bias"])
    assert torch.equal(w[768:, :D], sd["layers.0.self_attn.v_proj.weight"])
    assert not w[:, D + 1:].any()
    gu = enc._host["0.gu"]
    assert torch.equal(gu[:1024], sd["layers.0.mlp.gate_proj.weight"]) and torch.equal(gu[1024:], sd["layers.0.mlp.up_proj.weight"])
    assert enc.out_dim == 512
    with pytest.raises(ValueError):
        enc("no tokenizer was given")


def test_strategy_and_shape_errors():
    cfg = TE.tiny_reason1(num_hidden_layers=1)
    sd = TE.init_reason1_state_dict(cfg, seed=6)
    for s in ("mean_pooling", "pool_every_n_layers_and_concat"):
        with pytest.raises(NotImplementedError):
            TE.Reason1TextEncoder(dataclasses.replace(cfg, embedding_concat_strategy=s), state_dict=sd, device="cpu")
    with pytest.raises(ValueError, match="Invalid embedding_concat_strategy"):
        TE.Reason1TextEncoder(dataclasses.replace(cfg, embedding_concat_strategy="sum"), state_dict=sd, device="cpu")
    with pytest.raises(ValueError, match="multiple of 64"):
        TE.Reason1TextEncoder(dataclasses.replace(cfg, num_tokens=96), state_dict=sd, device="cpu")
    # widths the GEMMs are not built for
    odd = TE.tiny_reason1(num_hidden_layers=1, intermediate_size=1000)
    with pytest.raises(ValueError, match="own GEMM"):
        TE.Reason1TextEncoder(odd, state_dict=TE.init_reason1_state_dict(odd, seed=0), device="cpu", offload=True)
    with pytest.raises(ValueError):
        TE.Reason1TextEncoder(cfg, device="cpu")  # neither state_dict nor ckpt_path


def test_out_dim_mismatch_raises_before_any_upload(tmp_path):
    """build_text_encoder (what Video2WorldInference calls for text_encoder_path) refuses an encoder whose out_dim is not
    the net's crossattn_proj_in_channels."""
    cfg = TE.tiny_reason1()
    torch.save(TE.init_reason1_state_dict(cfg, seed=7), tmp_path / "enc.pt")
    with pytest.raises(ValueError, match="crossattn_proj_in_channels"):
        TE.build_text_encoder(str(tmp_path / "enc.pt"), None, expect_dim=100352, device="cpu")


def test_setup_arguments_carry_the_encoder_paths(tmp_path):
    from cosmos_predict2.config import SetupArguments

    p = tmp_path / "enc.pt"
    p.write_bytes(b"x")
    a = SetupArguments(output_dir=tmp_path, text_encoder_path=str(p), offload_text_encoder=True)
    assert a.text_encoder_path == str(p) and a.text_tokenizer_path is None and a.offload_text_encoder
    assert SetupArguments(output_dir=tmp_path).text_encoder_path is None
    with pytest.raises(ValueError):
        SetupArguments(output_dir=tmp_path, text_encoder_path=os.path.join(str(tmp_path), "missing.pt"))


def test_rope_tables_match_the_truth():
    c, s = TE.rope_tables(128, 1e6)
    tc, ts = T.rope_tables(128)
    assert c.dtype == BF16 and torch.equal(c, tc.to(BF16)) and torch.equal(s, ts.to(BF16))
    assert torch.equal(c[0].float(), torch.ones(128)) and not s[0].any()
