"""The Reason1 text encoder on the device (cosmos_predict2/text_encoder.py) against tests/reason1_truth.py, and through
the pipeline.

Gate (the project's, test_parity_depth_gpu.py): the HIP encoder's rel-L2 distance from the unrounded fp32 truth is at
most 1.1 x the bf16 truth's own distance from it (the bf16 truth = the same ops with every bf16 rounding, float64 GEMM
sums). No trained weights and no real tokenizer exist offline: parity with them is unpinned, as for every other net."""
import pytest
import torch

import reason1_truth as T
from cosmos_predict2 import text_encoder as TE

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def tiny(device):
    cfg = TE.tiny_reason1()
    sd = TE.init_reason1_state_dict(cfg, seed=11)
    enc = TE.Reason1TextEncoder(cfg, state_dict=sd, tokenizer=TE.byte_tokenizer(cfg.vocab_size), pad_id=0, device=device)
    return cfg, sd, enc


def _ids(cfg, B, L, seed, pad_from=None):
    ids = torch.randint(1, cfg.vocab_size, (B, L), generator=torch.Generator().manual_seed(seed))
    if pad_from is not None:
        ids[:, pad_from:] = 0  # a padded prompt: the tail repeats pad_id, unmasked as in the reference
    return ids


def _gate(name, hip, sd, ids, cfg):
    truth = T.encode(sd, ids, cfg.num_attention_heads, cfg.num_key_value_heads, rounded=False)
    ref = T.encode(sd, ids, cfg.num_attention_heads, cfg.num_key_value_heads, rounded=True)
    d_hip, d_ref, d_hr = T.rel_l2(hip, truth), T.rel_l2(ref, truth), T.rel_l2(hip, ref)
    print(f"{name}: hip-truth {d_hip:.3e}, bf16 truth-truth {d_ref:.3e}, hip-bf16 truth {d_hr:.3e}")
    assert d_hip <= 1.1 * d_ref, (d_hip, d_ref)
    return d_hip, d_ref


@pytest.mark.parametrize("L", [128, 512])
def test_tiny_encoder_against_truth(device, tiny, L):
    cfg, sd, enc = tiny
    ids = _ids(cfg, 1, L, seed=L, pad_from=L - L // 4)
    out = enc.encode_ids(ids)
    assert out.shape == (1, L, cfg.out_dim) and out.dtype == BF16 and out.is_cuda
    _gate(f"tiny L={L}", out.cpu(), sd, ids, cfg)
    # two runs are bit-identical
    assert torch.equal(enc.encode_ids(ids), out)
    # every column block is mean-normalised: mean ~ 0, std ~ 1 per token and layer
    blocks = out.float().view(L, cfg.num_hidden_layers, cfg.hidden_size)
    assert blocks.mean(-1).abs().max().item() < 2e-2 and (blocks.std(-1) - 1).abs().max().item() < 2e-2


def test_batch_entries_equal_single_calls(device, tiny):
    cfg, sd, enc = tiny
    ids = _ids(cfg, 2, 128, seed=5)
    both = enc.encode_ids(ids)
    for b in range(2):
        assert torch.equal(both[b], enc.encode_ids(ids[b:b + 1])[0]), b
    assert not torch.equal(both[0], both[1])


def test_offload_gives_the_same_bits(device, tiny):
    cfg, sd, enc = tiny
    ids = _ids(cfg, 1, 128, seed=6)
    off = TE.Reason1TextEncoder(cfg, state_dict=sd, device=device, offload=True)
    assert off._dev is None
    a = off.encode_ids(ids)
    assert off._dev is None  # parked again
    assert torch.equal(a, enc.encode_ids(ids)) and torch.equal(off.encode_ids(ids), a)


def test_prompt_call_and_cache(device, tiny):
    cfg, sd, enc = tiny
    a = enc("a red car drives through the rain")
    assert a.shape == (1, cfg.num_tokens, cfg.out_dim) and a.dtype == BF16
    assert enc("a red car drives through the rain") is a  # cached per prompt string
    b = enc("a blue boat")
    assert b is not a and not torch.equal(a, b)
    assert torch.equal(a, enc.encode_ids(enc.token_ids("a red car drives through the rain")))
    with pytest.raises(ValueError):
        enc.encode_ids(torch.full((1, 128), cfg.vocab_size))  # id outside the table: refused on the host
    with pytest.raises(ValueError):
        enc.encode_ids(torch.zeros(1, 96, dtype=torch.int64))


def test_one_layer_at_the_7b_widths(device):
    """hidden 3584, 28 / 4 heads, I 18944: the real GEMM shapes (N 4608 / 3584 / 37888, K 3648 / 3584 / 18944) and
    the 7 : 1 head grouping."""
    cfg = TE.Reason1Config(vocab_size=1000, num_hidden_layers=1)
    assert (cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_key_value_heads) == (3584, 18944, 28, 4)
    sd = TE.init_reason1_state_dict(cfg, seed=12)
    enc = TE.Reason1TextEncoder(cfg, state_dict=sd, device=device)
    ids = _ids(cfg, 1, 128, seed=7)
    out = enc.encode_ids(ids)
    _gate("one 7B-width layer L=128", out.cpu(), sd, ids, cfg)


def test_pipeline_takes_prompts(device, tiny, tmp_path):
    """Video2WorldInference with the tiny encoder given as text_encoder=, and again through text_encoder_path (a saved
    state dict; the byte stand-in tokenizer): it generates, the two ways agree, two prompts give different videos, and
    an encoder of the wrong width is refused at construction."""
    from cosmos_predict2.net_config import tiny_dit
    from cosmos_predict2.pipeline import Video2WorldInference

    cfg, sd, enc = tiny
    ncfg = tiny_dit(num_blocks=1, crossattn_proj_in_channels=cfg.out_dim)
    kw = dict(resolution="64,96", seed=1, num_steps=2, guidance=3)
    pipe = Video2WorldInference("2B/post-trained", device=device, net_cfg=ncfg, state_t=2, text_encoder=enc)
    assert pipe.text_encoder is enc
    a = pipe.generate_vid2world("a red car", None, **kw)
    b = pipe.generate_vid2world("a blue boat", None, **kw)
    assert a.shape == (1, 3, 5, 64, 96) and torch.isfinite(a).all()
    assert not torch.equal(a, b)
    del pipe
    path = tmp_path / "reason1_tiny.pt"
    torch.save({"model." + k: v for k, v in sd.items()}, path)
    pipe = Video2WorldInference("2B/post-trained", device=device, net_cfg=ncfg, state_t=2, text_encoder_path=str(path),
                                offload_text_encoder=True)
    assert isinstance(pipe.text_encoder, TE.Reason1TextEncoder) and pipe.text_encoder.offload
    assert torch.equal(pipe.text_encoder("a red car"), enc("a red car"))
    assert torch.equal(pipe.generate_vid2world("a red car", None, **kw), a)
    del pipe
    with pytest.raises(ValueError, match="crossattn_proj_in_channels"):
        Video2WorldInference("2B/post-trained", device=device, net_cfg=tiny_dit(num_blocks=1), state_t=2,
                             text_encoder_path=str(path))
    with pytest.raises(ValueError, match="crossattn_proj_in_channels"):
        Video2WorldInference("2B/post-trained", device=device, net_cfg=tiny_dit(num_blocks=1), state_t=2,
                             text_encoder=enc)
