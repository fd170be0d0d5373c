"""Reason1 text encoder on the device: prompt -> the [1, 512, 100352] embeddings `crossattn_proj` reads.

The reference computes its text embeddings online with Cosmos-Reason1-7B, the language half of Qwen2.5-VL-7B
(text_encoders/text_encoder.py:131-220, `compute_text_embeddings_online`): the prompt goes into a two-turn chat
(system line of :149, then the user text), through the tokenizer's chat template, is padded with pad_id or truncated
to 512 ids (:173-179), runs through the 28 decoder layers with `output_hidden_states=True` and no padding mask (so the
mask is causal only), and every hidden state after the embeddings is mean-normalised over its last dimension
(:119-129, :196-198) and concatenated (`full_concat`, :201-202): 28 x 3584 = 100352.

Here the projections run on the hand-written GEMMs (cp25_gemm_sm_epi where cp25_gemm_sm_plan takes the shape,
cp25_gemm_epi otherwise; always split 1, so the bits do not depend on the CU count) and everything between them on
csrc/text_ops.hip and csrc/attn_causal.hip:

    x  = embed_gather(ids)                                                   [n, D], n = B * L
    per layer:  h   = add_rmsnorm(x += mlp of the layer before, ln1)          [n, D + 64]: column D is 1.0
                qkv = h Wqkv^T                                               q | k | v fused, the bias as K column D
                rope_qk(qkv);  a = attn_causal(q, k, v)                      28 query heads on 4 key/value heads
                o   = a Wo^T
                h   = add_rmsnorm(x += o, ln2)
                m   = swiglu(h Wgu^T) Wdown^T                                gate | up fused
    hidden_states[i] (i < 28) is x after layer i's MLP has been added (the next layer's add_rmsnorm writes it);
    hidden_states[28] is the final norm of the last stream. mean_normalize writes each into its column block.

DESIGN.md section 6i has the arithmetic op by op and the deviations. Out of scope: the vision tower, lm_head,
generation, a K/V cache, parallel encoders, DCP checkpoints.
"""
from __future__ import annotations

import dataclasses
import os
import re
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from . import _native as N

SYSTEM_PROMPT = "You are a helpful assistant who will provide prompts to an image generator."  # text_encoder.py:149
# Qwen2.5-VL's chat template for text-only messages with add_generation_prompt=False, restated: what a plain
# `str -> ids` tokenizer is given. A tokenizer directory's own template is used instead.
CHAT_TEMPLATE = "<|im_start|>system\n{system}<|im_end|>\n<|im_start|>user\n{user}<|im_end|>\n"
HEAD_DIM = 128
_BIAS_PAD = 64  # K columns the QKV bias adds to the fused weight: column D holds the bias, the rest zeros
STRATEGIES = ("full_concat", "mean_pooling", "pool_every_n_layers_and_concat")


@dataclasses.dataclass(frozen=True)
class Reason1Config:
    """The text model's shape (text_encoder.py:48-62; Qwen2.5-VL-7B's rope_theta and rms_norm_eps)."""
    vocab_size: int = 152064
    hidden_size: int = 3584
    intermediate_size: int = 18944
    num_hidden_layers: int = 28
    num_attention_heads: int = 28
    num_key_value_heads: int = 4
    rms_norm_eps: float = 1e-6
    rope_theta: float = 1e6
    num_tokens: int = 512                      # NUM_EMBEDDING_PADDING_TOKENS
    embedding_concat_strategy: str = "full_concat"

    @property
    def out_dim(self) -> int:
        return self.num_hidden_layers * self.hidden_size

    @property
    def qkv_dim(self) -> int:
        return (self.num_attention_heads + 2 * self.num_key_value_heads) * HEAD_DIM


REASON1_7B = Reason1Config()


def tiny_reason1(**kw) -> Reason1Config:
    """A test-sized config (hidden 512, 4 / 2 heads, I 1024, 2 layers, vocab 1000): out_dim 1024."""
    base = dict(vocab_size=1000, hidden_size=512, intermediate_size=1024, num_hidden_layers=2, num_attention_heads=4,
                num_key_value_heads=2)
    base.update(kw)
    return Reason1Config(**base)


def reason1_state_dict_shapes(cfg: Reason1Config) -> Dict[str, Tuple[int, ...]]:
    """Key -> shape of the text model's state dict (transformers' bare layout)."""
    D, I = cfg.hidden_size, cfg.intermediate_size
    q, kv = cfg.num_attention_heads * HEAD_DIM, cfg.num_key_value_heads * HEAD_DIM
    shapes: Dict[str, Tuple[int, ...]] = {"embed_tokens.weight": (cfg.vocab_size, D), "norm.weight": (D,)}
    for i in range(cfg.num_hidden_layers):
        p = f"layers.{i}."
        shapes.update({
            p + "input_layernorm.weight": (D,), p + "post_attention_layernorm.weight": (D,),
            p + "self_attn.q_proj.weight": (q, D), p + "self_attn.q_proj.bias": (q,),
            p + "self_attn.k_proj.weight": (kv, D), p + "self_attn.k_proj.bias": (kv,),
            p + "self_attn.v_proj.weight": (kv, D), p + "self_attn.v_proj.bias": (kv,),
            p + "self_attn.o_proj.weight": (D, q),
            p + "mlp.gate_proj.weight": (I, D), p + "mlp.up_proj.weight": (I, D), p + "mlp.down_proj.weight": (D, I),
        })
    return shapes


def init_reason1_state_dict(cfg: Reason1Config, seed: int = 0, dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """Random weights at a trained net's scale: matrices N(0, 1 / fan_in), embeddings N(0, 1), non-trivial biases and
    norm weights (so that a test sees every one of them)."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in reason1_state_dict_shapes(cfg).items():
        if k.endswith("norm.weight") or k.endswith("layernorm.weight"):
            t = 0.75 + 0.5 * torch.rand(shape, generator=g)
        elif k.endswith(".bias"):
            t = 0.5 * torch.randn(shape, generator=g)
        elif k == "embed_tokens.weight":
            t = torch.randn(shape, generator=g)
        else:
            t = torch.randn(shape, generator=g) * shape[1] ** -0.5
        sd[k] = t.to(dtype)
    return sd


# ---------------------------------------------------------------- checkpoints
_SKIP = ("visual.", "model.visual.", "lm_head.")
_PREFIXES = ("model.language_model.", "language_model.model.", "language_model.", "model.")


def normalize_reason1_keys(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The text model's tensors under the bare key layout, from the reference's (`model.layers.N...`,
    `model.embed_tokens`, `model.norm`), transformers' (`model.language_model.` ...) or the bare one. `visual.*`,
    `lm_head.*` and `_extra_state` entries are skipped; any other unknown key raises."""
    out: Dict[str, torch.Tensor] = {}
    for key, v in sd.items():
        if key.startswith(_SKIP) or key.endswith("_extra_state") or not isinstance(v, torch.Tensor):
            continue
        k = key
        for p in _PREFIXES:
            if k.startswith(p):
                k = k[len(p):]
                break
        if not (k.startswith("layers.") or k in ("embed_tokens.weight", "norm.weight")):
            raise ValueError(f"unrecognised text-encoder checkpoint key {key!r}")
        if k in out:
            raise ValueError(f"checkpoint key {key!r} repeats {k!r}")
        out[k] = v
    return out


def load_reason1_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    """A .pt / .safetensors file or a folder of safetensors shards -> the normalised state dict."""
    from .checkpoint import _load

    if os.path.isdir(path):
        shards = sorted(f for f in os.listdir(path) if f.endswith(".safetensors"))
        if not shards:
            raise ValueError(f"{path} holds no .safetensors shards")
        sd: Dict[str, torch.Tensor] = {}
        for f in shards:
            part = _load(os.path.join(path, f))
            dup = set(part) & set(sd)
            if dup:
                raise ValueError(f"shard {f} repeats keys {sorted(dup)[:3]}")
            sd.update(part)
    else:
        sd = _load(path)
    return normalize_reason1_keys(sd)


def _check_state_dict(cfg: Reason1Config, sd: Dict[str, torch.Tensor]) -> None:
    shapes = reason1_state_dict_shapes(cfg)
    missing = [k for k in shapes if k not in sd]
    if missing:
        raise KeyError(f"text-encoder state dict misses {len(missing)} keys, e.g. {missing[:4]}")
    extra = [k for k in sd if k not in shapes]
    if extra:
        raise ValueError(f"text-encoder state dict has keys outside the config, e.g. {extra[:4]}")
    for k, shape in shapes.items():
        if tuple(sd[k].shape) != shape:
            raise ValueError(f"{k}: shape {tuple(sd[k].shape)}, the config wants {shape}")


# ---------------------------------------------------------------- prompts
def pad_or_truncate(ids: Sequence[int], pad_id: int, num_tokens: int) -> List[int]:
    """text_encoder.py:173-179: pad with pad_id to num_tokens ids, or keep the first num_tokens."""
    ids = [int(t) for t in ids]
    if num_tokens > len(ids):
        return ids + [int(pad_id)] * (num_tokens - len(ids))
    return ids[:num_tokens]


class PromptTokenizer:
    """prompt -> num_tokens ids. Either a local tokenizer directory opened with transformers (its own chat template and
    pad_token_id, as reason1/tokenizer/processor.py:74-91 does; never the network), or a plain callable `str -> ids`
    with a pad_id, which is given CHAT_TEMPLATE filled in."""

    def __init__(self, tokenizer: Optional[Callable[[str], Sequence[int]]] = None, pad_id: Optional[int] = None,
                 tokenizer_path: Optional[str] = None):
        if (tokenizer is None) == (tokenizer_path is None):
            raise ValueError("give exactly one of tokenizer (a callable str -> ids) and tokenizer_path")
        self._hf = None
        if tokenizer_path is not None:
            if not os.path.isdir(tokenizer_path):
                raise ValueError(f"tokenizer_path {tokenizer_path!r} is not a local directory")
            from transformers import AutoTokenizer

            self._hf = AutoTokenizer.from_pretrained(tokenizer_path, local_files_only=True)
            pad_id = self._hf.pad_token_id if pad_id is None else pad_id
        if pad_id is None:
            raise ValueError("the tokenizer needs a pad_id")
        self._fn = tokenizer
        self.pad_id = int(pad_id)

    def text(self, prompt: str) -> str:
        if self._hf is not None:
            conv = [{"role": "system", "content": [{"type": "text", "text": SYSTEM_PROMPT}]},
                    {"role": "user", "content": [{"type": "text", "text": prompt}]}]
            return self._hf.apply_chat_template(conv, tokenize=False, add_generation_prompt=False)
        return CHAT_TEMPLATE.format(system=SYSTEM_PROMPT, user=prompt)

    def __call__(self, prompt: str, num_tokens: int) -> List[int]:
        text = self.text(prompt)
        ids = self._hf(text)["input_ids"] if self._hf is not None else self._fn(text)
        return pad_or_truncate(ids, self.pad_id, num_tokens)


def byte_tokenizer(vocab_size: int) -> Callable[[str], List[int]]:
    """A stand-in tokenizer for tests and synthetic-weight runs: UTF-8 bytes modulo the vocabulary (ids 1 ..)."""
    return lambda text: [1 + b % (vocab_size - 1) for b in text.encode("utf-8")]


# ---------------------------------------------------------------- the encoder
def _require_gemm(n_out: int, k: int, what: str) -> None:
    if not N.gemm_supported(n_out, k):
        raise ValueError(f"{what} weight [{n_out}, {k}]: the own GEMM needs N % 256 == 0 and K % 64 == 0")


def _gemm(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """a [M, K] w [N, K]^T in bf16 on the small-M family where its plan takes the shape, else the 256 x 256 one; split 1
    always: one pass over K, the same bits from either."""
    M, K = a.shape
    if N.gemm_sm_plan(M, w.shape[0], K).small:
        return N.gemm_sm_epi(a, w, split=1)
    return N.gemm_epi(a, w)


def rope_tables(L: int, theta: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos / sin [L, 128] bf16 of Qwen2_5_VLRotaryEmbedding for positions arange(L): fp32 inv_freq and angles,
    cat(freqs, freqs), rounded to bf16 as the reference casts them to the activations' dtype. Host tensors."""
    inv_freq = 1.0 / (theta ** (torch.arange(0, HEAD_DIM, 2, dtype=torch.int64).float() / HEAD_DIM))
    freqs = torch.arange(L, dtype=torch.float32)[:, None] * inv_freq[None, :]
    emb = torch.cat([freqs, freqs], -1)
    return emb.cos().to(torch.bfloat16), emb.sin().to(torch.bfloat16)


class Reason1TextEncoder:
    """The pipeline's `text_encoder` callable: prompt -> [1, num_tokens, out_dim] bf16 on `device`.

    state_dict | ckpt_path: the weights (see load_reason1_checkpoint). tokenizer | tokenizer_path: see PromptTokenizer
    (tokenizer: a callable, with pad_id). offload=True parks the weights in host memory between encodes
    (inference/video2world.py:495-499). Results are cached per prompt string: the autoregressive and chunk loops
    re-encode the same two prompts for every chunk."""

    def __init__(self, cfg: Reason1Config = REASON1_7B, state_dict: Optional[Dict[str, torch.Tensor]] = None,
                 ckpt_path: Optional[str] = None, tokenizer: Union[None, Callable, PromptTokenizer] = None,
                 tokenizer_path: Optional[str] = None, pad_id: Optional[int] = None, device="cuda",
                 offload: bool = False):
        if cfg.embedding_concat_strategy != "full_concat":
            if cfg.embedding_concat_strategy in STRATEGIES:
                raise NotImplementedError(f"embedding_concat_strategy {cfg.embedding_concat_strategy!r} is not built: "
                                          "the released nets read full_concat (100352 channels)")
            raise ValueError(f"Invalid embedding_concat_strategy: {cfg.embedding_concat_strategy}")
        if cfg.num_attention_heads % cfg.num_key_value_heads:
            raise ValueError("num_attention_heads must be a multiple of num_key_value_heads")
        if cfg.num_tokens % 64:
            raise ValueError(f"num_tokens {cfg.num_tokens}: the causal attention needs a multiple of 64")
        if (state_dict is None) == (ckpt_path is None):
            raise ValueError("give exactly one of state_dict and ckpt_path")
        D, I = cfg.hidden_size, cfg.intermediate_size
        _require_gemm(cfg.qkv_dim, D + _BIAS_PAD, "q|k|v (with the bias column)")
        _require_gemm(D, cfg.num_attention_heads * HEAD_DIM, "o_proj")
        _require_gemm(2 * I, D, "gate|up")
        _require_gemm(D, I, "down_proj")
        self.cfg = cfg
        self.device = torch.device(device)
        self.offload = bool(offload)
        self.out_dim = cfg.out_dim
        if isinstance(tokenizer, PromptTokenizer):
            self.tokenizer = tokenizer
        elif tokenizer is None and tokenizer_path is None:
            self.tokenizer = None  # encode_ids only
        else:
            self.tokenizer = PromptTokenizer(tokenizer, pad_id, tokenizer_path)
        sd = normalize_reason1_keys(state_dict) if state_dict is not None else load_reason1_checkpoint(ckpt_path)
        _check_state_dict(cfg, sd)
        self._host = self._fuse(sd)
        self._dev: Optional[Dict[str, torch.Tensor]] = None
        self._rope: Dict[int, Tuple[torch.Tensor, torch.Tensor]] = {}
        self._cache: Dict[str, torch.Tensor] = {}
        if not self.offload:
            self._upload()

    # -- weights
    def _fuse(self, sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        """The GEMM operands in bf16 on the host: q|k|v rows fused, their biases as column D of a [*, D + 64] weight
        (columns D + 1 .. zero); gate|up rows fused."""
        cfg, bf = self.cfg, torch.bfloat16
        D = cfg.hidden_size
        w: Dict[str, torch.Tensor] = {"embed": sd["embed_tokens.weight"].to(bf).contiguous(),
                                      "norm": sd["norm.weight"].to(bf).contiguous()}
        for i in range(cfg.num_hidden_layers):
            p = f"layers.{i}."
            qkv = torch.zeros(cfg.qkv_dim, D + _BIAS_PAD, dtype=bf)
            r = 0
            for name in ("q_proj", "k_proj", "v_proj"):
                wt, b = sd[p + f"self_attn.{name}.weight"], sd[p + f"self_attn.{name}.bias"]
                qkv[r:r + wt.shape[0], :D] = wt.to(bf)
                qkv[r:r + wt.shape[0], D] = b.to(bf)
                r += wt.shape[0]
            w[f"{i}.qkv"] = qkv
            w[f"{i}.o"] = sd[p + "self_attn.o_proj.weight"].to(bf).contiguous()
            w[f"{i}.gu"] = torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], 0).to(bf).contiguous()
            w[f"{i}.down"] = sd[p + "mlp.down_proj.weight"].to(bf).contiguous()
            w[f"{i}.ln1"] = sd[p + "input_layernorm.weight"].to(bf).contiguous()
            w[f"{i}.ln2"] = sd[p + "post_attention_layernorm.weight"].to(bf).contiguous()
        return w

    @classmethod
    def synthetic(cls, cfg: Reason1Config = REASON1_7B, device="cuda", seed: int = 0, **kw) -> "Reason1TextEncoder":
        """An encoder with random weights drawn directly on the device, in the fused layout (benchmarks at the 7B size,
        where a host state dict would take minutes to draw): the distribution of init_reason1_state_dict, not its bits."""
        one = dataclasses.replace(cfg, num_hidden_layers=1, vocab_size=256)
        self = cls(one, state_dict=init_reason1_state_dict(one, seed), device="cpu", offload=True, **kw)
        self.cfg, self.out_dim, self.offload = cfg, cfg.out_dim, False
        self.device = torch.device(device)
        g = torch.Generator(device=self.device).manual_seed(seed)
        D = cfg.hidden_size

        def draw(*shape, scale=1.0, shift=0.0):
            return (torch.randn(shape, generator=g, device=self.device) * scale + shift).to(torch.bfloat16)

        dev = {"embed": draw(cfg.vocab_size, D), "norm": draw(D, scale=0.1, shift=1.0)}
        for i in range(cfg.num_hidden_layers):
            qkv = torch.zeros(cfg.qkv_dim, D + _BIAS_PAD, dtype=torch.bfloat16, device=self.device)
            qkv[:, :D] = draw(cfg.qkv_dim, D, scale=D ** -0.5)
            qkv[:, D] = draw(cfg.qkv_dim, scale=0.5)
            dev.update({f"{i}.qkv": qkv, f"{i}.o": draw(D, cfg.num_attention_heads * HEAD_DIM, scale=D ** -0.5),
                        f"{i}.gu": draw(2 * cfg.intermediate_size, D, scale=D ** -0.5),
                        f"{i}.down": draw(D, cfg.intermediate_size, scale=cfg.intermediate_size ** -0.5),
                        f"{i}.ln1": draw(D, scale=0.1, shift=1.0), f"{i}.ln2": draw(D, scale=0.1, shift=1.0)})
        self._host, self._dev = dev, dev  # resident only: there is no host copy to park
        return self

    def _upload(self) -> Dict[str, torch.Tensor]:
        if self._dev is None:
            self._dev = {k: v.to(self.device) for k, v in self._host.items()}
        return self._dev

    def _park(self) -> None:
        if self.offload:
            self._dev = None
            self._rope.clear()

    # -- forward
    def _tables(self, L: int) -> Tuple[torch.Tensor, torch.Tensor]:
        if L not in self._rope:
            c, s = rope_tables(L, self.cfg.rope_theta)
            self._rope[L] = (c.to(self.device), s.to(self.device))
        return self._rope[L]

    @torch.no_grad()
    def encode_ids(self, ids: torch.Tensor) -> torch.Tensor:
        """ids [B, L] (host or device integers; validated on the host) -> [B, L, out_dim] bf16: the concatenation of
        the mean-normalised hidden_states[1:]. L % 64 == 0."""
        if ids.dim() != 2:
            raise ValueError(f"encode_ids: ids must be [B, L], got {tuple(ids.shape)}")
        B, L = ids.shape
        if L % 64:
            raise ValueError(f"encode_ids: L = {L} is not a multiple of 64")
        cfg = self.cfg
        D, Hq, Hkv = cfg.hidden_size, cfg.num_attention_heads, cfg.num_key_value_heads
        n = B * L
        W = self._upload()
        with torch.cuda.device(self.device):
            cos, sin = self._tables(L)
            x = N.embed_gather(W["embed"], ids.detach().cpu())
            out = torch.empty((n, cfg.out_dim), dtype=torch.bfloat16, device=self.device)
            h_b = torch.empty((n, D + _BIAS_PAD), dtype=torch.bfloat16, device=self.device)
            h = torch.empty((n, D), dtype=torch.bfloat16, device=self.device)
            a = torch.empty((B, L, Hq, HEAD_DIM), dtype=torch.bfloat16, device=self.device)
            m = None
            for i in range(cfg.num_hidden_layers):
                N.add_rmsnorm(x, m, W[f"{i}.ln1"], eps=cfg.rms_norm_eps, h_ld=D + _BIAS_PAD, out=h_b)
                if i:
                    N.mean_normalize(x, out, (i - 1) * D)  # hidden_states[i]
                qkv = _gemm(h_b, W[f"{i}.qkv"])
                N.rope_qk(qkv, cos, sin, heads=Hq + Hkv)
                v4 = qkv.view(B, L, Hq + 2 * Hkv, HEAD_DIM)
                N.attn_causal(v4[:, :, :Hq], v4[:, :, Hq:Hq + Hkv], v4[:, :, Hq + Hkv:], out=a)
                o = _gemm(a.view(n, Hq * HEAD_DIM), W[f"{i}.o"])
                N.add_rmsnorm(x, o, W[f"{i}.ln2"], eps=cfg.rms_norm_eps, out=h)
                m = _gemm(N.swiglu(_gemm(h, W[f"{i}.gu"])), W[f"{i}.down"])
            N.add_rmsnorm(x, m, W["norm"], eps=cfg.rms_norm_eps, out=h)  # hidden_states[-1]: through the final norm
            N.mean_normalize(h, out, (cfg.num_hidden_layers - 1) * D)
        self._park()
        return out.view(B, L, cfg.out_dim)

    def token_ids(self, prompt: str) -> torch.Tensor:
        if self.tokenizer is None:
            raise ValueError("this encoder was built without a tokenizer: use encode_ids")
        return torch.tensor([self.tokenizer(prompt, self.cfg.num_tokens)], dtype=torch.int64)

    def __call__(self, prompt: str) -> torch.Tensor:
        hit = self._cache.get(prompt)
        if hit is None:
            hit = self.encode_ids(self.token_ids(prompt))
            self._cache[prompt] = hit
        return hit


def build_text_encoder(text_encoder_path: str, text_tokenizer_path: Optional[str], *, expect_dim: int, device,
                       offload: bool = False, cfg: Optional[Reason1Config] = None) -> Reason1TextEncoder:
    """The encoder the entry points build from `text_encoder_path` / `text_tokenizer_path`. cfg None: REASON1_7B, or, for
    a checkpoint of another size, the config its tensors imply (layers, widths, vocabulary). Without a tokenizer
    directory the byte stand-in is used only when the vocabulary is not Qwen's (a synthetic checkpoint); a real one
    needs its tokenizer. The encoder's out_dim must equal expect_dim (the net's crossattn_proj_in_channels)."""
    sd = load_reason1_checkpoint(text_encoder_path)
    if cfg is None:
        cfg = config_from_state_dict(sd)
    if cfg.out_dim != expect_dim:
        raise ValueError(f"text encoder out_dim {cfg.out_dim} ({cfg.num_hidden_layers} x {cfg.hidden_size}) != the "
                         f"net's crossattn_proj_in_channels {expect_dim}")
    if text_tokenizer_path is None:
        if cfg.vocab_size == REASON1_7B.vocab_size:
            raise ValueError("text_encoder_path needs text_tokenizer_path (a local Qwen2.5-VL tokenizer directory)")
        return Reason1TextEncoder(cfg, state_dict=sd, tokenizer=byte_tokenizer(cfg.vocab_size), pad_id=0, device=device,
                                  offload=offload)
    return Reason1TextEncoder(cfg, state_dict=sd, tokenizer_path=text_tokenizer_path, device=device, offload=offload)


def config_from_state_dict(sd: Dict[str, torch.Tensor]) -> Reason1Config:
    """The config a normalised state dict's tensors imply (head dim 128)."""
    for k in ("embed_tokens.weight", "layers.0.self_attn.q_proj.weight", "layers.0.self_attn.k_proj.weight",
              "layers.0.mlp.gate_proj.weight"):
        if k not in sd:
            raise KeyError(f"text-encoder state dict misses {k}")
    layers = [int(m.group(1)) for m in (re.match(r"layers\.(\d+)\.", k) for k in sd) if m]
    V, D = sd["embed_tokens.weight"].shape
    return Reason1Config(vocab_size=V, hidden_size=D, intermediate_size=sd["layers.0.mlp.gate_proj.weight"].shape[0],
                         num_hidden_layers=max(layers) + 1,
                         num_attention_heads=sd["layers.0.self_attn.q_proj.weight"].shape[0] // HEAD_DIM,
                         num_key_value_heads=sd["layers.0.self_attn.k_proj.weight"].shape[0] // HEAD_DIM)
