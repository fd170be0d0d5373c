"""Checkpoint loading for the reference's released files (safe loaders only).

DiT: a single .pt state dict with `net.`-prefixed keys (EMA already folded in; the reference loads it
with strict=False and skips `_extra_state`: cosmos_predict2/_src/predict2/utils/model_loader.py:100-177,
text2world_model_rectified_flow.py:761-803). VAE: Wan2.1 `tokenizer.pth` (encoder.*, conv1.*, conv2.*,
decoder.*; wan2pt1.py:648-670). Only `torch.load(weights_only=True)` / safetensors are used.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch


def _load(path: str) -> Dict[str, torch.Tensor]:
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file

        return load_file(path)
    obj = torch.load(path, map_location="cpu", weights_only=True)
    for key in ("model", "state_dict"):
        if isinstance(obj, dict) and key in obj and isinstance(obj[key], dict):
            obj = obj[key]
    return obj


def load_dit_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    sd = _load(path)
    return {k: v for k, v in sd.items() if isinstance(v, torch.Tensor) and not k.endswith("_extra_state")}


LoraAdapters = Dict[str, Tuple[torch.Tensor, torch.Tensor]]
_PEFT_PREFIX = "base_model.model."


def split_lora_state_dict(sd: Dict[str, torch.Tensor]) -> Tuple[Dict[str, torch.Tensor], LoraAdapters]:
    """Splits a peft-layout state dict into (base_sd, adapters); a plain dict comes back with no adapters.

    The reference post-trains with peft LoRA layers (add_lora, text2world_model_rectified_flow.py:923-1008), whose
    state dict holds the frozen weight of a wrapped module under `<module>.base_layer.weight` and the adapter under
    `<module>.lora_A.<name>.weight` [r, K] / `<module>.lora_B.<name>.weight` [N, r] (utils/model_loader.py:134-169
    maps the `base_layer.` keys). base_sd has `base_layer.` removed; adapters is {module: (A, B)} with the module
    named as in the net's state dict (`blocks.0.self_attn.q_proj`). Both adapter forms are read: peft's state-dict
    form with the adapter name (`lora_A.default.weight`) and the saved-adapter form without one (`lora_A.weight`,
    optionally under `base_model.model.`). As in MinimalV1LVGDiT.load_state_dict a `net.` prefix is dropped and
    `net_ema.` keys are skipped. The rank is the tensors' own; alpha is not part of a state dict (the caller has it).

    ValueError: a lora_A without its lora_B (or the reverse), more than one adapter name, tensors that are not
    matrices or whose ranks differ within a pair, and any other `lora_` key (embedding adapters, DoRA magnitudes):
    nothing is dropped silently."""
    base: Dict[str, torch.Tensor] = {}
    halves: Dict[str, Dict[str, torch.Tensor]] = {}
    names = set()
    for key, v in sd.items():
        if key.startswith("net_ema."):
            continue
        k = key[len(_PEFT_PREFIX):] if key.startswith(_PEFT_PREFIX) else key
        k = k[4:] if k.startswith("net.") else k
        parts = k.split(".")
        which = [i for i, s in enumerate(parts) if s in ("lora_A", "lora_B")]
        if which:
            i = which[-1]
            tail = parts[i + 1:]
            if i == 0 or tail[-1:] != ["weight"] or len(tail) > 2:
                raise ValueError(f"unrecognised LoRA key {key!r}")
            names.add(tail[0] if len(tail) == 2 else "")
            module = ".".join(parts[:i])
            if parts[i] in halves.setdefault(module, {}):
                raise ValueError(f"LoRA key {key!r} repeats {module}.{parts[i]}")
            halves[module][parts[i]] = v
        elif any(s.startswith("lora_") for s in parts):
            raise ValueError(f"unsupported LoRA key {key!r}: only lora_A / lora_B weight matrices can be merged")
        else:
            base[k.replace(".base_layer.", ".")] = v
    if len(names) > 1:
        raise ValueError(f"more than one adapter name in the state dict: {sorted(names)}")
    adapters: LoraAdapters = {}
    for module, h in halves.items():
        if "lora_A" not in h or "lora_B" not in h:
            have, lack = ("lora_A", "lora_B") if "lora_A" in h else ("lora_B", "lora_A")
            raise ValueError(f"{module}: {have} without its {lack}")
        a, b = h["lora_A"], h["lora_B"]
        if a.dim() != 2 or b.dim() != 2:
            raise ValueError(f"{module}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} are not matrices")
        if a.shape[0] != b.shape[1]:
            raise ValueError(f"{module}: lora_A has rank {a.shape[0]}, lora_B rank {b.shape[1]}")
        adapters[module] = (a, b)
    return base, adapters


def load_lora_adapters(path: str) -> LoraAdapters:
    """An adapter-only file (safetensors or .pt): its {module: (A, B)}; a file without adapters is an error."""
    _, adapters = split_lora_state_dict(load_dit_checkpoint(path))
    if not adapters:
        raise ValueError(f"{path} holds no lora_A / lora_B tensors")
    return adapters


def load_vae_checkpoint(path: str) -> Dict[str, torch.Tensor]:
    return {k: v for k, v in _load(path).items() if isinstance(v, torch.Tensor)}
