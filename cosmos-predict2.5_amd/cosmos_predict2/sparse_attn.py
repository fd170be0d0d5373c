"""Sparse-attention DiT: 3D neighborhood attention on the MI355X box kernel (cp25_attn_na3d).

The reference's net option `MiniTrainDIT(n_dense_blocks=..., natten_parameters=...)`
(networks/minimal_v4_dit.py:1284-1289, 1349-1350, 1439-1441) swaps the self-attention op of selected blocks for
`NattenA2AAttnOp` (networks/a2a_cp.py:222-226), a 3D neighborhood attention (modules/neighborhood_attn.py) in which a
query (t, h, w) sees only a box of keys around it. This module is the host side of that option:

* `NattenParams` / `adaptive_parameters`: the parameters and their per-input rescaling
  (NeighborhoodAttention.get_adaptive_parameters, neighborhood_attn.py:140-171);
* `axis_windows`: the per-axis window rule (below);
* `sparse_block_params`: which blocks stay dense (replace_selfattn_op_with_sparse_attn_op, minimal_v4_dit.py:1760-1796);
* `build_plan`: the two int32 tables the kernel walks: queries grouped into tiles that share one key box;
* `NeighborhoodAttnOp`: the plug-compatible op, forward(q, k, v, video_size=VideoSize(T, H, W)) -> [B, S, H D].

Window rule per axis (length L, window K, stride s, dilation d, non-causal), for index i:

    g  = i mod d                      # dilation group
    p  = i div d                      # position inside the group
    Lg = L div d + (1 if g < L mod d else 0)
    leader = min((p div s) * s + s div 2, Lg - 1)
    start  = clamp(leader - K div 2, 0, Lg - K)
    keys   = { g + (start + j) * d : j = 0 .. K-1 }

A query attends the product of its three per-axis key sets. NATTEN itself runs only on CUDA devices, so parity with its
kernels is not pinned here; the tests pin this rule and the facts NATTEN documents (exactly K keys per
axis, a centred window for odd K in the interior, block attention at s == K, dense attention at a full window).
"""
from __future__ import annotations

from collections import namedtuple
from dataclasses import dataclass
from typing import Any, Dict, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _native as N

BF16 = torch.bfloat16
VideoSize = namedtuple("VideoSize", ["T", "H", "W"])  # neighborhood_attn.py:47


def _triple(x, name: str) -> tuple:
    if isinstance(x, (bool, int, np.integer)):
        return (x, x, x)
    t = tuple(x)
    if len(t) != 3:
        raise ValueError(f"{name} must be a scalar or have 3 entries, got {x!r}")
    return t


@dataclass(frozen=True)
class NattenParams:
    """The reference's natten_parameters dict (neighborhood_attn.py:60-106) in hashable form."""

    window_size: tuple
    stride: Union[int, tuple] = 1
    dilation: Union[int, tuple] = 1
    is_causal: Union[bool, tuple] = False
    base_size: Optional[tuple] = None

    def __post_init__(self):
        w = tuple(int(x) for x in self.window_size)
        if len(w) != 3:
            raise ValueError(f"window_size must have 3 entries, got {self.window_size!r}")
        object.__setattr__(self, "window_size", w)
        for f in ("stride", "dilation"):
            v = getattr(self, f)
            object.__setattr__(self, f, int(v) if isinstance(v, (int, np.integer)) else
                               tuple(int(x) for x in _triple(v, f)))
        c = self.is_causal
        object.__setattr__(self, "is_causal", bool(c) if isinstance(c, (bool, np.bool_)) else
                           tuple(bool(x) for x in _triple(c, "is_causal")))
        if self.base_size is not None:
            b = tuple(int(x) for x in self.base_size)
            if len(b) != 3:
                raise ValueError(f"base_size must have 3 entries or be None, got {self.base_size!r}")
            object.__setattr__(self, "base_size", b)

    @classmethod
    def of(cls, p: Any) -> Optional["NattenParams"]:
        """A NattenParams from one, from the reference's dict (extra keys such as layer_id are dropped), or None."""
        if p is None or isinstance(p, cls):
            return p
        if isinstance(p, dict):
            if "window_size" not in p:
                raise ValueError("natten_parameters needs a window_size")
            return cls(**{k: p[k] for k in ("window_size", "stride", "dilation", "is_causal", "base_size") if k in p})
        raise ValueError(f"natten_parameters: a dict or NattenParams expected, got {type(p).__name__}")


def adaptive_parameters(params, input_shape: Sequence[int]) -> Tuple[tuple, tuple, tuple]:
    """(window, stride, dilation) for an input grid (T, H, W): get_adaptive_parameters (neighborhood_attn.py:140-171).
    Window entries <= 1 mean the full extent; with base_size the three are rescaled by input / base with the
    reference's clamps (round is Python's, half to even). Its closing assertions are ValueErrors here; a causal axis
    raises NotImplementedError."""
    p = NattenParams.of(params)
    shape = tuple(int(x) for x in input_shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"input shape (T, H, W) expected, got {input_shape!r}")
    if any(_triple(p.is_causal, "is_causal")):
        raise NotImplementedError("causal neighborhood attention is not built (the registered recipes are non-causal)")
    window = tuple(w if w > 1 else x for x, w in zip(shape, p.window_size))
    stride = _triple(p.stride, "stride")
    dilation = _triple(p.dilation, "dilation")
    if p.base_size is not None:
        base = tuple(b if b > 0 else x for x, b in zip(shape, p.base_size))
        scale = tuple(x / b for x, b in zip(shape, base))
        window = tuple(min(max(2, round(w * s)), x) for w, s, x in zip(window, scale, shape))
        stride = tuple(min(max(1, round(st * s)), w) for w, s, st in zip(window, scale, stride))
        max_dil = tuple(x // w for x, w in zip(shape, window))
        dilation = tuple(min(max(1, round(d * s)), md) for d, s, md in zip(dilation, scale, max_dil))
    if min(stride) < 1 or min(dilation) < 1:
        raise ValueError(f"stride {stride} and dilation {dilation} must be >= 1")
    if not all(x >= w * d for x, w, d in zip(shape, window, dilation)):
        raise ValueError(f"window {window} x dilation {dilation} does not fit the input {shape}")
    if not all(w >= s for w, s in zip(window, stride)):
        raise ValueError(f"stride {stride} exceeds the window {window}")
    return window, stride, dilation


def axis_windows(L: int, K: int, s: int = 1, d: int = 1) -> np.ndarray:
    """int64 [L, 2]: (dilation group g, window start inside the group) of every index of an axis, the rule in the
    module docstring; index i attends keys g + (start + j) d, j < K."""
    if not (K >= 1 and s >= 1 and d >= 1 and K * d <= L and s <= K):
        raise ValueError(f"axis of {L}: window {K}, stride {s}, dilation {d} do not fit")
    i = np.arange(L, dtype=np.int64)
    g, p = i % d, i // d
    Lg = L // d + (g < L % d)
    leader = np.minimum((p // s) * s + s // 2, Lg - 1)
    start = np.clip(leader - K // 2, 0, Lg - K)
    return np.stack([g, start], axis=1)


def sparse_block_params(num_blocks: int, n_dense_blocks: int, natten_parameters) -> List[Optional[NattenParams]]:
    """Per-block NattenParams, None for a dense block (replace_selfattn_op_with_sparse_attn_op,
    minimal_v4_dit.py:1760-1796): -1 = no sparse block; a list / tuple gives per-block parameters (None = dense) and
    must have num_blocks entries; with one dict 0 makes every block sparse, 1 keeps block num_blocks // 2 dense,
    n > 1 keeps np.linspace(0, num_blocks - 1, n, dtype=int) dense, n >= num_blocks is an error."""
    if n_dense_blocks == -1:
        return [None] * num_blocks
    if natten_parameters is None or (isinstance(natten_parameters, (list, tuple)) and len(natten_parameters) == 0):
        raise ValueError("natten_parameters must be given when n_dense_blocks > -1")
    if isinstance(natten_parameters, (list, tuple)):
        if len(natten_parameters) != num_blocks:
            raise ValueError("a list of NATTEN parameters must have one entry per block, got "
                             f"{len(natten_parameters)} for {num_blocks} blocks")
        return [NattenParams.of(p) for p in natten_parameters]
    if n_dense_blocks >= num_blocks or n_dense_blocks < -1:
        raise ValueError(f"n_dense_blocks ({n_dense_blocks}) must be in [-1, {num_blocks})")
    p = NattenParams.of(natten_parameters)
    dense = set()
    if n_dense_blocks == 1:
        dense.add(num_blocks // 2)
    elif n_dense_blocks > 1:
        dense.update(np.linspace(0, num_blocks - 1, n_dense_blocks, dtype=int).tolist())
    return [None if i in dense else p for i in range(num_blocks)]


@dataclass
class NaPlan:
    """What cp25_attn_na3d walks: q_tok int32 [n_tiles, 128] (token ids of each tile's query rows, -1 = empty slot),
    box int32 [n_tiles, 4] (first key index along t, h, w), for one grid and one set of adapted parameters."""

    grid: tuple
    window: tuple
    stride: tuple
    dilation: tuple
    q_tok: torch.Tensor
    box: torch.Tensor

    @property
    def n_tiles(self) -> int:
        return int(self.q_tok.shape[0])

    @property
    def keys_per_query(self) -> int:
        return int(np.prod(self.window))

    @property
    def density(self) -> float:
        return self.keys_per_query / float(np.prod(self.grid))


def plan_tables(grid: Sequence[int], window: Sequence[int], stride: Sequence[int], dilation: Sequence[int],
                tile_rows: int = N.NA_TILE_ROWS) -> Tuple[np.ndarray, np.ndarray]:
    """(q_tok [n_tiles, tile_rows], box [n_tiles, 4]) int32 numpy tables. Queries with the same (dilation group,
    window start) on every axis share one key box; each such group fills ceil(size / tile_rows) tiles in token order,
    the last one partly empty. Groups are laid out in (t, h, w) box order so that neighbouring tiles (neighbouring
    workgroups) read the same or adjacent K / V rows. Every index is checked against the grid here, before any
    launch."""
    T, H, W = (int(x) for x in grid)
    L = T * H * W
    ax = [axis_windows(n, int(k), int(s), int(d)) for n, k, s, d in zip((T, H, W), window, stride, dilation)]
    # a per-axis group key: group * L_axis + start (unique), then one int64 key per token, t-major
    keys = [a[:, 0] * n + a[:, 1] for a, n in zip(ax, (T, H, W))]
    kt, kh, kw = np.meshgrid(*keys, indexing="ij")
    key = ((kt * (H * H + H) + kh) * (W * W + W) + kw).reshape(-1)
    order = np.argsort(key, kind="stable")  # tokens grouped by box, ascending token id inside a group
    skey = key[order]
    bounds = np.flatnonzero(np.r_[True, skey[1:] != skey[:-1], True])
    q_rows, boxes = [], []
    for b0, b1 in zip(bounds[:-1], bounds[1:]):
        toks = order[b0:b1]
        t, h, w = np.unravel_index(int(toks[0]), (T, H, W))
        first = [int(a[i, 0] + a[i, 1] * d) for a, i, d in zip(ax, (t, h, w), dilation)]
        for c0 in range(0, len(toks), tile_rows):
            row = np.full(tile_rows, -1, dtype=np.int64)
            chunk = toks[c0:c0 + tile_rows]
            row[:len(chunk)] = chunk
            q_rows.append(row)
            boxes.append(first + [0])
    q_tok = np.stack(q_rows).astype(np.int32)
    box = np.asarray(boxes, dtype=np.int32)
    # fault safety: every query id and every corner of every box inside the grid, every token exactly once
    live = q_tok[q_tok >= 0]
    if live.size != L or not np.array_equal(np.sort(live), np.arange(L)) or np.any(q_tok[:, 0] < 0):
        raise AssertionError("neighborhood plan: the tiles do not hold every token exactly once")
    last = box[:, :3] + (np.asarray(window) - 1) * np.asarray(dilation)
    if box.min() < 0 or np.any(last >= np.asarray([T, H, W])):
        raise AssertionError("neighborhood plan: a key box leaves the grid")
    return q_tok, box


def build_plan(grid: Sequence[int], params, device) -> NaPlan:
    """The plan of a (T, H, W) grid under natten parameters (adapted to the grid), tables on `device`."""
    window, stride, dilation = adaptive_parameters(params, grid)
    q_tok, box = plan_tables(grid, window, stride, dilation)
    return NaPlan(grid=tuple(int(x) for x in grid), window=window, stride=stride, dilation=dilation,
                  q_tok=torch.from_numpy(q_tok).to(device), box=torch.from_numpy(box).to(device))


class PlanCache:
    """Plans by (grid, parameters): built once (a host-to-device copy), then reused by every launch."""

    def __init__(self, device):
        self.device = device
        self._plans: Dict[tuple, NaPlan] = {}

    def get(self, grid: Sequence[int], params) -> NaPlan:
        key = (tuple(int(x) for x in grid), NattenParams.of(params))
        if key not in self._plans:
            self._plans[key] = build_plan(key[0], key[1], self.device)
        return self._plans[key]


class NeighborhoodAttnOp(torch.nn.Module):
    """Drop-in sparse `Attention.attn_op` mirroring NattenA2AAttnOp (a2a_cp.py:222-226):
    forward(q, k, v [B, S, H, D], video_size=VideoSize(T, H, W)) -> [B, S, H*D] bf16. T == 1 runs dense attention
    (neighborhood_attn.py:226-228). A context-parallel group of more than one rank is not served."""

    def __init__(self, *args: Any, natten_parameters=None, softmax_scale: Optional[float] = None, **kwargs: Any):
        del args, kwargs
        super().__init__()
        if natten_parameters is None:
            raise ValueError("NeighborhoodAttnOp needs natten_parameters")
        self.params = NattenParams.of(natten_parameters)
        if any(_triple(self.params.is_causal, "is_causal")):
            raise NotImplementedError("causal neighborhood attention is not built")
        self.softmax_scale = softmax_scale
        self.pg = None
        self._plans: Optional[PlanCache] = None

    def set_context_parallel_group(self, process_group, ranks=None, stream=None) -> None:
        del ranks, stream
        self.pg = process_group

    def forward(self, query: torch.Tensor, key: torch.Tensor, value: torch.Tensor,
                video_size: Optional[VideoSize] = None) -> torch.Tensor:
        if video_size is None:
            raise ValueError("NeighborhoodAttnOp needs video_size=(T, H, W)")
        if not (query.shape == key.shape == value.shape) or query.dim() != 4:
            raise ValueError(f"neighborhood attention needs q/k/v [B, S, H, D] of one shape, got {tuple(query.shape)} "
                             f"{tuple(key.shape)} {tuple(value.shape)}")
        if self.pg is not None and torch.distributed.get_world_size(self.pg) > 1:
            raise NotImplementedError("neighborhood attention under context parallelism is not built")
        B, S, H, D = query.shape
        T, Hg, Wg = (int(x) for x in video_size)
        if S != T * Hg * Wg:
            raise ValueError(f"mismatch between seqlen {S} and video_size {tuple(video_size)}")
        if T < 1:
            raise ValueError(f"invalid dimension T={T}")
        q, k, v = query.to(BF16), key.to(BF16), value.to(BF16)
        if T == 1:  # image input: dense attention
            return N.attn_fwd(q, k, v, softmax_scale=self.softmax_scale).reshape(B, S, H * D)
        if self._plans is None or self._plans.device != q.device:
            self._plans = PlanCache(q.device)
        plan = self._plans.get((T, Hg, Wg), self.params)
        return N.attn_na3d(q, k, v, plan, softmax_scale=self.softmax_scale).reshape(B, S, H * D)
