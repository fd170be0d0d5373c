"""CPU: the neighborhood-attention host side (cosmos_predict2/sparse_attn.py): the per-axis window rule against hand
values and the brute-force mask of tests/na_truth.py, the adaptive parameters, the dense-block choice, the kernel plan
and the sparse model names. No kernel launches."""
import numpy as np
import pytest
import torch

import __graft_entry__  # noqa: F401  (sets sys.path)
import na_truth as NT
from cosmos_predict2 import sparse_attn as SA
from cosmos_predict2.config import SetupArguments
from cosmos_predict2.net_config import MODELS, DiTConfig, tiny_dit

P7 = dict(window_size=(-1, 12, 24), stride=(1, 4, 8), base_size=(-1, 44, 80))


def _starts(L, K, s=1, d=1):
    return SA.axis_windows(L, K, s, d)[:, 1].tolist()


def _keys(L, K, s, d, i):
    g, st = SA.axis_windows(L, K, s, d)[i]
    return {int(g + (st + j) * d) for j in range(K)}


def test_axis_rule_hand_values():
    s = _starts(44, 12, 4)
    assert s[:8] == [0] * 8 and s[8:12] == [4] * 4 and s[40:44] == [32] * 4
    s = _starts(80, 24, 8)
    assert s[:16] == [0] * 16 and s[16:24] == [8] * 8 and s[72:80] == [56] * 8
    assert _starts(20, 4, 4) == [4 * (i // 4) for i in range(20)]  # K == s: block attention
    assert _keys(11, 3, 1, 3, 0) == {0, 3, 6}
    assert _keys(11, 3, 1, 3, 9) == {3, 6, 9}
    assert _keys(11, 3, 1, 3, 8) == {2, 5, 8}


def test_axis_rule_documented_facts():
    # odd K, stride 1, interior: the window is centred on the query; every index sees exactly K distinct keys
    for L, K in ((17, 5), (9, 3), (12, 7)):
        st = _starts(L, K)
        for i in range(K // 2, L - K // 2):
            assert st[i] == i - K // 2
    for L, K, s, d in ((44, 12, 4, 1), (11, 3, 1, 3), (13, 6, 4, 2), (9, 4, 1, 2)):
        for i in range(L):
            ks = _keys(L, K, s, d, i)
            assert len(ks) == K and min(ks) >= 0 and max(ks) < L
    assert _starts(8, 8, 3) == [0] * 8  # a full window is dense attention
    with pytest.raises(ValueError):
        SA.axis_windows(10, 6, 1, 2)
    with pytest.raises(ValueError):
        SA.axis_windows(10, 3, 4, 1)


def _mask_from_rule(grid, window, stride, dilation):
    T, H, W = grid
    ax = [SA.axis_windows(n, k, s, d) for n, k, s, d in zip(grid, window, stride, dilation)]
    sets = [[[int(a[i, 0] + (a[i, 1] + j) * d) for j in range(k)] for i in range(n)]
            for a, n, k, d in zip(ax, grid, window, dilation)]
    mask = torch.zeros(T * H * W, T * H * W, dtype=torch.bool)
    for t in range(T):
        for h in range(H):
            for w in range(W):
                keys = [(a * H + b) * W + c for a in sets[0][t] for b in sets[1][h] for c in sets[2][w]]
                mask[(t * H + h) * W + w, keys] = True
    return mask


@pytest.mark.parametrize("case", sorted(NT.NA_CASES))
def test_rule_reproduces_brute_force_mask(case):
    grid, params = NT.NA_CASES[case]
    window, stride, dilation = SA.adaptive_parameters(params, grid)
    truth = NT.na_mask(*grid, params)
    assert torch.equal(_mask_from_rule(grid, window, stride, dilation), truth)
    assert (truth.sum(1) == int(np.prod(window))).all()
    if case == "e_full":
        assert truth.all()


def test_adaptive_parameters():
    assert SA.adaptive_parameters(P7, (31, 44, 80)) == ((31, 12, 24), (1, 4, 8), (1, 1, 1))
    assert SA.adaptive_parameters(P7, (24, 30, 52)) == ((24, 8, 16), (1, 3, 5), (1, 1, 1))
    assert SA.adaptive_parameters(SA.NattenParams(**P7), (31, 44, 80))[0] == (31, 12, 24)
    # int stride / dilation broadcast; window <= 1 is the full extent
    assert SA.adaptive_parameters(dict(window_size=(1, 0, 3), stride=1, dilation=(1, 1, 2)), (4, 5, 6)) == \
        ((4, 5, 3), (1, 1, 1), (1, 1, 2))
    assert SA.adaptive_parameters(dict(window_size=(-1, 2, 3), stride=2, dilation=(1, 2, 2)), (4, 5, 6)) == \
        ((4, 2, 3), (2, 2, 2), (1, 2, 2))
    with pytest.raises(ValueError):  # x >= w * d
        SA.adaptive_parameters(dict(window_size=(-1, 4, 4), dilation=(1, 2, 1)), (2, 6, 8))
    with pytest.raises(ValueError):  # w >= s
        SA.adaptive_parameters(dict(window_size=(-1, 4, 4), stride=(1, 5, 1)), (2, 8, 8))
    with pytest.raises(NotImplementedError):
        SA.adaptive_parameters(dict(window_size=(-1, 4, 4), is_causal=(True, False, False)), (2, 8, 8))
    with pytest.raises(NotImplementedError):
        SA.adaptive_parameters(dict(window_size=(-1, 4, 4), is_causal=True), (2, 8, 8))
    hash(SA.NattenParams(**P7))
    assert SA.NattenParams.of(dict(P7, layer_id=3)) == SA.NattenParams(**P7)


def _sparse_ids(blocks):
    return {i for i, p in enumerate(blocks) if p is None}


def test_dense_block_choice():
    assert _sparse_ids(SA.sparse_block_params(28, 7, P7)) == {0, 4, 9, 13, 18, 22, 27}
    assert _sparse_ids(SA.sparse_block_params(28, 1, P7)) == {14}
    assert _sparse_ids(SA.sparse_block_params(28, 0, P7)) == set()
    assert SA.sparse_block_params(28, -1, P7) == [None] * 28
    assert SA.sparse_block_params(28, -1, None) == [None] * 28
    lst = [P7, None, dict(window_size=(-1, 4, 4))]
    got = SA.sparse_block_params(3, 0, lst)
    assert got[1] is None and got[0] == SA.NattenParams(**P7) and got[2].window_size == (-1, 4, 4)
    with pytest.raises(ValueError):
        SA.sparse_block_params(4, 0, lst)
    with pytest.raises(ValueError):
        SA.sparse_block_params(28, 28, P7)
    with pytest.raises(ValueError):
        SA.sparse_block_params(28, 3, None)


@pytest.mark.parametrize("case", sorted(NT.NA_CASES) + ["metric_small"])
def test_plan_covers_every_token_with_its_box(case):
    grid, params = NT.NA_CASES[case] if case in NT.NA_CASES else ((3, 11, 20), P7)
    window, stride, dilation = SA.adaptive_parameters(params, grid)
    q_tok, box = SA.plan_tables(grid, window, stride, dilation)
    T, H, W = grid
    L = T * H * W
    assert q_tok.dtype == np.int32 and box.dtype == np.int32 and q_tok.shape[1] == 128 and box.shape == (len(q_tok), 4)
    live = q_tok[q_tok >= 0]
    assert sorted(live.tolist()) == list(range(L))  # every token in exactly one slot
    assert (q_tok[:, 0] >= 0).all() and q_tok.max() < L and q_tok.min() >= -1
    truth = NT.na_mask(T, H, W, dict(window_size=window, stride=stride, dilation=dilation))
    for row, (t0, h0, w0, _) in zip(q_tok, box.tolist()):
        keys = [((t0 + a * dilation[0]) * H + h0 + b * dilation[1]) * W + w0 + c * dilation[2]
                for a in range(window[0]) for b in range(window[1]) for c in range(window[2])]
        assert min(keys) >= 0 and max(keys) < L
        want = torch.zeros(L, dtype=torch.bool)
        want[keys] = True
        for tok in row[row >= 0].tolist():
            assert torch.equal(truth[tok], want), (case, tok)


def test_plan_at_the_metric_grid_is_dense_in_tiles():
    """720p: 72 boxes of 992 .. 3968 queries; tiles of 128 rows are > 95 % full."""
    window, stride, dilation = SA.adaptive_parameters(P7, (31, 44, 80))
    q_tok, box = SA.plan_tables((31, 44, 80), window, stride, dilation)
    assert len(np.unique(box, axis=0)) == 72
    assert (q_tok >= 0).mean() > 0.95


def test_model_names_and_config_defaults(tmp_path):
    for name, blocks, dense in (("2B/sparse-7dense", 28, 7), ("14B/sparse-9dense", 36, 9)):
        net, smp = MODELS[name]
        assert net.num_blocks == blocks and net.n_dense_blocks == dense
        assert net.natten_parameters == SA.NattenParams(**P7)
        per = SA.sparse_block_params(net.num_blocks, net.n_dense_blocks, net.natten_parameters)
        assert sum(p is None for p in per) == dense
        assert SetupArguments(output_dir=tmp_path, model=name).model == name
        hash(net)
    assert MODELS["2B/sparse-7dense"][1] == MODELS["2B/post-trained"][1]
    assert MODELS["14B/sparse-9dense"][1] == MODELS["14B/pre-trained"][1]
    assert MODELS["2B/sparse-7dense"][0].replace(n_dense_blocks=-1, natten_parameters=()) == MODELS["2B/post-trained"][0]
    d = DiTConfig()
    assert d.n_dense_blocks == -1 and d.natten_parameters == ()
    assert SA.sparse_block_params(d.num_blocks, d.n_dense_blocks, d.natten_parameters) == [None] * d.num_blocks
    cfg = tiny_dit(num_blocks=3, n_dense_blocks=0, natten_parameters=[dict(window_size=(-1, 4, 6)), None, P7])
    assert cfg.natten_parameters[1] is None and isinstance(cfg.natten_parameters[0], SA.NattenParams)
    hash(cfg)
