"""LoRA post-trained checkpoints through the net and the pipeline: the adapters are merged into the bf16 weights once
(cp25_lora_merge) and three ways to the same net give the same bits.

  route 1  load_state_dict of the peft-layout dict (base_layer. keys + lora_A / lora_B): merged ahead of every derived
           copy;
  route 2  load_state_dict of the base dict, then merge_lora: q / k / v merged into row slices of the fused q|k|v
           weights, derived copies rebuilt;
  route 3  load_state_dict of a plain dict whose weights this test merged on the CPU with lora_truth.merge_restated.

The forward outputs of the three are torch.equal, at linear_precision "bf16" and "fp8" (the fp8 weight cache must
quantise merged weights), on the tiny net (D 512, 2 blocks; 2 latent frames on a 4 x 4 patch grid, B = 2) and on the
tiny cross-view net, whose cross_view_attn targets reach w_cv_qkv. Adapters: rank 8, alpha 16 (scale 2), on the
recipe's six targets of every attention the net has."""
import pytest
import torch

import lora_truth as lt
from cosmos_predict2.dit import MinimalV1LVGDiT, init_state_dict
from cosmos_predict2.net_config import tiny_dit

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
RANK, ALPHA = 8, 16.0
SCALE32 = lt.fp32_scale(1.0, ALPHA, RANK)


def _cfg(kind):
    if kind == "single":
        return tiny_dit(num_blocks=2)
    return tiny_dit(num_blocks=2, n_cameras_emb=3, state_t=2, adaln_view_embedding=True,
                    cross_view_attn_map=((1, 2), (0,), (0, 1)))


def _targets(cfg):
    attns = ["self_attn", "cross_attn"] + (["cross_view_attn"] if cfg.cross_view_attn_map else [])
    out = []
    for i in range(cfg.num_blocks):
        for a in attns:
            out += [f"blocks.{i}.{a}.{m}" for m in ("q_proj", "k_proj", "v_proj", "output_proj")]
        out += [f"blocks.{i}.mlp.layer1", f"blocks.{i}.mlp.layer2"]
    return out


def _adapters(base, modules, rank=RANK, seed=50):
    out = {}
    for j, m in enumerate(modules):
        n, k = base[m + ".weight"].shape
        _, a, b = lt.make_case(n, k, rank, seed=seed + j)
        out[m] = (a, b)
    return out


def _peft_layout(base, adapters, name=".default"):
    sd = {}
    for k, v in base.items():
        m = k[: -len(".weight")] if k.endswith(".weight") else None
        sd["net." + (m + ".base_layer.weight" if m in adapters else k)] = v
    for m, (a, b) in adapters.items():
        sd[f"net.{m}.lora_A{name}.weight"] = a
        sd[f"net.{m}.lora_B{name}.weight"] = b
    return sd


def _premerged(base, adapters, scale32=SCALE32):
    sd = dict(base)
    for m, (a, b) in adapters.items():
        sd[m + ".weight"] = lt.merge_restated(base[m + ".weight"], a, b, scale32)
    return sd


_WORLD = {}


def _world(kind):
    """Per net kind, once: config, base dict, adapters, the peft-layout dict and the CPU-merged plain dict."""
    if kind not in _WORLD:
        cfg = _cfg(kind)
        base = init_state_dict(cfg, seed=3, zero_adaln_out=False)
        ad = _adapters(base, _targets(cfg))
        _WORLD[kind] = (cfg, base, ad, _peft_layout(base, ad), _premerged(base, ad))
    return _WORLD[kind]


def _inputs(cfg, device):
    g = torch.Generator().manual_seed(9)
    V = 2 if cfg.n_cameras_emb else 1
    T = 2 * V
    x = torch.randn(2, 16, T, 8, 8, generator=g)
    mask = torch.zeros(2, 1, T, 8, 8)
    mask[:, :, ::2] = 1
    t = torch.tensor([[0.3] * T, [0.7] * T])
    ctx = torch.randn(2, 512 * V, cfg.crossattn_proj_in_channels, generator=g).to(BF16)
    kw = {}
    if cfg.n_cameras_emb:
        kw["view_indices_B_T"] = torch.tensor([[0, 2]]).repeat_interleave(2, dim=1).repeat(2, 1).to(device)
    return (x.to(device).to(BF16), t.to(device), ctx.to(device)), dict(
        condition_video_input_mask_B_C_T_H_W=mask.to(device), **kw)


def _net(cfg, device, sd, precision="bf16", **load_kw):
    net = MinimalV1LVGDiT(cfg, device=device)
    net.set_linear_precision(precision)
    net.load_state_dict(sd, **load_kw)
    return net


def _forward(net, cfg, device):
    args, kw = _inputs(cfg, device)
    out = net(*args, **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    return out


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
@pytest.mark.parametrize("kind", ["single", "crossview"])
def test_routes_identical_to_premerged_net(device, kind, precision):
    cfg, base, ad, peft, merged = _world(kind)
    n1 = _net(cfg, device, peft, precision, lora_alpha=ALPHA)
    n2 = _net(cfg, device, base, precision)
    n2.merge_lora(ad, alpha=ALPHA)
    n3 = _net(cfg, device, merged, precision)
    info = {"modules": len(ad), "rank": RANK, "alpha": ALPHA, "scale": SCALE32}
    assert n1.lora_info == [info] and n2.lora_info == [info] and n3.lora_info == []
    for i in range(cfg.num_blocks):
        assert torch.equal(n1.w_qkv[i], n3.w_qkv[i]) and torch.equal(n2.w_qkv[i], n3.w_qkv[i])
        if cfg.cross_view_attn_map:
            assert torch.equal(n1.w_cv_qkv[i], n3.w_cv_qkv[i]) and torch.equal(n2.w_cv_qkv[i], n3.w_cv_qkv[i])
            assert not torch.equal(n3.w_cv_qkv[i], torch.cat(
                [base[f"blocks.{i}.cross_view_attn.{m}_proj.weight"] for m in "qkv"], 0).to(device))
    assert sorted(n1.sd) == sorted(n3.sd) == sorted(n2.sd)
    for k in n3.sd:
        assert torch.equal(n1.sd[k], n3.sd[k]) and torch.equal(n2.sd[k], n3.sd[k]), k
    o3 = _forward(n3, cfg, device)
    assert torch.equal(_forward(n1, cfg, device), o3)
    assert torch.equal(_forward(n2, cfg, device), o3)
    if precision == "fp8":
        assert n3._fp8_w and sorted(n1._fp8_w) == sorted(n3._fp8_w)
        for k, (w8, ws) in n3._fp8_w.items():
            assert torch.equal(n2._fp8_w[k][0].view(torch.uint8), w8.view(torch.uint8))
            assert torch.equal(n2._fp8_w[k][1], ws)


def test_merge_after_forward_drops_the_fp8_cache(device):
    """merge_lora on a net that has already run in fp8: the cached fp8 weights are of the old weights and must go."""
    cfg, base, ad, _, merged = _world("single")
    n2 = _net(cfg, device, base, "fp8")
    o_base = _forward(n2, cfg, device)
    assert n2._fp8_w
    n2.merge_lora(ad, alpha=ALPHA)
    assert not n2._fp8_w
    o3 = _forward(_net(cfg, device, merged, "fp8"), cfg, device)
    assert torch.equal(_forward(n2, cfg, device), o3) and not torch.equal(o_base, o3)


def test_adapter_has_an_effect_and_scale_zero_has_none(device):
    cfg, base, ad, peft, merged = _world("single")
    o_base = _forward(_net(cfg, device, base), cfg, device)
    o_lora = _forward(_net(cfg, device, peft, lora_alpha=ALPHA), cfg, device)
    assert not torch.equal(o_lora, o_base)
    rel = ((o_lora - o_base).norm() / o_base.norm()).item()
    print(f"adapter effect on the output: rel-L2 {rel:.3e}")
    assert rel > 1e-3
    n0 = _net(cfg, device, peft, lora_alpha=ALPHA, lora_scale=0.0)
    assert n0.lora_info[0]["scale"] == 0.0
    assert torch.equal(_forward(n0, cfg, device), o_base)
    n0 = _net(cfg, device, base)
    n0.merge_lora(ad, alpha=ALPHA, scale=0.0)
    assert torch.equal(_forward(n0, cfg, device), o_base)
    # alpha None is alpha = r (scale 1), which is another net than alpha 16
    n_r = _net(cfg, device, peft)
    assert n_r.lora_info[0]["alpha"] == float(RANK) and n_r.lora_info[0]["scale"] == 1.0
    assert torch.equal(n_r.w_qkv[0][:512].cpu(),
                       lt.merge_restated(base["blocks.0.self_attn.q_proj.weight"], *ad["blocks.0.self_attn.q_proj"], 1.0))


@pytest.mark.parametrize("wan_fp32", [False, True])
def test_non_recipe_target_reaches_the_final_weight(device, wan_fp32):
    cfg = tiny_dit(num_blocks=2, use_wan_fp32_strategy=wan_fp32)
    base = init_state_dict(cfg, seed=3, zero_adaln_out=False)
    ad = _adapters(base, ["final_layer.linear", "t_embedder.1.linear_1", "blocks.1.adaln_modulation_mlp.2"], rank=4)
    s32 = lt.fp32_scale(0.5, 6.0, 4)
    merged = _premerged(base, ad, s32)
    n1 = _net(cfg, device, _peft_layout(base, ad, name=""), lora_alpha=6.0, lora_scale=0.5)
    n2 = _net(cfg, device, base)
    n2.merge_lora(ad, alpha=6.0, scale=0.5)
    n3 = _net(cfg, device, merged)
    want = merged["final_layer.linear.weight"]
    assert not torch.equal(want, base["final_layer.linear.weight"])
    for n in (n1, n2, n3):
        assert torch.equal(n.w_final.cpu(), want.float())
        if not wan_fp32:
            assert torch.equal(n.w_final_bf16[: want.shape[0]].cpu(), want) and not n.w_final_bf16[want.shape[0]:].any()
        assert torch.equal(n.w_t1.cpu(), merged["t_embedder.1.linear_1.weight"].float())
        assert torch.equal(n.w_ada2, n3.w_ada2)
    assert not torch.equal(n3.w_ada2.cpu()[5], base["blocks.1.adaln_modulation_mlp.2.weight"].float())
    o3 = _forward(n3, cfg, device)
    assert torch.equal(_forward(n1, cfg, device), o3) and torch.equal(_forward(n2, cfg, device), o3)
    assert not torch.equal(_forward(_net(cfg, device, base), cfg, device), o3)


def test_errors(device):
    cfg, base, ad, peft, _ = _world("single")
    a, b = ad["blocks.0.self_attn.q_proj"]
    net = _net(cfg, device, base)
    w0 = net.w_qkv[0].clone()
    good = {"blocks.0.self_attn.q_proj": (a, b)}
    for module in ("blocks.7.self_attn.q_proj", "blocks.0.cross_view_attn.q_proj", "blocks.0.self_attn.q_norm",
                   "blocks.0.self_attn.qkv_proj"):
        with pytest.raises(KeyError):
            net.merge_lora({**good, module: (a, b)})
    for bad in ((a.t().contiguous(), b), (a, b[:-1]), (a[:, :-8], b), (a[:4], b), (a[0], b)):
        with pytest.raises(ValueError):
            net.merge_lora({**good, "blocks.0.self_attn.k_proj": bad})
    with pytest.raises(ValueError):  # nothing to merge is the caller's mistake, not a silent no-op
        net.merge_lora({})
    with pytest.raises(ValueError):  # a rank past the kernel's 256
        net.merge_lora({"blocks.0.self_attn.q_proj": (torch.zeros(257, 512), torch.zeros(512, 257))})
    torch.cuda.synchronize()
    assert torch.equal(net.w_qkv[0], w0) and net.lora_info == []  # nothing was merged by the failed calls
    with pytest.raises(RuntimeError):
        MinimalV1LVGDiT(cfg, device=device).merge_lora(good)
    # route 1, strict or not: an adapter that cannot be merged raises instead of being dropped
    extra = dict(peft)
    extra["net.blocks.9.mlp.layer1.lora_A.default.weight"] = a
    extra["net.blocks.9.mlp.layer1.lora_B.default.weight"] = b
    for strict in (True, False):
        with pytest.raises(KeyError):
            _net(cfg, device, extra, strict=strict)
    wrong = dict(peft)
    wrong["net.blocks.0.mlp.layer1.lora_B.default.weight"] = torch.zeros(100, RANK)
    with pytest.raises(ValueError):
        _net(cfg, device, wrong, strict=False)
    with pytest.raises(KeyError):  # peft keys without strict's blessing still need their base weight
        _net(cfg, device, {k: v for k, v in peft.items() if "lora_" in k or "mlp.layer1" not in k}, strict=False)


def test_stacking_two_adapters(device):
    """Two merge_lora calls stack: each is its own rounded merge of the weights the last one left."""
    cfg, base, ad, _, _ = _world("single")
    m = "blocks.1.mlp.layer2"
    a1, b1 = ad[m]
    a2, b2 = ad["blocks.0.mlp.layer2"]
    net = _net(cfg, device, base)
    net.merge_lora({m: (a1, b1)}, alpha=ALPHA)
    net.merge_lora({m: (a2, b2)})
    want = lt.merge_restated(lt.merge_restated(base[m + ".weight"], a1, b1, SCALE32), a2, b2, 1.0)
    assert torch.equal(net.sd[m + ".weight"].cpu(), want)
    assert [i["modules"] for i in net.lora_info] == [1, 1] and [i["scale"] for i in net.lora_info] == [SCALE32, 1.0]


def test_callers_device_tensors_are_not_merged_into(device):
    """A state dict that already lives on the device in bf16 is taken without a copy; the merge must not write into
    the caller's tensors (both routes), and the nets still equal the pre-merged one."""
    cfg, base, ad, _, merged = _world("single")
    dev_base = {k: v.to(device) for k, v in base.items()}
    dev_ad = {m: (a.to(device), b.to(device)) for m, (a, b) in ad.items()}
    n1 = _net(cfg, device, _peft_layout(dev_base, dev_ad), lora_alpha=ALPHA)
    n2 = _net(cfg, device, dev_base)
    n2.merge_lora(dev_ad, alpha=ALPHA)
    torch.cuda.synchronize()
    for k, v in base.items():
        assert torch.equal(dev_base[k].cpu(), v), k
    for k in ("blocks.0.cross_attn.k_proj.weight", "blocks.1.mlp.layer1.weight"):
        assert torch.equal(n1.sd[k].cpu(), merged[k]) and torch.equal(n2.sd[k].cpu(), merged[k])


@pytest.mark.parametrize("fmt", ["safetensors", "pt"])
def test_pipeline_end_to_end(device, tmp_path, fmt):
    from safetensors.torch import save_file

    from cosmos_predict2.pipeline import Video2WorldInference

    cfg, base, ad, peft, merged = _world("single")
    want = _net(cfg, device, merged).w_qkv[0]
    ckpt = str(tmp_path / "base.pt")
    torch.save({"net." + k: v for k, v in base.items()}, ckpt)
    adapter_sd = {}
    for m, (a, b) in ad.items():
        adapter_sd[f"base_model.model.net.{m}.lora_A.weight"] = a
        adapter_sd[f"base_model.model.net.{m}.lora_B.weight"] = b
    lora = str(tmp_path / ("adapter." + fmt))
    if fmt == "safetensors":
        save_file(adapter_sd, lora)
    else:
        torch.save(adapter_sd, lora)
    pipe = Video2WorldInference("2B/post-trained", net_cfg=cfg, ckpt_path=ckpt, lora_path=lora, lora_alpha=ALPHA,
                                device=device)
    assert torch.equal(pipe.model.net.w_qkv[0], want)
    assert pipe.model.net.lora_info == [{"modules": len(ad), "rank": RANK, "alpha": ALPHA, "scale": SCALE32}]
    del pipe
    if fmt == "pt":  # a checkpoint that is itself peft-layout needs no lora_path
        peft_ckpt = str(tmp_path / "peft.pt")
        torch.save(peft, peft_ckpt)
        pipe = Video2WorldInference("2B/post-trained", net_cfg=cfg, ckpt_path=peft_ckpt, lora_alpha=ALPHA,
                                    device=device)
        assert torch.equal(pipe.model.net.w_qkv[0], want)
        assert pipe.model.net.lora_info[0]["modules"] == len(ad)
