"""CPU restatement of the reference's camera-conditioned Video2World pieces -- TEST HELPER, not a test.

Paths relative to cosmos_predict2/_src/ of the reference.

(a) the net: predict2/camera/networks/minimal_v4_dit_camera_conditioned.py Block.forward (:1121-1247) is
    MiniTrainDIT's Block.forward with `cam_emb = self.cam_encoder(camera)` (:1189) added to the self-attention's
    LN-modulated input (:1194); CameraMiniTrainDIT.forward hands the same `camera` to every block (:1650-1658) and
    camera_conditioned_minimal_v1_lvg_dit.py:31-62 adds the mask channel and timestep_scale as MinimalV1LVGDiT does.
    Restated over oracle.dit's public pieces (ln_mod, adaln, te_rmsnorm, apply_rope, sdpa, dit_forward).
(b) the sampler: predict2/camera/models/camera_conditioned_video2world_model_rectified_flow.py:155-327 over
    oracle.sampler.denoise and oracle.unipc.UniPC.
(c) the rays: imaginaire/modules/camera.py:172-236 (get_camera_rays, get_plucker_rays) with get_camera_center
    (:266-278), image2camera (:359-374), camera2world (:318-337), invert_pose (:119-138), to_homogeneous (:282-296),
    as the fp32 op sequence the reference runs, its float64 twin, and THIS BUILD'S packing of the rays into token rows
    (the reference ships no packing).
"""
from __future__ import annotations

import contextlib

import torch
import torch.nn.functional as F

from oracle import dit as odit
from oracle import sampler as osamp
from oracle.unipc import UniPC


# ----------------------------------------------------------------------------- (a) net
def camera_block_forward(cfg, sd, i, x, emb, lora, ctx, freqs, camera):
    """Camera Block.forward (minimal_v4_dit_camera_conditioned.py:1121-1247), x [B, T, H, W, D], camera
    [B, T, H, W, cam_dim]: oracle.dit.block_forward's one-view path with the one added op."""
    p = f"blocks.{i}."
    nh, hd = cfg["num_heads"], cfg["model_channels"] // cfg["num_heads"]
    act = odit.act_dtype()
    _w, _lin = odit._w, odit._lin
    # :1134-1165 AdaLN-LoRA modulation (fp32 autocast), cast to x's dtype, broadcast over (h, w)
    mods = []
    for m in ("self_attn", "cross_attn", "mlp"):
        mods += [t[:, :, None, None, :].to(act) for t in odit.adaln(sd, p + f"adaln_modulation_{m}", emb, lora)]
    sh_sa, sc_sa, g_sa, sh_ca, sc_ca, g_ca, sh_ml, sc_ml, g_ml = mods
    B, T, H, W, D = x.shape
    # :1172-1177 normalized_x = LN(x) * (1 + scale) + shift
    normalized_x = odit.ln_mod(x, sh_sa, sc_sa)
    # :1189 cam_emb = self.cam_encoder(camera): a bias-free Linear in the net's dtype
    cam_emb = _lin(camera.to(act), _w(sd, p + "cam_encoder.weight"))
    # :1191-1203 self-attention on normalized_x + cam_emb (one tensor op on two tensors of the net's dtype)
    h = (normalized_x + cam_emb).reshape(B, T * H * W, D)
    q = _lin(h, _w(sd, p + "self_attn.q_proj.weight")).reshape(B, -1, nh, hd)
    k = _lin(h, _w(sd, p + "self_attn.k_proj.weight")).reshape(B, -1, nh, hd)
    v = _lin(h, _w(sd, p + "self_attn.v_proj.weight")).reshape(B, -1, nh, hd)
    q = odit.apply_rope(odit.te_rmsnorm(q, _w(sd, p + "self_attn.q_norm.weight")).float(), freqs)
    k = odit.apply_rope(odit.te_rmsnorm(k, _w(sd, p + "self_attn.k_norm.weight")).float(), freqs)
    o = odit.sdpa(q.to(act), k.to(act), v.to(act))
    o = _lin(o, _w(sd, p + "self_attn.output_proj.weight")).reshape(B, T, H, W, D)
    x = x + g_sa * o  # :1204
    # :1206-1237 cross-attention (no RoPE, no camera term)
    h = odit.ln_mod(x, sh_ca, sc_ca).reshape(B, T * H * W, D)
    q = odit.te_rmsnorm(_lin(h, _w(sd, p + "cross_attn.q_proj.weight")).reshape(B, -1, nh, hd),
                        _w(sd, p + "cross_attn.q_norm.weight"))
    k = odit.te_rmsnorm(_lin(ctx, _w(sd, p + "cross_attn.k_proj.weight")).reshape(B, -1, nh, hd),
                        _w(sd, p + "cross_attn.k_norm.weight"))
    v = _lin(ctx, _w(sd, p + "cross_attn.v_proj.weight")).reshape(B, -1, nh, hd)
    o = _lin(odit.sdpa(q, k, v), _w(sd, p + "cross_attn.output_proj.weight")).reshape(B, T, H, W, D)
    x = o * g_ca + x
    # :1239-1246 MLP
    h = odit.ln_mod(x, sh_ml, sc_ml)
    y = _lin(F.gelu(_lin(h, _w(sd, p + "mlp.layer1.weight"))), _w(sd, p + "mlp.layer2.weight"))
    return x + g_ml * y


@contextlib.contextmanager
def _camera_blocks(camera):
    """oracle.dit.dit_forward with every block replaced by the camera block: CameraMiniTrainDIT.forward is
    MiniTrainDIT.forward with `camera=camera` handed to each block (:1650-1658), nothing else differs."""
    plain = odit.block_forward

    def block(cfg, sd, i, x, emb, lora, ctx, freqs, n_views=1, view_mod=None, view_ids=None):
        assert n_views == 1 and view_mod is None
        return camera_block_forward(cfg, sd, i, x, emb, lora, ctx, freqs, camera)

    odit.block_forward = block
    try:
        yield
    finally:
        odit.block_forward = plain


def camera_dit_forward(cfg, sd, x_B_C_T_H_W, timesteps_B_T, crossattn_emb, cond_mask_B_1_T_H_W, camera):
    """CameraConditionedMinimalV1LVGDiT.forward (camera_conditioned_minimal_v1_lvg_dit.py:31-62) -> [B, C, T, H, W]
    fp32. camera [B or 1, T, Hp, Wp, cam_dim] on the patch grid."""
    B = x_B_C_T_H_W.shape[0]
    cam = camera.expand(B, *camera.shape[1:])
    with _camera_blocks(cam):
        return odit.dit_forward(cfg, sd, x_B_C_T_H_W, timesteps_B_T, crossattn_emb, cond_mask_B_1_T_H_W)


# ----------------------------------------------------------------------------- (b) sampler
def reorder_source_first(x, dim=1):
    """camera_list = chunk(camera, 3, dim=1); cat(camera_list[1], camera_list[0], camera_list[2]) (:186-187)."""
    c = torch.chunk(x, 3, dim=dim)
    return torch.cat((c[1], c[0], c[2]), dim=dim)


def camera_mask(B, T, H, W, n, dtype=torch.float32):
    """set_camera_conditioned_video_condition (camera/configs/camera_conditioned/conditioner.py:51-65): ones on
    frames [n, 2n) of the whole time axis; T == 1 conditions nothing."""
    m = torch.zeros(B, 1, T, H, W, dtype=dtype)
    if T > 1:
        m[:, :, n: n * 2] += 1
    return m


def camera_generate(cfg_dit, sd, source_latent, ctx_cond, ctx_uncond, *, num_cond=1, guidance=1.5, seed=1,
                    num_steps=35, shift=5.0, cond_frame_t=-1.0, dit_fn=None, return_trajectory=False):
    """generate_samples_from_batch (:236-327) with get_velocity_fn_from_batch (:155-233). dit_fn(cfg, sd, x, t, ctx,
    mask) is the net of one CFG branch (the camera is the same in both: close over it)."""
    x0 = source_latent.float()
    B, C, Ts, H, W = x0.shape
    zeros = torch.zeros_like(x0)
    gt = torch.cat([zeros, x0, zeros], dim=2)                                   # :205
    mask = camera_mask(B, 3 * Ts, H, W, num_cond, dtype=gt.dtype)               # :207-214
    seg = osamp.arch_invariant_rand((B, C, Ts, H, W), seed)                     # :286-294 the same seed twice
    noise = torch.cat([seg, x0, seg.clone()], dim=2)                            # :296
    sched = UniPC(num_steps, shift=shift, use_karras=False)                     # :301
    x = noise                                                                    # :307
    traj = []
    for t in sched.timesteps:                                                    # :309-319
        t_B_T = torch.stack([t]).unsqueeze(0)
        vc = osamp.denoise(cfg_dit, sd, noise, x, t_B_T, ctx_cond, gt, mask, cond_frame_t, dit_fn=dit_fn)
        vu = osamp.denoise(cfg_dit, sd, noise, x, t_B_T, ctx_uncond, gt, mask, cond_frame_t, dit_fn=dit_fn)
        v = vc + guidance * (vc - vu)                                            # :228-230
        x = sched.step(v, t, x)
        traj.append(x.clone())
    chunks = torch.chunk(x, 3, dim=2)                                            # :324-325
    out = (chunks[0], chunks[2])
    return (out, x, traj) if return_trajectory else out


# ----------------------------------------------------------------------------- (c) rays
def intrinsics_matrix(params):
    """(fx, fy, cx, cy) [..., 4] -> K [..., 3, 3] (intrinsic_params_to_matrices, camera.py:378-395)."""
    K = torch.zeros(*params.shape[:-1], 3, 3, dtype=params.dtype)
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = (params[..., 0], params[..., 1],
                                                                           params[..., 2], params[..., 3], 1.0)
    return K


def plucker_rays(cam_pose, cam_intr, image_size, dtype=torch.float32):
    """get_plucker_rays (camera.py:214-236) over get_camera_rays (:172-210), op for op, in `dtype`: float32 is the
    reference's own arithmetic (every helper computes in float32), float64 its twin. cam_pose [F, 3, 4] world-to-camera,
    cam_intr [F, 3, 3] -> [F, H * W, 6] = [moment | direction]."""
    H, W = image_size
    pose, K = cam_pose.to(dtype), cam_intr.to(dtype)
    y_range = torch.arange(H, dtype=dtype).add_(0.5)                                # :190-194
    x_range = torch.arange(W, dtype=dtype).add_(0.5)
    y_grid, x_grid = torch.meshgrid(y_range, x_range, indexing="ij")
    xy = torch.stack([x_grid, y_grid], dim=-1).view(-1, 2).repeat(*pose.shape[:-2], 1, 1)
    hom = torch.cat([xy, torch.ones_like(xy[..., :1])], dim=-1)                     # to_homogeneous :292-295
    grid_camera = hom @ torch.linalg.inv(K).transpose(-1, -2)                       # image2camera :371-373
    R, t = pose[..., :3], pose[..., 3:]
    R_inv = R.transpose(-1, -2)                                                     # invert_pose :130-137
    pose_inv = torch.cat([R_inv, -R_inv @ t], dim=-1)
    pts = torch.cat([grid_camera, torch.ones_like(grid_camera[..., :1])], dim=-1)   # camera2world :330-332
    grid_world = pts @ pose_inv.transpose(-1, -2)
    center = (-R.transpose(-1, -2) @ t).squeeze(-1)                                 # get_camera_center :276-277
    center_hw = center.unsqueeze(-2).expand_as(grid_world)
    rays = grid_world - center_hw                                                   # :200
    rays = rays / rays.norm(dim=-1, keepdim=True).clamp_min(1e-8)                   # :202-206
    moment = torch.linalg.cross(center_hw, rays)                                    # :234
    return torch.cat([moment, rays], dim=-1)                                        # :235


def pack_tokens(plucker_F_HW_6, Hp, Wp):
    """THIS BUILD'S packing (the reference has none): [F, (16 Hp)(16 Wp), 6] -> [F * Hp * Wp, 1536], token order
    (frame, hp, wp), feature order "(c m n)" with c over [moment | direction], m / n the token's 16 x 16 pixels."""
    Fr = plucker_F_HW_6.shape[0]
    x = plucker_F_HW_6.view(Fr, Hp, 16, Wp, 16, 6).permute(0, 1, 3, 5, 2, 4)
    return x.reshape(Fr * Hp * Wp, 6 * 256)


def plucker_token_rows(w2c, intrinsics, Hp, Wp, dtype=torch.float64):
    """w2c [F, 3, 4], intrinsics [F, 4] (fx, fy, cx, cy) -> packed rows [F * Hp * Wp, 1536] in `dtype`."""
    return pack_tokens(plucker_rays(w2c, intrinsics_matrix(intrinsics.double()), (16 * Hp, 16 * Wp), dtype), Hp, Wp)


def bf16_half_ulp(x64):
    """Half the spacing of bf16 (8 significant bits) at |x|: 2^(floor(log2 |x|) - 8); 0 at 0. The largest error of
    rounding to nearest at that magnitude."""
    a = x64.double().abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    return torch.where(a > 0, torch.pow(2.0, e - 8), torch.zeros_like(a))


def rot(axis, deg):
    a = torch.deg2rad(torch.tensor(float(deg), dtype=torch.float64))
    c, s = torch.cos(a).item(), torch.sin(a).item()
    m = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]],
         "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    return torch.tensor(m, dtype=torch.float64)


def pose(R, t):
    return torch.cat([R, torch.tensor(t, dtype=torch.float64).view(3, 1)], dim=1).float()


# The cases of tests/test_camera_ops_gpu.py and of the CPU premise test: F = 2 frames on a 2 x 3 patch grid
# (32 x 48 pixels). name -> (w2c [2, 3, 4] fp32, intrinsics [2, 4] fp32).
PLUCKER_HP, PLUCKER_WP = 2, 3


def plucker_cases():
    Hpx, Wpx = 16 * PLUCKER_HP, 16 * PLUCKER_WP
    eye = torch.eye(3, dtype=torch.float64)

    def intr(f, cx=None, cy=None):
        return [f * Wpx, f * Wpx, Wpx / 2 if cx is None else cx, Hpx / 2 if cy is None else cy]

    cases = {
        "identity": ([pose(eye, [0, 0, 0]), pose(eye, [0, 0, 0])], [intr(0.5), intr(1.0)]),
        "rot_x60_y45": ([pose(rot("x", 60), [4, 0, 0]), pose(rot("y", -45), [1.5, -2.0, 3.0])],
                        [intr(1.0), intr(1.5)]),
        "rot_z30_t0": ([pose(rot("z", 30) @ rot("x", -20), [0, 0, 0]), pose(rot("z", -60), [0.5, 2.5, -3.0])],
                       [intr(0.5), intr(1.0)]),
        "offcentre": ([pose(rot("y", 25) @ rot("x", 10), [-2.0, 1.0, 3.3]), pose(rot("x", -35), [0.1, -0.2, 0.3])],
                      [intr(1.5, cx=0.37 * Wpx, cy=0.61 * Hpx), intr(1.0, cx=0.55 * Wpx, cy=0.42 * Hpx)]),
    }
    return {k: (torch.stack(p), torch.tensor(i, dtype=torch.float32)) for k, (p, i) in cases.items()}
