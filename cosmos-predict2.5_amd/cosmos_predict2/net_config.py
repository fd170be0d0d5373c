"""Network / sampler hyper-parameters of the Cosmos-Predict2.5 checkpoints this build serves.

Values follow the reference's registered configs:
  * net: COSMOS_V1_2B_NET_MININET / COSMOS_V1_14B_NET_MININET
    (cosmos_predict2/_src/predict2/configs/video2world/defaults/net.py:58-94) with the rectified-flow
    experiment overrides (configs/video2world/experiment/reason_embeddings/
    model_2B_reason_1p1_rectified_flow.py:300-338, model_14b_reason_1p1_rectified_flow.py:322-344);
  * sampler: Stage-c_pt_4-Index-2-Size-2B-Res-720-Fps-16-Note-rf_with_edm_ckpt
    (configs/video2world/experiment/specialized_model/SFT_2B_RF.py:752-768: Karras sigmas,
    conditional_frame_timestep 0.1) for 2B post-trained; shift-5 linspace for the pre-trained models.
"""
from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass, field


@dataclass(frozen=True)
class DiTConfig:
    model_channels: int = 2048
    num_heads: int = 16
    num_blocks: int = 28
    mlp_ratio: float = 4.0
    in_channels: int = 16  # latent channels (MinimalV1LVGDiT adds +1 for the condition mask)
    out_channels: int = 16
    patch_spatial: int = 2
    patch_temporal: int = 1
    concat_padding_mask: bool = True
    crossattn_emb_channels: int = 1024
    use_crossattn_projection: bool = True
    crossattn_proj_in_channels: int = 100352
    adaln_lora_dim: int = 256
    max_img_h: int = 240
    max_img_w: int = 240
    max_frames: int = 128
    rope_h_extrapolation_ratio: float = 3.0
    rope_w_extrapolation_ratio: float = 3.0
    rope_t_extrapolation_ratio: float = 1.0
    rope_enable_fps_modulation: bool = False
    timestep_scale: float = 0.001
    use_wan_fp32_strategy: bool = True
    # action conditioning (cosmos_predict2/_src/predict2/action/networks/action_conditioned_minimal_v1_lvg_dit.py):
    # action_dim > 0 adds action_embedder_B_D / _B_3D (Linear-GELU(tanh)-Linear MLPs) whose outputs are
    # added to the timestep embedding and the AdaLN-LoRA term before t_embedding_norm.
    action_dim: int = 0
    # > 0: ActionChunkConditionedMinimalV1LVGDiT (:182-346): actions grouped per latent frame
    # (temporal_compression_ratio of them), latent frame 0 gets a zero embedding;
    # 0: ActionConditionedMinimalV1LVGDiT (:48-179): one embedding of the whole chunk for every frame
    action_per_latent_frame: int = 0
    num_action_per_chunk: int = 12
    action_hidden: int = 0  # hidden width of the embedder MLPs (0 = 4 * model_channels)
    # multi-view (cosmos_predict2/_src/predict2_multiview/networks/multiview_dit.py:268-325): n_cameras_emb > 0
    # adds view_embeddings (nn.Embedding(n_cameras_emb, view_condition_dim)) concatenated to the input
    # channels of every view (concat_view_embedding); views are stacked along T (state_t latent frames
    # each), self-attention runs over all views jointly, RoPE positions restart per view
    # (MultiCameraVideoRopePosition3DEmb :103-130), cross-attention is per view (512 text tokens each, :40-55)
    n_cameras_emb: int = 0
    view_condition_dim: int = 0
    state_t: int = 0
    # cross-view multi-view net (MultiViewCrossDiT, predict2_multiview/networks/multiview_cross_dit.py:502-869):
    # adaln_view_embedding adds adaln_view_embedder (nn.Embedding(n_cameras_emb, D)) + adaln_view_proj (Linear(D, 9D))
    # whose 9 chunks are added to every block's shift / scale / gate per view (:355-404); a non-empty
    # cross_view_attn_map (neighbour view ids per view id) enables per-view self-attention plus a CrossViewAttention
    # sub-layer after it (:115-228, 436-450): per latent frame, each view's tokens attend to its neighbours' tokens of
    # the same frame, un-gated residual after an affine LayerNorm
    adaln_view_embedding: bool = False
    cross_view_attn_map: tuple = ()
    # sparse self-attention (MiniTrainDIT(n_dense_blocks, natten_parameters), networks/minimal_v4_dit.py:1284-1289,
    # 1349-1350, 1439-1441; replace_selfattn_op_with_sparse_attn_op :1743-1813): -1 = every block dense. Otherwise
    # natten_parameters is one sparse_attn.NattenParams for every sparse block (0: all blocks sparse, 1: the middle block
    # dense, n > 1: np.linspace(0, num_blocks - 1, n, dtype=int) dense) or a tuple of per-block NattenParams / None
    # (None = dense). The reference's dicts and lists are converted to that hashable form on construction.
    n_dense_blocks: int = -1
    natten_parameters: tuple = ()
    # camera conditioning (CameraMiniTrainDIT, camera/networks/minimal_v4_dit_camera_conditioned.py): camera_dim > 0
    # adds every block's cam_encoder = Linear(camera_dim, model_channels, bias=False) (:1079-1080), whose output is
    # added to the self-attention's LN-modulated input (:1189-1194). 1536 = 6 Pluecker channels x the 16 x 16 pixels
    # of one token (8x VAE, 2x patch): the class's cam_dim default.
    camera_dim: int = 0

    def __post_init__(self):
        p = self.natten_parameters
        if p is None or (isinstance(p, (list, tuple)) and len(p) == 0):
            object.__setattr__(self, "natten_parameters", ())
            return
        from .sparse_attn import NattenParams  # (here: sparse_attn binds the native library, this module does not)

        if isinstance(p, (list, tuple)):
            object.__setattr__(self, "natten_parameters", tuple(NattenParams.of(x) for x in p))
        else:
            object.__setattr__(self, "natten_parameters", NattenParams.of(p))

    @property
    def head_dim(self) -> int:
        return self.model_channels // self.num_heads

    @property
    def patch_features(self) -> int:
        # (in_channels + cond mask + padding mask) * p_t * p_s * p_s
        return ((self.in_channels + 1 + int(self.concat_padding_mask) + self.view_condition_dim)
                * self.patch_temporal * self.patch_spatial ** 2)

    @property
    def mlp_hidden(self) -> int:
        return int(self.model_channels * self.mlp_ratio)

    @property
    def action_in_features(self) -> int:
        per = self.action_per_latent_frame or self.num_action_per_chunk
        return self.action_dim * per

    @property
    def action_hidden_features(self) -> int:
        return self.action_hidden or 4 * self.model_channels

    def replace(self, **kw) -> "DiTConfig":
        return dataclasses.replace(self, **kw)


@dataclass(frozen=True)
class SamplerConfig:
    """Text2WorldModelRectifiedFlowConfig / Video2WorldModelRectifiedFlowConfig fields used at inference."""

    state_ch: int = 16
    state_t: int = 24
    shift: float = 5.0
    use_kerras_sigma_at_inference: bool = False
    conditional_frame_timestep: float = -1.0
    denoise_replace_gt_frames: bool = True
    cfg_mode: str = "video2world"  # "video2world": c + g(c-u) ; "text2world": u + g(c-u)
    resolution: str = "720"
    # "unipc": the rectified-flow loop above. "dmd2": the distilled few-step student loop in the TrigFlow
    # parameterisation (distill/models/video2world_model_distill_dmd2.py:421-492 around denoise_edm,
    # models/video2world_model_rectified_flow.py:214-346): one single-branch evaluation per selected time, no CFG, no
    # solver history (model.DistilledSamplingRun). The fields below are read by that loop only
    # (Video2WorldModelDistillationConfigDMD2TrigFlow :60-82 and the BaseDistillConfig fields it inherits).
    sampler: str = "unipc"
    selected_sampling_time: tuple = ()  # TrigFlow times, descending from pi / 2; the loop appends the final 0
    trig_scaling: str = "rectified_flow"  # config.scaling: "rectified_flow" or "edm" (denoiser_scaling.py)
    sigma_data: float = 1.0
    sigma_conditional: float = 1e-4  # noise level of the conditioning frames: t_cond = atan(sigma_conditional / sigma_data)
    change_time_embed: bool = False  # the student's c_noise(t) = t (denoise_edm :268-270)
    # "dmd2_stream": the causal / self-forcing action student, one latent frame at a time over a K/V cache
    # (model.StreamingRun; interactive/models/action_video2world_self_forcing.py:449-577). It reads the TrigFlow fields
    # above and cache_frame_size: the number of past frames a frame attends to (-1: all of the clip's; the reference's
    # generate_streaming_video argument, --cache_frame_size of interactive/inference/action_video2world_streaming.py:74-79)
    cache_frame_size: int = -1


DIT_2B = DiTConfig()
DIT_14B = DiTConfig(model_channels=5120, num_heads=40, num_blocks=36)

SAMPLER_2B_POST_TRAINED = SamplerConfig(use_kerras_sigma_at_inference=True, conditional_frame_timestep=0.1)
SAMPLER_PRE_TRAINED = SamplerConfig()
# robot/action-cond (checkpoint_db.py:469-492, experiment ..._action_conditioned_rectified_flow_bridge_13frame_256x320,
# exp_2B_action_conditioned_rectify_flow.py:617-657): ActionChunk net, action_dim 7, 4 actions per latent
# frame, state_t = 1 + 12 // 4 = 4 (13 frames at 256x320), shift-5 linspace schedule, no conditional-frame
# timestep; the 2B net's rope / timestep / crossattn overrides of the base rectified-flow experiment
# (:308-320) apply on top of the /net group default.
DIT_2B_ACTION = DIT_2B.replace(action_dim=7, action_per_latent_frame=4)
SAMPLER_ACTION = SamplerConfig(state_t=4, resolution="256")
# auto/multiview (checkpoint_db.py:397-415, experiment buttercup_predict2p5_2b_7views_res720p_fps30_t8_..._nofps,
# predict2_multiview/configs/vid2vid/experiment/buttercup/buttercup2p5_rectified_flow.py:30-75, 529-550;
# net COSMOS_V1_2B_MULTIVIEW_NET, defaults/net.py:26-63): 7 camera embeddings of 7 channels, state_t 8 per
# view (29 frames), RoPE h/w 3.0, t 8/24, fps modulation off; CFG uncond + g (cond - uncond)
# (multiview_vid2vid_model_rectified_flow.py:381); the first n latent frames of every view are conditioned.
# Both multi-view nets set use_wan_fp32_strategy=False (defaults/net.py:52, 105): the t-embedding, AdaLN and final
# layer run in the net's bf16 (MinimalV1LVGDiT._time_modulation_bf16, scale_timesteps).
DIT_2B_MULTIVIEW = DIT_2B.replace(n_cameras_emb=7, view_condition_dim=7, state_t=8,
                                  rope_t_extrapolation_ratio=8.0 / 24.0, use_wan_fp32_strategy=False)
SAMPLER_MULTIVIEW = SamplerConfig(state_t=8, cfg_mode="text2world", resolution="720")
# cross-view multi-view net (COSMOS_V1_2B_MULTIVIEW_CROSSVIEW_NET, predict2_multiview/configs/vid2vid/defaults/net.py:
# 76-107: adaln view embedding, no view-embedding input channels, cross-view attention) with the crossview experiment's
# neighbour map (experiment/buttercup/buttercup2p5_rectified_flow.py:387-399) in the view ids of
# predict2_multiview/scripts/inference.py:61-69 (front_wide 0, cross_right 1, rear_right 2, rear_tele 3, rear_left 4,
# cross_left 5, front_tele 6); state_t, RoPE and use_wan_fp32_strategy=False as the multiview net above.
CROSS_VIEW_MAP_7 = ((5, 1, 6), (0, 2), (1, 3), (4, 2), (5, 3), (0, 4), (0,))
DIT_2B_MULTIVIEW_CROSSVIEW = DIT_2B.replace(n_cameras_emb=7, view_condition_dim=0, state_t=8,
                                            rope_t_extrapolation_ratio=8.0 / 24.0, adaln_view_embedding=True,
                                            cross_view_attn_map=CROSS_VIEW_MAP_7, use_wan_fp32_strategy=False)

# DMD2-distilled 4-step student (distill/configs/experiment/experiments_dmd2_trigflow.py:163-193, the base config of
# experiment dmd2_trigflow_distill_cosmos_predict2_2B_bidirectional :266-286, and the config class
# distill/models/video2world_model_distill_dmd2.py:60-82): times (pi / 2, atan 15, atan 5, atan 5/3) = rectified-flow t 1, 0.75, 0.5, 0.25 under shift 5 (:179, :80-81),
# scaling "rectified_flow" (:166), sigma_data 1 (:181), sigma_conditional 1e-4 (:180), state_t 24 (:182), resolution
# "720" (:164); denoise_replace_gt_frames True is Video2WorldConfig's default (models/video2world_model.py:52), which
# the config class inherits, and change_time_embed is left at its False default.
# The student net is distill/configs/defaults/net.py:32-57 (COSMOS_V1_2B_NET: MinimalV1LVGDiT, the 2B layout; hydra net
# "cosmos_v1_2B_student", :82, selected at experiments_dmd2_trigflow.py:60) with the experiment's net=dict(...) (:118-128: RoPE h/w 3.0, t 1.0, no fps modulation, crossattn projection from 100352).
# Neither sets timestep_scale nor use_wan_fp32_strategy, so MinimalV1LVGDiT's and MiniTrainDIT's own defaults hold:
# timestep_scale 1.0 (networks/minimal_v1_lvg_dit.py:25) and use_wan_fp32_strategy False (networks/minimal_v4_dit.py:
# 1352): c_noise in [0, 1] reaches the embedder unscaled and the t-embedding, AdaLN and final layer run in bf16
# (MinimalV1LVGDiT._time_modulation_bf16), unlike the rectified-flow experiments' overrides (0.001, True).
# crossattn_emb_channels 1024 is MiniTrainDIT's default (:1328).
DIT_2B_DISTILLED = DIT_2B.replace(timestep_scale=1.0, use_wan_fp32_strategy=False)
SAMPLER_2B_DISTILLED = SamplerConfig(sampler="dmd2",
                                     selected_sampling_time=(math.pi / 2, math.atan(15), math.atan(5), math.atan(5 / 3)),
                                     trig_scaling="rectified_flow", sigma_data=1.0, sigma_conditional=0.0001,
                                     state_t=24, denoise_replace_gt_frames=True, resolution="720")

# Causal / self-forcing action student, streamed frame by frame over a K/V cache (paths under
# cosmos_predict2/_src/predict2/interactive/). Net: ACTION_CAUSAL_KVCACHE_COSMOS_V1_2B_NET_MININET (configs/net.py:122-130:
# ActionChunkCausalDITwithConditionalMaskKVCache, model_channels 2048, 28 blocks, 16 heads, no per-block absolute
# pos-emb, rope t 1.0) over BASE_NET_KWARGS (:30-50: max_img 240 x 240, 128 frames, 16 in / out channels, patch 2 / 1,
# padding-mask channel, AdaLN-LoRA 256, rope h / w 1.0), with the experiment's net=dict(...) on top
# (configs/experiment/exp_action_self_forcing.py:92-105: action_dim 29, temporal_compression_ratio 4 = actions per
# latent frame, rope h / w 3.0, t 24 / 24, fps modulation off, crossattn projection 100352 -> 1024). Neither sets
# timestep_scale nor use_wan_fp32_strategy, so the class defaults hold: 1.0 (networks/dit_action_causal.py:71) and False
# (networks/dit_causal.py:614); mlp_ratio 4.0 (:589); the embedder MLPs' hidden width 4 * model_channels
# (dit_action_causal.py:83-84). The +1 condition-mask input channel is dit_action_causal.py:549-553.
# Sampler (exp_action_self_forcing.py:147, 160-163): scaling "rectified_flow", the four student times, sigma_conditional
# 1e-4, sigma_data 1.0, state_t = 1 + 12 // 4 = 4; resolution "720" (:145) is the training bucket, the streaming script
# takes H, W from its --resolution argument (inference/action_video2world_streaming.py:198-202).
# Where CausalDIT / CausalBlock differ from MiniTrainDIT / Block is listed in DESIGN.md §6e (state-dict names are the
# same; the image-context cross-attention and the per-block absolute pos-emb are not built by this net).
DIT_2B_ACTION_STREAMING = DIT_2B.replace(action_dim=29, action_per_latent_frame=4, timestep_scale=1.0,
                                         use_wan_fp32_strategy=False, rope_h_extrapolation_ratio=3.0,
                                         rope_w_extrapolation_ratio=3.0, rope_t_extrapolation_ratio=1.0)
SAMPLER_ACTION_STREAMING = SamplerConfig(sampler="dmd2_stream",
                                         selected_sampling_time=(math.pi / 2, math.atan(15), math.atan(5),
                                                                 math.atan(5 / 3)),
                                         trig_scaling="rectified_flow", sigma_data=1.0, sigma_conditional=0.0001,
                                         state_t=4, resolution="720", cache_frame_size=-1)

# Sparse-attention nets: the sparsity the reference's "..._sparse-attn_7dense" (2B) and "..._9dense" (14B) experiments
# put on the net (configs/video2world/experiment/resume_text2world/sparse_2B.py, sparse_14B.py): neighborhood window
# (-1, 12, 24) = every frame, 12 x 24 patches, stride (1, 4, 8), given at the 720p patch grid (-1, 44, 80) and rescaled
# to other grids; 7 of 28 / 9 of 36 blocks stay dense, spread evenly. 8.2 % of the keys per sparse block at 720p.
# (Kept as plain values: DiTConfig converts them to sparse_attn.NattenParams.)
NATTEN_720P_W12X24 = dict(window_size=(-1, 12, 24), stride=(1, 4, 8), base_size=(-1, 44, 80))
DIT_2B_SPARSE_7DENSE = DIT_2B.replace(n_dense_blocks=7, natten_parameters=NATTEN_720P_W12X24)
DIT_14B_SPARSE_9DENSE = DIT_14B.replace(n_dense_blocks=9, natten_parameters=NATTEN_720P_W12X24)

# Camera-conditioned Video2World (paths under cosmos_predict2/_src/predict2/camera/). Net: hydra net
# "cosmos_v1_2B_net_camera_conditioned" (configs/camera_conditioned/net.py:34-63, :105: CameraConditionedMinimalV1LVGDiT,
# model_channels 2048, 16 heads, 28 blocks, no per-block absolute pos-emb, rope t 1.0 over the 7B dict's rope h / w 1.0),
# selected by experiment multicamera_video2video_rectified_flow_2b_res_720_fps16
# (configs/camera_conditioned/experiment/exp_2b.py:150-186), whose base is the rectified-flow experiment of
# 2B/post-trained (:153, Stage-c_pt_4-Index-2-...-rf_with_edm_ckpt). That base's model.config.net dict overrides the /net
# group default (configs/video2world/experiment/reason_embeddings/model_2B_reason_1p1_rectified_flow.py:312-325): RoPE
# h / w 3.0, t 24 / 24 (:314-316), fps modulation off (:313), timestep_scale 0.001 (:317; the class default is 1.0,
# networks/camera_conditioned_minimal_v1_lvg_dit.py:25), use_wan_fp32_strategy True (:324), crossattn projection 100352 ->
# 1024 (:321-323). cam_dim is the block's default 1536 (networks/minimal_v4_dit_camera_conditioned.py:1025).
# Sampler: the base experiment's conditional_frame_timestep 0.1 (specialized_model/SFT_2B_RF.py:766) reaches the inherited
# denoise; its Karras flag does not show, because the camera model's own loop calls set_timesteps(num_steps, shift=shift)
# without it (models/camera_conditioned_video2world_model_rectified_flow.py:301). state_t 24 is one of the three equal
# segments [target 0 | source | target 1] the latent time axis holds (:296), CFG cond + g (cond - uncond) (:230).
DIT_2B_CAMERA = DIT_2B.replace(camera_dim=1536)
SAMPLER_CAMERA = SamplerConfig(use_kerras_sigma_at_inference=False, conditional_frame_timestep=0.1, state_t=24,
                               cfg_mode="video2world", resolution="720")

# model name (cosmos_predict2/config.py ModelKey.name) -> (net, sampler)
MODELS = {
    "2B/post-trained": (DIT_2B, SAMPLER_2B_POST_TRAINED),
    "2B/pre-trained": (DIT_2B, SAMPLER_PRE_TRAINED),
    "14B/pre-trained": (DIT_14B, SAMPLER_PRE_TRAINED),
    "2B/robot/action-cond": (DIT_2B_ACTION, SAMPLER_ACTION),
    "2B/auto/multiview": (DIT_2B_MULTIVIEW, SAMPLER_MULTIVIEW),
    # the reference registers this net (hydra net "cosmos_v1_2B_multiview_crossview") but ships no checkpoint for it
    "2B/auto/multiview-crossview": (DIT_2B_MULTIVIEW_CROSSVIEW, SAMPLER_MULTIVIEW),
    # the reference ships the distillation recipe and the student's inference loop but no checkpoint key for a
    # distilled model (checkpoint_db.py has none): this entry serves a student distilled with that recipe
    "2B/distilled": (DIT_2B_DISTILLED, SAMPLER_2B_DISTILLED),
    # likewise no checkpoint key: the streaming action student trained with interactive/'s self-forcing recipe
    "2B/robot/action-cond/streaming": (DIT_2B_ACTION_STREAMING, SAMPLER_ACTION_STREAMING),
    # the reference ships sparse attention as a net option plus training recipes on its EDM stage; it has no
    # checkpoint key and no rectified-flow experiment for it, so (the footing of "2B/distilled") these entries serve a
    # 2.5 net post-trained with that sparsity, under the rectified-flow samplers of 2B/post-trained / 14B/pre-trained
    "2B/sparse-7dense": (DIT_2B_SPARSE_7DENSE, SAMPLER_2B_POST_TRAINED),
    "14B/sparse-9dense": (DIT_14B_SPARSE_9DENSE, SAMPLER_PRE_TRAINED),
    # the reference registers the camera net and its rectified-flow experiment but ships no checkpoint key for it
    # (the footing of "2B/distilled"): this entry serves a 2B net post-trained for camera control with that recipe
    "2B/camera-cond": (DIT_2B_CAMERA, SAMPLER_CAMERA),
}

# Subset of VIDEO_RES_SIZE_INFO (cosmos_predict2/_src/predict2/datasets/utils.py:44-67); the model's
# default resolution is the "9,16" entry read as (H, W) (text2world_model_rectified_flow.py:872-873).
VIDEO_RES_SIZE_INFO = {
    "720": {"1,1": (960, 960), "4,3": (960, 704), "3,4": (704, 960), "16,9": (1280, 704), "9,16": (704, 1280)},
    "480": {"1,1": (480, 480), "4,3": (640, 480), "3,4": (480, 640), "16,9": (768, 432), "9,16": (432, 768)},
    "256": {"1,1": (256, 256), "4,3": (320, 256), "3,4": (256, 320), "16,9": (320, 192), "9,16": (192, 320)},
}


def tiny_dit(**kw) -> DiTConfig:
    """A small configuration with the 2B layout for tests (head dim 128)."""
    base = DiTConfig(model_channels=512, num_heads=4, num_blocks=2, crossattn_emb_channels=256,
                     crossattn_proj_in_channels=384, adaln_lora_dim=64)
    return base.replace(**kw)
