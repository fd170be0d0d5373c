/*
 * cp25.h -- C ABI of the MI355X-native cosmos-predict2.5 sampler kernels (libcp25.so, gfx950).
 *
 * This is the drop-in boundary below the reference's Python operator plug points. Each entry point
 * names the reference interface it replaces (paths relative to the reference repository root,
 * cosmos_predict2/_src/predict2/...). The Python side (cosmos-predict2.5_amd/cosmos_predict2/_native.py)
 * binds these with ctypes; INTEGRATION.md shows the binding a reference maintainer would add.
 *
 * Contract for every function:
 *   - pointers are device pointers (HBM); strides and sizes are in ELEMENTS, int64;
 *   - bf16 tensors are passed as void* holding IEEE bfloat16 bits, fp32 tensors as float*;
 *   - the call is stream-ordered on `stream`, never allocates, never synchronises, is re-entrant
 *     and hipGraph-capturable; the caller owns all memory (PyTorch's caching allocator);
 *   - returns 0 (CP25_OK) or a negative code checked on the host before launching:
 *       -22 bad shape/stride/pointer, -95 unsupported dtype/head-dim/width, -5 launch failure.
 */
#ifndef CP25_H
#define CP25_H

#include <stdint.h>
#include <hip/hip_runtime_api.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------- tensor descriptors
 * SURVEY.md §8(b)5's descriptor form, for the entry points a reference-side binding most often calls with
 * framework tensors: cp25_attn_fwd_t, cp25_gemm_epi_t, cp25_conv3d_t. A descriptor carries the device pointer, the
 * dtype, the rank and per-dimension sizes and strides (in elements). These entry points check every descriptor on
 * the host and return CP25_ERR_DTYPE (-95) for a wrong dtype, CP25_ERR_INVAL (-22) for a rank / shape / stride /
 * pointer mismatch, before any GPU work; then they run the pointer entry point of the same op. The other entry points
 * keep plain pointers plus sizes (INTEGRATION.md §3 gives the reason). */
#define CP25_MAX_DIMS 6
#define CP25_DT_BF16 1
#define CP25_DT_F32 2
#define CP25_DT_F8E4M3 3
#define CP25_DT_U8 4
typedef struct cp25_tensor {
  void* data;                      /* device pointer */
  int32_t dtype;                   /* CP25_DT_* */
  int32_t ndim;                    /* <= CP25_MAX_DIMS */
  int64_t shape[CP25_MAX_DIMS];
  int64_t strides[CP25_MAX_DIMS];  /* elements */
} cp25_tensor;

/* cp25_attn_fwd over descriptors: q / o [B, Lq, H, D], k / v [B, Lk, H, D], bf16, D = 128, unit head-dim stride. With
 * a workspace of at least cp25_attn_workspace_bytes(B, H, Lq, cp25_attn_plan(B, H, Lq, Lk, D)) bytes the planned
 * key-range split runs (cp25_attn_fwd_split), else the unsplit launch. Replaces: networks/attention.py:90-181. */
int cp25_attn_fwd_t(const cp25_tensor* q, const cp25_tensor* k, const cp25_tensor* v, const cp25_tensor* o,
                    float softmax_scale, void* workspace, size_t ws_bytes, hipStream_t stream);

/* cp25_gemm_epi over descriptors: c [M, N] = epi(a [M, K] w [N, K]^T), bf16, unit inner strides; epilogue
 * CP25_EPI_NONE or CP25_EPI_GELU (the other epilogues take more operands: cp25_gemm_res / _hnorm / _qkv).
 * Replaces: block nn.Linear layers, minimal_v4_dit.py:227-254, 354-363, 401-432. */
int cp25_gemm_epi_t(const cp25_tensor* a, const cp25_tensor* w, const cp25_tensor* c, int epilogue,
                    hipStream_t stream);

/* cp25_conv3d over descriptors: x [T, Hin, Win, Cin] channels-last frames (each contiguous, any frame stride) after
 * pad_front zero frames (the causal padding), weight [Cout, KT, KH, KW, Cin], bias [Cout] or NULL, out contiguous
 * [Tout, Ho, Wo, Cout] whose sizes must match the conv's, all bf16. Replaces: CausalConv3d.forward
 * (tokenizers/wan2pt1.py:44-62). */
int cp25_conv3d_t(const cp25_tensor* x, int pad_front, const cp25_tensor* weight, const cp25_tensor* bias,
                  const cp25_tensor* out, int stride_t, int stride_hw, int pad_top, int pad_left, int pad_bottom,
                  int pad_right, hipStream_t stream);

/* ---------------------------------------------------------------- attention
 * softmax(Q K^T * softmax_scale) V, non-causal, no mask; bf16 in/out, fp32 accumulation.
 * q: [B, Lq, H, D] addressed by q_strides = {batch, token, head} (head dim contiguous), same for
 * k/v ([B, Lk, H, D]) and o ([B, Lq, H, D]). D must be 128. All strides multiples of 8 elements.
 * Replaces: networks/attention.py:90-181 `attention()` as called by MinimalA2AAttnOp
 * (networks/a2a_cp.py:208-219) for self-attention (minimal_v4_dit.py:431) and cross-attention
 * (minimal_v4_dit.py:1216-1226; Lk = 512 text tokens). */
int cp25_attn_fwd(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk, int D,
                  const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                  const int64_t* o_strides, float softmax_scale, hipStream_t stream);

/* Key-range split ("split-KV") form of cp25_attn_fwd, same arguments and result: each (b, h, 256-query
 * block) is processed by n_split workgroups over consecutive key ranges of ceil(ceil(Lk/64)/n_split)
 * 64-key tiles, which write fp32 partial outputs + log-sum-exp into `workspace`
 * (>= cp25_attn_workspace_bytes(B, H, Lq, n_split) bytes, 16-B aligned), merged into o by a second,
 * stream-ordered launch. Used where B*H*ceil(Lq/256) workgroups would leave the last round of CUs
 * mostly idle (a context-parallel shard's queries against the gathered keys, a head chunk of the
 * K/V all-gather pipeline). n_split = 1 is cp25_attn_fwd. Same reference interface as cp25_attn_fwd;
 * the split is the MI355X work decomposition, the result equals the unsplit softmax up to fp32/bf16
 * rounding. */
int cp25_attn_fwd_split(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk, int D,
                        const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                        const int64_t* o_strides, float softmax_scale, int n_split, void* workspace,
                        size_t ws_bytes, hipStream_t stream);

/* cp25_attn_fwd_split with caller-supplied upper bounds of the query and key norms:
 * q_norm_bound >= max |q| and k_norm_bound >= max |k| over all rows (0 = unknown). Softmax is shift invariant, so a
 * row's shift only has to keep its terms inside the fp32 / bf16 range. When both bounds are given and
 * b = q_norm_bound * k_norm_bound * softmax_scale * log2(e) <= 98, every score of a row lies in [-b_row, b_row]
 * (Cauchy-Schwarz, b_row from the row's own |q|) and the row uses the fixed shift max(b_row - 96, 0): no max
 * reduction and no output rescale per key tile, the row's largest term >= 2^-100 and every term <= 2^96. Otherwise (or with a 0 bound) the
 * rows run an online max (tile 0 sets the shift to the row max; later tiles move it up, rescaling O and the sum, only
 * when a row max exceeds it by more than 24): any data. Same result as cp25_attn_fwd_split up to rounding. The DiT
 * passes sqrt(D) * max|q_norm.weight| and sqrt(D) * max|k_norm.weight|: the q/k RMSNorm (minimal_v4_dit.py:355-358)
 * bounds every normed row by them and RoPE preserves the norm. */
int cp25_attn_fwd_bounded(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk,
                          int D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                          const int64_t* o_strides, float softmax_scale, float q_norm_bound, float k_norm_bound,
                          int n_split, void* workspace, size_t ws_bytes, hipStream_t stream);

/* cp25_attn_fwd_bounded over a PRE-SCALED q (rows already multiplied by softmax_scale * log2(e), e.g. by
 * cp25_head_rmsnorm_rope_scaled): P = exp2(q k^T - shift) with the row's shift as the initial accumulator of its
 * Q K^T MFMA chains, so no per-score multiply or subtract. Bounds (of the scaled q and of k; 0 = unknown) pick the
 * shift as in cp25_attn_fwd_bounded: product <= 96 no shift, <= 98 a fixed per-row shift, else the online max.
 * Rounds q * scale to bf16 instead of q (the same single bf16 rounding of the query). Replaces the same reference
 * code as cp25_attn_fwd_bounded; the DiT's default form. */
int cp25_attn_fwd_prescaled(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk, int D,
                            const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                            const int64_t* o_strides, float q_norm_bound, float k_norm_bound, int n_split,
                            void* workspace, size_t ws_bytes, hipStream_t stream);

/* cp25_attn_fwd_prescaled with a data-tight key bound in device memory: the max of k_norm_slots[32 i], i < n_slots
 * (n_slots <= 64; the [64][32] buffer cp25_head_rmsnorm_rope_nmax filled on k) bounds |k| over all keys. Where the host bounds already
 * allow the zero shift (product <= 96) this is cp25_attn_fwd_prescaled. Otherwise the same grid is launched twice
 * (stream-ordered, no host synchronisation): a 256-query block whose own bound max|q_row| max|k| is <= 96 runs the
 * zero-shift loop in the first launch, any other block the online max in the second, so trained q/k norm weights
 * (whose weight-based bounds exceed 96) keep the fast loop wherever the data allows. A row's mode depends on its
 * block, so context-parallel shards must not use this form when they need bit-identical rows. Same reference op as
 * cp25_attn_fwd_bounded. */
int cp25_attn_fwd_prescaled_kslots(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk,
                                   int D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                   const int64_t* o_strides, float q_norm_bound, float k_norm_bound,
                                   const float* k_norm_slots, int n_slots, int n_split, void* workspace,
                                   size_t ws_bytes, hipStream_t stream);

/* cp25_attn_fwd_prescaled (k_norm_slots NULL) / _kslots with the query normalisation done in the kernel: q holds the
 * raw q projection (the QKV GEMM output) and every workgroup applies cp25_head_rmsnorm_rope's arithmetic to its Q
 * fragments as they load: the per-head RMSNorm over 128 (q_norm_weight [128] bf16, eps), the rotate-half RoPE of
 * the row's token (cos_tab / sin_tab [Lq][64] fp32, indexed by the query row; both NULL: none) and the factor
 * q_scale (the softmax scale * log2 e of the prescaled form), with the same partial-sum order and roundings, so the
 * output equals cp25_head_rmsnorm_rope_scaled followed by cp25_attn_fwd_prescaled bit for bit, without that
 * pass over q in HBM (Attention.compute_qkv's q_norm + apply_rotary_pos_emb, minimal_v4_dit.py:401-419, then
 * attention(), networks/attention.py:90-181). Per-block kernel forms only (a short-key launch that would take the
 * persistent form runs one workgroup per query block instead). */
int cp25_attn_fwd_prescaled_qnorm(const void* q, const void* k, const void* v, void* o, int B, int H, int Lq, int Lk,
                                  int D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                  const int64_t* o_strides, float q_norm_bound, float k_norm_bound,
                                  const float* k_norm_slots, int n_slots, const void* q_norm_weight,
                                  const float* cos_tab, const float* sin_tab, float eps, float q_scale, int n_split,
                                  void* workspace, size_t ws_bytes, hipStream_t stream);

/* dst[r, c] = OCP e4m3(bf16 src[r, c] * scale) (saturated to +-448, round to nearest even), row strides in
 * elements; width % 16 == 0. The fixed-scale fp8 copies of q and k for cp25_attn_fwd_prescaled_fp8qk. */
int cp25_cast_fp8_e4m3(const void* src, int64_t src_stride, void* dst, int64_t dst_stride, int64_t n_rows,
                       int64_t width, float scale, hipStream_t stream);

/* The config-5 fp8 option's attention: cp25_attn_fwd_prescaled (zero shift: bound product <= 60) with q and k given
 * as OCP e4m3 (one byte per
 * element; strides in elements = bytes, multiples of 16): q8 = e4m3(q * softmax_scale * log2(e) * 2^s),
 * k8 = e4m3(k * 2^-s) (cp25_cast_fp8_e4m3; the power-of-two scales cancel in q k^T, so no per-score multiply
 * returns). Q K^T runs on v_mfma_f32_32x32x64_f8f6f4; P and V stay bf16, o is bf16. The bounds are those of
 * the scaled bf16 rows, as for cp25_attn_fwd_prescaled. No reference counterpart (the reference has no fp8
 * path); replaces the same attention call. */
int cp25_attn_fwd_prescaled_fp8qk(const void* q8, const void* k8, const void* v, void* o, int B, int H, int Lq, int Lk,
                                  int D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                  const int64_t* o_strides, float q_norm_bound, float k_norm_bound, int n_split,
                                  void* workspace, size_t ws_bytes, hipStream_t stream);

/* V for the fp8 P.V of cp25_attn_fwd_prescaled_fp8: v_amax[b * H + h] = max |v| over the head's L rows (float,
 * device memory, B * H entries), then v8t = e4m3(v * 448 / amax) laid out [B][H][ceil(L / 64)][128 d][64 key
 * bytes], the keys of each 64-key tile permuted to the order the kernel's P^T operand holds them (zero keys pad
 * the last tile). v: bf16 [B, L, H, 128] by element strides (e.g. the v columns of the fused qkv buffer). Two
 * HBM passes over v, no host synchronisation. cp25_v_fp8t_bytes gives the v8t size. */
int64_t cp25_v_fp8t_bytes(int B, int H, int L);
int cp25_cast_v_fp8t(const void* v, const int64_t* v_strides, int B, int H, int L, int D, void* v8t, float* v_amax,
                     hipStream_t stream);

/* The config-5 fp8 option's whole attention: cp25_attn_fwd_prescaled_fp8qk's e4m3 Q K^T, then O^T += V^T P^T on
 * v_mfma_f32_32x32x64_f8f6f4 with P = exp2(S - shift) as e5m2 (shift = max(0, 1.13 q_norm_bound k_norm_bound - 15)
 * keeps every P <= 2^15, inside e5m2, whatever the data) and V^T from cp25_cast_v_fp8t's v8t (O rescaled by
 * amax / 448 at the end). The softmax stays fp32 with no per-score multiply and no running max. Requires
 * 1.13 q_norm_bound k_norm_bound <= 30 (the window [2^-15, 2^15] then holds a term of every row unless the row's
 * scores all sit at the bottom of the bound; such a row is written as zeros, never NaN); CP25_ERR_INVAL otherwise.
 * o bf16. No reference counterpart; replaces the same attention call. */
int cp25_attn_fwd_prescaled_fp8(const void* q8, const void* k8, const void* v8t, const float* v_amax, void* o, int B,
                                int H, int Lq, int Lk, int D, const int64_t* q_strides, const int64_t* k_strides,
                                const int64_t* o_strides, float q_norm_bound, float k_norm_bound, int n_split,
                                void* workspace, size_t ws_bytes, hipStream_t stream);

/* Name of the kernel form cp25_attn_fwd_bounded (prescaled = 0, fp8 = 0), _prescaled (prescaled = 1), _prescaled_kslots
 * (prescaled = 2),
 * _prescaled_fp8qk (fp8 = 1) or _prescaled_fp8 (fp8 = 2) launches for these arguments (a static string), e.g.
 * "attn_fwd_m16<self, prescaled, online max>": what a bench or log reports as the kernel that ran. */
const char* cp25_attn_kernel(int Lk, float softmax_scale, float q_norm_bound, float k_norm_bound, int prescaled,
                             int fp8);

/* Bytes of workspace cp25_attn_fwd_split / _bounded need (0 for n_split <= 1). */
size_t cp25_attn_workspace_bytes(int B, int H, int Lq, int n_split);

/* Bytes of workspace with which an unsplit (n_split = 1) bf16 self-attention launch of _split / _bounded / _prescaled
 * (Lk > 4096, no key-norm slots) runs its last, partial round of workgroups as a tail split: the first
 * (nwg - nwg % CUs) query blocks as one launch of whole rounds, the remaining ones as key-range splits merged into o
 * (the split launches' arithmetic). 0 when the shape has no such tail or it would not pay. Passing less (or no
 * workspace) runs the launch whole, as one grid. */
size_t cp25_attn_tail_workspace_bytes(int B, int H, int Lq, int Lk);

/* The key-range split the library picks for this shape on the current device (>= 1; a round model of
 * one workgroup per CU), or a negative error code. */
int cp25_attn_plan(int B, int H, int Lq, int Lk, int D);

/* Kernel form of the short-key (Lk <= 4096: the text cross-attention, minimal_v4_dit.py:1216-1226) launches of
 * cp25_attn_fwd / _bounded / _prescaled: 1 (default) the persistent form (one workgroup per CU walking a run of
 * query blocks as one K/V tile stream, the next block's Q staged through LDS; unsplit launches in the zero-shift or
 * online modes with Lk > 64), 0 one workgroup per query block. Both forms are bit-identical. Returns the previous
 * form, or CP25_ERR_INVAL for another value. */
int cp25_attn_cross_select(int form);

/* Kernel form of the long-key self-attention launches (Lk > 4096) of cp25_attn_fwd_prescaled / _kslots / _qnorm that
 * are bf16, not a gated pair and whose norm bounds give the fixed-shift mode (every long-key launch with a bound
 * product <= 110): 1 (default) the library's routing, attn_fwd_wq (one wave per SIMD) with 384 query rows per
 * workgroup past 8192 keys and 320 up to there (a third / a fifth less K / V staging traffic per launch than
 * attn_fwd_m16's 256-row blocks); 0 attn_fwd_m16 everywhere; 320 / 384 that width
 * wherever attn_fwd_wq supports the launch (a width this library was not built with is refused). Every form computes
 * each output row with the same operations in the same order, so whole launches are bit-identical; the forms differ
 * in which rows a planned launch's tail round computes as merged key splits (cp25_attn_tail_workspace_bytes covers
 * the selected form). Online-max, gated, fp8 and short-key launches always run attn_fwd_m16 / attn_fwd_f8.
 * cp25_attn_kernel names the kernel a launch takes under the current form. Set only through this call, never from
 * the environment. Returns the previous form, or CP25_ERR_INVAL for another value. */
int cp25_attn_self_select(int form);

/* 3D neighborhood attention: every query of the (T, Hg, Wg) token grid (token = (t Hg + h) Wg + w, L = T Hg Wg)
 * attends the box of window[0] x window[1] x window[2] keys (dilation[i] apart along axis i) that the host plan
 * assigns to its tile; softmax over those keys only, bf16 in / out, fp32 accumulation, P rounded to bf16 before P V.
 * q / k / v / o: [B, L, H, D] addressed by {batch, token, head} element strides as cp25_attn_fwd takes them (the DiT's
 * token-major [n, B, 3D] QKV buffer works in place); D must be 128, strides multiples of 8 elements, pointers 16-B
 * aligned. The plan is two int32 device tables: q_tok [n_tiles][tile_rows] (tile_rows must be 128), the token id of
 * each query row of a tile, -1 for an empty slot, slot 0 of every tile a real token; box [n_tiles][4], the first key
 * index of the tile's box along t, h, w (fourth entry unused). All queries of a tile share the box, so the kernel
 * applies no per-query mask; it clamps key tokens into [0, L) and skips q_tok entries outside it. window and dilation
 * are host arrays of 3 ints with window[i] * dilation[i] <= extent[i] (else CP25_ERR_INVAL, as for D != 128 or bad
 * strides). prescaled != 0: q rows already carry softmax_scale * log2(e) (cp25_head_rmsnorm_rope_scaled) and
 * softmax_scale is unused. Replaces: NeighborhoodAttention.forward (modules/neighborhood_attn.py:172-252, NATTEN's
 * neighborhood_attention_generic; CUDA compute capabilities 80 / 90 / 100 only) as plugged in by NattenA2AAttnOp
 * (networks/a2a_cp.py:222-226) through replace_selfattn_op_with_sparse_attn_op (minimal_v4_dit.py:1743-1813). */
int cp25_attn_na3d(const void* q, const void* k, const void* v, void* o, int B, int H, int T, int Hg, int Wg, int D,
                   const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                   const int64_t* o_strides, const int* q_tok, const int* box, int n_tiles, int tile_rows,
                   const int* window, const int* dilation, float softmax_scale, int prescaled, hipStream_t stream);

/* ---------------------------------------------------------------- DiT block elementwise
 * Activations are token-major [n_tok, B, D] bf16 (batch inner). Row (tok, b) uses modulation row
 * (b, t) with t = (tok0 + tok) / hw (frame index; tok0 = first global token of this CP shard).
 * The kernels of this section move rows in 16-byte pieces: every bf16 pointer (and cp25_final_ln_mod's out) must be
 * 16-B aligned and every bf16 element stride a multiple of 8, or the call returns CP25_ERR_INVAL before any launch.
 *
 * cp25_ln_mod: if y != NULL first x' = x + gate * y (two bf16 roundings, stored to x_out [n_tok,B,D]);
 * then h_out = LayerNorm(x', no affine, eps) * (1 + scale) + shift with the reference's bf16
 * rounding after every torch op. x is read as x[tok * x_st + b * x_sb] (x_sb = 0 broadcasts one
 * row to every batch entry). gate/shift/scale: bf16, element (b, t, d) at b*mod_sb + t*mod_st + d.
 * D in {512, 1024, 2048, 4096, 5120}.
 * Replaces: Block.forward _fn + gated residuals, minimal_v4_dit.py:1171-1179, 1204, 1237, 1246. */
int cp25_ln_mod(const void* x, int64_t x_st, int64_t x_sb, const void* y, const void* gate, const void* shift,
                const void* scale, int64_t mod_sb, int64_t mod_st, void* x_out, void* h_out, int64_t n_tok, int B,
                int D, int64_t tok0, int64_t hw, float eps, hipStream_t stream);

/* cp25_ln_mod with h emitted as the fp8 operand of the next GEMM (config 5's fp8 option): h8_out
 * [n_tok * B, D] OCP E4M3 and h_scale [n_tok * B] fp32, exactly cp25_quant_fp8_rows applied to the bf16 h
 * cp25_ln_mod would write (which is not written). Same replaced reference code as cp25_ln_mod. */
int cp25_ln_mod_fp8(const void* x, int64_t x_st, int64_t x_sb, const void* y, const void* gate, const void* shift,
                    const void* scale, int64_t mod_sb, int64_t mod_st, void* x_out, void* h8_out, float* h_scale,
                    int64_t n_tok, int B, int D, int64_t tok0, int64_t hw, float eps, hipStream_t stream);

/* cp25_ln_mod / cp25_ln_mod_fp8 for the camera-conditioned net: the block's self-attention reads
 * `normalized_x + cam_emb` (camera/networks/minimal_v4_dit_camera_conditioned.py:1189-1194), one more bf16 tensor op
 * on the LN-modulated activation, so h = bf16(h_ln_mod + cam) with one more rounding than cp25_ln_mod; x', x_out, the
 * statistics and every earlier rounding point are cp25_ln_mod's. cam: bf16, the row of local token tok and batch entry
 * b at cam[tok * cam_st + b * cam_sb] (cam_sb = 0 shares one row across the batch; cam_st >= D, so a column view of a
 * wider buffer is legal). cam 16-B aligned, cam_st and cam_sb multiples of 8, else CP25_ERR_INVAL. The fp8 form
 * quantises that h per row (max|h| / 448), as cp25_ln_mod_fp8 does. */
int cp25_ln_mod_cam(const void* x, int64_t x_st, int64_t x_sb, const void* y, const void* gate, const void* shift,
                    const void* scale, int64_t mod_sb, int64_t mod_st, const void* cam, int64_t cam_st, int64_t cam_sb,
                    void* x_out, void* h_out, int64_t n_tok, int B, int D, int64_t tok0, int64_t hw, float eps,
                    hipStream_t stream);
int cp25_ln_mod_cam_fp8(const void* x, int64_t x_st, int64_t x_sb, const void* y, const void* gate, const void* shift,
                        const void* scale, int64_t mod_sb, int64_t mod_st, const void* cam, int64_t cam_st,
                        int64_t cam_sb, void* x_out, void* h8_out, float* h_scale, int64_t n_tok, int B, int D,
                        int64_t tok0, int64_t hw, float eps, hipStream_t stream);

/* Final layer prologue under the reference's fp32 autocast: [x' = x + gate*y (bf16)], then
 * out = LayerNorm_fp32(x') * (1 + scale) + shift in fp32 (shift/scale fp32).
 * Replaces: FinalLayer.forward, minimal_v4_dit.py:974-991 (and the last block's MLP residual :1246). */
int cp25_final_ln_mod(const void* x, const void* y, const void* gate, int64_t gmod_sb, int64_t gmod_st,
                      const float* shift, const float* scale, int64_t mod_sb, int64_t mod_st, float* out,
                      int64_t n_tok, int B, int D, int64_t tok0, int64_t hw, float eps, hipStream_t stream);

/* Affine LayerNorm of n_rows bf16 rows (row stride x_stride / y_stride elements, multiples of 8; 16-B aligned
 * pointers): y = (x - mean) * rstd * weight + bias in fp32 with fp32 statistics, one bf16 rounding (nn.LayerNorm with
 * elementwise_affine on bf16). D in {512, 1024, 2048, 4096, 5120}.
 * Replaces: MultiViewCrossBlock.layer_norm_cross_view_attn, predict2_multiview/networks/multiview_cross_dit.py:290,
 * :441. */
int cp25_layer_norm(const void* x, int64_t x_stride, const void* weight, const void* bias, void* y, int64_t y_stride,
                    int64_t n_rows, int D, float eps, hipStream_t stream);

/* In-place per-head RMSNorm (weight[128] bf16, eps) of heads [head_off, head_off + H*128) of every
 * row of a bf16 [n_rows, row_stride] buffer, then (if cos_tab != NULL) rotate-half RoPE in fp32
 * with cos/sin tables [n_tok, 64] fp32 indexed by token = row / B, result rounded to bf16.
 * If out2 != NULL the result is also written to out2[row * out2_stride + h*128 + d].
 * Replaces: Attention.compute_qkv norm + TE RoPE + attention() recast, minimal_v4_dit.py:410-420,
 * networks/attention.py:107-109. */
int cp25_head_rmsnorm_rope(void* buf, int64_t row_stride, int64_t n_rows, int B, int H, int head_off,
                           const void* weight, const float* cos_tab, const float* sin_tab, void* out2,
                           int64_t out2_stride, float eps, hipStream_t stream);

/* cp25_head_rmsnorm_rope with the result multiplied by out_scale (fp32) before its bf16 rounding: the
 * fp8 option's q = q * softmax_scale * log2(e), so its attention needs no per-score multiply
 * (cp25_attn_fwd_prescaled). out_scale = 1 is cp25_head_rmsnorm_rope exactly. */
int cp25_head_rmsnorm_rope_scaled(void* buf, int64_t row_stride, int64_t n_rows, int B, int H, int head_off,
                                  const void* weight, const float* cos_tab, const float* sin_tab, void* out2,
                                  int64_t out2_stride, float eps, float out_scale, hipStream_t stream);

/* cp25_head_rmsnorm_rope_scaled that also measures the result: the 64 slots norm_max_slots[32 i] (a float [64][32]
 * buffer in device memory, zeroed by the caller; slots one 128-B line apart so the atomics spread over L2 channels)
 * receive, by atomic max, the largest |row| (L2 norm over a head's 128 bf16 values as written) of the call (the max
 * of the 64 is the max over all rows and heads). For k, that is the data-tight key bound
 * cp25_attn_fwd_prescaled_kslots reads; NULL slots: cp25_head_rmsnorm_rope_scaled. */
int cp25_head_rmsnorm_rope_nmax(void* buf, int64_t row_stride, int64_t n_rows, int B, int H, int head_off,
                                const void* weight, const float* cos_tab, const float* sin_tab, void* out2,
                                int64_t out2_stride, float eps, float out_scale, float* norm_max_slots,
                                hipStream_t stream);

/* dst[r, 0:width] = src[r, 0:width] for bf16 rows (K/V export before the CP all-gather); width and both strides
 * multiples of 8, src and dst 16-B aligned. */
int cp25_copy_rows(const void* src, int64_t src_stride, void* dst, int64_t dst_stride, int64_t n_rows, int64_t width,
                   hipStream_t stream);

/* In-place exact (erf) GELU on n bf16 values (n % 8 == 0, x 16-B aligned).
 * Replaces: GPT2FeedForward activation, minimal_v4_dit.py:249-254. */
int cp25_gelu(void* x, int64_t n, hipStream_t stream);

/* fp32 linear layers: C[b][M, N] = act(A[b][M, K] W[b][N, K]^T + R[b][M, N]) in fp32 on v_mfma_f32_16x16x4_f32 (fp32
 * operands, products and sums). Batch entry b's matrices at a + b * a_batch_stride (etc.); A / W / C row-major with
 * leading dims lda / ldw / ldc (floats; lda, ldw and the A / W batch strides multiples of 4, a / w 16-B aligned). R
 * (NULL: none) at r + b * r_batch_stride + row * ldr + col: ldr = 0 is a bias vector, r_batch_stride = 0 one addend
 * for every entry. act 0: none, 1: SiLU (x * sigmoid(x)) after the addend. K % 32 == 0 (-95 otherwise), any M / N,
 * batch <= 65535. Launches with few tiles (the 62-row conditioning GEMMs) split K over several workgroups when a
 * workspace of cp25_gemm_f32_workspace_floats(M, N, K, batch) floats is given (partial sums, then a second pass adds
 * them in slice order, then R and act); with none, or a smaller one, one slice runs. The slice plan depends only on
 * the shape: a given shape always sums in the same order. Without a workspace an output row's sum does not depend on
 * M (the final linear passes none: a context-parallel shard's rows equal the whole sequence's, bit for bit).
 * Replaces the fp32 F.linear calls of the reference's fp32 conditioning (use_wan_fp32_strategy,
 * minimal_v4_dit.py): TimestepEmbedding linear_1 + SiLU and linear_2 (:727-788), the blocks' AdaLN-LoRA
 * modulation Linear(D, A) / Linear(A, 3D) + the LoRA term (:1136-1154; all 3 x num_blocks sub-layers as one GEMM and
 * one batched GEMM), the final layer's AdaLN (:974-991) and its Linear(D, p p C) (:993-995). */
int cp25_gemm_f32(const float* a, int64_t lda, int64_t a_batch_stride, const float* w, int64_t ldw,
                  int64_t w_batch_stride, const float* r, int64_t ldr, int64_t r_batch_stride, float* c, int64_t ldc,
                  int64_t c_batch_stride, int M, int N, int K, int batch, int act, float* workspace,
                  int64_t workspace_floats, hipStream_t stream);
int64_t cp25_gemm_f32_workspace_floats(int M, int N, int K, int batch);

/* ---------------------------------------------------------------- block projections (GEMM + epilogue)
 * C[M, N] = epi(A[M, K] W[N, K]^T): A, W, C bf16 row-major with leading dims lda / ldw / ldc (elements,
 * multiples of 8, pointers 16-B aligned), fp32 accumulation, one bf16 rounding of the product.
 * epilogue CP25_EPI_NONE: C = bf16(A W^T); CP25_EPI_GELU: C = bf16(gelu_erf(bf16(A W^T))), the same
 * arithmetic as cp25_gelu on the stored product. N must be a multiple of 256 and K of 64 (-95 otherwise:
 * the caller keeps its library GEMM for other shapes); any M.
 * Replaces: the block nn.Linear layers (no bias) of networks/minimal_v4_dit.py -- Attention q/k/v/
 * output projections (:354-363, :401-404, :432; the DiT runs q|k|v as one fused [3D, D] weight) and
 * GPT2FeedForward layer1 + exact GELU (:227-254, CP25_EPI_GELU) and layer2. */
#define CP25_EPI_NONE 0
#define CP25_EPI_GELU 1
#define CP25_EPI_RES 2
#define CP25_EPI_HNORM 3
#define CP25_EPI_QKV 4
int cp25_gemm_epi(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
                  int epilogue, hipStream_t stream);

/* cp25_gemm_epi with the per-head q RMSNorm as the epilogue (CP25_EPI_HNORM): every 128-column head of each output row
 * of bf16(A W^T) normalised over its 128 values (norm_weight [128] bf16, eps) and multiplied by out_scale, with the
 * partial sums, butterfly and roundings of cp25_head_rmsnorm_rope (no RoPE): bit-identical to cp25_gemm_epi followed
 * by cp25_head_rmsnorm_rope_scaled on the output, one HBM pass fewer. Replaces the cross-attention's q_proj + q_norm
 * (minimal_v4_dit.py:401-404, :411-419; the text cross-attention has no RoPE). K / 64 must be even (else
 * CP25_ERR_DTYPE: run the two ops). */
int cp25_gemm_hnorm(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
                    const void* norm_weight, float eps, float out_scale, hipStream_t stream);

/* The fused q|k|v projection with the k columns' per-head RMSNorm + 3D RoPE in the epilogue (CP25_EPI_QKV): output
 * columns [k_col0, k_col0 + k_cols) (multiples of 256) get cp25_head_rmsnorm_rope's arithmetic with k_norm_weight
 * [128] bf16, eps and the rotate-half RoPE of token row / B (cos_tab / sin_tab [M / B][64] fp32; both NULL: none),
 * the other columns are bf16(A W^T): bit-identical to cp25_gemm_epi followed by cp25_head_rmsnorm_rope on the k
 * columns, one HBM pass over k fewer (Attention.compute_qkv's k_proj + k_norm + RoPE, minimal_v4_dit.py:401-419).
 * K / 64 must be even (else CP25_ERR_DTYPE: run the two ops). */
int cp25_gemm_qkv(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
                  int k_col0, int k_cols, const void* k_norm_weight, const float* cos_tab, const float* sin_tab, int B,
                  float eps, hipStream_t stream);

/* cp25_gemm_epi with the block's gated residual as the epilogue: C = bf16(x + bf16(gate * bf16(A W^T))), the two
 * bf16 roundings of the reference's `x + gate * y` (cp25_ln_mod's residual, bit for bit). Output row r is token
 * tok = r / B, batch entry b = r % B of a token-major [n_tok, B, N] activation (B divides 16); x element
 * (tok, b, col) at x + tok * x_st + b * x_sb + col (x_sb = 0 broadcasts one row over the batch), gate element
 * (b, frame, col) at gate + b * g_sb + frame * g_st + col with frame = (tok0 + tok) / hw (tok0 = the CP shard's first
 * token; hw >= 16 / B). All strides multiples of 8 elements, 16-B aligned bases. C may not alias x. The next cp25_ln_mod then
 * runs with y = NULL on C.
 * Replaces: the gated residuals of Block.forward (minimal_v4_dit.py:1204, :1237, :1246) fused into the output
 * projection (:432), the cross-attention output projection and GPT2FeedForward layer2 (:227-254). */
int cp25_gemm_res(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
                  const void* x, int64_t x_st, int64_t x_sb, const void* gate, int64_t g_sb, int64_t g_st, int B,
                  int64_t tok0, int64_t hw, hipStream_t stream);

/* ---------------------------------------------------------------- small-M block projections (streaming per-frame forward)
 * The four entry points above for M from 1 to a few thousand rows, where their 256 x 256 tiles leave most CUs idle:
 * 64 x 128 output tiles, one per workgroup (gemm_small.hip). Each takes its counterpart's arguments, with the same
 * meanings and host checks, followed by (split, workspace, workspace_bytes). N % 256 == 0 and K % 64 == 0 (-95
 * otherwise), any parity of K / 64 for every epilogue (CP25_EPI_HNORM and CP25_EPI_QKV included: unlike
 * cp25_gemm_hnorm / _qkv these do not refuse odd K / 64).
 *   split == 1: one pass, no workspace (workspace may be NULL). Every output element is the same MFMA chain as in
 *     cp25_gemm_*: bit-identical to them on any data, for every epilogue.
 *   split == S > 1: K is cut into S contiguous runs of whole 64-deep K-tiles (the first (K / 64) % S runs one tile
 *     longer); each run accumulates in fp32 into workspace [S][M][N], a second kernel adds an element's S sums in
 *     ascending run order in fp32, rounds once to bf16 and applies the epilogue once. Bits depend on S only: not on M,
 *     the CU count or timing (no atomics). S <= K / 64 (-22 otherwise); workspace 16-B aligned with at least
 *     cp25_gemm_sm_workspace_bytes(M, N, K, S) bytes (-22 otherwise, before any launch).
 *   split == 0: the S of cp25_gemm_sm_plan for the current device.
 * A row's result does not depend on M in either form.
 * Replaces: the same nn.Linear layers as cp25_gemm_epi / _res / _hnorm / _qkv, as the causal student's per-frame
 * forward runs them on one latent frame's rows (interactive/networks/dit_causal.py: CausalAttention's q/k/v/output
 * projections, the cross-attention's q and output projections, GPT2FeedForward layer1 / layer2, and the PatchEmbed
 * linear at K = 128). */
int cp25_gemm_sm_epi(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
                     int epilogue, int split, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cp25_gemm_sm_res(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
                     const void* x, int64_t x_st, int64_t x_sb, const void* gate, int64_t g_sb, int64_t g_st, int B,
                     int64_t tok0, int64_t hw, int split, void* workspace, int64_t workspace_bytes, hipStream_t stream);
int cp25_gemm_sm_hnorm(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
                       const void* norm_weight, float eps, float out_scale, int split, void* workspace,
                       int64_t workspace_bytes, hipStream_t stream);
int cp25_gemm_sm_qkv(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
                     int k_col0, int k_cols, const void* k_norm_weight, const float* cos_tab, const float* sin_tab, int B,
                     float eps, int split, void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* The plan of a small-M launch (gemm_route.h, a pure function of its arguments): bit 0 set when the small family runs
 * this shape (clear: cp25_gemm_*'s 256 x 256 tiles measured faster, or the shape is outside the family's range),
 * bits 8-15 the K split S (>= 1), bits 16-23 and 24-30 the output tile's rows / 16 and columns / 16; or a negative error
 * code. cus: the CU count to plan for; 0: the current device's, or 256 without a device. */
int cp25_gemm_sm_plan(int M, int N, int K, int epilogue, int cus);

/* Bytes of workspace a small-M launch with this split needs: split * M * N * 4 for split > 1, else 0. */
int64_t cp25_gemm_sm_workspace_bytes(int M, int N, int K, int split);

/* The config-5 fp8 option's block projections on the same hand-written GEMM (no reference counterpart: the reference
 * has no fp8 path): C[M, N] = bf16((A[M, K] W[N, K]^T) * a_scale[m] * w_scale[n]) with A and W OCP e4m3 bytes
 * (row-scaled activations from cp25_ln_mod_fp8 / cp25_quant_fp8_rows / cp25_gelu_quant_fp8; per-output-channel weight
 * scales), fp32 accumulation on v_mfma_scale_f32_16x16x128_f8f6f4 -- torch._scaled_mm's definition with row / column
 * scales. N % 256 == 0, K % 256 == 0 (-95 otherwise), lda / ldw multiples of 16 bytes, any M. cp25_gemm_fp8_res adds
 * cp25_gemm_res's gated-residual epilogue (same x / gate arguments).
 * Replaces: the block nn.Linear layers of minimal_v4_dit.py (:400-432, :227-254) in the fp8 option. */
int cp25_gemm_fp8(const void* a, int64_t lda, const float* a_scale, const void* w, int64_t ldw, const float* w_scale,
                  void* c, int64_t ldc, int M, int N, int K, hipStream_t stream);
int cp25_gemm_fp8_res(const void* a, int64_t lda, const float* a_scale, const void* w, int64_t ldw,
                      const float* w_scale, void* c, int64_t ldc, int M, int N, int K, const void* x, int64_t x_st,
                      int64_t x_sb, const void* gate, int64_t g_sb, int64_t g_st, int B, int64_t tok0, int64_t hw,
                      hipStream_t stream);

/* Latents live in "patch layout" [n_tok, 64] fp32, element (tok, p*16 + c), p = p1*2 + p2 (the
 * final layer's "(p1 p2 t C)" order). cp25_patchify builds the x_embedder input rows [n_tok, 72]
 * bf16 (feature c*4 + p): channels 0..15 = gt*mask + x*(1-mask) (gt may be NULL), channel 16 = the
 * per-frame condition mask, channel 17 = padding mask (pad_mask [n_tok, 4] bf16 or NULL = 0).
 * Replaces: video2world_model_rectified_flow.py:105-107, minimal_v1_lvg_dit.py:46,
 * minimal_v4_dit.py:1547-1554 and PatchEmbed's rearrange (:873-878). */
int cp25_patchify(const float* xs, const float* gt, const float* frame_mask, const void* pad_mask, void* out,
                  int64_t n_tok, int64_t tok0, int64_t hw, hipStream_t stream);

/* cp25_patchify into rows of out_ld elements (out_ld >= 72, a multiple of 8), columns 72 .. out_ld - 1 zeroed: with
 * out_ld = 128 the rows are the K = 128 operand of the own GEMM (cp25_gemm_epi) against the x_embedder weight
 * zero-padded to 128 columns, the same sums as K = 72. */
int cp25_patchify_ld(const float* xs, const float* gt, const float* frame_mask, const void* pad_mask, void* out,
                     int64_t out_ld, int64_t n_tok, int64_t tok0, int64_t hw, hipStream_t stream);

/* v_out[tok, j] from the final-layer output net [n_tok, B, 64] fp32 (B = 1 or 2 = cond, uncond):
 * per branch v_b = (noise - gt) * mask + net_b * (1 - mask) (skipped if gt == NULL), then
 * cfg_mode 0: v = v_c + guidance (v_c - v_u)   (Video2World, video2world_model_rectified_flow.py:209)
 * cfg_mode 1: v = v_u + guidance (v_c - v_u)   (Text2World, text2world_model_rectified_flow.py:511)
 * Replaces: Video2WorldModelRectifiedFlow.denoise :131-136, velocity_fn :206-210, MiniTrainDIT.unpatchify. */
int cp25_cfg_velocity(const float* net, int B, const float* noise, const float* gt, const float* frame_mask,
                      float guidance, int cfg_mode, float* v_out, int64_t n_tok, int64_t tok0, int64_t hw,
                      hipStream_t stream);

/* ---------------------------------------------------------------- distilled (DMD2 / TrigFlow) student steps
 * The few-step student loop (distill/models/video2world_model_distill_dmd2.py:421-492) around its denoiser
 * (models/video2world_model_rectified_flow.py:214-346, net_type "student"). Both kernels work on the patch layout
 * above, index their per-frame tables (frame_mask fp32, c_* float64, one entry per latent frame) by (tok0 + tok) / hw
 * as cp25_patchify does, and compute in fp64 as the reference's float64 state and coefficients make PyTorch do, one
 * IEEE operation per torch op (no contraction). The masks are used arithmetically, a * mask + b * (1 - mask), as
 * written there. xs / gt / net / noise / out 16-B aligned (four fp32 move at once), the float64 tables 8-B aligned,
 * sigma_data > 0; -22 otherwise.
 *
 * cp25_trig_patchify_ld: cp25_patchify_ld's rows (feature order, mask channel 16, pad channel 17, columns 72 ..
 * out_ld - 1 zeroed; out_ld >= 72, a multiple of 8) with channels 0..15 = (gt / sigma_data) * mask + (x * c_in[frame])
 * * (1 - mask) in fp64 (x * c_in[frame] when gt == NULL: no conditioning), rounded float64 -> float32 -> bf16, the two
 * roundings of `tensor.to(torch.bfloat16)` on a float64 tensor.
 * Replaces: video2world_model_rectified_flow.py:262-266 (scaling, net_state_in = xt * c_in), :274-301 (conditioning
 * frames / sigma_data, frame replacement), :304 (the cast) plus cp25_patchify_ld's sources. */
int cp25_trig_patchify_ld(const float* xs, const float* gt, const float* frame_mask, const double* c_in,
                          double sigma_data, const void* pad_mask, void* out, int64_t out_ld, int64_t n_tok,
                          int64_t tok0, int64_t hw, hipStream_t stream);

/* In place on the fp32 state xs [n_tok, 64], from the student net's output net [n_tok, 1, 64] fp32 (the layout
 * cp25_cfg_velocity reads at B = 1):
 *   x0 = c_skip[frame] * double(xs) + c_out[frame] * double(net)                              (:325-328)
 *   replace_gt != 0 and gt != NULL: x0 = double(gt) * mask + x0 * (1 - mask)                  (:331-336)
 *   last == 0: xs = float((cos_next * x0) / sigma_data + double(float(sin_next) * noise))     (dmd2 :486-488)
 *   last != 0: xs = nan_to_num(float(x0)): NaN -> 0, +-inf -> +-FLT_MAX                       (dmd2 :489-492)
 * The division is an fp64 division (sigma_data need not be a power of two). `math.sin(t_next) * init_noise` is a
 * python scalar times a float32 tensor, which PyTorch evaluates in fp32 before the float64 sum widens it: hence
 * float(sin_next) * noise. noise may be NULL when last != 0; gt, frame_mask may be NULL when nothing is replaced.
 * Replaces: video2world_model_rectified_flow.py:322-336 and video2world_model_distill_dmd2.py:485-492. */
int cp25_trig_x0_step(float* xs, const float* net, const float* noise, const float* gt, const float* frame_mask,
                      const double* c_skip, const double* c_out, int replace_gt, double sigma_data, double cos_next,
                      double sin_next, int last, int64_t n_tok, int64_t tok0, int64_t hw, hipStream_t stream);

/* ---------------------------------------------------------------- streaming causal action student (stream_ops.hip)
 * The KV-cached per-frame student (interactive/models/action_video2world_self_forcing.py:170-227, 383-577 around
 * interactive/networks/dit_causal.py:1062-1159). Its arithmetic is bf16, op by op: every torch op there is one
 * operation on bf16 tensors, evaluated in fp32 and rounded once to bf16 (NaN -> 0x7FC0, as c10::BFloat16 rounds). The
 * state, the noise and the outputs are bf16 in the patch layout above, one latent frame, one batch entry. The scalar
 * coefficients are bf16 tensors in the reference and are passed as floats that hold bf16 values exactly; -22 for a
 * float that does not, for a misaligned (16 B) pointer or a bad size.
 *
 * cp25_kv_put: rows r = tok * B + b of the fused QKV buffer qkv [n_tok * B, ld] bf16: columns [k_col0, k_col0 + D) ->
 * k_cache[b, row0 + tok, :], [v_col0, v_col0 + D) -> v_cache[b, row0 + tok, :], caches [B, cache_rows, D] with batch /
 * row strides cache_sb / cache_sr (elements), as 16-byte moves, one launch for both. D, ld, the column offsets and the
 * strides are multiples of 8; row0 + n_tok <= cache_rows. Replaces AttenOpWithKV's `k_cache[:, s:e] = k` pair. */
int cp25_kv_put(const void* qkv, int64_t ld, int64_t k_col0, int64_t v_col0, int64_t D, void* k_cache, void* v_cache,
                int64_t cache_sb, int64_t cache_sr, int64_t cache_rows, int B, int64_t n_tok, int64_t row0,
                hipStream_t stream);

/* cp25_patchify_ld's rows of one frame from the bf16 state xs [n_tok, 64]: channels 0..15 = bf16(x * c_in), channel 16
 * = mask, channel 17 = pad_mask ([n_tok, 4] bf16, NULL = 0), columns 72 .. 127 zeroed when out_ld = 128. out_ld is 72
 * or 128 (-95 otherwise). Replaces denoise_edm_seq :206, :211 and forward_seq's mask concatenation. */
int cp25_stream_patchify_ld(const void* xs, float c_in, float mask, const void* pad_mask, void* out, int64_t out_ld,
                            int64_t n_tok, hipStream_t stream);

/* From the bf16 state xs [n_tok, 64] and the net output net [n_tok, 1, 64] fp32 (rounded to bf16 first, the
 * reference's `.to(dtype=x.dtype)`), into out [n_tok, 64] bf16 (may be xs):
 *   x0 = bf16(bf16(c_skip * x) + bf16(c_out * net))                                                  (:226)
 *   last != 0: out = x0
 *   last == 0: out = bf16(bf16(bf16(cos_next * x0) * (1.0f / float(sigma_data))) + bf16(sin_next * noise))  (:442-444)
 * cos_next / sin_next: cos / sin of the 0-dim bf16 tensor t_next, already rounded to bf16. `/ self.sigma_data` divides
 * a device tensor by a Python float, which PyTorch evaluates as a multiplication by the fp32 reciprocal. noise
 * [n_tok, 64] bf16, may be NULL when last != 0. */
int cp25_stream_x0_step(const void* xs, const float* net, const void* noise, void* out, float c_skip, float c_out,
                        float cos_next, float sin_next, double sigma_data, int last, int64_t n_tok,
                        hipStream_t stream);

/* One generated latent frame of the batched streaming state, xs [Hp * Wp * B, 64] bf16 (row = tok * B + b,
 * tok = i * Wp + j, feature (p1 * 2 + p2) * 16 + c), into the VAE decoder's input of that frame, dst [B][2 Hp][2 Wp][16]
 * bf16 channels-last, un-normalised:
 *   dst[b][2 i + p1][2 j + p2][c] = bf16(float(bf16(float(x) / float(inv_std[c]))) + float(mean[c]))
 * inv_std, mean: [16] bf16 device tensors (16-byte aligned, as xs and dst). The division is the IEEE-rounded fp32
 * division of cp25_u8_to_clip; each (tok, b, p) is 32 contiguous bytes in and out, moved as 16-byte vectors. -22 for a
 * misaligned pointer or a non-positive B, Hp or Wp.
 * Replaces, per frame: the B from_patch_layout copies and their stack, then the decode's permute + .contiguous() and
 * `zl / inv_std + mean` (the un-normalisation of WanVAE.decode, tokenizers/wan2pt1.py:555-558, on the frame
 * generate_next_frame returns, interactive/models/action_video2world_self_forcing.py:383-447). */
int cp25_stream_latent_clip(const void* xs, const void* inv_std, const void* mean, void* dst, int B, int Hp, int Wp,
                            hipStream_t stream);

/* ---------------------------------------------------------------- UniPC sampler update
 * Host-computed fp32 coefficients of one FlowUniPCMultistepScheduler.step. */
typedef struct cp25_unipc_params {
  float sigma;      /* sigmas[step_index] */
  int use_corr;     /* corrector active */
  int order_c;      /* 1 or 2 */
  float c_a, c_b, c_c, c_inv_rk, c_rho0, c_rho_last;
  int order_p;      /* 1 or 2 */
  float p_a, p_b, p_c, p_inv_rk, p_rho0;
} cp25_unipc_params;

/* One fused, bit-exact UniPC step over n fp32 elements, in place on x (sample), m0/m1 (the two
 * converted model outputs of the history) and last (last_sample); v = the velocity prediction.
 * Replaces: FlowUniPCMultistepScheduler.step elementwise math, models/fm_solvers_unipc.py:266-335,
 * 337-464, 466-601, 630-713. */
int cp25_unipc_step(float* x, const float* v, float* m0, float* m1, float* last, int64_t n,
                    const cp25_unipc_params* params, hipStream_t stream);

/* ---------------------------------------------------------------- Wan2.1 VAE
 * Activations are channels-last frames [H][W][C] bf16.
 *
 * cp25_conv3d: implicit-GEMM convolution out[to] = sum_{kt,kh,kw,ci} W[co][kt][kh][kw][ci] *
 * in(frame to*stride_t + kt)[hi][wi][ci] + bias[co] (fp32 accumulation, bf16 output), then
 * (if residual != NULL) out = out + residual (bf16 add). `frames` is a table of n_frames (<= 24)
 * frame pointers [Hin][Win][Cin]; a NULL entry is a zero frame (causal padding). Spatial: pad_top /
 * pad_left / pad_bottom / pad_right zeros, stride_hw; upsample=1 first nearest-upsamples the input 2x.
 * out: [Tout][Ho][Wo][Cout]; with out_split = c > 0 (Cout == 2c) output channel co >= c goes to frame
 * 2*to + 1, channel co - c (the upsample3d time_conv interleave), out being [2*Tout][Ho][Wo][c].
 * Cin % 16 == 0 (pad channels on the host). Weight layout [Cout][KT][KH][KW][Cin] bf16.
 * Replaces: CausalConv3d.forward (tokenizers/wan2pt1.py:44-62), Resample convs (:96-110, :133-145,
 * :159), ResidualBlock shortcut + residual add (:204, :222), AttentionBlock to_qkv / proj (:236-261),
 * WanVAE_ conv1 / conv2 (:494-495). */
int cp25_conv3d(const void* const* frames, int n_frames, const void* weight, const void* bias, const void* residual,
                void* out, int Hin, int Win, int Cin, int Cout, int Tout, int KT, int KH, int KW, int stride_t,
                int stride_hw, int pad_top, int pad_left, int pad_bottom, int pad_right, int upsample, int out_split,
                hipStream_t stream);

/* cp25_conv3d over n_clips independent clips of Tc = Tout / n_clips output frames each, in one launch (the VAE on a
 * batch of clips in lock-step). The table holds n_clips runs of Fc = (Tc - 1) * stride_t + KT entries, clip c's run at
 * entries c * Fc .. c * Fc + Fc - 1 (its causal history, then its frames; NULL = a zero frame). Output frame `to`
 * belongs to clip to / Tc and reads entries (to / Tc) * Fc + (to % Tc) * stride_t + kt, so no window straddles two
 * clips; out is [Tout][Ho][Wo][Cout] with clip c's frames at c * Tc .. (with out_split, [2 * Tout] and 2 c Tc ..), and
 * residual likewise. Everything else is cp25_conv3d, which is the n_clips = 1 case of the same kernels (one clip may
 * bring more than Fc frames; the surplus is not read). Returns -22 before any launch, writing nothing, if
 * n_clips < 1, Tout % n_clips != 0, or (n_clips > 1) n_clips * Fc > 24 or n_clips * Fc != n_frames. */
int cp25_conv3d_clips(const void* const* frames, int n_frames, int n_clips, const void* weight, const void* bias,
                      const void* residual, void* out, int Hin, int Win, int Cin, int Cout, int Tout, int KT, int KH,
                      int KW, int stride_t, int stride_hw, int pad_top, int pad_left, int pad_bottom, int pad_right,
                      int upsample, int out_split, hipStream_t stream);

/* Kernel choice of cp25_conv3d for the 3x3 stride-1 convs: 0 (default) the LDS-halo kernel where it applies, 1 the
 * per-tap implicit GEMM everywhere (A/B runs and tests; same arithmetic up to summation order), 2 the round-2 halo
 * kernel with 4 waves per workgroup (one per SIMD; bit-identical to 0, which runs 8). Returns the previous mode. The
 * initial mode is read once at library load from CP25_CONV_KERNEL ("tap" = 1). */
int cp25_conv3d_select(int mode);

/* y = F.normalize(x, dim=C) * sqrt(C) * gamma [then SiLU] per pixel of n_pix channels-last pixels,
 * with the reference's bf16 rounding after each torch op. C % 32 == 0, C/32 in {1,2,3,6,12}.
 * Replaces: RMS_norm.forward (+ nn.SiLU) in ResidualBlock / head / AttentionBlock (wan2pt1.py:65-77,
 * :195-203, :235, :313-315, :413). */
int cp25_rms_norm_silu(const void* x, const void* gamma, void* y, int64_t n_pix, int C, int do_silu,
                       hipStream_t stream);

/* o = softmax(q k^T * scale) v per frame, one head of D = 384 (the Wan VAE AttentionBlock), bf16 in / out, fp32
 * scores and sums, bf16 P. q [T][Lq][D], k / v [T][Lk][D], o [T][Lq][D] given as base pointers with row strides
 * (ld*) and frame strides (f*) in elements (multiples of 8, 16-B aligned bases), so q / k / v can be column
 * slices of the to_qkv output [T][L][3D]. Flash kernel (no score matrix in HBM): one pass over the keys with the
 * softmax shift fixed at the first key tile's row max; a query block whose later scores exceed it by more than 2^24
 * is redone by a second launch with the exact row max of all keys. Replaces F.scaled_dot_product_attention in
 * AttentionBlock.forward (tokenizers/wan2pt1.py:225-261, q, k, v = [b*t, 1, h*w, c]). Returns CP25_ERR_DTYPE for
 * D != 384. `workspace` (cp25_vae_attn_workspace_bytes(T, Lq, Lk, D) bytes, 16-B aligned, required) holds the
 * per-block redo flags and, when the query blocks do not cover the GPU and the keys are split over several
 * workgroups, their partials, merged by a further kernel on the same stream. */
int64_t cp25_vae_attn_workspace_bytes(int T, int Lq, int Lk, int D);
int cp25_vae_attn(const void* q, int64_t ldq, int64_t fq, const void* k, int64_t ldk, int64_t fk, const void* v,
                  int64_t ldv, int64_t fv, void* o, int64_t ldo, int64_t fo, int T, int Lq, int Lk, int D, float scale,
                  void* workspace, int64_t workspace_bytes, hipStream_t stream);

/* p[r, :] = softmax(s[r, :] * scale) for `rows` rows of `cols` fp32 scores (row stride ld_s elements)
 * -> bf16 probabilities (row stride ld_p); vector loads/stores when rows are 16-B / 8-B aligned. The
 * round-1 VAE AttentionBlock ran S = Q K^T (library GEMM, fp32 out), this kernel, and P V (library GEMM);
 * since round 2 it runs cp25_vae_attn and this entry point is kept for the A/B and its tests. */
int cp25_softmax_rows(const float* s, int64_t rows, int cols, int64_t ld_s, float scale, void* p, int64_t ld_p,
                      hipStream_t stream);

/* fp8 activation operand of the DiT's fp8 linear layers (config 5's "fp8 MFMA"; the GEMM is cp25_gemm_fp8 /
 * cp25_gemm_fp8_res, hand-written; torch._scaled_mm is only the tests' reference). Per row m of x [n_rows, k] bf16 (contiguous, k in {512, 1024, 1536,
 * 2048, 3072, 4096, 5120, 6144, 8192, 20480}): scale[m] = max|x[m, :]| / 448 and q[m, :] = fp8_e4m3(x[m, :] * (448 / max(max|x[m, :]|, 2^-100)))
 * (OCP E4M3, round to nearest even, saturated), so x ~= q * scale; an all-zero row gives q = 0, scale 0, and a row below
 * the 2^-100 floor (where 448 / max would overflow) gives q = 0 with its tiny scale.
 * cp25_gelu_quant_fp8 quantises GELU(x) rounded to bf16 (Abramowitz-Stegun 7.1.26 erfc: within ~1 bf16 ulp
 * of cp25_gelu's exact-erf value, far below the fp8 rounding).
 * Replaces: the bf16 operand of nn.Linear in Attention (minimal_v4_dit.py:400-432) and GPT2FeedForward
 * (:227-254, whose GELU it fuses); the reference itself has no fp8 inference path. */
int cp25_quant_fp8_rows(const void* x, void* q, float* scale, int64_t n_rows, int64_t k, hipStream_t stream);
int cp25_gelu_quant_fp8(const void* x, void* q, float* scale, int64_t n_rows, int64_t k, hipStream_t stream);

/* ---------------------------------------------------------------- pixels (uint8 frames <-> the VAE's clips)
 * Strides are in elements of the tensor's own type and may describe planar or channels-last memory.
 *
 * cp25_resize_crop_u8: antialiased bilinear resize fused with the centre crop, on N uint8 frames of C <= 4 channels.
 * src is indexed by src_strides = (n, c, y, x) over [N][C][Hin][Win]; dst points at the first pixel of the th x tw
 * crop window and is indexed by dst_strides = (n, c, y, x). The separable triangle filter comes as per-axis device
 * tables over the full resized extent (rh, rw): start[out] (first source index), count[out] (taps used, <= taps) and
 * w[out][taps] fp32 (rows sum to 1), with start non-decreasing; the window is rows [top, top + th) x columns
 * [left, left + tw) of that extent and only the window is computed. Per output pixel: an fp32 sum over the taps in
 * ascending x for each source row (kept fp32), an fp32 sum of those over the rows in ascending y, rint (half to
 * even), clamp to [0, 255]; the order is fixed, so a pixel's value depends on neither the tile, the window nor the
 * layout. One launch: a workgroup stages the source bytes of its 8 x 32 output tile in LDS (dword loads where a
 * row's bytes are contiguous and aligned), writes the horizontal pass to an fp32 LDS tile and runs the vertical pass
 * from it; no intermediate in HBM. Reads stay inside [0, Hin) x [0, Win) of a frame, writes inside the window.
 * Supported: Hin <= 4 rh and Win <= 4 rw (downscale by at most 4; any upscale), taps in [1, 9]; else CP25_ERR_INVAL
 * before any launch. Replaces: resize_input (inference/video2world.py:75-97: torchvision resize + center_crop). */
int cp25_resize_crop_u8(const void* src, const int64_t* src_strides, int N, int C, int Hin, int Win, void* dst,
                        const int64_t* dst_strides, const int32_t* y_start, const int32_t* y_count, const float* y_w,
                        int y_taps, const int32_t* x_start, const int32_t* x_count, const float* x_w, int x_taps, int rh,
                        int rw, int top, int left, int th, int tw, hipStream_t stream);

/* uint8 video, indexed by src_strides = (c, t, y, x) over [C][T][H][W], C <= 16 -> the VAE encoder's contiguous
 * channels-last clip dst [T][H][W][16] bf16 (16-B aligned): channel c < C = bf16(float(bf16(float(u) / 127.5f)) -
 * 1.0f), the two bf16 roundings of `video.to(bfloat16) / 127.5 - 1.0`; channels >= C are written as zeros.
 * Replaces: _normalize_video_databatch_inplace (text2world_model_rectified_flow.py:735-736) and the NCTHW ->
 * channels-last permute and 3 -> 16 channel pad in front of the encoder. */
int cp25_u8_to_clip(const void* src, const int64_t* src_strides, int C, int T, int H, int W, void* dst,
                    hipStream_t stream);

/* bf16 clip indexed by src_strides = (t, y, x, c) over [T][H][W][C], C <= 4 (the decoder's channels-last output) ->
 * uint8 indexed by dst_strides = (t, y, x, c): u = trunc(clamp((float(v) + 1) / 2, 0, 1) * 255) in fp32. On every
 * non-NaN bf16 value this equals the reference's three quantisations: the autoregressive write-back
 * ((v / 2 + 0.5).clamp(0, 1) * 255).to(uint8) (inference/video2world.py:796-804), (clamp((v + 1) / 2, 0, 1) *
 * 255).to(uint8) of the action loop and (((1 + v) / 2) * 255).clamp(0, 255).to(uint8) of save_video. NaN input is
 * unspecified. */
int cp25_clip_to_u8(const void* src, const int64_t* src_strides, int T, int H, int W, int C, void* dst,
                    const int64_t* dst_strides, hipStream_t stream);

/* ---------------------------------------------------------------- camera features
 * Per-pixel Pluecker rays of one camera per latent frame, packed into the rows the camera-conditioned net's
 * cam_encoder (Linear(1536, D), camera/networks/minimal_v4_dit_camera_conditioned.py:1080) multiplies.
 * w2c [F, 3, 4] fp32 world-to-camera [R | t]; intrinsics [F, 4] fp32 (fx, fy, cx, cy) at the pixel size
 * (16 Hp, 16 Wp); out [F * Hp * Wp, 1536] bf16 contiguous, token order (frame, hp, wp), feature order "(c m n)":
 * c over [moment (3) | direction (3)], m / n the rows / columns of the token's 16 x 16 pixels. Per pixel centre
 * (u + 0.5, v + 0.5): direction = unit(R^T K^-1 (u, v, 1)), moment = o x direction with o = -R^T t, in fp32 without
 * contraction, rounded to bf16 once at the store. The ray arithmetic is get_plucker_rays
 * (_src/imaginaire/modules/camera.py:172-236); the packing is this build's own (the reference ships none). */
int cp25_plucker_tokens(const float* w2c, const float* intrinsics, void* out, int F, int Hp, int Wp,
                        hipStream_t stream);

/* ---------------------------------------------------------------- LoRA adapter merge (lora_ops.hip)
 * Folds one peft LoRA adapter into a bf16 weight, in place, once at load time: the reference injects adapters into
 * q_proj, k_proj, v_proj, output_proj, mlp.layer1 and mlp.layer2 (add_lora, text2world_model_rectified_flow.py:923-1008;
 * rank 32, alpha 32 by default, :92-96), keeps the LoRA parameters in fp32 (:1004) and loads checkpoints whose base
 * weights sit under `base_layer.` keys (utils/model_loader.py:134-169). It runs them unmerged,
 * base(x) + B(A x) * scale; this build merges, so every GEMM and fused epilogue of the hot path is unchanged.
 *
 * w: bf16 view [n_rows, k_cols] with leading dimension ldw >= k_cols (elements), e.g. the k rows of a fused q|k|v
 * weight. a [rank, k_cols] and b [n_rows, rank] fp32 contiguous. Per element, in fp32 without contraction:
 *   acc = 0; for j = 0 .. rank - 1 ascending: acc = acc + (b[n, j] * a[j, k])       (product and sum each rounded)
 *   w[n, k] = bf16_rne(float(w[n, k]) + acc * scale)                                (one product, one sum, one rounding)
 * so the result equals the same sequence of fp32 torch ops bit for bit. 1 <= rank <= 256; k_cols % 8 == 0, ldw % 8 == 0,
 * w and a 16-B aligned; -22 otherwise. Any n_rows. Each element is read and written by one lane; rows outside the view
 * and columns [k_cols, ldw) are never touched. No atomics, no workspace. */
int cp25_lora_merge(void* w, int64_t ldw, const float* a, const float* b, int64_t n_rows, int64_t k_cols, int rank,
                    float scale, hipStream_t stream);

/* ---------------------------------------------------------------- Reason1 text encoder (text_ops.hip, attn_causal.hip)
 * The language half of Qwen2.5-VL-7B as the reference's online text encoder runs it (text_encoders/text_encoder.py:
 * 131-220): everything between the projections, which run on cp25_gemm_epi / cp25_gemm_sm_epi. Rows are n = B * L
 * tokens, all activations bf16, every reference op one fp32 evaluation rounded to bf16 (NaN canonical). Leading
 * dimensions are in elements and multiples of 8, base pointers 16-B aligned; -22 otherwise, before any launch.
 *
 * cp25_embed_gather: out[r, 0:D] = table[ids[r], :] for n rows (embed_tokens, reason1/networks/qwen2_5_vl.py:1226).
 * table [V, D] contiguous, ids int32 on the device. The caller validates 0 <= id < V on the host; a row whose id is
 * outside the table is written as zeros and reads nothing. */
int cp25_embed_gather(const void* table, int64_t V, int64_t D, const int32_t* ids, void* out, int64_t out_ld, int64_t n,
                      hipStream_t stream);

/* The residual add and the next Qwen2RMSNorm (qwen2_5_vl.py:1135, :1141: `hidden_states = residual + hidden_states`,
 * then Qwen2RMSNorm.forward, :215-232, eps 1e-6):
 *   x[r, :] = bf16(x[r, :] + y[r, :])                       (written in place; y == NULL: x is left as it is)
 *   h[r, c] = bf16(w[c] * bf16(x[r, c] * (1 / sqrt(sum_c x[r, c]^2 / D + eps))))
 * with an fp32 sum in a fixed order and IEEE divide and sqrt. h has its own leading dimension h_ld >= D, a multiple of
 * 64: if h_ld > D, h[r, D] = 1.0 and h[r, D + 1 : h_ld] = 0, so that a bias rides as column D of the next GEMM's
 * weight. D % 8 == 0, D <= 8192 (-95 above), h_ld - D <= 2048. */
int cp25_add_rmsnorm(void* x, int64_t x_ld, const void* y, int64_t y_ld, const void* w, void* h, int64_t h_ld,
                     int64_t n, int64_t D, float eps, hipStream_t stream);

/* 1-D rotate-half RoPE in place on heads 0 .. heads - 1 (128 wide each, the q heads then the k heads) of the fused
 * QKV rows buf [n, ld]: position = row mod L, cos / sin [L, 128] bf16 tables made on the host,
 *   q = bf16(bf16(q * cos) + bf16(rotate_half(q) * sin)),  rotate_half(q) = cat(-q[64:], q[:64])
 * (apply_multimodal_rotary_pos_emb, qwen2_5_vl.py:662-700, whose three mrope sections all hold arange for a text-only
 * prompt). n % L == 0, ld >= 128 heads. */
int cp25_rope_qk(void* buf, int64_t ld, int64_t n, int L, int heads, const void* cos_t, const void* sin_t,
                 hipStream_t stream);

/* out[r, 0:I] = bf16(bf16(silu(gu[r, 0:I])) * gu[r, I:2I]) for the fused gate | up rows gu [n, ld >= 2 I]
 * (Qwen2MLP.forward, qwen2_5_vl.py:647-659); silu(x) = x / (1 + exp(-x)) in fp32 as PyTorch's device kernel. I % 8 == 0. */
int cp25_swiglu(const void* gu, int64_t ld, void* out, int64_t out_ld, int64_t n, int64_t I, hipStream_t stream);

/* TextEncoder.mean_normalize (text_encoders/text_encoder.py:119-129) of one layer's hidden state x [n, D] into columns
 * [col0, col0 + D) of out [n, out_ld] (the full_concat of :201-202), in the reference's op order on bf16 tensors:
 *   m = bf16(sum x / D); s = bf16(sqrt(sum (x - mean)^2 / (D - 1))); out = bf16(bf16(x - m) / bf16(s + 1e-8))
 * with fp32 sums in a fixed order, the std about the unrounded fp32 mean. 16 <= D <= 8192, D % 8 == 0, col0 % 8 == 0. */
int cp25_mean_normalize(const void* x, int64_t x_ld, void* out, int64_t out_ld, int64_t col0, int64_t n, int64_t D,
                        hipStream_t stream);

/* Causal grouped-query attention, head dim 128 (anything else: -22): o[b, i, h] = softmax over keys j <= i of
 * (q[b, i, h] . k[b, j, g] * softmax_scale) v[b, j, g], g = h / (Hq / Hkv). Replaces the causal flash attention of the
 * Qwen2.5-VL decoder layers (qwen2_5_vl.py:829-940, Qwen2_5_VLFlashAttention2.forward) for a text-only prompt without a padding
 * mask. q / o have Hq heads, k / v Hkv heads, Hq % Hkv == 0, L % 64 == 0. *_strides = (batch, token, head) element
 * strides, multiples of 8 with token and head strides >= 128, so q / k / v can be column views of the fused QKV
 * buffer. fp32 scores and sums, exact online row max, bf16 P; key tiles above the diagonal are not read and the
 * diagonal tile is masked before the row max. No workspace, one launch. */
int cp25_attn_causal(const void* q, const void* k, const void* v, void* o, int B, int Hq, int Hkv, int L, int D,
                     const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                     const int64_t* o_strides, float softmax_scale, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CP25_H */
