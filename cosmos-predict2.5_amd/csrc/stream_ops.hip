// The streaming (causal, KV-cached) action student's per-frame pieces for gfx950.
//
//   cp25_kv_put             : the frame's K and V column blocks of the fused [n, 3D] QKV rows -> the rows of one slot
//                             of the block's K and V ring caches [B, slot_row, H, hd], one launch for both
//                             (AttenOpWithKV's store, interactive/networks/dit_causal.py:1129-1149)
//   cp25_stream_patchify_ld : EDM preconditioning x * c_in in bf16 + the x_embedder's patch rows of one frame
//                             (denoise_edm_seq, interactive/models/action_video2world_self_forcing.py:206, :211,
//                             forward_seq's mask channel, interactive/networks/dit_action_causal.py:625)
//   cp25_stream_x0_step     : x0 = c_skip x + c_out net (:226), then x0 itself (last step) or the re-noising
//                             cos(t_next) x0 / sigma_data + sin(t_next) noise (:442-444)
//   cp25_stream_latent_clip : one generated frame of the token-major state -> the VAE decoder's channels-last input of
//                             that frame, un-normalised (from_patch_layout + the permute and `zl / inv_std + mean` of
//                             WanVAE._decode_clip; the reference's decode, tokenizers/wan2pt1.py:555-558)
//
// The student's arithmetic is bf16 op by op: every torch op of the reference is one operation on bf16 tensors, which
// PyTorch's elementwise kernels evaluate in fp32 and round once to bf16 (DESIGN.md §6e has the operand-by-operand
// derivation). So each line below is one fp32 operation followed by one bf16 rounding, in the reference's order and
// association, FP contraction off. `x / sigma_data` with a Python-float divisor is PyTorch's multiplication by the
// fp32 reciprocal 1.0f / float(sigma_data), not a division. All global accesses are 16-byte vector moves.
#include <initializer_list>

#include "cp25_common.h"

#pragma clang fp contract(off)

namespace {
inline bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

// a float that is exactly a bf16 value (NaN included)
inline bool is_bf16_value(float f) {
  unsigned u;
  __builtin_memcpy(&u, &f, 4);
  return (u & 0xffffu) == 0;
}

// float -> bf16 as torch's c10::BFloat16 rounds: nearest even, every NaN the canonical 0x7FC0
__device__ __forceinline__ unsigned short tbf(float f) { return f != f ? (unsigned short)0x7FC0 : f2bf(f); }
__device__ __forceinline__ float rtb(float f) { return bf2f(tbf(f)); }

// ---------------------------------------------------------------- K / V ring-cache store
// One lane per 16-byte chunk: chunk id -> (row = tok * B + b, which = K | V, column chunk).
__global__ void __launch_bounds__(256) kv_put_kernel(const unsigned short* __restrict__ qkv, int64_t ld, int64_t k_col0,
                                                     int64_t v_col0, int D8, unsigned short* __restrict__ kc,
                                                     unsigned short* __restrict__ vc, int64_t cache_sb,
                                                     int64_t cache_sr, int B, int64_t n_tok, int64_t row0) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per_row = 2 * (int64_t)D8;
  if (i >= n_tok * B * per_row) return;
  const int64_t row = i / per_row;
  const int c = (int)(i % per_row);
  const int which = c / D8, cc = c % D8;
  const int64_t tok = row / B;
  const int b = (int)(row % B);
  const u16x8 w = *reinterpret_cast<const u16x8*>(qkv + row * ld + (which ? v_col0 : k_col0) + cc * 8);
  unsigned short* dst = (which ? vc : kc) + b * cache_sb + (row0 + tok) * cache_sr + cc * 8;
  *reinterpret_cast<u16x8*>(dst) = w;
}

// ---------------------------------------------------------------- preconditioning + patch rows
// xs in patch layout [tok, 64] bf16 (index p*16 + c); out [tok, out_ld] bf16 with feature index c*4 + p for c in 0..17
// (cp25_patchify's rows). 16 lanes per token: lanes 0..7 write channels 2l, 2l + 1 (eight features, 16 bytes), lane 8
// the mask | padding-mask features 64..71, lanes 9..15 the zero columns 72..127 of a K = 128 row.
__global__ void __launch_bounds__(256) stream_patchify_kernel(const unsigned short* __restrict__ xs, float c_in,
                                                              float mask, const unsigned short* __restrict__ pad_mask,
                                                              unsigned short* __restrict__ out, int64_t out_ld,
                                                              int64_t n_tok) {
  const int64_t tok = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (tok >= n_tok) return;
  const int l = threadIdx.x & 15;
  unsigned short* o = out + tok * out_ld;
  if (l < 8) {
    // the token's 64 values as eight 16-byte chunks; chunk (p, half) holds channels 8 half .. 8 half + 7 of p
    const int half = l >> 2, off = (2 * l) & 7;
    u16x8 r;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const u16x8 w = *reinterpret_cast<const u16x8*>(xs + tok * 64 + p * 16 + half * 8);
      unsigned short a = 0, b = 0;
#pragma unroll
      for (int e = 0; e < 8; ++e) {  // select without a dynamic vector index
        if (e == off) a = w[e];
        if (e == off + 1) b = w[e];
      }
      r[p] = tbf(bf2f(a) * c_in);  // x * c_in, one bf16 op
      r[4 + p] = tbf(bf2f(b) * c_in);
    }
    *reinterpret_cast<u16x8*>(o + 8 * l) = r;
  } else if (l == 8) {
    const unsigned short mb = tbf(mask);
    u16x8 t = {mb, mb, mb, mb, 0, 0, 0, 0};
    if (pad_mask != nullptr) {
      const u16x4 pm = *reinterpret_cast<const u16x4*>(pad_mask + tok * 4);
#pragma unroll
      for (int k = 0; k < 4; ++k) t[4 + k] = pm[k];
    }
    *reinterpret_cast<u16x8*>(o + 64) = t;
  } else if (out_ld == 128) {
    const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    *reinterpret_cast<u16x8*>(o + 72 + (l - 9) * 8) = z;
  }
}

// ---------------------------------------------------------------- x0 and re-noising
// One lane per eight consecutive elements of a token; net is the B = 1 final-layer output, already in patch layout.
__global__ void __launch_bounds__(256) stream_x0_step_kernel(const unsigned short* __restrict__ xs,
                                                             const float* __restrict__ net,
                                                             const unsigned short* __restrict__ noise,
                                                             unsigned short* __restrict__ out, float c_skip,
                                                             float c_out, float cos_next, float sin_next, float inv_sd,
                                                             int last, int64_t n8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const u16x8 x = *reinterpret_cast<const u16x8*>(xs + i * 8);
  const f32x4 f0 = *reinterpret_cast<const f32x4*>(net + i * 8);
  const f32x4 f1 = *reinterpret_cast<const f32x4*>(net + i * 8 + 4);
  u16x8 nz = {0, 0, 0, 0, 0, 0, 0, 0};
  if (!last) nz = *reinterpret_cast<const u16x8*>(noise + i * 8);
  u16x8 r;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float fn = rtb(k < 4 ? f0[k & 3] : f1[k & 3]);  // net output .to(bfloat16)
    const float a = rtb(c_skip * bf2f(x[k]));             // c_skip * x
    const float b = rtb(c_out * fn);                      // c_out * net_output
    const float x0 = rtb(a + b);                          // +
    if (last) {
      r[k] = tbf(x0);
    } else {
      const float c = rtb(cos_next * x0);            // cos(t_next) * x0
      const float q = rtb(c * inv_sd);               // / sigma_data: times the fp32 reciprocal
      const float s = rtb(sin_next * bf2f(nz[k]));   // sin(t_next) * noise
      r[k] = tbf(q + s);                             // +
    }
  }
  *reinterpret_cast<u16x8*>(out + i * 8) = r;
}
// ---------------------------------------------------------------- state rows -> the decoder's un-normalised frame
// One lane per 16-byte chunk of the row-major input: chunk id -> (row = tok * B + b, p = p1 * 2 + p2, channel half).
// dst [B][2 Hp][2 Wp][16]: pixel (2 i + p1, 2 j + p2) of clip b, tok = i * Wp + j. Two bf16 ops per element: the IEEE
// fp32 division by inv_std[c], then the addition of mean[c].
__global__ void __launch_bounds__(256) stream_latent_clip_kernel(const unsigned short* __restrict__ xs,
                                                                 const unsigned short* __restrict__ inv_std,
                                                                 const unsigned short* __restrict__ mean,
                                                                 unsigned short* __restrict__ dst, int B, int Hp, int Wp,
                                                                 int64_t n_chunks) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_chunks) return;
  const int64_t row = i >> 3;
  const int c8 = (int)(i & 7);
  const int p1 = c8 >> 2, p2 = (c8 >> 1) & 1, half = c8 & 1;
  const int64_t tok = row / B;
  const int b = (int)(row % B);
  const int64_t ti = tok / Wp, tj = tok % Wp;
  const u16x8 x = *reinterpret_cast<const u16x8*>(xs + i * 8);
  const u16x8 is = *reinterpret_cast<const u16x8*>(inv_std + half * 8);
  const u16x8 mu = *reinterpret_cast<const u16x8*>(mean + half * 8);
  u16x8 r;
#pragma unroll
  for (int k = 0; k < 8; ++k) r[k] = tbf(rtb(bf2f(x[k]) / bf2f(is[k])) + bf2f(mu[k]));
  const int64_t pix = ((int64_t)b * (2 * Hp) + (2 * ti + p1)) * (2 * (int64_t)Wp) + (2 * tj + p2);
  *reinterpret_cast<u16x8*>(dst + pix * 16 + half * 8) = r;
}
}  // namespace

extern "C" int cp25_kv_put(const void* qkv, int64_t ld, int64_t k_col0, int64_t v_col0, int64_t D, void* k_cache,
                           void* v_cache, int64_t cache_sb, int64_t cache_sr, int64_t cache_rows, int B, int64_t n_tok,
                           int64_t row0, hipStream_t stream) {
  if (!qkv || !k_cache || !v_cache || B <= 0 || n_tok <= 0 || D <= 0 || D > (1 << 20)) return CP25_ERR_INVAL;
  if (D % 8 || ld % 8 || k_col0 % 8 || v_col0 % 8 || cache_sb % 8 || cache_sr % 8) return CP25_ERR_INVAL;
  if (k_col0 < 0 || v_col0 < 0 || k_col0 + D > ld || v_col0 + D > ld) return CP25_ERR_INVAL;
  if (cache_sr < D || row0 < 0 || cache_rows <= 0 || row0 + n_tok > cache_rows) return CP25_ERR_INVAL;
  if (B > 1 && cache_sb < cache_rows * cache_sr) return CP25_ERR_INVAL;
  if (!aligned16({qkv, k_cache, v_cache})) return CP25_ERR_INVAL;
  const int64_t total = n_tok * B * 2 * (D / 8);
  if (cdiv(total, 256) > 0x7fffffff) return CP25_ERR_DTYPE;
  hipLaunchKernelGGL(kv_put_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, (const unsigned short*)qkv,
                     ld, k_col0, v_col0, (int)(D / 8), (unsigned short*)k_cache, (unsigned short*)v_cache, cache_sb,
                     cache_sr, B, n_tok, row0);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

extern "C" int cp25_stream_patchify_ld(const void* xs, float c_in, float mask, const void* pad_mask, void* out,
                                       int64_t out_ld, int64_t n_tok, hipStream_t stream) {
  if (!xs || !out || n_tok <= 0 || cdiv(n_tok, 16) > 0x7fffffff) return CP25_ERR_INVAL;
  if (out_ld != 72 && out_ld != 128) return CP25_ERR_DTYPE;
  if (!aligned16({xs, out}) || ((uintptr_t)pad_mask & 7)) return CP25_ERR_INVAL;
  if (!is_bf16_value(c_in) || !is_bf16_value(mask)) return CP25_ERR_INVAL;  // bf16 tensors in the reference
  hipLaunchKernelGGL(stream_patchify_kernel, dim3((unsigned)cdiv(n_tok, 16)), dim3(256), 0, stream,
                     (const unsigned short*)xs, c_in, mask, (const unsigned short*)pad_mask, (unsigned short*)out,
                     out_ld, n_tok);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

extern "C" int cp25_stream_x0_step(const void* xs, const float* net, const void* noise, void* out, float c_skip,
                                   float c_out, float cos_next, float sin_next, double sigma_data, int last,
                                   int64_t n_tok, hipStream_t stream) {
  if (!xs || !net || !out || n_tok <= 0 || cdiv(n_tok * 8, 256) > 0x7fffffff) return CP25_ERR_INVAL;
  if (!last && !noise) return CP25_ERR_INVAL;
  if (!aligned16({xs, net, out, last ? nullptr : noise})) return CP25_ERR_INVAL;
  if (!(sigma_data > 0.0)) return CP25_ERR_INVAL;
  if (!is_bf16_value(c_skip) || !is_bf16_value(c_out)) return CP25_ERR_INVAL;
  if (!last && (!is_bf16_value(cos_next) || !is_bf16_value(sin_next))) return CP25_ERR_INVAL;
  const float inv_sd = 1.0f / (float)sigma_data;  // PyTorch's `tensor / python_scalar` on the device
  hipLaunchKernelGGL(stream_x0_step_kernel, dim3((unsigned)cdiv(n_tok * 8, 256)), dim3(256), 0, stream,
                     (const unsigned short*)xs, net, (const unsigned short*)noise, (unsigned short*)out, c_skip, c_out,
                     cos_next, sin_next, inv_sd, last, n_tok * 8);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

extern "C" int cp25_stream_latent_clip(const void* xs, const void* inv_std, const void* mean, void* dst, int B, int Hp,
                                       int Wp, hipStream_t stream) {
  if (!xs || !inv_std || !mean || !dst || B <= 0 || Hp <= 0 || Wp <= 0) return CP25_ERR_INVAL;
  if (!aligned16({xs, inv_std, mean, dst})) return CP25_ERR_INVAL;
  const int64_t n_chunks = (int64_t)Hp * Wp * B * 8;
  if (cdiv(n_chunks, 256) > 0x7fffffff) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(stream_latent_clip_kernel, dim3((unsigned)cdiv(n_chunks, 256)), dim3(256), 0, stream,
                     (const unsigned short*)xs, (const unsigned short*)inv_std, (const unsigned short*)mean,
                     (unsigned short*)dst, B, Hp, Wp, n_chunks);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}
