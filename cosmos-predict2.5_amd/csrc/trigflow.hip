// The distilled (DMD2 / TrigFlow) student's per-step arithmetic for gfx950: the two elementwise halves that bracket
// the DiT forward of one few-step sampling step.
//
//   cp25_trig_patchify_ld : EDM preconditioning (xt * c_in), conditioning-frame replacement (gt / sigma_data), the
//                           cast to the net dtype and the x_embedder's patch rows, in one launch
//                           (video2world_model_rectified_flow.py:262-266, :274-309 + cp25_patchify_ld's sources)
//   cp25_trig_x0_step     : x0 reconstruction (c_skip xt + c_out net), GT-frame replacement, and either the TrigFlow
//                           re-noising to the next time or the final nan_to_num, in place on the fp32 state
//                           (video2world_model_rectified_flow.py:325-336, video2world_model_distill_dmd2.py:485-492)
//
// The reference keeps the loop state and the scaling coefficients in float64 and PyTorch's type promotion makes every
// product and sum above a float64 operation, so both kernels compute in fp64, one IEEE operation per torch op in the
// reference's order (FP contraction off: a fused multiply-add rounds once where torch rounds twice). The mask
// arithmetic is the reference's `a * mask + b * (1 - mask)` as written, not a select, so a non-finite b in a masked
// frame gives the NaN it gives there. 16 bytes per lane and access: four fp32 elements of a token.
#include <initializer_list>

#include "cp25_common.h"

#pragma clang fp contract(off)

namespace {
inline bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

// xs / gt in patch layout [tok, 64] (index p*16 + c); out [tok, out_ld] bf16 with feature index c*4 + p for c in
// 0..17 (cp25_patchify's rows). 16 lanes per token: lane l reads elements p*16 + c0 .. c0 + 3 (p = l / 4, c0 = 4 (l % 4)).
__global__ void __launch_bounds__(256) trig_patchify_kernel(const float* __restrict__ xs, const float* __restrict__ gt,
                                                            const float* __restrict__ frame_mask,
                                                            const double* __restrict__ c_in, double sigma_data,
                                                            const unsigned short* __restrict__ pad_mask,
                                                            unsigned short* __restrict__ out, int64_t out_ld,
                                                            int64_t n_tok, int64_t tok0, int64_t hw) {
  const int64_t tok = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  if (tok >= n_tok) return;
  const int l = threadIdx.x & 15;
  const int p = l >> 2, c0 = (l & 3) * 4;
  const int64_t frame = (tok0 + tok) / hw;
  const float mf = frame_mask[frame];
  const double ci = c_in[frame];
  const int64_t e = tok * 64 + p * 16 + c0;
  const f32x4 x = *reinterpret_cast<const f32x4*>(xs + e);
  f32x4 g = {0.f, 0.f, 0.f, 0.f};
  if (gt != nullptr) g = *reinterpret_cast<const f32x4*>(gt + e);
  unsigned short* o = out + tok * out_ld;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    double v = (double)x[k] * ci;  // xt * c_in
    if (gt != nullptr) {
      const double m = (double)mf;
      const double cond = (double)g[k] / sigma_data;  // gt_frames.type_as(net_state_in) / sigma_data
      const double a = cond * m;
      const double om = 1.0 - m;
      v = a + v * om;
    }
    o[(c0 + k) * 4 + p] = f2bf((float)v);  // .to(bfloat16) of a float64 tensor rounds through fp32
  }
  if (l == 0) {
    const unsigned short mb = f2bf(mf);
    u16x8 t = {mb, mb, mb, mb, 0, 0, 0, 0};
    if (pad_mask != nullptr) {
#pragma unroll
      for (int k = 0; k < 4; ++k) t[4 + k] = pad_mask[tok * 4 + k];
    }
    *reinterpret_cast<u16x8*>(o + 64) = t;
  }
  const u16x8 z = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t c = 72 + l * 8; c < out_ld; c += 128) *reinterpret_cast<u16x8*>(o + c) = z;  // the GEMM's K padding
}

__device__ __forceinline__ float nan_to_num_f32(float v) {  // torch.nan_to_num defaults
  if (v != v) return 0.f;
  if (v == __builtin_inff()) return 3.402823466e38f;
  if (v == -__builtin_inff()) return -3.402823466e38f;
  return v;
}

// One lane per four consecutive elements of a token; net is the B = 1 final-layer output, already in patch layout.
__global__ void __launch_bounds__(256) trig_x0_step_kernel(float* __restrict__ xs, const float* __restrict__ net,
                                                           const float* __restrict__ noise,
                                                           const float* __restrict__ gt,
                                                           const float* __restrict__ frame_mask,
                                                           const double* __restrict__ c_skip,
                                                           const double* __restrict__ c_out, double sigma_data,
                                                           double cos_next, float sin_next, int last, int64_t n_tok,
                                                           int64_t tok0, int64_t hw) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_tok * 16) return;
  const int64_t tok = i >> 4;
  const int64_t frame = (tok0 + tok) / hw;
  const double cs = c_skip[frame], co = c_out[frame];
  const int64_t e = i * 4;
  const f32x4 x = *reinterpret_cast<const f32x4*>(xs + e);
  const f32x4 f = *reinterpret_cast<const f32x4*>(net + e);
  f32x4 g = {0.f, 0.f, 0.f, 0.f}, nz = {0.f, 0.f, 0.f, 0.f};
  double m = 0.0;
  if (gt != nullptr) {  // NULL unless replace_gt (the host entry)
    g = *reinterpret_cast<const f32x4*>(gt + e);
    m = (double)frame_mask[frame];
  }
  if (!last) nz = *reinterpret_cast<const f32x4*>(noise + e);
  f32x4 r;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double a = cs * (double)x[k];
    const double b = co * (double)f[k];
    double x0 = a + b;  // c_skip * xt + c_out * net_output
    if (gt != nullptr) {
      const double ga = (double)g[k] * m;
      const double om = 1.0 - m;
      x0 = ga + x0 * om;  // gt_frames * mask + x0_pred * (1 - mask)
    }
    if (last) {
      r[k] = nan_to_num_f32((float)x0);
    } else {
      const double c = cos_next * x0;
      const double q = c / sigma_data;
      const float sn = sin_next * nz[k];  // python float * float32 tensor: an fp32 product
      r[k] = (float)(q + (double)sn);     // float64 + float32 -> float64; .float() at the next step's entry
    }
  }
  *reinterpret_cast<f32x4*>(xs + e) = r;
}
}  // namespace

extern "C" int cp25_trig_patchify_ld(const float* xs, const float* gt, const float* frame_mask, const double* c_in,
                                     double sigma_data, const void* pad_mask, void* out, int64_t out_ld, int64_t n_tok,
                                     int64_t tok0, int64_t hw, hipStream_t stream) {
  if (!xs || !frame_mask || !c_in || !out || n_tok <= 0 || tok0 < 0 || hw <= 0 || out_ld < 72 || out_ld % 8)
    return CP25_ERR_INVAL;
  if (!aligned16({xs, gt, out}) || ((uintptr_t)c_in & 7) || ((uintptr_t)frame_mask & 3) || ((uintptr_t)pad_mask & 1))
    return CP25_ERR_INVAL;
  if (!(sigma_data > 0.0)) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(trig_patchify_kernel, dim3((unsigned)cdiv(n_tok, 16)), dim3(256), 0, stream, xs, gt, frame_mask,
                     c_in, sigma_data, (const unsigned short*)pad_mask, (unsigned short*)out, out_ld, n_tok, tok0, hw);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

extern "C" int cp25_trig_x0_step(float* xs, const float* net, const float* noise, const float* gt,
                                 const float* frame_mask, const double* c_skip, const double* c_out, int replace_gt,
                                 double sigma_data, double cos_next, double sin_next, int last, int64_t n_tok,
                                 int64_t tok0, int64_t hw, hipStream_t stream) {
  if (!xs || !net || !c_skip || !c_out || n_tok <= 0 || tok0 < 0 || hw <= 0) return CP25_ERR_INVAL;
  if (!last && !noise) return CP25_ERR_INVAL;
  const float* g = replace_gt ? gt : nullptr;
  if (g != nullptr && !frame_mask) return CP25_ERR_INVAL;
  if (!aligned16({xs, net, last ? nullptr : noise, g}) || (((uintptr_t)c_skip | (uintptr_t)c_out) & 7) ||
      ((uintptr_t)frame_mask & 3))
    return CP25_ERR_INVAL;
  if (!(sigma_data > 0.0)) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(trig_x0_step_kernel, dim3((unsigned)cdiv(n_tok * 16, 256)), dim3(256), 0, stream, xs, net, noise, g,
                     frame_mask, c_skip, c_out, sigma_data, cos_next, (float)sin_next, last, n_tok, tok0, hw);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}
