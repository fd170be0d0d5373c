// Row kernels of the Reason1 (Qwen2.5-VL-7B language model) text encoder for gfx950: everything between the GEMMs.
//
//   cp25_embed_gather   : rows of the [V, D] embedding table by token id (embed_tokens, reason1/networks/qwen2_5_vl.py)
//   cp25_add_rmsnorm    : the residual add and Qwen2RMSNorm of the next sub-layer in one pass
//   cp25_rope_qk        : rotate-half 1-D RoPE on the q and k heads of the fused QKV rows, in place
//   cp25_swiglu         : silu(gate) * up of the fused gate | up rows (Qwen2MLP, :647-659)
//   cp25_mean_normalize : TextEncoder.mean_normalize of one layer's hidden state into its column block of the result
//                         (text_encoders/text_encoder.py:119-129, :196-202)
//
// The encoder's arithmetic is bf16 op by op, as stream_ops.hip's: every torch op of the reference is one operation on
// bf16 tensors, evaluated in fp32 and rounded once to bf16 (NaN canonical, as c10::BFloat16 rounds). Each line below is
// one fp32 operation and one rounding in the reference's order, FP contraction off; row statistics are fp32 sums in a
// fixed order (lane chunks ascending, a wave butterfly, the four waves ascending), so a row's bits depend on nothing but
// the row. One workgroup of 256 lanes per row, each lane holding up to four 16-byte chunks of it in registers, so a
// row is read once. All global accesses are 16-byte vector moves.
#include <initializer_list>

#include "cp25_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kRowThreads = 256;
constexpr int kRowChunks = 4;                             // 16-byte chunks a lane holds
constexpr int kRowMaxD = kRowThreads * kRowChunks * 8;    // 8192

inline bool aligned16(std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= (uintptr_t)p;
  return (bits & 15) == 0;
}

// float -> bf16 as torch's c10::BFloat16 rounds: nearest even, every NaN the canonical 0x7FC0
__device__ __forceinline__ unsigned short tbf(float f) { return f != f ? (unsigned short)0x7FC0 : f2bf(f); }
__device__ __forceinline__ float rtb(float f) { return bf2f(tbf(f)); }

// the sum of one value per lane over the workgroup, in a fixed order, returned to every lane; `red` is 4 floats of LDS
__device__ __forceinline__ float block_sum(float v, float* red) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  __syncthreads();  // the previous use of red is over
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// ---------------------------------------------------------------- token gather
// One lane per 16-byte chunk of an output row. The wrapper has validated the ids; an id outside the table still
// forms no address (the row is written as zeros).
__global__ void __launch_bounds__(256) embed_gather_kernel(const unsigned short* __restrict__ table, int64_t V, int D8,
                                                           const int* __restrict__ ids, unsigned short* __restrict__ out,
                                                           int64_t out_ld, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * D8) return;
  const int64_t row = i / D8;
  const int c = (int)(i % D8);
  const int64_t id = ids[row];
  u16x8 w = {0, 0, 0, 0, 0, 0, 0, 0};
  if (id >= 0 && id < V) w = *reinterpret_cast<const u16x8*>(table + id * (int64_t)D8 * 8 + c * 8);
  *reinterpret_cast<u16x8*>(out + row * out_ld + c * 8) = w;
}

// ---------------------------------------------------------------- residual add + RMSNorm
__global__ void __launch_bounds__(kRowThreads) add_rmsnorm_kernel(unsigned short* __restrict__ x, int64_t x_ld,
                                                                  const unsigned short* __restrict__ y, int64_t y_ld,
                                                                  const unsigned short* __restrict__ w,
                                                                  unsigned short* __restrict__ h, int64_t h_ld, int D,
                                                                  float eps) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const int D8 = D >> 3;
  unsigned short* xr = x + row * x_ld;
  float xv[kRowChunks][8];
  float ss = 0.f;
#pragma unroll
  for (int j = 0; j < kRowChunks; ++j) {
    const int c = threadIdx.x + j * kRowThreads;
    if (c < D8) {
      u16x8 a = *reinterpret_cast<const u16x8*>(xr + c * 8);
      if (y != nullptr) {
        const u16x8 b = *reinterpret_cast<const u16x8*>(y + row * y_ld + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] = tbf(bf2f(a[e]) + bf2f(b[e]));  // hidden_states = residual + hidden_states
        *reinterpret_cast<u16x8*>(xr + c * 8) = a;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xv[j][e] = bf2f(a[e]);
        ss += xv[j][e] * xv[j][e];
      }
    }
  }
  ss = block_sum(ss, red);
  const float rstd = 1.0f / sqrtf(ss / (float)D + eps);  // IEEE divide and sqrt (the build's flag)
  unsigned short* hr = h + row * h_ld;
#pragma unroll
  for (int j = 0; j < kRowChunks; ++j) {
    const int c = threadIdx.x + j * kRowThreads;
    if (c < D8) {
      const u16x8 g = *reinterpret_cast<const u16x8*>(w + c * 8);
      u16x8 r;
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = tbf(bf2f(g[e]) * rtb(xv[j][e] * rstd));  // weight * hidden.to(bf16)
      *reinterpret_cast<u16x8*>(hr + c * 8) = r;
    }
  }
  // the bias column: 1.0 at column D, zeros up to h_ld
  const int pad8 = (int)((h_ld - D) >> 3);
  if ((int)threadIdx.x < pad8) {
    u16x8 r = {0, 0, 0, 0, 0, 0, 0, 0};
    if (threadIdx.x == 0) r[0] = 0x3F80;
    *reinterpret_cast<u16x8*>(hr + D + threadIdx.x * 8) = r;
  }
}

// ---------------------------------------------------------------- rotary
// One lane per (row, head, chunk c < 8): elements 8 c .. 8 c + 7 and their rotate-half partners 64 + 8 c .. of one head.
__global__ void __launch_bounds__(256) rope_qk_kernel(unsigned short* __restrict__ buf, int64_t ld, int heads,
                                                      const unsigned short* __restrict__ cos_t,
                                                      const unsigned short* __restrict__ sin_t, int L, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * heads * 8) return;
  const int c = (int)(i & 7);
  const int64_t rh = i >> 3;
  const int head = (int)(rh % heads);
  const int64_t row = rh / heads;
  const int pos = (int)(row % L);
  unsigned short* p = buf + row * ld + head * 128 + c * 8;
  const u16x8 lo = *reinterpret_cast<const u16x8*>(p);
  const u16x8 hi = *reinterpret_cast<const u16x8*>(p + 64);
  const u16x8 cl = *reinterpret_cast<const u16x8*>(cos_t + pos * 128 + c * 8);
  const u16x8 chh = *reinterpret_cast<const u16x8*>(cos_t + pos * 128 + 64 + c * 8);
  const u16x8 sl = *reinterpret_cast<const u16x8*>(sin_t + pos * 128 + c * 8);
  const u16x8 sh = *reinterpret_cast<const u16x8*>(sin_t + pos * 128 + 64 + c * 8);
  u16x8 ol, oh;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float a = bf2f(lo[e]), b = bf2f(hi[e]);
    // (q * cos) + (rotate_half(q) * sin), rotate_half(q) = cat(-q[64:], q[:64]): three bf16 ops (the negation is exact)
    ol[e] = tbf(rtb(a * bf2f(cl[e])) + rtb(-b * bf2f(sl[e])));
    oh[e] = tbf(rtb(b * bf2f(chh[e])) + rtb(a * bf2f(sh[e])));
  }
  *reinterpret_cast<u16x8*>(p) = ol;
  *reinterpret_cast<u16x8*>(p + 64) = oh;
}

// ---------------------------------------------------------------- SwiGLU
// One lane per 16-byte chunk of an output row. silu as PyTorch's device kernel evaluates it on a bf16 tensor:
// x / (1 + exp(-x)) in fp32 (ActivationSiluKernel.cu), one rounding.
__global__ void __launch_bounds__(256) swiglu_kernel(const unsigned short* __restrict__ gu, int64_t ld, int I8,
                                                     unsigned short* __restrict__ out, int64_t out_ld, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n * I8) return;
  const int64_t row = i / I8;
  const int c = (int)(i % I8);
  const u16x8 g = *reinterpret_cast<const u16x8*>(gu + row * ld + c * 8);
  const u16x8 u = *reinterpret_cast<const u16x8*>(gu + row * ld + (int64_t)I8 * 8 + c * 8);
  u16x8 r;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = bf2f(g[e]);
    const float s = rtb(x / (1.0f + expf(-x)));  // act_fn(gate_proj(x))
    r[e] = tbf(s * bf2f(u[e]));                  // * up_proj(x)
  }
  *reinterpret_cast<u16x8*>(out + row * out_ld + c * 8) = r;
}

// ---------------------------------------------------------------- mean-normalise
// (t - t.mean(-1)) / (t.std(-1) + 1e-8) on a bf16 tensor: the mean and the unbiased std are fp32 reductions rounded to
// bf16, the std taken about the fp32 mean (two passes over the registers, no cancellation).
__global__ void __launch_bounds__(kRowThreads) mean_normalize_kernel(const unsigned short* __restrict__ x, int64_t x_ld,
                                                                     unsigned short* __restrict__ out, int64_t out_ld,
                                                                     int64_t col0, int D) {
  __shared__ float red[4];
  const int64_t row = blockIdx.x;
  const int D8 = D >> 3;
  float xv[kRowChunks][8];
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kRowChunks; ++j) {
    const int c = threadIdx.x + j * kRowThreads;
    if (c < D8) {
      const u16x8 a = *reinterpret_cast<const u16x8*>(x + row * x_ld + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        xv[j][e] = bf2f(a[e]);
        s += xv[j][e];
      }
    }
  }
  const float mean = block_sum(s, red) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < kRowChunks; ++j) {
    const int c = threadIdx.x + j * kRowThreads;
    if (c < D8) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = xv[j][e] - mean;
        q += d * d;
      }
    }
  }
  const float stdv = rtb(sqrtf(block_sum(q, red) / (float)(D - 1)));  // tensor.std(dim=-1)
  const float den = rtb(stdv + 1e-8f);                                  // + 1e-8
  const float mb = rtb(mean);                                           // tensor.mean(dim=-1)
  unsigned short* o = out + row * out_ld + col0;
#pragma unroll
  for (int j = 0; j < kRowChunks; ++j) {
    const int c = threadIdx.x + j * kRowThreads;
    if (c < D8) {
      u16x8 r;
#pragma unroll
      for (int e = 0; e < 8; ++e) r[e] = tbf(rtb(xv[j][e] - mb) / den);  // (tensor - mean) / (std + 1e-8)
      *reinterpret_cast<u16x8*>(o + c * 8) = r;
    }
  }
}

inline bool row_grid_ok(int64_t n) { return n > 0 && n <= 0x7fffffff; }
}  // namespace

extern "C" int cp25_embed_gather(const void* table, int64_t V, int64_t D, const int32_t* ids, void* out, int64_t out_ld,
                                 int64_t n, hipStream_t stream) {
  if (!table || !ids || !out || V <= 0 || n <= 0 || D <= 0 || D > (1 << 20)) return CP25_ERR_INVAL;
  if (D % 8 || out_ld % 8 || out_ld < D) return CP25_ERR_INVAL;
  if (!aligned16({table, out}) || ((uintptr_t)ids & 3)) return CP25_ERR_INVAL;
  const int64_t total = n * (D / 8);
  if (cdiv(total, 256) > 0x7fffffff) return CP25_ERR_DTYPE;
  hipLaunchKernelGGL(embed_gather_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream,
                     (const unsigned short*)table, V, (int)(D / 8), ids, (unsigned short*)out, out_ld, n);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

extern "C" int cp25_add_rmsnorm(void* x, int64_t x_ld, const void* y, int64_t y_ld, const void* w, void* h,
                                int64_t h_ld, int64_t n, int64_t D, float eps, hipStream_t stream) {
  if (!x || !w || !h || !row_grid_ok(n)) return CP25_ERR_INVAL;
  if (D <= 0 || D % 8 || x_ld % 8 || x_ld < D || (y && (y_ld % 8 || y_ld < D))) return CP25_ERR_INVAL;
  if (D > kRowMaxD) return CP25_ERR_DTYPE;
  if (h_ld < D || h_ld % 64 || h_ld - D > kRowThreads * 8) return CP25_ERR_INVAL;
  if (!(eps > 0.f) || !aligned16({x, y, w, h})) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(add_rmsnorm_kernel, dim3((unsigned)n), dim3(kRowThreads), 0, stream, (unsigned short*)x, x_ld,
                     (const unsigned short*)y, y_ld, (const unsigned short*)w, (unsigned short*)h, h_ld, (int)D, eps);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

extern "C" int cp25_rope_qk(void* buf, int64_t ld, int64_t n, int L, int heads, const void* cos_t, const void* sin_t,
                            hipStream_t stream) {
  if (!buf || !cos_t || !sin_t || n <= 0 || L <= 0 || heads <= 0 || heads > 4096) return CP25_ERR_INVAL;
  if (n % L || ld % 8 || ld < (int64_t)heads * 128) return CP25_ERR_INVAL;
  if (!aligned16({buf, cos_t, sin_t})) return CP25_ERR_INVAL;
  const int64_t total = n * heads * 8;
  if (cdiv(total, 256) > 0x7fffffff) return CP25_ERR_DTYPE;
  hipLaunchKernelGGL(rope_qk_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, (unsigned short*)buf, ld,
                     heads, (const unsigned short*)cos_t, (const unsigned short*)sin_t, L, n);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

extern "C" int cp25_swiglu(const void* gu, int64_t ld, void* out, int64_t out_ld, int64_t n, int64_t I,
                           hipStream_t stream) {
  if (!gu || !out || n <= 0 || I <= 0 || I > (1 << 24)) return CP25_ERR_INVAL;
  if (I % 8 || ld % 8 || out_ld % 8 || ld < 2 * I || out_ld < I) return CP25_ERR_INVAL;
  if (!aligned16({gu, out})) return CP25_ERR_INVAL;
  const int64_t total = n * (I / 8);
  if (cdiv(total, 256) > 0x7fffffff) return CP25_ERR_DTYPE;
  hipLaunchKernelGGL(swiglu_kernel, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, stream, (const unsigned short*)gu,
                     ld, (int)(I / 8), (unsigned short*)out, out_ld, n);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

extern "C" int cp25_mean_normalize(const void* x, int64_t x_ld, void* out, int64_t out_ld, int64_t col0, int64_t n,
                                   int64_t D, hipStream_t stream) {
  if (!x || !out || !row_grid_ok(n)) return CP25_ERR_INVAL;
  if (D < 16 || D % 8 || x_ld % 8 || x_ld < D) return CP25_ERR_INVAL;
  if (D > kRowMaxD) return CP25_ERR_DTYPE;
  if (col0 < 0 || col0 % 8 || out_ld % 8 || col0 + D > out_ld) return CP25_ERR_INVAL;
  if (!aligned16({x, out})) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(mean_normalize_kernel, dim3((unsigned)n), dim3(kRowThreads), 0, stream, (const unsigned short*)x,
                     x_ld, (unsigned short*)out, out_ld, col0, (int)D);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}
