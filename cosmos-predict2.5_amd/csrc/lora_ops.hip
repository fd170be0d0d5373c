// LoRA adapter merge for gfx950: W += (B A) * scale, in place on a bf16 weight view, once at load time.
//
//   cp25_lora_merge : W[n, k] = bf16(float(W[n, k]) + (sum_j B[n, j] * A[j, k]) * scale)
//
// The reference post-trains with peft adapters on the attention and MLP projections (add_lora,
// text2world_model_rectified_flow.py:923-1008; LoRA parameters upcast to fp32 at :1004) and runs them unmerged. This
// build folds the adapter into the bf16 weight once, so the sampler's GEMMs and fused epilogues stay as they are.
//
// Arithmetic, per element, FP contraction off (a fused multiply-add rounds once where the restatement in separate fp32
// torch ops rounds twice): acc = 0; for j ascending: acc = acc + (B[n, j] * A[j, k]); then one fp32 product
// acc * scale, one fp32 sum with float(W) and one round-to-nearest-even to bf16. peft's own merge rounds the delta to
// bf16 before the sum; this rounds once.
//
// Shape of the kernel: a workgroup of 512 lanes owns a 64-row x 256-column tile of W. A lane owns 8 consecutive
// columns (one 16-B bf16 access) of 4 consecutive rows, 32 fp32 accumulators. The rank is walked in chunks of 32: the
// chunk's A rows [32][256] and B columns [64][32] are staged in the LDS (40.5 KB) and the accumulators carry across
// chunks, so the j order is ascending for every rank. Per j a lane reads its 8 A values as two conflict-free 16-B LDS
// reads and its 4 B values as one 16-B broadcast read, for 64 multiply / add lane-ops. Every W element is read and
// written by exactly one lane; rows >= N and columns >= K (the view's guard columns up to ldw) are never touched. No
// atomics, no workspace.
#include "cp25_common.h"

#pragma clang fp contract(off)

namespace {
constexpr int kTileN = 64;    // rows of W per workgroup
constexpr int kTileK = 256;   // columns of W per workgroup
constexpr int kChunk = 32;    // rank entries staged per pass
constexpr int kRowsPerLane = 4;
constexpr int kThreads = 512;  // 32 column lanes x 16 row groups

__global__ void __launch_bounds__(kThreads) lora_merge_kernel(unsigned short* __restrict__ w, int64_t ldw,
                                                              const float* __restrict__ a,
                                                              const float* __restrict__ b, int64_t n_rows,
                                                              int64_t k_cols, int rank, float scale) {
  // A chunk as [j][half][lane column][4]: a lane's columns 8 tx .. 8 tx + 3 in half 0, + 4 .. + 7 in half 1, so each of
  // its two 16-B reads is contiguous across the 32 column lanes
  __shared__ f32x4 a_s[kChunk][2][32];
  // B chunk transposed, [j][row]: a lane's 4 rows are one 16-B read; the row pitch of 68 floats keeps that read
  // 16-B aligned and spreads the staging writes (consecutive j) over the banks
  __shared__ __attribute__((aligned(16))) float b_s[kChunk][kTileN + 4];

  const int tid = threadIdx.x;
  const int tx = tid & 31, ty = tid >> 5;
  const int64_t n0 = (int64_t)blockIdx.x * kTileN;
  const int64_t k0 = (int64_t)blockIdx.y * kTileK;
  const int64_t k = k0 + tx * 8;
  const bool col_ok = k < k_cols;  // K % 8 == 0: a lane's 8 columns are inside or outside together

  u16x8 wv[kRowsPerLane];
#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i) {
    const int64_t n = n0 + ty * kRowsPerLane + i;
    wv[i] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
    if (col_ok && n < n_rows) wv[i] = *reinterpret_cast<const u16x8*>(w + n * ldw + k);
  }

  float acc[kRowsPerLane][8];
#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;

  for (int j0 = 0; j0 < rank; j0 += kChunk) {
    const int jn = min(kChunk, rank - j0);
    if (j0) __syncthreads();  // the previous chunk has been read
    // A rows j0 .. j0 + jn - 1, columns k0 .. k0 + 255: 64 16-B loads per row, 8 rows per pass
    for (int jj = tid >> 6; jj < jn; jj += kThreads / 64) {
      const int c4 = tid & 63;
      const int64_t kc = k0 + c4 * 4;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (kc < k_cols) v = *reinterpret_cast<const f32x4*>(a + (int64_t)(j0 + jj) * k_cols + kc);
      a_s[jj][c4 & 1][c4 >> 1] = v;
    }
    // B rows n0 .. n0 + 63, columns j0 .. j0 + jn - 1 (any rank: scalar loads)
    for (int e = tid; e < kTileN * kChunk; e += kThreads) {
      const int row = e / kChunk, jj = e % kChunk;
      const int64_t n = n0 + row;
      float v = 0.f;
      if (jj < jn && n < n_rows) v = b[n * rank + j0 + jj];
      b_s[jj][row] = v;
    }
    __syncthreads();
    for (int jj = 0; jj < jn; ++jj) {
      const f32x4 a0 = a_s[jj][0][tx], a1 = a_s[jj][1][tx];
      const f32x4 b4 = *reinterpret_cast<const f32x4*>(&b_s[jj][ty * kRowsPerLane]);
#pragma unroll
      for (int i = 0; i < kRowsPerLane; ++i) {
        const float bv = b4[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float p0 = bv * a0[e];
          const float p1 = bv * a1[e];
          acc[i][e] = acc[i][e] + p0;
          acc[i][4 + e] = acc[i][4 + e] + p1;
        }
      }
    }
  }

#pragma unroll
  for (int i = 0; i < kRowsPerLane; ++i) {
    const int64_t n = n0 + ty * kRowsPerLane + i;
    if (!col_ok || n >= n_rows) continue;
    u16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = acc[i][e] * scale;
      o[e] = f2bf(bf2f(wv[i][e]) + d);
    }
    *reinterpret_cast<u16x8*>(w + n * ldw + k) = o;
  }
}
}  // namespace

extern "C" int cp25_lora_merge(void* w, int64_t ldw, const float* a, const float* b, int64_t n_rows, int64_t k_cols,
                               int rank, float scale, hipStream_t stream) {
  if (!w || !a || !b || n_rows <= 0 || k_cols <= 0 || k_cols % 8 || ldw < k_cols || ldw % 8) return CP25_ERR_INVAL;
  if (rank < 1 || rank > 256) return CP25_ERR_INVAL;
  if ((((uintptr_t)w | (uintptr_t)a) & 15) || ((uintptr_t)b & 3)) return CP25_ERR_INVAL;
  const int64_t gx = cdiv(n_rows, kTileN), gy = cdiv(k_cols, kTileK);
  if (gx > 0x7fffffffLL || gy > 65535) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(lora_merge_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, stream,
                     (unsigned short*)w, ldw, a, b, n_rows, k_cols, rank, scale);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}
