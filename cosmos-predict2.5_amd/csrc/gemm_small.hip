// Small-M block GEMMs for the streaming per-frame forward (gfx950): C[M, N] = epi(A[M, K] W[N, K]^T), bf16 in / out,
// fp32 accumulation on v_mfma_f32_16x16x32_bf16, for M from 1 to a few thousand rows, where gemm.hip's 256 x 256 tiles
// leave most of the 256 CUs idle (320 rows x 2048 columns are 16 tiles). Entry points cp25_gemm_sm_epi / _res /
// _hnorm / _qkv (include/cp25.h): the operands, host checks and epilogues of cp25_gemm_epi / _res / _hnorm / _qkv,
// followed by (split, workspace, workspace_bytes). Replaces the same nn.Linear layers, as the causal student runs them
// one latent frame at a time (interactive/networks/dit_causal.py).
//
// Design: one 64 x 128 output tile per 256-thread workgroup, 4 waves as 2 (M) x 2 (N), each 32 x 64
// (2 x 4 accumulators); K in 64-deep tiles staged global -> LDS by LDS-DMA into gemm.hip's XOR-swizzled image (16-B
// chunk c of row r at chunk c ^ ((r >> 1) & 7)), a ring of 24-KiB K-tile buffers with all but one of them in flight
// behind a counted vmcnt and one raw barrier per K-tile (these launches have about one workgroup per CU, so the depth of
// the DMA stream, not the occupancy, has to cover the memory latency; the 8-phase persistent schedule needs a
// 256 x 256 tile per CU, which is what these shapes do not have). A 128-column head lies inside one workgroup.
//   * split == 1, gemm_sm_kernel<epi, false>: one pass, no workspace. Every output element is gemm_nt_8ph's MFMA chain:
//     32-deep steps in ascending K into one accumulator, lane group fg holding k = 8 fg .. 8 fg + 7 of each step; the
//     epilogues are cp25_common.h's pieces in gemm.hip's order. Bit-identical to cp25_gemm_* on any data, any K / 64
//     parity (HNORM and QKV included: this kernel has one form for both parities).
//   * split == S > 1: gemm_sm_kernel<NONE, true> runs S x the workgroups, run r of a tile accumulating K-tiles
//     [run_begin(r), run_begin(r) + run_len(r)) (gemm_route.h) as above and writing its fp32 sums to workspace
//     [r][M][N] with ordinary 16-B vector stores; gemm_sm_reduce<epi> then adds an element's S sums in ascending run
//     order in fp32, rounds once to bf16 and applies the epilogue once. The order is fixed by construction (no atomics,
//     no arrival order): bits depend on S, not on M, the CU count or timing.
// Rows are independent of M in both forms (a row's tile position only selects which workgroup computes it).
#include "cp25_common.h"
#include "gemm_route.h"

#include <algorithm>
#include <cstdlib>

#pragma clang fp contract(off)

namespace {

using namespace cp25gemm;

constexpr int kATile = kSmBM * kSmBK * 2;  // 8 KiB
constexpr int kWTile = kSmBN * kSmBK * 2;  // 16 KiB
constexpr int kStage = kATile + kWTile;    // 24 KiB per K-tile; the epilogue's C tile (bf16 16 KiB / fp32 32 KiB) reuses them
constexpr int kLoadsPerTile = 6;           // LDS-DMA instructions per thread and K-tile: 2 A pieces + 4 W pieces
static_assert(kSmBM * kSmBN * 4 <= 2 * kStage, "the fp32 partial tile is staged through the K-tile buffers");
static_assert(kSmBN == 128, "one head (128 columns) per workgroup: the HNORM / QKV epilogues");

typedef __attribute__((address_space(3))) void* lds_void_ptr;

// the epilogue operands (gemm.hip's ResEpi): CP25_EPI_RES x / gate by token-major row, CP25_EPI_HNORM / _QKV norm
// weight, eps, scale, RoPE tables and the k column range
struct SmEpi {
  const unsigned short* x; int64_t x_st, x_sb;
  const unsigned short* gate; int64_t g_sb, g_st;
  int B; int64_t tok0, hw;
  const unsigned short* nw; float n_eps, n_scale;
  const float* rcos; const float* rsin; int n_lo, n_hi;
};

__device__ __forceinline__ void glds16(const void* src, lds_void_ptr dst) {
  __builtin_amdgcn_global_load_lds(src, dst, 16, 0, 0);
}

// wait until at most n K-tiles of this thread's LDS-DMA are still in flight (the VM counter retires in order)
__device__ __forceinline__ void wait_tiles_in_flight(int n) {
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(18)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); break;
  }
}
static_assert(kLoadsPerTile == 6, "wait_tiles_in_flight counts 6 loads per K-tile");

// The epilogue of one item: v = the 8 bf16 products of row `row` (< M), columns [col, col + 8); li = (col / 8) % 16 is
// the item's place in its 128-column head, whose 16 items sit in 16 consecutive lanes (all of them active here).
// gemm_nt_8ph's arithmetic per epilogue, from the same pieces (gelu_erf, res8, hn_*), in the same order.
template <int kEpi>
__device__ __forceinline__ u32x4 epi_item(u32x4 v, int row, int col, int li, const SmEpi& re) {
  if constexpr (kEpi == CP25_EPI_GELU) {
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      o[w] = (unsigned)f2bf(gelu_erf(bf2f((unsigned short)(v[w] & 0xffffu)))) |
             ((unsigned)f2bf(gelu_erf(bf2f((unsigned short)(v[w] >> 16)))) << 16);
    return o;
  } else if constexpr (kEpi == CP25_EPI_RES) {
    const int tok = row / re.B, b = row % re.B;
    const int64_t frame = (re.tok0 + tok) / re.hw;
    const u32x4 xv = *reinterpret_cast<const u32x4*>(re.x + (int64_t)tok * re.x_st + b * re.x_sb + col);
    const u32x4 gv = *reinterpret_cast<const u32x4*>(re.gate + b * re.g_sb + frame * re.g_st + col);
    return res8(v, xv, gv);
  } else if constexpr (kEpi == CP25_EPI_HNORM || kEpi == CP25_EPI_QKV) {
    const u32x4 nwv = *reinterpret_cast<const u32x4*>(re.nw + li * 8);
    float f[8];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      f[2 * w] = bf2f((unsigned short)(v[w] & 0xffffu));
      f[2 * w + 1] = bf2f((unsigned short)(v[w] >> 16));
    }
    float ss = hn_sumsq8(f);
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 16);
    const float rstd = hn_rstd(ss, re.n_eps);
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] = hn_norm(f[e], rstd, bf2f((unsigned short)(nwv[e >> 1] >> (16 * (e & 1)))));
    if constexpr (kEpi == CP25_EPI_QKV) {
      if (re.rcos != nullptr) {  // launch-uniform
        const int dlo = (li & 7) * 8;
        const float sgn = li < 8 ? -1.f : 1.f;
        const float* cp = re.rcos + (int64_t)(row / re.B) * 64 + dlo;
        const float* sp = re.rsin + (int64_t)(row / re.B) * 64 + dlo;
        const f32x4 c0 = *reinterpret_cast<const f32x4*>(cp), c1 = *reinterpret_cast<const f32x4*>(cp + 4);
        const f32x4 s0 = *reinterpret_cast<const f32x4*>(sp), s1 = *reinterpret_cast<const f32x4*>(sp + 4);
        float partner[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) partner[e] = __shfl_xor(f[e], 8, 16);
#pragma unroll
        for (int e = 0; e < 8; ++e)
          f[e] = hn_rope(f[e], partner[e], sgn, e < 4 ? c0[e & 3] : c1[e & 3], e < 4 ? s0[e & 3] : s1[e & 3]);
      }
    }
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      o[w] = (unsigned)f2bf(f[2 * w] * re.n_scale) | ((unsigned)f2bf(f[2 * w + 1] * re.n_scale) << 16);
    if constexpr (kEpi == CP25_EPI_QKV) {
      // q and v heads pass through (the whole head decides: uniform over its 16 lanes, so the shuffles above ran
      // with every lane of the group)
      const int head0 = col - li * 8;
      if (head0 < re.n_lo || head0 >= re.n_hi) o = v;
    }
    return o;
  } else {
    return v;
  }
}

// kPartial = false: the exact form (split 1). kPartial = true: run blockIdx-derived r of S, fp32 sums to ws[r][M][N].
// kStages K-tile buffers, kStages - 1 K-tiles of LDS-DMA in flight: with about one workgroup per CU (what these shapes
// give) it is the depth of this stream, not the occupancy, that covers the memory latency.
template <int kEpi, bool kPartial, int kStages>
__global__ void __launch_bounds__(kSmThreads)
gemm_sm_kernel(const unsigned short* __restrict__ A, int64_t lda, const unsigned short* __restrict__ W, int64_t ldw,
               unsigned short* __restrict__ C, int64_t ldc, float* __restrict__ ws, int M, int N, int K, int S, SmEpi re) {
  static_assert(kStages >= 2 && kStages <= 6, "2 .. 6 K-tile buffers (wait_tiles_in_flight covers 0 .. 4 in flight)");
  __shared__ __attribute__((aligned(16))) char smem[kStages * kStage];

  // tile order: the row tiles of one (column tile, run) are neighbours, so the workgroups of an XCD share a W slab
  const int mt = (M + kSmBM - 1) / kSmBM;
  const int logical = xcd_remap(blockIdx.x, gridDim.x);
  const int m0 = (logical % mt) * kSmBM;
  const int rest = logical / mt;
  const int run = kPartial ? rest % S : 0;
  const int n0 = (kPartial ? rest / S : rest) * kSmBN;
  const int nk = K / kSmBK;
  const int kb = kPartial ? run_begin(nk, S, run) : 0;
  const int ke = kPartial ? kb + run_len(nk, S, run) : nk;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;

  // ---- LDS-DMA staging: a piece = 8 rows x 128 B per wave instruction; wave w fills A pieces 2w, 2w+1 and W pieces
  // 4w .. 4w+3. Lane l writes LDS bytes [16 l, 16 l + 16) of the piece = row l / 8, chunk position l % 8, and loads
  // global chunk (l % 8) ^ swz(row): the swizzle is on the source side. Rows past M re-read row M - 1 (never stored).
  const int prow = lane >> 3, ppos = lane & 7;
  const unsigned short* a_src[2];
  const unsigned short* w_src[4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int r = (wave * 2 + j) * 8 + prow;
    a_src[j] = A + (int64_t)min(m0 + r, M - 1) * lda + (ppos ^ ((r >> 1) & 7)) * 8;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int r = (wave * 4 + j) * 8 + prow;
    w_src[j] = W + (int64_t)(n0 + r) * ldw + (ppos ^ ((r >> 1) & 7)) * 8;
  }
  auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
    char* sa = smem + buf * kStage;
    char* sw = sa + kATile;
#pragma unroll
    for (int j = 0; j < 2; ++j) glds16(a_src[j] + kt * kSmBK, (lds_void_ptr)(sa + (wave * 2 + j) * 1024));
#pragma unroll
    for (int j = 0; j < 4; ++j) glds16(w_src[j] + kt * kSmBK, (lds_void_ptr)(sw + (wave * 4 + j) * 1024));
  };

  // ---- fragment reads: lane (fr = l % 16, fg = l / 16) reads row fr, k-chunk 4 s + fg of 32-deep step s (the
  // 16x16x32 operand layout: k = 8 fg .. 8 fg + 7 of the step); fragment rows start at multiples of 16
  const int fr = lane & 15, fg = lane >> 4;
  int f_off[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) f_off[s] = fr * 128 + 16 * ((4 * s + fg) ^ ((fr >> 1) & 7));

  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // K-tile t of the run lives in buffer (t - kb) % kStages. Iteration kt: [counted vmcnt: this thread's part of K-tile
  // kt has landed; lgkmcnt(0): its reads of K-tile kt - 1 are done] raw barrier [every wave's part has landed, and
  // the buffer of K-tile kt - 1 is free] issue K-tile kt + kStages - 1 into that buffer; read and multiply K-tile kt.
  // Raw s_barrier: a __syncthreads() fence would drain the DMA with vmcnt(0). All LDS is one array.
#pragma unroll
  for (int p = 0; p < kStages - 1; ++p)
    if (kb + p < ke) issue(kb + p, p);
  int buf = 0;
  for (int kt = kb; kt < ke; ++kt) {
    wait_tiles_in_flight(min(kStages - 2, ke - 1 - kt));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    if (kt + kStages - 1 < ke) issue(kt + kStages - 1, buf == 0 ? kStages - 1 : buf - 1);
    const char* sa = smem + buf * kStage + wm * 32 * 128;
    const char* sw = smem + buf * kStage + kATile + wn * 64 * 128;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8 af[2], wf[4];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = *reinterpret_cast<const bf16x8*>(sa + i * 16 * 128 + f_off[s]);
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(sw + j * 16 * 128 + f_off[s]);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], wf[j], acc[i][j], 0, 0, 0);
    }
    buf = buf + 1 == kStages ? 0 : buf + 1;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();  // every wave is done reading the last K-tile; no DMA is in flight

  // ---- the tile through the LDS (no DMA in flight, every wave past its last read): accumulator (i, j) register r is
  // row wm 32 + 16 i + 4 fg + r, column wn 64 + 16 j + fr
  if constexpr (kPartial) {
    float* st = reinterpret_cast<float*>(smem);  // [64][128] fp32
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[(wm * 32 + 16 * i + 4 * fg + r) * kSmBN + wn * 64 + 16 * j + fr] = acc[i][j][r];
    __syncthreads();
    float* dst = ws + ((int64_t)run * M + m0) * N + n0;
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int idx = it * kSmThreads + tid;  // 64 rows x 32 chunks of 16 B
      const int r = idx >> 5, c4 = idx & 31;
      if (m0 + r < M)
        *reinterpret_cast<f32x4*>(dst + (int64_t)r * N + c4 * 4) = *reinterpret_cast<const f32x4*>(st + r * kSmBN + c4 * 4);
    }
  } else {
    unsigned short* st = reinterpret_cast<unsigned short*>(smem);  // [64][128] bf16
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          st[(wm * 32 + 16 * i + 4 * fg + r) * kSmBN + wn * 64 + 16 * j + fr] = f2bf(acc[i][j][r]);
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = it * kSmThreads + tid;  // 64 rows x 16 items: a head's 16 items in 16 consecutive lanes
      const int r = idx >> 4, li = idx & 15;
      const u32x4 v = *reinterpret_cast<const u32x4*>(st + r * kSmBN + li * 8);
      const u32x4 o = epi_item<kEpi>(v, min(m0 + r, M - 1), n0 + li * 8, li, re);
      if (m0 + r < M) *reinterpret_cast<u32x4*>(C + (int64_t)(m0 + r) * ldc + n0 + li * 8) = o;
    }
  }
}

// The split form's second pass: item (row, 8 columns) adds its S partial sums in ascending run order in fp32, rounds
// once to bf16 and applies the epilogue. N % 128 == 0: a head's 16 items are 16 consecutive, aligned threads.
template <int kEpi>
__global__ void __launch_bounds__(kSmThreads)
gemm_sm_reduce(const float* __restrict__ ws, unsigned short* __restrict__ C, int64_t ldc, int M, int N, int S, SmEpi re) {
  const int nch = N / 8;
  const int64_t idx = (int64_t)blockIdx.x * kSmThreads + threadIdx.x;
  const int row_raw = (int)(idx / nch), ch = (int)(idx % nch);
  const int row = min(row_raw, M - 1);  // threads past the end (whole heads of them) redo the last row, unstored
  const float* p = ws + (int64_t)row * N + ch * 8;
  f32x4 s0 = *reinterpret_cast<const f32x4*>(p), s1 = *reinterpret_cast<const f32x4*>(p + 4);
  for (int r = 1; r < S; ++r) {
    p += (int64_t)M * N;
    const f32x4 t0 = *reinterpret_cast<const f32x4*>(p), t1 = *reinterpret_cast<const f32x4*>(p + 4);
    s0 += t0;
    s1 += t1;
  }
  u32x4 v;
  v[0] = (unsigned)f2bf(s0[0]) | ((unsigned)f2bf(s0[1]) << 16);
  v[1] = (unsigned)f2bf(s0[2]) | ((unsigned)f2bf(s0[3]) << 16);
  v[2] = (unsigned)f2bf(s1[0]) | ((unsigned)f2bf(s1[1]) << 16);
  v[3] = (unsigned)f2bf(s1[2]) | ((unsigned)f2bf(s1[3]) << 16);
  const u32x4 o = epi_item<kEpi>(v, row, ch * 8, ch & 15, re);
  if (row_raw < M) *reinterpret_cast<u32x4*>(C + (int64_t)row * ldc + ch * 8) = o;
}

int device_cus() {  // the current device's CU count, or 256 without one
  static int n_cu[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (!n_cu[dev] && hipDeviceGetAttribute(&n_cu[dev], hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) {
    n_cu[dev] = 0;
    return 256;
  }
  return n_cu[dev] > 0 ? n_cu[dev] : 256;
}

// K-tile buffers per workgroup. CP25_GEMM_SM_STAGES (3, 4 or 6; a lab switch, read per launch) overrides the
// default for A/B runs (tools/bench_gemm_small.py --stages): tile order and arithmetic do not depend on it.
constexpr int kDefaultStages = 3;  // measured: 3 (two workgroups per CU) <= 4 <= 6 at every shape and split
int stages_now() {
  const char* e = getenv("CP25_GEMM_SM_STAGES");
  const int v = e ? atoi(e) : kDefaultStages;
  return v == 3 || v == 4 || v == 6 ? v : kDefaultStages;
}

template <int kEpi, bool kPartial>
void launch_gemm(int stages, dim3 grid, hipStream_t stream, const unsigned short* A, int64_t lda, const unsigned short* Wp,
                 int64_t ldw, unsigned short* Cp, int64_t ldc, float* ws, int M, int N, int K, int S, const SmEpi& re) {
  const dim3 block(kSmThreads);
  if (stages == 6)
    hipLaunchKernelGGL((gemm_sm_kernel<kEpi, kPartial, 6>), grid, block, 0, stream, A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re);
  else if (stages == 4)
    hipLaunchKernelGGL((gemm_sm_kernel<kEpi, kPartial, 4>), grid, block, 0, stream, A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re);
  else
    hipLaunchKernelGGL((gemm_sm_kernel<kEpi, kPartial, 3>), grid, block, 0, stream, A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re);
}

template <int kEpi>
void launch_pair(const unsigned short* A, int64_t lda, const unsigned short* Wp, int64_t ldw, unsigned short* Cp,
                 int64_t ldc, float* ws, int M, int N, int K, int S, const SmEpi& re, hipStream_t stream) {
  const unsigned tiles = (unsigned)(ceil_div(M, kSmBM) * (N / kSmBN));
  const int stages = stages_now();
  if (S == 1) {
    launch_gemm<kEpi, false>(stages, dim3(tiles), stream, A, lda, Wp, ldw, Cp, ldc, nullptr, M, N, K, 1, re);
  } else {
    launch_gemm<CP25_EPI_NONE, true>(stages, dim3(tiles * S), stream, A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re);
    const unsigned items = (unsigned)ceil_div((int64_t)M * (N / 8), kSmThreads);
    hipLaunchKernelGGL((gemm_sm_reduce<kEpi>), dim3(items), dim3(kSmThreads), 0, stream, (const float*)ws, Cp, ldc, M, N,
                       S, re);
  }
}

int sm_launch(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M, int N, int K,
              int epilogue, const SmEpi& re, int split, void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  // cp25_gemm_*'s checks (gemm.hip, gemm_launch), without its K / 64 parity limit
  if (!a || !w || !c || M <= 0 || N <= 0 || K <= 0) return CP25_ERR_INVAL;
  if (N % 256 != 0 || K % kSmBK != 0) return CP25_ERR_DTYPE;
  if (lda < K || ldw < K || ldc < N || (lda % 8) || (ldw % 8) || (ldc % 8)) return CP25_ERR_INVAL;
  if (lda >= (1 << 22) || ldw >= (1 << 22)) return CP25_ERR_INVAL;
  if (((uintptr_t)a | (uintptr_t)w | (uintptr_t)c) & 15) return CP25_ERR_INVAL;
  if (epilogue < CP25_EPI_NONE || epilogue > CP25_EPI_QKV) return CP25_ERR_INVAL;
  if (epilogue == CP25_EPI_QKV) {
    if (re.B <= 0 || re.n_lo < 0 || re.n_hi > N || re.n_lo % 256 || re.n_hi % 256 || re.n_lo >= re.n_hi ||
        (!re.rcos) != (!re.rsin) || (((uintptr_t)re.rcos | (uintptr_t)re.rsin) & 15))
      return CP25_ERR_INVAL;
  }
  if (epilogue == CP25_EPI_HNORM || epilogue == CP25_EPI_QKV) {
    if (!re.nw || ((uintptr_t)re.nw & 15) || !(re.n_eps >= 0.f) || !(re.n_scale > 0.f)) return CP25_ERR_INVAL;
  }
  if (epilogue == CP25_EPI_RES) {
    if (!re.x || !re.gate || re.B <= 0 || 16 % re.B || re.hw < 16 / re.B || re.tok0 < 0 || (re.x_st % 8) || (re.x_sb % 8) ||
        (re.g_sb % 8) || (re.g_st % 8) || (((uintptr_t)re.x | (uintptr_t)re.gate) & 15))
      return CP25_ERR_INVAL;
    if ((int64_t)(M - 1) / re.B * re.x_st >= (1ll << 40)) return CP25_ERR_INVAL;
  }
  if (split < 0) return CP25_ERR_INVAL;
  const int S = split == 0 ? gemm_plan(M, N, K, epilogue, device_cus()).split : split;
  if (S > K / kSmBK || S > kMaxSplit) return CP25_ERR_INVAL;
  if (small_blocks(M, N, S) > 0x7fffffff || ceil_div((int64_t)M * (N / 8), kSmThreads) > 0x7fffffff) return CP25_ERR_INVAL;
  if (S > 1) {
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < workspace_bytes_of(M, N, K, S))
      return CP25_ERR_INVAL;
  }
  const unsigned short* A = (const unsigned short*)a;
  const unsigned short* Wp = (const unsigned short*)w;
  unsigned short* Cp = (unsigned short*)c;
  float* ws = (float*)workspace;
  switch (epilogue) {
    case CP25_EPI_GELU: launch_pair<CP25_EPI_GELU>(A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re, stream); break;
    case CP25_EPI_RES: launch_pair<CP25_EPI_RES>(A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re, stream); break;
    case CP25_EPI_HNORM: launch_pair<CP25_EPI_HNORM>(A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re, stream); break;
    case CP25_EPI_QKV: launch_pair<CP25_EPI_QKV>(A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re, stream); break;
    default: launch_pair<CP25_EPI_NONE>(A, lda, Wp, ldw, Cp, ldc, ws, M, N, K, S, re, stream);
  }
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

}  // namespace

extern "C" int cp25_gemm_sm_plan(int M, int N, int K, int epilogue, int cus) {
  if (M <= 0 || N <= 0 || K <= 0 || cus < 0 || epilogue < CP25_EPI_NONE || epilogue > CP25_EPI_QKV) return CP25_ERR_INVAL;
  if (N % 256 != 0 || K % kSmBK != 0) return CP25_ERR_DTYPE;
  return pack_plan(gemm_plan(M, N, K, epilogue, cus > 0 ? cus : device_cus()));
}

extern "C" int64_t cp25_gemm_sm_workspace_bytes(int M, int N, int K, int split) {
  return workspace_bytes_of(M, N, K, split);
}

extern "C" int cp25_gemm_sm_epi(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M,
                                int N, int K, int epilogue, int split, void* workspace, int64_t workspace_bytes,
                                hipStream_t stream) {
  if (epilogue == CP25_EPI_RES || epilogue == CP25_EPI_HNORM || epilogue == CP25_EPI_QKV)
    return CP25_ERR_INVAL;  // their operands: _res / _hnorm / _qkv
  const SmEpi re{};
  return sm_launch(a, lda, w, ldw, c, ldc, M, N, K, epilogue, re, split, workspace, workspace_bytes, stream);
}

extern "C" int cp25_gemm_sm_res(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M,
                                int N, int K, const void* x, int64_t x_st, int64_t x_sb, const void* gate, int64_t g_sb,
                                int64_t g_st, int B, int64_t tok0, int64_t hw, int split, void* workspace,
                                int64_t workspace_bytes, hipStream_t stream) {
  const SmEpi re{(const unsigned short*)x, x_st, x_sb, (const unsigned short*)gate, g_sb, g_st, B, tok0, hw};
  return sm_launch(a, lda, w, ldw, c, ldc, M, N, K, CP25_EPI_RES, re, split, workspace, workspace_bytes, stream);
}

extern "C" int cp25_gemm_sm_hnorm(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M,
                                  int N, int K, const void* norm_weight, float eps, float out_scale, int split,
                                  void* workspace, int64_t workspace_bytes, hipStream_t stream) {
  SmEpi re{};
  re.nw = (const unsigned short*)norm_weight;
  re.n_eps = eps;
  re.n_scale = out_scale;
  return sm_launch(a, lda, w, ldw, c, ldc, M, N, K, CP25_EPI_HNORM, re, split, workspace, workspace_bytes, stream);
}

extern "C" int cp25_gemm_sm_qkv(const void* a, int64_t lda, const void* w, int64_t ldw, void* c, int64_t ldc, int M,
                                int N, int K, int k_col0, int k_cols, const void* k_norm_weight, const float* cos_tab,
                                const float* sin_tab, int B, float eps, int split, void* workspace,
                                int64_t workspace_bytes, hipStream_t stream) {
  SmEpi re{};
  re.nw = (const unsigned short*)k_norm_weight;
  re.n_eps = eps;
  re.n_scale = 1.f;
  re.rcos = cos_tab;
  re.rsin = sin_tab;
  re.B = B;
  re.n_lo = k_col0;
  re.n_hi = k_col0 + k_cols;
  return sm_launch(a, lda, w, ldw, c, ldc, M, N, K, CP25_EPI_QKV, re, split, workspace, workspace_bytes, stream);
}
