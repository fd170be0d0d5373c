// The host-side plan of a small-M block GEMM launch (gemm_small.hip), once: whether the small family runs the shape at
// all, its output tile, and the K split S. Plain C++17 with no HIP in it, so a host compiler alone builds and tests it
// (tests/host/gemm_route_main.cpp); the CU count is a parameter. gemm_small.hip's launch and the C entry points
// (cp25_gemm_sm_plan, cp25_gemm_sm_workspace_bytes) both take the plan from here.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace cp25gemm {

constexpr int kSmBM = 64, kSmBN = 128, kSmBK = 64;  // the small family's output tile and K-tile
constexpr int kSmThreads = 256;                     // 4 waves as 2 (M) x 2 (N), 32 x 64 each
constexpr int kMaxSplit = 64;                       // packed into 8 bits below; K / 64 bounds it first in practice

// epilogue codes of include/cp25.h (CP25_EPI_*), restated so that the header stays HIP-free
constexpr int kEpiNone = 0, kEpiGelu = 1, kEpiRes = 2, kEpiHnorm = 3, kEpiQkv = 4;

// The thresholds, from the per-shape measurement of profiles/r14/small_gemm/SUMMARY.md (one MI355X, 256 CUs; the 2B
// net's four launch shapes at 320 and 1200 rows against gemm_nt_8ph, weights streamed from HBM):
//   * the small family won (by 1.5 - 3.3 x) every launch of up to 320 workgroups at split 1 and lost (by 9 - 13 %) the
//     two of 912 and 1216: it runs a shape while its unsplit launch is at most one co-resident round of workgroups,
//     kSmBlocksPerCu per CU (its 72 KiB of LDS admit two). Nothing between 320 and 912 workgroups was measured.
//   * a K split paid only where the unsplit launch left more than half of the CUs without a workgroup (80 workgroups:
//     N = 2048 at 320 rows), and then with runs of 16 K-tiles: S = 2 at K = 2048 (15.8 against 18.8 us), S = 8 at
//     K = 8192 (32.3 against 59.4 us; S = 4: 33.3); at 240 - 320 workgroups every split measured slower than none.
constexpr int kSmBlocksPerCu = 2;
constexpr int kSplitMinRunTiles = 16;  // K-tiles per run, at least
constexpr int kSplitMax = 8;           // runs, at most

struct GemmPlan {
  bool small;  // the small family runs this shape (false: gemm_nt_8ph's 256 x 256 tiles)
  int bm, bn;  // output tile of the small family
  int split;   // S >= 1: K is cut into S contiguous runs of whole K-tiles
};

constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

constexpr bool shape_ok(int M, int N, int K) { return M > 0 && N > 0 && K > 0 && N % 256 == 0 && K % kSmBK == 0; }

// K-tiles [begin, begin + len) of run r of S over nk K-tiles: the first nk % S runs are one tile longer
constexpr int run_begin(int nk, int S, int r) { return r * (nk / S) + (r < nk % S ? r : nk % S); }
constexpr int run_len(int nk, int S, int r) { return nk / S + (r < nk % S ? 1 : 0); }

// workgroups of the small family's launch at split S
constexpr int64_t small_blocks(int M, int N, int S) { return ceil_div(M, kSmBM) * (N / kSmBN) * S; }

// The plan's S: 1 unless the unsplit launch leaves more than half of the CUs idle; then the largest power of two up to
// kSplitMax whose runs keep kSplitMinRunTiles K-tiles. The epilogue does not enter: the four measured shapes carry the
// QKV, residual and GELU epilogues, and the choice followed the workgroup count and K alone; it stays in the signature
// for a measurement that separates them.
inline int split_of(int M, int N, int K, int epilogue, int cus) {
  (void)epilogue;
  if (2 * small_blocks(M, N, 1) > cus) return 1;
  const int nk = K / kSmBK;
  int S = 1;
  while (2 * S <= kSplitMax && nk / (2 * S) >= kSplitMinRunTiles) S *= 2;
  return S;
}

inline GemmPlan gemm_plan(int M, int N, int K, int epilogue, int cus) {
  GemmPlan p{false, kSmBM, kSmBN, 1};
  if (!shape_ok(M, N, K) || cus <= 0 || epilogue < kEpiNone || epilogue > kEpiQkv) return p;
  p.small = small_blocks(M, N, 1) <= (int64_t)kSmBlocksPerCu * cus;
  if (p.small) p.split = split_of(M, N, K, epilogue, cus);
  return p;
}

// bit 0: small; bits 8-15: S; bits 16-23: bm / 16; bits 24-30: bn / 16
inline int pack_plan(const GemmPlan& p) {
  return (p.small ? 1 : 0) | (p.split << 8) | ((p.bm / 16) << 16) | ((p.bn / 16) << 24);
}

// bytes of the fp32 partial sums [S][M][N] of a split launch; 0 for S <= 1 (the exact form needs no workspace)
inline int64_t workspace_bytes_of(int M, int N, int K, int split) {
  if (!shape_ok(M, N, K) || split <= 1 || split > K / kSmBK) return 0;
  return (int64_t)split * M * N * 4;
}

}  // namespace cp25gemm
