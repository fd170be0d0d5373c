// attn_fwd_wq (round 13): the DiT's long-key self-attention with ONE wave per SIMD and 16 kNQ query rows per wave,
// 64 kNQ per workgroup (kNQ = 5: 320 rows, kNQ = 6: 384), gfx950, bf16 in / out, head dim 128. Replaces the same
// reference op as attn_fwd_m16 (attn_fwd.hip): cosmos_predict2/_src/predict2/networks/attention.py:90-181,
// softmax(Q K^T / sqrt(D)) V, no mask, non-causal.
//
// Why: every workgroup streams the whole K and V of its (b, h) from the L2 into the LDS once, so the
// staging traffic of a launch is (Lq / R) Lk 512 B per (b, h) for R query rows per workgroup, and that traffic's energy
// is what sets the power-limited clock of the loop (profiles/r6/w64/SUMMARY.md). attn_fwd_m16 has R = 256; here R = 320
// or 384, and every K / V fragment read from the LDS feeds kNQ MFMAs instead of two.
//
// Arithmetic: every output element is the same MFMA chains, in the same order, on the same operands as attn_fwd_m16
// (v_mfma_f32_16x16x32_bf16: S^T = K Q^T over the d steps s = 0..3 with the row's shift as the initial C; O^T += V^T P^T
// over the key steps in key order; row sums by MFMA on an all-ones V^T row over the bf16 P; the same v_exp_f32, bf16
// pack, in-kernel q RMSNorm + RoPE + prescale, fixed-shift rule floor(min(b_row + kPDrop, 126 - b_row)), split partials
// and lse), so the outputs are bit-identical (tests/test_attn_wide_gpu.py). Zero shift (kMode 1) and fixed shift
// (kMode 0) only: the online max, the gated pair, the fp8 forms and the cross-attention stay on attn_fwd_m16.
//
// Registers (one wave per SIMD: 256 VGPRs + 256 AGPRs per lane). "a"-constrained asm operands, which the compiler keeps
// in the accumulator file and never touches between the asm MFMAs: O^T[16 db + 4 g + i][16 qb + c] (oacc[db][qb], 32 kNQ),
// the row sums (lacc[qb], 4 kNQ), the all-ones operand (4) and the Q fragments of the first kQA query blocks (16 each:
// what is left of 256). The other Q blocks, the shifts (minit, 4 kNQ) and the pipeline's S / P live in arch VGPRs.
//
// The in-wave software pipeline runs on 32-key HALF stages (with 64-key stages S^T and P^T of two stages are 48 kNQ
// registers, which does not fit): S^T of two half stages is 16 kNQ, P^T of two is 8 kNQ. Half stage u (keys 32 u ..
// 32 u + 31 of the workgroup's key range) has, in its MFMA stream, the row sums of P(u - 1) (kNQ), P.V(u - 1) (8 V^T
// fragments x kNQ) and Q K^T(u + 1) (2 key blocks x 4 d steps x kNQ), and in the issue gaps between them the softmax of
// S(u) (per query block 8 v_exp_f32 and 4 bf16 packs: 12 kNQ instructions, placed by the compile-time gap plan below),
// the operand reads two fragments ahead (a ring of three) and the LDS-DMA pieces.
//
// The LDS image of a 64-key K or V tile is attn_wq_image.h's (round 18): plain 256-B rows, four to a 1-KiB DMA piece,
// the pieces 1056 B apart, so that row r starts 32 (r & 7) bytes into the 256-B bank window as in attn_fwd_m16's
// 288-B rows (the same conflict-free ds_read_b128 K reads and ds_read_b64_tr_b16 V reads, one base register each),
// but a tile is 16 pieces instead of 18 and no DMA lane fetches padding: every wave moves four pieces of every image.
// A buffer is TWO such images back to back, two buffers each of K and V (135 168 B), and there is ONE buffer flip,
// DMA batch, vmcnt(0) drain and workgroup barrier per 128 keys (round 17; round 13 had one per 64). Iteration t is the
// four half stages u = 4 t + 1 .. 4 t + 4:
// stage st reads V(2 t + (st >> 1)) (key step st & 1) and K(2 t + 1 + (st >> 1)) (key blocks 2 (st & 1), + 1) and
// nothing else, so K's buffers are cut one tile later than V's: iteration t reads the K buffer {K(2 t + 1), K(2 t + 2)}
// and the V buffer {V(2 t), V(2 t + 1)}, and the 16 DMA pieces a wave moves (8 of K(2 t + 3), K(2 t + 4), 8 of
// V(2 t + 2), V(2 t + 3)) go to the two buffers the previous iteration read. Each wave drains its pieces (vmcnt(0))
// before the closing barrier, which publishes them. The DMA is the bounds-checked buffer form: rows past the last key
// read as zeros, so the ragged tile and the virtual tiles past it need no path of their own; scores of keys >= Lk
// are set to -inf before their softmax (P = 0 exactly), per half stage.
//
// Prologue: K(0) (as the last image of K buffer 1), K(1), K(2), V(0), V(1) by DMA, then "iteration -1" of two stages
// without P.V and without the first softmax: Q K^T(0), softmax S(0), Q K^T(1). The loop then runs ceil(ntk / 2)
// iterations. Its last Q K^T and softmax work on a virtual tile no one reads, and with an odd tile count its last two
// stages on a virtual V tile too: P = 0 exactly on zero V rows, which adds +0 to O^T and to the row sums.
#include "attn_common.h"
#include "attn_wq_image.h"

namespace cp25attn {
namespace {

constexpr int kAheadWq = 2;             // operand fragments read ahead of their MFMAs
constexpr int kRingWq = kAheadWq + 1;
static_assert(kWqThreads == 4 * 64, "one wave per SIMD");

// ---- the gap plan of one half stage: 17 kNQ MFMA slots. Slot m < kNQ: the row sum of query block m; then fragment
// f = (m - kNQ) / kNQ (0-7: V^T block db = f of P.V; 8-15: K fragment j = f - 8, key block j & 1, d step j >> 1) x query
// block (m - kNQ) % kNQ. A fragment's first MFMA is its "read gap": the reads of the fragment kAheadWq later follow
// it, and DMA slot d rides in the read gap of the iteration's fragment d, its M0 set in the gap before. The softmax's
// 12 kNQ instructions (per query block e0 e1 c0 e2 e3 c1 e4 e5 c2 e6 e7 c3) take the other gaps in slot order. One
// v_exp fills a gap's issue slots (8 of the MFMA's 16 cycles).
constexpr int wq_stage(int nq) { return 17 * nq; }
constexpr int wq_frag(int nq, int m) { return m < nq ? -1 : (m - nq) / nq; }
constexpr int wq_qb(int nq, int m) { return m < nq ? m : (m - nq) % nq; }
constexpr bool wq_read_gap(int nq, int m) { return m >= nq && (m - nq) % nq == 0; }
constexpr int wq_sm_op(int nq, int m) {  // the softmax instruction in the gap after stage slot m, or -1
  if (wq_read_gap(nq, m)) return -1;
  int idx = 0;
  for (int x = 0; x < m; ++x) idx += !wq_read_gap(nq, x);
  return idx < 12 * nq ? idx : -1;
}
constexpr int wq_sm_count(int nq) {
  int n = 0;
  for (int m = 0; m < wq_stage(nq); ++m) n += wq_sm_op(nq, m) >= 0;
  return n;
}
static_assert(wq_sm_count(5) == 60 && wq_sm_count(6) == 72, "every softmax instruction has a gap");
// 64-key tiles per loop iteration (one buffer flip, one DMA batch, one vmcnt(0) drain and one workgroup barrier each):
// two, so the LDS holds two buffers of two 64-key images each for K and for V. -DCP25_WQ_PARENT_LOOP (tools/lab
// only, never libcp25.so) rebuilds round 13's loop for A/B runs: one tile per iteration, the fifth DMA piece on
// waves 0-1 alone.
// -DCP25_WQ_PAD_IMAGE (lab only) keeps round 17's image for A/B runs: attn_fwd_m16's 64 rows of 288 B, 18 pieces a
// tile, the padding lanes re-reading the tile's first 16 B, pieces 16-17 of the two images of a buffer on waves 0-1 and
// 2-3 (the parent loop implies it).
// -DCP25_WQ_HEAD_RSRC (lab only) computes the tile descriptors at the head of the iteration, behind the barrier, as
// rounds 13 and 17 did; the product makes them by adds in the last gaps of the iteration before, under MFMAs (round
// 18: shipped together with the image, profiles/r18/attn_image/SUMMARY.md). The parent loop implies it.
#ifdef CP25_WQ_PARENT_LOOP
#define CP25_WQ_ITER_TILES 1
#ifndef CP25_WQ_PAD_IMAGE
#define CP25_WQ_PAD_IMAGE
#endif
#ifndef CP25_WQ_HEAD_RSRC
#define CP25_WQ_HEAD_RSRC
#endif
#endif
#ifndef CP25_WQ_ITER_TILES
#define CP25_WQ_ITER_TILES 2
#endif
constexpr int wq_iter_tiles(int) { return CP25_WQ_ITER_TILES; }
#ifdef CP25_WQ_PAD_IMAGE
constexpr bool kWqPad = true;
#else
constexpr bool kWqPad = false;
#endif
#ifdef CP25_WQ_HEAD_RSRC
constexpr bool kWqHeadRsrc = true;
#else
constexpr bool kWqHeadRsrc = false;
#endif
static_assert(kKBuf16 == kVBuf16, "K and V images of one size");
constexpr int kWqImg = kWqPad ? kKBuf16 : wqimg::kImage;  // one 64-key image
// a wave's pieces j = 0..3 of an image: LDS byte kWqPieceAt wave + kWqPieceStep j of it
constexpr int kWqPieceAt = kWqPad ? 1024 : wqimg::kPieceStride;
constexpr int kWqPieceStep = 4 * kWqPieceAt;
// lane offsets of a wave per operand: one per piece j, and the pad image's fifth (pieces 16-17)
constexpr int kWqOffs = kWqPad ? 5 : 4;
// DMA slots of a wave per iteration: 4 K + 4 V pieces per tile. The pad image: one tile, 5 K + 5 V pieces (the fifth
// on waves 0-1 only: 18 pieces a tile over 4 waves); two tiles, 9 + 9: pieces 0-15 of both images on every wave, pieces
// 16-17 of image 0 on waves 0-1 and of image 1 on waves 2-3
constexpr int wq_dma_n(int it) { return !kWqPad ? 8 * it : it == 1 ? 10 : 18; }
// DMA slot d (K first, then V) in the gap after iteration slot M, or -1: the read gaps of the iteration's first
// wq_dma_n fragments; its M0 one gap earlier
constexpr int wq_dma_at(int nq, int it, int M) {
  const int st = M / wq_stage(nq), m = M % wq_stage(nq);
  if (st >= 2 * it || !wq_read_gap(nq, m)) return -1;
  const int F = 16 * st + wq_frag(nq, m);
  return F < wq_dma_n(it) ? F : -1;
}
constexpr int wq_m0_at(int nq, int it, int M) { return wq_dma_at(nq, it, M + 1); }

// the bounds-checked buffer descriptor of one K or V tile (rows past the tile's last key read as zero)
__device__ __forceinline__ u32x4 tile_rsrc(const char* base, int64_t sl, int rows) {
  const uint64_t p = (uint64_t)base;
  const unsigned n = rows > 0 ? (unsigned)((rows - 1) * sl * 2 + 2 * kD) : 0u;
  return u32x4{(unsigned)p, (unsigned)(p >> 32) & 0xffffu, n, 0x00020000u};
}

#define WQ_MFMA "v_mfma_f32_16x16x32_bf16 "

template <int kNQ, int kMode, int kTail = 0>
__global__ void __launch_bounds__(kWqThreads, 1) attn_fwd_wq(AttnArgs a) {
  static_assert(kMode == 0 || kMode == 1, "kMode: 0 fixed shift, 1 zero shift");
  static_assert(kNQ >= 4 && kNQ <= 6, "query blocks per wave");
  constexpr int kIT = wq_iter_tiles(kNQ);  // 64-key tiles per iteration
  static_assert(kIT == 1 || kIT == 2, "tiles per iteration");
  constexpr int kBuf = kIT * kWqImg;       // one buffer: kIT images back to back
  constexpr int VB0 = 2 * kBuf;            // K buffers 0, 1, then V buffers 0, 1
  static_assert(4 * kBuf <= 163840, "the CU's LDS");
  __shared__ __attribute__((aligned(16))) char smem[4 * kBuf];
  // the last piece of the last image of the last buffer (wave 3, j = 3) ends inside smem
  static_assert(kWqPad || 3 * kBuf + (kIT - 1) * kWqImg + wqimg::piece_dst(wqimg::wave_piece(3, 3)) +
                                  wqimg::kPieceBytes <= 4 * kBuf,
                "every DMA piece lands inside smem");
  static_assert(kWqPad || (wqimg::piece_dst(wqimg::wave_piece(1, 0)) == kWqPieceAt &&
                           wqimg::piece_dst(wqimg::wave_piece(0, 1)) == kWqPieceStep),
                "a wave's piece destinations: base + step j");
  constexpr bool kInit = kMode != 1;  // the shift rides in the Q K^T chains' initial C
  constexpr int kPar = kIT == 1 ? 1 : 0;  // iteration T reads the K buffer (T + kPar) & 1 and the V buffer T & 1
  constexpr int kND = wq_dma_n(kIT);
  constexpr int kR = kRingWq;
  constexpr int kRowsW = 16 * kNQ;    // query rows per wave
  constexpr int kRowsG = 4 * kRowsW;  // per workgroup
  constexpr int kNS = wq_stage(kNQ);
  // Q blocks whose fragments fit the accumulator file beside O^T, the row sums and the ones operand
  constexpr int kQA = (256 - 36 * kNQ - 4) / 16 < kNQ ? (256 - 36 * kNQ - 4) / 16 : kNQ;

  const int tile = xcd_remap(blockIdx.x, gridDim.x);
  const int qblk = tile % a.nqb;
  const int bhs = tile / a.nqb;
  const int split = bhs % a.nsplit, bh = bhs / a.nsplit;
  const int b = bh / a.H, h = bh % a.H;
  const int key0 = split * a.tps * kKBlk;
  const int Lk = min(a.Lk - key0, a.tps * kKBlk);
  const int ntk = (Lk + kKBlk - 1) / kKBlk;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int c16 = lane & 15;
  const int g = lane >> 4;
  const int row_w = qblk * kRowsG + wave * kRowsW;  // the wave's first query row

  const unsigned short* qp = a.q + b * a.q_sb + h * a.q_sh;
  const char* const kbase = (const char*)(a.k + b * a.k_sb + h * a.k_sh + (int64_t)key0 * a.k_sl);
  const char* const vbase = (const char*)(a.v + b * a.v_sb + h * a.v_sh + (int64_t)key0 * a.v_sl);

  // ---- LDS-DMA: piece P of a 64-key image (16 per image) goes to image byte 1056 P, lane l bringing the 16 B at
  // byte column 16 (l & 15) of the tile's row 32 (P >> 3) + (P & 7) + 8 (l >> 4) (attn_wq_image.h). Every wave moves
  // the pieces wave + 4 j, j = 0..3, of every image: four lane offsets per operand.
  // Bounds-checked buffer loads, checked per lane: rows past the tile's last key (the ragged tile, which may end
  // between the four rows of a piece, and the virtual tiles past Lk) read as zero.
  // The pad image (lab): piece p of 18 is image bytes [1024 p, +1024) of the 64 x 288-B image, lane l the 16 B at 16 l
  // of it: row bb / 288, column bb % 288, attn_fwd_m16's dma_tile; the lanes of the row padding (columns >= 256, which
  // no fragment read touches) re-read the tile's first 16 B. The fifth offset is piece 16 + (wave & 1): of image 0 on
  // waves 0-1 and of image 1 on waves 2-3, so a wave moves 9 pieces of the two images of a buffer (one tile per
  // iteration: piece 16 + wave on waves 0-1).
  const int wave5 = kIT == 1 ? wave : (wave & 1);  // the fifth piece's lane block
  const int img5 = kIT == 1 ? 0 : (wave >> 1);     // and its image
  int dk[kWqOffs], dv[kWqOffs];
#pragma unroll
  for (int j = 0; j < kWqOffs; ++j) {
    if constexpr (kWqPad) {
      const int bb = 1024 * ((j < 4 ? wave : wave5) + 4 * j) + 16 * lane;
      const int row = bb / kKStride16, cb = bb - row * kKStride16;
      dk[j] = cb < 2 * kD ? row * (int)(a.k_sl * 2) + cb : 0;
      dv[j] = cb < 2 * kD ? row * (int)(a.v_sl * 2) + cb : 0;
    } else {
      const int P = wqimg::wave_piece(wave, j);
      const int row = wqimg::piece_row(P, lane), cb = wqimg::piece_col(lane);
      dk[j] = row * (int)(a.k_sl * 2) + cb;
      dv[j] = row * (int)(a.v_sl * 2) + cb;
    }
  }
  const unsigned lds_wave = (unsigned)(uintptr_t)(lds_char_ptr)smem + (unsigned)kWqPieceAt * (unsigned)wave;
  // the pad image's fifth piece's destination: byte 16384 + 1024 (wave & 1) of image img5 (the 16384 rides in the M0
  // add)
  [[maybe_unused]] const unsigned lds_wave5 =
      (unsigned)(uintptr_t)(lds_char_ptr)smem + 1024u * (unsigned)wave5 + (unsigned)kWqImg * (unsigned)img5;
  auto k_rsrc = [&](int t) __attribute__((always_inline)) {
    return tile_rsrc(kbase + (int64_t)t * kKBlk * a.k_sl * 2, a.k_sl, min(Lk - t * kKBlk, kKBlk));
  };
  auto v_rsrc = [&](int t) __attribute__((always_inline)) {
    return tile_rsrc(vbase + (int64_t)t * kKBlk * a.v_sl * 2, a.v_sl, min(Lk - t * kKBlk, kKBlk));
  };
  // M0 = the wave's LDS destination of a piece (an SALU write; the load that reads it is at least one MFMA later). The
  // add writes SCC: declared, or the compiler keeps a compare's SCC live across the statement (it did, in the prologue:
  // a descriptor's row-count select read the add's carry and the tile landed as zeros)
  auto set_m0 = [&](unsigned dst, auto OFFC) __attribute__((always_inline)) {
    asm volatile("s_add_u32 m0, %0, %1" ::"s"(dst), "i"(decltype(OFFC)::value) : "memory", "scc");
  };
  auto dma_load = [&](const u32x4& rs, int off) __attribute__((always_inline)) {
    asm volatile("buffer_load_dwordx4 %0, %1, 0 offen lds" ::"v"(off), "s"(rs) : "memory");
  };
  // prologue: one piece into LDS byte dst + OFFC (the nops: the descriptor's SALU writes -> the load that reads it)
  auto dma_piece = [&](const u32x4& rs, int off, unsigned dst, auto OFFC) __attribute__((always_inline)) {
    set_m0(dst, OFFC);
    asm volatile("s_nop 4" ::: "memory");
    dma_load(rs, off);
  };
  // prologue: pieces 0-15 of one image whose LDS byte offset is at (every wave its four)
  auto dma_img = [&](const u32x4& rs, const int* offs, unsigned at) __attribute__((always_inline)) {
    static_for<4>([&](auto JC) __attribute__((always_inline)) {
      dma_piece(rs, offs[decltype(JC)::value], lds_wave + at,
                std::integral_constant<int, kWqPieceStep * decltype(JC)::value>{});
    });
  };
  // prologue: the kIT images of the buffer at LDS byte offset at, tiles t0 .. t0 + kIT - 1 (the pad image: with their
  // pieces 16-17)
  auto dma_buf = [&](auto rsrc, const int* offs, int t0, unsigned at) __attribute__((always_inline)) {
    if constexpr (!kWqPad) {
#pragma unroll
      for (int i = 0; i < kIT; ++i) dma_img(rsrc(t0 + i), offs, at + (unsigned)(i * kWqImg));
    } else if constexpr (kIT == 1) {
      const u32x4 rs = rsrc(t0);
      dma_img(rs, offs, at);
      if (wave < 2) dma_piece(rs, offs[4], lds_wave + at, std::integral_constant<int, 16384>{});
    } else {
      const u32x4 rs0 = rsrc(t0), rs1 = rsrc(t0 + 1);
      dma_img(rs0, offs, at);
      dma_img(rs1, offs, at + (unsigned)kWqImg);
      if (wave < 2) dma_piece(rs0, offs[4], lds_wave5 + at, std::integral_constant<int, 16384>{});
      else dma_piece(rs1, offs[4], lds_wave5 + at, std::integral_constant<int, 16384>{});
    }
  };

  // K(0), K(1) .. K(kIT), V(0) .. V(kIT - 1) first: their flight overlaps the Q loads and the q normalisation. The
  // prologue reads K(0) as the last image of the K buffer "iteration -1" reads; iteration 0 reads K(1) .. K(kIT) from
  // the other K buffer and V(0) .. V(kIT - 1) from V buffer 0
  constexpr unsigned kK0At = (unsigned)(((kPar + 1) & 1) * kBuf + (kIT - 1) * kWqImg);
  {
    const u32x4 rs = k_rsrc(0);
    dma_img(rs, dk, kK0At);
    // (waves 0-1: lds_wave5 of image 0 is lds_wave)
    if constexpr (kWqPad)
      if (wave < 2) dma_piece(rs, dk[kWqOffs - 1], lds_wave + kK0At, std::integral_constant<int, 16384>{});
  }
  dma_buf(k_rsrc, dk, 1, (unsigned)((kPar & 1) * kBuf));
  dma_buf(v_rsrc, dv, 0, (unsigned)VB0);

  // ---- Q fragments Q[16 qb + c][32 s + 8 g .. +7] of rows row_w + 16 qb + c ----
  bf16x8 qa[kNQ][4];
#pragma unroll
  for (int qb = 0; qb < kNQ; ++qb) {
    const int r = row_w + 16 * qb + c16;
    const unsigned short* src = qp + (int64_t)min(r, a.Lq - 1) * a.q_sl + 8 * g;
#pragma unroll
    for (int s = 0; s < 4; ++s) qa[qb][s] = *reinterpret_cast<const bf16x8*>(src + 32 * s);
  }
  if (a.qn_w != nullptr) {
    // attn_fwd_m16's in-kernel q RMSNorm + RoPE + prescale, operation for operation, on the kNQ query blocks
    bf16x8 wv[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) wv[s] = *reinterpret_cast<const bf16x8*>(a.qn_w + 32 * s + 8 * g);
    const bool rope = a.qn_cos != nullptr;
    const f32x2 scale2 = {a.qn_scale, a.qn_scale};
#pragma unroll
    for (int qb = 0; qb < kNQ; ++qb) {
      const int r = row_w + 16 * qb + c16;
      f32x4 rc[2][2], rsn[2][2];
      if (rope) {
        const int64_t t0 = (a.qn_row0 + min(r, a.Lq - 1)) * 64 + 8 * g;
#pragma unroll
        for (int s1 = 0; s1 < 2; ++s1)
#pragma unroll
          for (int hf = 0; hf < 2; ++hf) {
            rc[s1][hf] = *reinterpret_cast<const f32x4*>(a.qn_cos + t0 + 32 * s1 + 4 * hf);
            rsn[s1][hf] = *reinterpret_cast<const f32x4*>(a.qn_sin + t0 + 32 * s1 + 4 * hf);
          }
      }
      f32x2 x[4][4];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          x[s][q] = f32x2{static_cast<float>(qa[qb][s][2 * q]), static_cast<float>(qa[qb][s][2 * q + 1])};
      f32x2 c01[8], c23[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        c01[e] = f32x2{x[0][e >> 1][e & 1], x[1][e >> 1][e & 1]};
        c23[e] = f32x2{x[2][e >> 1][e & 1], x[3][e >> 1][e & 1]};
      }
      const f32x2 p01 = hn2_sumsq8(c01), p23 = hn2_sumsq8(c23);
      const f32x2 aa = p01 + p23;
      float ss = aa.x + aa.y;
      ss += __shfl_xor(ss, 32);
      ss += __shfl_xor(ss, 16);
      const float rstd = hn_rstd(ss, a.qn_eps);
      const f32x2 rstd2 = {rstd, rstd};
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          x[s][q] = hn2_norm(x[s][q], rstd2,
                             f32x2{static_cast<float>(wv[s][2 * q]), static_cast<float>(wv[s][2 * q + 1])});
      f32x2 y[4][4];
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) y[s][q] = x[s][q];
      if (rope) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 cc = rc[s & 1][q >> 1], sn = rsn[s & 1][q >> 1];
            const int o = 2 * (q & 1);
            y[s][q] = hn2_rope(x[s][q], x[s ^ 2][q], s < 2 ? -1.f : 1.f, f32x2{cc[o], cc[o + 1]},
                               f32x2{sn[o], sn[o + 1]});
          }
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const bf16x2v hh = __builtin_convertvector(y[s][q] * scale2, bf16x2v);
          qa[qb][s][2 * q] = hh.x;
          qa[qb][s][2 * q + 1] = hh.y;
        }
    }
  }

  // ---- the rows' softmax shifts (fixed: from |q_row| and the key bound, attn_fwd_m16's rule) ----
  float m_run[kNQ];
#pragma unroll
  for (int qb = 0; qb < kNQ; ++qb) m_run[qb] = 0.f;
  if constexpr (kMode == 0) {
#pragma unroll
    for (int qb = 0; qb < kNQ; ++qb) {
      float qq = 0.f;
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float x = static_cast<float>(qa[qb][s][e]);
          qq = fmaf(x, x, qq);
        }
      const float b_row = sqrtf(group4_sum(qq)) * a.kbound;
      m_run[qb] = floorf(fminf(b_row + kPDrop, 126.f - b_row));
    }
  }
  f32x4 minit[kNQ];
#pragma unroll
  for (int qb = 0; qb < kNQ; ++qb) {
    minit[qb] = f32x4{-m_run[qb], -m_run[qb], -m_run[qb], -m_run[qb]};
    // opaque from here on: a broadcast the compiler may otherwise rematerialise right ahead of the asm MFMA that takes
    // it as C (a VALU write -> MFMA operand hazard it does not pad for asm)
    asm volatile("" : "+v"(minit[qb]));
  }

  // O^T, the row sums, the ones operand and the first kQA Q blocks into the accumulator file (v_accvgpr_write -> MFMA
  // operand: 2 wait states, inside the statement that ties each there); the other Q blocks opaque in VGPRs
  f32x4 oacc[8][kNQ], lacc[kNQ];
#pragma unroll
  for (int db = 0; db < 8; ++db)
#pragma unroll
    for (int qb = 0; qb < kNQ; ++qb) {
      oacc[db][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
      asm volatile("s_nop 2" : "+a"(oacc[db][qb]));
    }
#pragma unroll
  for (int qb = 0; qb < kNQ; ++qb) {
    lacc[qb] = f32x4{0.f, 0.f, 0.f, 0.f};
    asm volatile("s_nop 2" : "+a"(lacc[qb]));
  }
  static_for<kNQ>([&](auto QC) __attribute__((always_inline)) {
    constexpr int qb = decltype(QC)::value;
    (void)qa;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if constexpr (qb < kQA) asm volatile("s_nop 2" : "+a"(qa[qb][s]));
      else asm volatile("s_nop 2" : "+v"(qa[qb][s]));
    }
  });
  // the all-ones A operand of the row-sum MFMAs, in the accumulator file (as a VGPR constant the compiler may
  // rematerialise it with a v_mov right ahead of the first row-sum MFMA)
  typedef short s16x8v __attribute__((ext_vector_type(8)));
  bf16x8 ones8 = __builtin_bit_cast(bf16x8, s16x8v{0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80, 0x3f80});
  asm volatile("s_nop 2" : "+a"(ones8));
  // the fragment reads' lane bases: row c16, bytes 16 g of a K image; row 4 g + (c16 >> 2), bytes 8 (c16 & 3) of a V
  // image (lane = 16 g + c16)
  const unsigned k_rd_lds =
      (unsigned)(uintptr_t)(lds_char_ptr)smem +
      (unsigned)(kWqPad ? c16 * kKStride16 + 16 * g : wqimg::k_lane_base(lane));
  const unsigned v_rd_lds =
      (unsigned)(uintptr_t)(lds_char_ptr)smem + (unsigned)VB0 +
      (unsigned)(kWqPad ? (4 * g + (c16 >> 2)) * kVStride16 + 8 * (c16 & 3) : wqimg::v_lane_base(lane));

  f32x4 S[2][2][kNQ];  // S^T of two half stages: [half-stage parity][key block of the half][query block]
  bf16x8 P[2][kNQ];    // P^T of two half stages: [half-stage parity][query block]
  bf16x8 ring[kR];
  float ex[2];
  unsigned pk[4];
  unsigned k_cur = 0, v_cur = 0;  // this iteration's K(t + 1) / V(t) read bases

  // fragment F of an iteration (stage F / 16, f = F % 16; stage st works on image st >> 1 of the iteration's K and V
  // buffers, half st & 1 of it): f < 8 the V^T fragment (db = f, key step = st & 1: two transposed reads), f >= 8 the K
  // fragment (key block 2 (st & 1) + ((f - 8) & 1), d step (f - 8) >> 1)
  auto issue = [&](auto FC, auto SLOTC) __attribute__((always_inline)) {
    constexpr int F = decltype(FC)::value, slot = decltype(SLOTC)::value;
    constexpr int st = F / 16, f = F % 16;
    constexpr int img = (st >> 1) * kWqImg, hs = st & 1;
    static_assert(img + kWqImg <= 65536, "ds_read offset field");
    (void)ring;
    (void)k_cur;
    (void)v_cur;
    if constexpr (f >= 8) {
      constexpr int j = f - 8;
      constexpr int kb = 2 * hs + (j & 1), s = j >> 1;
      constexpr int off = img + (kWqPad ? kb * 16 * kKStride16 + 64 * s : wqimg::k_imm(kb, s));
      static_assert(off < 65536, "ds_read offset field");
      asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(ring[slot]) : "v"(k_cur), "i"(off));
    } else {
      constexpr int off = img + (kWqPad ? 32 * hs * kVStride16 + 32 * f : wqimg::v_imm(hs, 0, f));
      constexpr int off_hi = img + (kWqPad ? (32 * hs + 16) * kVStride16 + 32 * f : wqimg::v_imm(hs, 1, f));
      static_assert(off_hi < 65536, "ds_read offset field");
      s16x4 lo, hi;
      asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(lo) : "v"(v_cur), "i"(off));
      asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(hi) : "v"(v_cur), "i"(off_hi));
      typedef short s16x8 __attribute__((ext_vector_type(8)));
      const s16x8 r = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      ring[slot] = __builtin_bit_cast(bf16x8, r);
    }
  };

  // scores of keys >= Lk of the half stage whose first key is k0 (S[SP]): -inf, so P = 0 exactly. Rare (the ragged
  // tile and the virtual one); the nops let the MFMAs that wrote S[SP] finish
  auto mask_keys = [&](auto SPC, int k0) __attribute__((always_inline)) {
    constexpr int SP = decltype(SPC)::value;
    if (__builtin_expect(k0 + 32 > Lk, 0)) {
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
#pragma unroll
      for (int kbl = 0; kbl < 2; ++kbl)
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (k0 + 16 * kbl + 4 * g + i >= Lk) {
#pragma unroll
            for (int qb = 0; qb < kNQ; ++qb) S[SP][kbl][qb][i] = -INFINITY;
          }
    }
  };

  // The DMA's wave-uniform state (SGPRs): the descriptors of the tiles iteration t fetches, K(kIT (t + 1) + 1 + i) and
  // V(kIT (t + 1) + i), i < kIT (the pad image's rk5 / rv5: the fifth piece's image). Past the last tile: an empty
  // range, the pieces land as zeros. The product makes them by adds from a running base and row count in steps, which
  // the loop takes for iteration t + 1 in the last three gaps of iteration t (they carry nothing else), so that the
  // SALU work sits under MFMAs. The lab form (kWqHeadRsrc) computes them at the head of the iteration, behind the
  // barrier with no MFMA in flight.
  u32x4 rk[kIT], rv[kIT];
  [[maybe_unused]] u32x4 rk5 = {0u, 0u, 0u, 0u}, rv5 = {0u, 0u, 0u, 0u};
  const int64_t kstep = (int64_t)kKBlk * a.k_sl * 2, vstep = (int64_t)kKBlk * a.v_sl * 2;
  const char* kp = kbase + (kIT + 1) * kstep;
  const char* vp = vbase + kIT * vstep;
  int rows_k = Lk - (kIT + 1) * kKBlk, rows_v = Lk - kIT * kKBlk;
  auto dma_next = [&](auto CC) __attribute__((always_inline)) {
    constexpr int c = decltype(CC)::value;
    if constexpr (c == 0) {
#pragma unroll
      for (int i = 0; i < kIT; ++i) rk[i] = tile_rsrc(kp + i * kstep, a.k_sl, min(rows_k - i * kKBlk, kKBlk));
      kp += kIT * kstep;
      rows_k -= kIT * kKBlk;
    } else if constexpr (c == 1) {
#pragma unroll
      for (int i = 0; i < kIT; ++i) rv[i] = tile_rsrc(vp + i * vstep, a.v_sl, min(rows_v - i * kKBlk, kKBlk));
      vp += kIT * vstep;
      rows_v -= kIT * kKBlk;
    } else if constexpr (kWqPad && kIT == 2) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        rk5[e] = img5 ? rk[kIT - 1][e] : rk[0][e];
        rv5[e] = img5 ? rv[kIT - 1][e] : rv[0][e];
      }
    }
  };
  if constexpr (!kWqHeadRsrc) static_for<3>(dma_next);
  constexpr int kNextAt = (2 * kIT - 1) * wq_stage(kNQ) + wq_stage(kNQ) - 3;  // the iteration slot of dma_next's step 0
  static_assert(!wq_read_gap(kNQ, wq_stage(kNQ) - 3) && !wq_read_gap(kNQ, wq_stage(kNQ) - 2) &&
                    !wq_read_gap(kNQ, wq_stage(kNQ) - 1) && wq_sm_op(kNQ, wq_stage(kNQ) - 3) < 0,
                "a stage's last three gaps carry no read and no softmax instruction");

  // One iteration t: the half stages st = 0 .. 2 kIT - 1, hs = st & 1, on image st >> 1 of the iteration's K and V
  // buffers. Stage st's row sums and P.V read P[hs] and the V image's key step hs; its Q K^T reads the K image's key
  // blocks 2 hs, 2 hs + 1 and writes S[hs]; its softmax reads S[1 - hs] and writes P[1 - hs]. FULL: the loop's
  // iteration; else the prologue (two stages on K(0): no P.V, no first softmax, no DMA).
  auto body = [&](auto FULLC, int t) __attribute__((always_inline)) {
    constexpr bool FULL = decltype(FULLC)::value;
    constexpr int NST = FULL ? 2 * kIT : 2;  // half stages
    constexpr int NF = FULL ? 16 * NST : 16;  // live fragments, in order
    constexpr auto frag_of = [](int n) constexpr { return FULL ? n : (n < 8 ? 8 + n : 16 + n); };
    constexpr auto seq_of = [](int F) constexpr { return FULL ? F : (F < 16 ? F - 8 : F - 16); };
    constexpr auto nreads = [](int F) constexpr { return F % 16 < 8 ? 2 : 1; };
    // the first key of the scores stage 0's softmax works on (stage st's: + 32 st)
    const int key_sm = FULL ? 64 * kIT * t + 32 : -32;
    unsigned dst_k = 0, dst_v = 0, dst_k5 = 0, dst_v5 = 0;
    if constexpr (FULL) {
      k_cur = k_rd_lds + (((t + kPar) & 1) ? (unsigned)kBuf : 0u);
      v_cur = v_rd_lds + ((t & 1) ? (unsigned)kBuf : 0u);
      mask_keys(std::integral_constant<int, 1>{}, key_sm);
      if constexpr (kWqHeadRsrc) {
#pragma unroll
        for (int i = 0; i < kIT; ++i) {
          rk[i] = k_rsrc(kIT * (t + 1) + 1 + i);
          rv[i] = v_rsrc(kIT * (t + 1) + i);
        }
        if constexpr (kWqPad && kIT == 2) dma_next(std::integral_constant<int, 2>{});
      }
      // the next iteration's tiles go into the two buffers the previous iteration read
      const unsigned at_k = ((t + 1 + kPar) & 1) ? (unsigned)kBuf : 0u;
      const unsigned at_v = (unsigned)VB0 + (((t + 1) & 1) ? (unsigned)kBuf : 0u);
      dst_k = lds_wave + at_k;
      dst_v = lds_wave + at_v;
      if constexpr (kWqPad && kIT == 2) {  // pieces 16-17: of image 0 on waves 0-1, of image 1 on waves 2-3
        dst_k5 = lds_wave5 + at_k;
        dst_v5 = lds_wave5 + at_v;
      }
    } else {
      k_cur = k_rd_lds + kK0At;  // K(0)
      v_cur = v_rd_lds;          // (no P.V in the prologue)
    }
    // DMA slot d of the iteration: its M0, then (one gap later) its load
    auto dma_m0 = [&](auto DC) __attribute__((always_inline)) {
      constexpr int d = decltype(DC)::value, i = d % (kND / 2);
      constexpr bool isk = d < kND / 2;
      (void)dst_k;
      (void)dst_v;
      (void)dst_k5;
      (void)dst_v5;
      if constexpr (kWqPad && kIT == 1) {
        if (i < 4 || wave < 2) set_m0(isk ? dst_k : dst_v, std::integral_constant<int, 4096 * i>{});
      } else if constexpr (i < 4 * kIT) {  // piece j = i % 4 of image i / 4
        set_m0(isk ? dst_k : dst_v, std::integral_constant<int, (i / 4) * kWqImg + kWqPieceStep * (i % 4)>{});
      } else {
        set_m0(isk ? dst_k5 : dst_v5, std::integral_constant<int, 16384>{});
      }
    };
    auto dma_ld = [&](auto DC) __attribute__((always_inline)) {
      constexpr int d = decltype(DC)::value, i = d % (kND / 2);
      constexpr bool isk = d < kND / 2;
      (void)rk;
      (void)rv;
      (void)rk5;
      (void)rv5;
      if constexpr (kWqPad && kIT == 1) {
        if (i < 4 || wave < 2) dma_load(isk ? rk[0] : rv[0], isk ? dk[i] : dv[i]);
      } else if constexpr (i < 4 * kIT) {
        dma_load(isk ? rk[i / 4] : rv[i / 4], isk ? dk[i % 4] : dv[i % 4]);
      } else {
        dma_load(isk ? rk5 : rv5, isk ? dk[kWqOffs - 1] : dv[kWqOffs - 1]);
      }
    };
    static_for<kAheadWq>([&](auto IC) __attribute__((always_inline)) {
      constexpr int n = decltype(IC)::value;
      issue(std::integral_constant<int, frag_of(n)>{}, std::integral_constant<int, n % kR>{});
    });
    __builtin_amdgcn_sched_barrier(0);
    static_for<NST * kNS>([&](auto MC) __attribute__((always_inline)) {
      constexpr int M = decltype(MC)::value;
      constexpr int st = M / kNS, m = M % kNS, hs = st & 1;
      constexpr int f = wq_frag(kNQ, m), qb = wq_qb(kNQ, m);
      constexpr int F = 16 * st + (f < 0 ? 0 : f);
      constexpr bool has_mfma = f >= 8 || FULL;
      constexpr bool has_sm = st >= 1 || FULL;
      (void)S;  // (asm operands, named: clang's implicit capture into a generic lambda misses them otherwise)
      (void)ex;
      (void)pk;
      (void)oacc;
      (void)lacc;
      (void)ones8;
      (void)P;
      (void)minit;
      (void)qa;
      (void)ring;
      if constexpr (m == 0 && st >= 1) {
        if constexpr (!FULL) asm volatile("s_nop 15" ::: "memory");  // no MFMA ahead of the softmax's first S reads
        mask_keys(std::integral_constant<int, 1 - hs>{}, key_sm + 32 * st);
        __builtin_amdgcn_sched_barrier(0);
      }
      if constexpr (has_mfma) {
        if constexpr (f >= 0 && qb == 0) {  // fragment F opens: its reads (not the later fragments') have landed
          constexpr int n = seq_of(F);
          constexpr int pending = [=]() constexpr {
            int p = 0;
            for (int i = 1; i < kAheadWq; ++i)
              if (n + i < NF) p += nreads(frag_of(n + i));
            return p;
          }();
          asm volatile("s_waitcnt lgkmcnt(%0)" ::"i"(pending), "v"(ring[n % kR]) : "memory");
        }
        if constexpr (f < 0) {  // row sums: all-ones x P^T
          asm volatile(WQ_MFMA "%0, %1, %2, %0" : "+a"(lacc[qb]) : "a"(ones8), "v"(P[hs][qb]));
        } else if constexpr (f < 8) {  // O^T[db] += V^T(db, key step st) P^T
          asm volatile(WQ_MFMA "%0, %1, %2, %0" : "+a"(oacc[f][qb]) : "v"(ring[seq_of(F) % kR]), "v"(P[hs][qb]));
        } else {  // S^T[kbl] (+)= K(kbl, s) Q^T(s)
          constexpr int kbl = (f - 8) & 1, s = (f - 8) >> 1;
          constexpr int ri = seq_of(F) % kR;
          if constexpr (qb < kQA) {
            if constexpr (s == 0 && kInit)
              asm volatile(WQ_MFMA "%0, %1, %2, %3"
                           : "=&v"(S[hs][kbl][qb]) : "v"(ring[ri]), "a"(qa[qb][s]), "v"(minit[qb]));
            else if constexpr (s == 0)
              asm volatile(WQ_MFMA "%0, %1, %2, 0" : "=&v"(S[hs][kbl][qb]) : "v"(ring[ri]), "a"(qa[qb][s]));
            else
              asm volatile(WQ_MFMA "%0, %1, %2, %0" : "+v"(S[hs][kbl][qb]) : "v"(ring[ri]), "a"(qa[qb][s]));
          } else {
            if constexpr (s == 0 && kInit)
              asm volatile(WQ_MFMA "%0, %1, %2, %3"
                           : "=&v"(S[hs][kbl][qb]) : "v"(ring[ri]), "v"(qa[qb][s]), "v"(minit[qb]));
            else if constexpr (s == 0)
              asm volatile(WQ_MFMA "%0, %1, %2, 0" : "=&v"(S[hs][kbl][qb]) : "v"(ring[ri]), "v"(qa[qb][s]));
            else
              asm volatile(WQ_MFMA "%0, %1, %2, %0" : "+v"(S[hs][kbl][qb]) : "v"(ring[ri]), "v"(qa[qb][s]));
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      // ---- the gap after slot M ----
      if constexpr (has_mfma && f >= 0 && qb == 0) {
        constexpr int n = seq_of(F) + kAheadWq;
        if constexpr (n < NF) issue(std::integral_constant<int, frag_of(n)>{}, std::integral_constant<int, n % kR>{});
      }
      if constexpr (FULL) {
        constexpr int dm = wq_m0_at(kNQ, kIT, M), dl = wq_dma_at(kNQ, kIT, M);
        if constexpr (dm >= 0) dma_m0(std::integral_constant<int, dm>{});
        if constexpr (dl >= 0) dma_ld(std::integral_constant<int, dl>{});
        if constexpr (!kWqHeadRsrc && M >= kNextAt && M < kNextAt + 3)  // (this iteration's loads are long issued)
          dma_next(std::integral_constant<int, M - kNextAt>{});
      }
      if constexpr (has_sm) {
        if constexpr (!has_mfma) asm volatile("s_nop 1" ::: "memory");  // trans -> VALU use without an MFMA between
        constexpr int op = wq_sm_op(kNQ, m);
        if constexpr (op >= 0) {
          constexpr int q = op / 12, r = op % 12, pair = r / 3, w = r % 3;
          if constexpr (w < 2) {
            constexpr int j = 2 * pair + w;
            asm volatile("v_exp_f32 %0, %1" : "=v"(ex[w]) : "v"(S[1 - hs][j >> 2][q][j & 3]));
          } else {
            // the bf16 pack as a compiler conversion (v_cvt_pk_bf16_f32), pinned to this gap by the asm statement that
            // uses it
            pk[pair] = __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2{ex[0], ex[1]}, bf16x2v));
            asm volatile("" ::"v"(pk[pair]));
            if constexpr (pair == 3) P[1 - hs][q] = __builtin_bit_cast(bf16x8, u32x4{pk[0], pk[1], pk[2], pk[3]});
          }
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    });
    if constexpr (FULL) {
      // P stays allocated to the end of the iteration: no register an MFMA of this iteration reads is handed to a
      // load of the same iteration (an asm load may land before the MFMA issued just ahead of it read its operand)
      static_for<kNQ>([&](auto QC) __attribute__((always_inline)) {
        constexpr int qb = decltype(QC)::value;
        (void)P;
        asm volatile("" ::"v"(P[0][qb]), "v"(P[1][qb]));
      });
    }
    // this wave's DMA pieces landed. Every piece is drained here: leaving pieces in flight across the barrier
    // (vmcnt(N) > 0) gave wrong results in every variant tried on gfx950; they are issued in the
    // first third of the iteration instead, so the drain finds them landed
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
  };

  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // K(0), K(1), V(0)
  __builtin_amdgcn_s_barrier();
  body(std::false_type{}, -1);
  const int nit = (ntk + kIT - 1) / kIT;  // an odd tile count ends in a half-full iteration: P = 0 on zero V rows
  for (int t = 0; t < nit; ++t) body(std::true_type{}, t);

  // ---- epilogue: O^T[16 db + 4 g + i][16 qb + c] = oacc[db][qb][i]: row row_w + 16 qb + c ----
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // the last MFMAs' accumulator writes -> v_accvgpr_read
#pragma unroll
  for (int db = 0; db < 8; ++db)
#pragma unroll
    for (int qb = 0; qb < kNQ; ++qb) asm volatile("s_nop 0" : "+a"(oacc[db][qb]));
#pragma unroll
  for (int qb = 0; qb < kNQ; ++qb) asm volatile("s_nop 0" : "+a"(lacc[qb]));
#pragma unroll
  for (int qb = 0; qb < kNQ; ++qb) {
    const int q_row = row_w + 16 * qb + c16;
    const float l_tot = lacc[qb][0];
    float inv = 1.f / l_tot;
    // contract guard: a norm bound below the real norms can only show as an overflowed row sum
    if (l_tot > 3.0e38f) inv = __uint_as_float(0x7fc00000u);
    if (q_row >= a.Lq) continue;
    if (a.nsplit > 1) {
      const int64_t row = ((int64_t)(split * a.B + b) * a.H + h) * a.Lq + q_row;
      float* op = a.o_part + row * kD + 4 * g;
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        f32x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = oacc[db][qb][e] * inv;
        *reinterpret_cast<f32x4*>(op + 16 * db) = w;
      }
      if (g == 0) a.lse_part[row] = m_run[qb] + __log2f(l_tot);
    } else {
      unsigned short* op = a.o + b * a.o_sb + h * a.o_sh + (int64_t)q_row * a.o_sl + 4 * g;
#pragma unroll
      for (int db = 0; db < 8; ++db) {
        u16x4 w;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = f2bf(oacc[db][qb][e] * inv);
        *reinterpret_cast<u16x4*>(op + 16 * db) = w;
      }
    }
  }
}

#undef WQ_MFMA

}  // namespace

// Built: 320 and 384 rows, fixed shift. Every long-key launch with usable norm bounds is in the fixed mode (attn_route's
// long-key rule, round 6), so the zero-shift form (kMode 1: the same stream without the initial C) has no launch to serve
// and is not instantiated.
AttnKernel wq_kernel(int rows, int mode, bool tail) {
  if (mode != 0) return nullptr;
  if (rows == 320) return tail ? attn_fwd_wq<5, 0, 1> : attn_fwd_wq<5, 0>;
  if (rows == 384) return tail ? attn_fwd_wq<6, 0, 1> : attn_fwd_wq<6, 0>;
  return nullptr;
}

}  // namespace cp25attn
