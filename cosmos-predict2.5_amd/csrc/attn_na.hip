// 3D neighborhood (box) attention for the sparse-attention DiT (gfx950): bf16 in / out, head dim 128.
//
//   cp25_attn_na3d : o[q] = softmax over the query's key box (q k^T * scale) v, the box being the product of a
//                    window of Kt x Kh x Kw keys (dilations dt, dh, dw) of the (T, H, W) token grid. Replaces
//                    NeighborhoodAttention.forward (modules/neighborhood_attn.py:172-252, NATTEN's
//                    neighborhood_attention_generic) as called by NattenA2AAttnOp (networks/a2a_cp.py:222-226).
//
// The host plan (cosmos_predict2/sparse_attn.py build_plan) groups the queries into tiles of 128 rows that share ONE
// key box (same window start and dilation group on every axis), so the kernel carries no per-query mask: the only
// masked keys are those of the ragged last 64-key tile. Two int32 device tables describe the plan:
//   q_tok[n_tiles][128] : token id of each query row of the tile, -1 = empty slot (a group smaller than the tile);
//                         slot 0 of every tile is a real token;
//   box[n_tiles][4]     : the box's first key index along t, h, w (fourth entry unused).
// Key c of a box (0 <= c < Kt Kh Kw, w fastest) is token ((t0 + jt dt) H + h0 + jh dh) W + w0 + jw dw.
//
// Design: one workgroup = 4 waves = one (tile, head, batch); each wave owns 32 query rows and the whole head dim,
// as vae_attn.hip does at d = 384:
//   * swapped products: S^T = K Q^T (v_mfma_f32_32x32x16_bf16, 8 k-steps over d; the query on the lane, Q^T
//     fragments gathered once by q_tok into 32 VGPRs), then O^T = V^T P^T with the S accumulators converted to bf16
//     in place as the B operand and V^T read by ds_read_b64_tr_b16; O^T is 4 d-blocks of 32 x 32;
//   * K / V rows (256 B each, one 16-lane x 16 B load) are gathered by token id into LDS in 64-key tiles,
//     double-buffered and register-staged one tile ahead; rows padded to 272 B (K) and 320 B (V) keep the K row reads
//     and the transposed V reads bank-conflict-free. Each wave decodes the tile's 64 token ids once (lane = key) and
//     hands them to the staging lanes by a wave shuffle;
//   * online row max, rescaling O and the row sum only when a tile's row max exceeds the shift by more than 2^24
//     (attn_common.h kLazy); P rounded to bf16 for P V, fp32 everywhere else, O normalised once.
// Tiles are ordered by box on the host and the 1-D grid is XCD-remapped with the tile index fastest, so the
// workgroups that share an L2 walk the same box of the same head.
// Fault safety: the plan is validated on the host before the first launch; the kernel still clamps every key token
// into [0, L) and treats a q_tok entry outside [0, L) as an empty slot, so no address is formed from a pad or from a
// corrupt table.
#include "attn_common.h"

namespace {

using namespace cp25attn;

constexpr int kNaRows = 128;                       // query rows per tile (4 waves x 32)
constexpr int kNaThreads = 256;
constexpr int kNaKStride = 272;                    // K row in LDS: 256 + 16
constexpr int kNaVStride = 320;                    // V row in LDS: 256 + 64
constexpr int kNaKBuf = kKBlk * kNaKStride;        // 17408
constexpr int kNaVBuf = kKBlk * kNaVStride;        // 20480
constexpr int kNaStage = kNaKBuf + kNaVBuf;        // 37888 (two stages: 75776 B, two workgroups per CU)
constexpr int kNaPerThread = kKBlk * 16 / kNaThreads;  // 16-B chunks per thread per K (or V) tile: 4

struct NaArgs {
  const unsigned short* q; const unsigned short* k; const unsigned short* v; unsigned short* o;
  int64_t q_sb, q_sl, q_sh;
  int64_t k_sb, k_sl, k_sh;
  int64_t v_sb, v_sl, v_sh;
  int64_t o_sb, o_sl, o_sh;
  const int* q_tok;
  const int* box;
  int n_tiles, H;
  int gH, gW, L;          // token grid (h, w extents) and token count
  int Kh, Kw, nkeys;      // window extents along h, w; keys per box
  int dt, dh, dw;
  float scale_log2;       // softmax scale * log2(e) (1 for a pre-scaled q)
};

__global__ void __launch_bounds__(kNaThreads, 2) attn_na3d_kernel(NaArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kNaStage];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hl = lane >> 5;
  const int wg = xcd_remap(blockIdx.x, gridDim.x);
  const int tile = wg % a.n_tiles;
  const int bh = wg / a.n_tiles;
  const int head = bh % a.H, batch = bh / a.H;
  const unsigned short* Q = a.q + batch * a.q_sb + head * a.q_sh;
  const unsigned short* K = a.k + batch * a.k_sb + head * a.k_sh;
  const unsigned short* V = a.v + batch * a.v_sb + head * a.v_sh;
  unsigned short* O = a.o + batch * a.o_sb + head * a.o_sh;
  const int t0 = a.box[4 * tile], h0 = a.box[4 * tile + 1], w0 = a.box[4 * tile + 2];
  const int nt = (a.nkeys + kKBlk - 1) / kKBlk;

  // this lane's query row: an empty slot computes on the tile's first row (a real token) and stores nothing
  const int* qt = a.q_tok + (int64_t)tile * kNaRows;
  int q_id = qt[wave * 32 + l31];
  const bool q_live = q_id >= 0 && q_id < a.L;
  if (!q_live) q_id = min(max(qt[0], 0), a.L - 1);

  // Q^T fragments (B operand of S^T = K Q^T): lane (query l31, d 16 s + 8 hl .. + 8), 32 VGPRs
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(Q + (int64_t)q_id * a.q_sl + 16 * s + 8 * hl);

  // token id of key `lane` of tile t (keys past the box repeat its last key: their scores are masked to -inf)
  auto key_token = [&](int t) __attribute__((always_inline)) {
    const int c = min(t * kKBlk + lane, a.nkeys - 1);
    const int jw = c % a.Kw, r = c / a.Kw;
    const int jh = r % a.Kh, jt = r / a.Kh;
    const int tok = ((t0 + jt * a.dt) * a.gH + h0 + jh * a.dh) * a.gW + w0 + jw * a.dw;
    return min(max(tok, 0), a.L - 1);
  };
  // staging: thread t moves chunks t + 256 i (i < 4) of the K and V tiles: row (t >> 4) + 16 i, 16-B chunk t & 15
  u32x4 sk[kNaPerThread], sv[kNaPerThread];
  const int row0 = tid >> 4, ch = tid & 15;
  auto load_tile = [&](int t) __attribute__((always_inline)) {
    const int tok = key_token(t);
#pragma unroll
    for (int i = 0; i < kNaPerThread; ++i) {
      const int64_t key = __shfl(tok, (row0 + 16 * i) & 63);
      sk[i] = *reinterpret_cast<const u32x4*>(K + key * a.k_sl + ch * 8);
      sv[i] = *reinterpret_cast<const u32x4*>(V + key * a.v_sl + ch * 8);
    }
  };
  auto write_tile = [&](int buf) __attribute__((always_inline)) {
    char* kb = smem + buf * kNaStage;
    char* vb = kb + kNaKBuf;
#pragma unroll
    for (int i = 0; i < kNaPerThread; ++i) {
      const int r = row0 + 16 * i;
      *reinterpret_cast<u32x4*>(kb + r * kNaKStride + ch * 16) = sk[i];
      *reinterpret_cast<u32x4*>(vb + r * kNaVStride + ch * 16) = sv[i];
    }
  };

  // per-lane LDS read offsets: K rows (key l31 of a 32-key half, d 16 s + 8 hl); V^T transposed reads as vae_attn.hip
  const int k_rd = l31 * kNaKStride + 16 * hl;
  const int grp = lane >> 4, gi = lane & 15;
  const int tq = gi >> 2, tp = gi & 3;
  const int v_rd = kNaKBuf + (4 * (grp >> 1) + tq) * kNaVStride + 32 * (grp & 1) + 8 * tp;

  f32x16 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float l_run = 0.f, m_run = -INFINITY;

  load_tile(0);
  write_tile(0);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int buf = t & 1;
    if (t + 1 < nt) load_tile(t + 1);
    const char* kb = smem + buf * kNaStage;
    // S^T of the tile's two 32-key halves: register r of half hf holds key 32 hf + 8 (r / 4) + 4 hl + r % 4
    f32x16 S[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int r = 0; r < 16; ++r) S[hf][r] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bf16x8 kr = *reinterpret_cast<const bf16x8*>(kb + k_rd + hf * 32 * kNaKStride + 32 * s);
        S[hf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kr, qf[s], S[hf], 0, 0, 0);
      }
    }
    if ((t + 1) * kKBlk > a.nkeys) {  // the ragged last tile: the only mask
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (t * kKBlk + 32 * hf + 8 * (r >> 2) + 4 * hl + (r & 3) >= a.nkeys) S[hf][r] = -INFINITY;
    }
    // online row max (the row's scores sit in lanes l31 and l31 + 32); every tile holds at least one real key
    float tmax = S[0][0];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, S[hf][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32)) * a.scale_log2;
    if (__any(tmax > m_run + kLazy)) {  // wave-uniform; tile 0 always (m_run = -inf)
      const float m_new = fmaxf(m_run, tmax);
      const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // 0 at tile 0
      l_run *= alpha;
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
      m_run = m_new;
    }
    // P^T as the B operand of O^T = V^T P^T: k-step ks = 2 hf + sp holds registers 8 sp .. 8 sp + 7 of half hf
    bf16x8 pb[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f(fmaf(S[ks >> 1][8 * (ks & 1) + j], a.scale_log2, -m_run));
        l_run += p;
        pb[ks][j] = static_cast<__bf16>(p);
      }
    const char* vb = smem + buf * kNaStage + v_rd;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
        typedef __attribute__((address_space(3))) const char* lds_cptr;
        const int off = 16 * ks * kNaVStride + 64 * d;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds_cptr)(vb + off));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds_cptr)(vb + off + 8 * kNaVStride));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 r8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, r8), pb[ks], o[d], 0, 0, 0);
      }
    if (t + 1 < nt) write_tile(buf ^ 1);  // tile t - 1's buffer: every wave passed the last barrier
    __syncthreads();
  }

  // epilogue: O^T lane (query l31), register r of d-block d holds d = 32 d + 8 (r / 4) + 4 hl + r % 4
  if (!q_live) return;
  const float inv = 1.f / (l_run + __shfl_xor(l_run, 32));
  unsigned short* orow = O + (int64_t)q_id * a.o_sl;
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      u16x4 w;
#pragma unroll
      for (int e = 0; e < 4; ++e) w[e] = f2bf(o[d][4 * g + e] * inv);
      *reinterpret_cast<u16x4*>(orow + 32 * d + 8 * g + 4 * hl) = w;
    }
}

bool na_strides_ok(const int64_t* s) { return s && s[0] >= 0 && s[1] >= kD && s[2] >= kD && !((s[0] | s[1] | s[2]) % 8); }

}  // namespace

extern "C" int cp25_attn_na3d(const void* q, const void* k, const void* v, void* o, int B, int H, int T, int Hg, int Wg,
                              int D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                              const int64_t* o_strides, const int* q_tok, const int* box, int n_tiles,
                              int tile_rows, const int* window, const int* dilation, float softmax_scale, int prescaled,
                              hipStream_t stream) {
  if (!q || !k || !v || !o || !q_tok || !box || !window || !dilation) return CP25_ERR_INVAL;
  if (D != kD || tile_rows != kNaRows) return CP25_ERR_INVAL;
  if (B <= 0 || H <= 0 || T <= 0 || Hg <= 0 || Wg <= 0 || n_tiles <= 0) return CP25_ERR_INVAL;
  const int64_t L = (int64_t)T * Hg * Wg;
  if (L > (1 << 21)) return CP25_ERR_INVAL;
  if (!na_strides_ok(q_strides) || !na_strides_ok(k_strides) || !na_strides_ok(v_strides) || !na_strides_ok(o_strides))
    return CP25_ERR_INVAL;
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)o)) & 15) return CP25_ERR_INVAL;
  if ((((uintptr_t)q_tok) | ((uintptr_t)box)) & 3) return CP25_ERR_INVAL;
  const int ext[3] = {T, Hg, Wg};
  for (int i = 0; i < 3; ++i)  // a window of K keys at dilation d spans (K - 1) d + 1 <= L positions
    if (window[i] < 1 || dilation[i] < 1 || (int64_t)window[i] * dilation[i] > ext[i]) return CP25_ERR_INVAL;
  if (!prescaled && !(softmax_scale > 0.f)) return CP25_ERR_INVAL;
  if (n_tiles > L || (int64_t)n_tiles * H * B > 0x7fffffff) return CP25_ERR_INVAL;
  NaArgs a;
  a.q = (const unsigned short*)q; a.k = (const unsigned short*)k; a.v = (const unsigned short*)v;
  a.o = (unsigned short*)o;
  a.q_sb = q_strides[0]; a.q_sl = q_strides[1]; a.q_sh = q_strides[2];
  a.k_sb = k_strides[0]; a.k_sl = k_strides[1]; a.k_sh = k_strides[2];
  a.v_sb = v_strides[0]; a.v_sl = v_strides[1]; a.v_sh = v_strides[2];
  a.o_sb = o_strides[0]; a.o_sl = o_strides[1]; a.o_sh = o_strides[2];
  a.q_tok = q_tok; a.box = box; a.n_tiles = n_tiles; a.H = H;
  a.gH = Hg; a.gW = Wg; a.L = (int)L;
  a.Kh = window[1]; a.Kw = window[2]; a.nkeys = window[0] * window[1] * window[2];
  a.dt = dilation[0]; a.dh = dilation[1]; a.dw = dilation[2];
  a.scale_log2 = prescaled ? 1.f : softmax_scale * 1.4426950408889634f;
  hipLaunchKernelGGL(attn_na3d_kernel, dim3((unsigned)((int64_t)n_tiles * H * B)), dim3(kNaThreads), 0, stream, a);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}
