// Causal grouped-query attention for the Reason1 (Qwen2.5-VL language model) text encoder (gfx950): bf16 in / out,
// head dim 128.
//
//   cp25_attn_causal : o[b, i, h] = softmax_{j <= i}(q[b, i, h] . k[b, j, h / (Hq / Hkv)] * scale) v[b, j, h / (Hq / Hkv)]
//                      Replaces the flash_attn_func(causal=True) call of Qwen2_5_VLFlashAttention2 / the sdpa of the
//                      text decoder layers (reason1/networks/qwen2_5_vl.py) for a text-only prompt without a padding
//                      mask (text_encoders/text_encoder.py:186-189).
//
// A plain kernel: it is under 1 % of the encoder's FLOPs. Its data path is attn_na.hip's, whose fragment layouts
// tests/test_sparse_attn_exact_gpu.py pins element by element: one workgroup = 2 waves = one 64-row query block of
// one (batch, query head); each wave owns 32 query rows and the whole head dim.
//   * swapped products: S^T = K Q^T (v_mfma_f32_32x32x16_bf16, 8 k-steps over d; the query on the lane, its Q^T
//     fragments loaded once into 32 VGPRs), then O^T = V^T P^T with the S accumulators converted to bf16 in place as the
//     B operand and V^T read by ds_read_b64_tr_b16; O^T is 4 d-blocks of 32 x 32;
//   * the 64-key K and V tiles go through one LDS buffer each (rows padded to 272 B and 320 B: conflict-free K row
//     reads and transposed V reads), loaded between two barriers: no look-ahead, no register staging;
//   * query block qb reads key tiles 0 .. qb only: tiles wholly above the diagonal are never touched. Tile qb is the
//     diagonal one: its scores with key > query are set to -inf BEFORE the row max, so a masked key can neither move
//     the shift nor contribute (exp2(-inf) = 0). Every row keeps at least its own key, so the max is finite;
//   * exact online row max per query row (Qwen has no q / k norm, so there is no bound to fix a shift by): O and the
//     row sum are rescaled by exp2(m_old - m_new) at every tile; P rounded to bf16 for P V, fp32 everywhere else, the
//     row sum of the unrounded P, O normalised once.
// Bounds: L % 64 == 0 is required, so every key row t 64 + r (t <= qb) and query row qb 64 + r is below L; no address
// is formed from anything but the launch arguments.
#include "attn_common.h"

namespace {

using namespace cp25attn;

constexpr int kCaRows = 64;                        // query rows per workgroup (2 waves x 32)
constexpr int kCaThreads = 128;
constexpr int kCaKStride = 272;                    // K row in LDS: 256 + 16
constexpr int kCaVStride = 320;                    // V row in LDS: 256 + 64
constexpr int kCaKBuf = kKBlk * kCaKStride;        // 17408
constexpr int kCaVBuf = kKBlk * kCaVStride;        // 20480
constexpr int kCaPerThread = kKBlk * 16 / kCaThreads;  // 16-B chunks per thread per K (or V) tile: 8
static_assert(kKBlk == 64 && kD == 128, "the tile geometry below");

struct CaArgs {
  const unsigned short* q; const unsigned short* k; const unsigned short* v; unsigned short* o;
  int64_t q_sb, q_sl, q_sh;
  int64_t k_sb, k_sl, k_sh;
  int64_t v_sb, v_sl, v_sh;
  int64_t o_sb, o_sl, o_sh;
  int Hq, group;          // query heads; query heads per key/value head
  int nqb;                // query blocks per (b, h) = L / 64
  float scale_log2;       // softmax scale * log2(e)
};

__global__ void __launch_bounds__(kCaThreads) attn_causal_kernel(CaArgs a) {
  __shared__ __attribute__((aligned(16))) char smem[kCaKBuf + kCaVBuf];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l31 = lane & 31, hl = lane >> 5;
  // the longest query blocks first
  const int qb = a.nqb - 1 - (int)(blockIdx.x % a.nqb);
  const int bh = blockIdx.x / a.nqb;
  const int head = bh % a.Hq, batch = bh / a.Hq;
  const int kvh = head / a.group;
  const unsigned short* Q = a.q + batch * a.q_sb + head * a.q_sh;
  const unsigned short* K = a.k + batch * a.k_sb + kvh * a.k_sh;
  const unsigned short* V = a.v + batch * a.v_sb + kvh * a.v_sh;
  unsigned short* O = a.o + batch * a.o_sb + head * a.o_sh;

  const int q_loc = wave * 32 + l31;               // this lane's query row within the block
  const int64_t q_id = (int64_t)qb * kCaRows + q_loc;

  // Q^T fragments (B operand of S^T = K Q^T): lane (query l31, d 16 s + 8 hl .. + 8), 32 VGPRs
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = *reinterpret_cast<const bf16x8*>(Q + q_id * a.q_sl + 16 * s + 8 * hl);

  // staging: thread t moves chunks t + 128 i (i < 8) of the K and V tiles: row (t >> 4) + 8 i, 16-B chunk t & 15
  const int row0 = tid >> 4, ch = tid & 15;

  // per-lane LDS read offsets: K rows (key l31 of a 32-key half, d 16 s + 8 hl); V^T transposed reads as attn_na.hip
  const int k_rd = l31 * kCaKStride + 16 * hl;
  const int grp = lane >> 4, gi = lane & 15;
  const int tq = gi >> 2, tp = gi & 3;
  const int v_rd = kCaKBuf + (4 * (grp >> 1) + tq) * kCaVStride + 32 * (grp & 1) + 8 * tp;

  f32x16 o[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
  float l_run = 0.f, m_run = -INFINITY;

  for (int t = 0; t <= qb; ++t) {
    __syncthreads();  // tile t - 1 has been read by both waves
#pragma unroll
    for (int i = 0; i < kCaPerThread; ++i) {
      const int r = row0 + 8 * i;
      const int64_t key = (int64_t)t * kKBlk + r;
      *reinterpret_cast<u32x4*>(smem + r * kCaKStride + ch * 16) =
          *reinterpret_cast<const u32x4*>(K + key * a.k_sl + ch * 8);
      *reinterpret_cast<u32x4*>(smem + kCaKBuf + r * kCaVStride + ch * 16) =
          *reinterpret_cast<const u32x4*>(V + key * a.v_sl + ch * 8);
    }
    __syncthreads();
    // S^T of the tile's two 32-key halves: register r of half hf holds key 32 hf + 8 (r / 4) + 4 hl + r % 4
    f32x16 S[2];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
      for (int r = 0; r < 16; ++r) S[hf][r] = 0.f;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const bf16x8 kr = *reinterpret_cast<const bf16x8*>(smem + k_rd + hf * 32 * kCaKStride + 32 * s);
        S[hf] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kr, qf[s], S[hf], 0, 0, 0);
      }
    }
    if (t == qb) {  // the diagonal tile: keys after the query, masked before the row max
#pragma unroll
      for (int hf = 0; hf < 2; ++hf)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (32 * hf + 8 * (r >> 2) + 4 * hl + (r & 3) > q_loc) S[hf][r] = -INFINITY;
    }
    // online row max (the row's scores sit in lanes l31 and l31 + 32); key 0 of the tile is never masked
    float tmax = S[0][0];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf)
#pragma unroll
      for (int r = 0; r < 16; ++r) tmax = fmaxf(tmax, S[hf][r]);
    tmax = fmaxf(tmax, __shfl_xor(tmax, 32)) * a.scale_log2;
    const float m_new = fmaxf(m_run, tmax);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);  // 0 at tile 0, 1 while the max stands
    l_run *= alpha;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[d][r] *= alpha;
    m_run = m_new;
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
    const char* vb = smem + v_rd;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int d = 0; d < 4; ++d) {
        typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
        typedef __attribute__((address_space(3))) const char* lds_cptr;
        const int off = 16 * ks * kCaVStride + 64 * d;
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds_cptr)(vb + off));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(lds_cptr)(vb + off + 8 * kCaVStride));
        typedef short s16x8 __attribute__((ext_vector_type(8)));
        const s16x8 r8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
        o[d] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, r8), pb[ks], o[d], 0, 0, 0);
      }
  }

  // epilogue: O^T lane (query l31), register r of d-block d holds d = 32 d + 8 (r / 4) + 4 hl + r % 4
  const float inv = 1.f / (l_run + __shfl_xor(l_run, 32));
  unsigned short* orow = O + q_id * a.o_sl;
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

bool ca_strides_ok(const int64_t* s) { return s && s[0] >= 0 && s[1] >= kD && s[2] >= kD && !((s[0] | s[1] | s[2]) % 8); }

}  // namespace

extern "C" int cp25_attn_causal(const void* q, const void* k, const void* v, void* o, int B, int Hq, int Hkv, int L,
                                int D, const int64_t* q_strides, const int64_t* k_strides, const int64_t* v_strides,
                                const int64_t* o_strides, float softmax_scale, hipStream_t stream) {
  if (!q || !k || !v || !o) return CP25_ERR_INVAL;
  if (D != kD) return CP25_ERR_INVAL;
  if (B <= 0 || Hq <= 0 || Hkv <= 0 || Hq % Hkv || L <= 0 || L % kCaRows || L > (1 << 20)) return CP25_ERR_INVAL;
  if (!ca_strides_ok(q_strides) || !ca_strides_ok(k_strides) || !ca_strides_ok(v_strides) || !ca_strides_ok(o_strides))
    return CP25_ERR_INVAL;
  if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)v) | ((uintptr_t)o)) & 15) return CP25_ERR_INVAL;
  if (!(softmax_scale > 0.f)) return CP25_ERR_INVAL;
  const int nqb = L / kCaRows;
  if ((int64_t)nqb * Hq * B > 0x7fffffff) return CP25_ERR_INVAL;
  CaArgs a;
  a.q = (const unsigned short*)q; a.k = (const unsigned short*)k; a.v = (const unsigned short*)v;
  a.o = (unsigned short*)o;
  a.q_sb = q_strides[0]; a.q_sl = q_strides[1]; a.q_sh = q_strides[2];
  a.k_sb = k_strides[0]; a.k_sl = k_strides[1]; a.k_sh = k_strides[2];
  a.v_sb = v_strides[0]; a.v_sl = v_strides[1]; a.v_sh = v_strides[2];
  a.o_sb = o_strides[0]; a.o_sl = o_strides[1]; a.o_sh = o_strides[2];
  a.Hq = Hq; a.group = Hq / Hkv; a.nqb = nqb;
  a.scale_log2 = softmax_scale * 1.4426950408889634f;
  hipLaunchKernelGGL(attn_causal_kernel, dim3((unsigned)((int64_t)nqb * Hq * B)), dim3(kCaThreads), 0, stream, a);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}
