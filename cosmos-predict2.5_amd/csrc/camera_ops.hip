// Camera features on the device (gfx950): per-pixel Pluecker rays packed into the token rows the camera-conditioned
// net's cam_encoder reads (camera/networks/minimal_v4_dit_camera_conditioned.py:1080, :1189).
//
//   cp25_plucker_tokens : world-to-camera poses [F, 3, 4] + (fx, fy, cx, cy) [F, 4], one per latent frame, ->
//                         [F * Hp * Wp, 1536] bf16 rows, the A operand of the encoder GEMM.
//
// The ray arithmetic is the reference's get_plucker_rays (_src/imaginaire/modules/camera.py:172-236): unit direction of
// the pixel centre's ray in world coordinates and the moment o x d about the camera centre o = -R^T t. The reference
// holds no code that packs the rays into the 1536-wide token feature (its camera datasets are mocks): the
// "(c m n)" packing below, c over [moment | direction], m / n the 16 x 16 pixels of a token (8x VAE, 2x patch), is
// this build's own, after PatchEmbed's channel-major pattern.
#include "cp25_common.h"

#pragma clang fp contract(off)

namespace {

// One workgroup per token (frame f, patch row hp, patch column wp), one thread per pixel (m, n) of its 16 x 16 pixels.
// Feature c of pixel (m, n) goes to column c * 256 + m * 16 + n: for each c the 256 threads write one 512-byte run.
__global__ void __launch_bounds__(256) plucker_tokens_kernel(const float* __restrict__ w2c,
                                                             const float* __restrict__ intr,
                                                             unsigned short* __restrict__ out, int Hp, int Wp) {
  const int64_t tok = blockIdx.x;
  const int hw = Hp * Wp;
  const int f = (int)(tok / hw);
  const int r = (int)(tok % hw);
  const int hp = r / Wp, wp = r % Wp;
  const int j = threadIdx.x;
  const int m = j >> 4, n = j & 15;
  const float* P = w2c + (int64_t)f * 12;  // rows [R | t]
  const float* K = intr + (int64_t)f * 4;
  const float u = (float)(wp * 16 + n) + 0.5f;
  const float v = (float)(hp * 16 + m) + 0.5f;
  // K^-1 (u, v, 1): the pixel centre at depth 1 in camera coordinates
  const float xc = (u - K[2]) / K[0];
  const float yc = (v - K[3]) / K[1];
  float d[3], o[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    d[i] = (P[i] * xc + P[4 + i] * yc) + P[8 + i];                      // R^T p
    o[i] = -((P[i] * P[3] + P[4 + i] * P[7]) + P[8 + i] * P[11]);       // -R^T t
  }
  const float nrm = fmaxf(sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]), 1e-8f);
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = d[i] / nrm;
  float mo[3];
  mo[0] = o[1] * d[2] - o[2] * d[1];
  mo[1] = o[2] * d[0] - o[0] * d[2];
  mo[2] = o[0] * d[1] - o[1] * d[0];
  unsigned short* row = out + tok * 1536 + j;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    row[i * 256] = f2bf(mo[i]);
    row[(3 + i) * 256] = f2bf(d[i]);
  }
}

}  // namespace

extern "C" int cp25_plucker_tokens(const float* w2c, const float* intrinsics, void* out, int F, int Hp, int Wp,
                                   hipStream_t stream) {
  if (!w2c || !intrinsics || !out || F <= 0 || Hp <= 0 || Wp <= 0) return CP25_ERR_INVAL;
  if ((((uintptr_t)w2c | (uintptr_t)intrinsics) & 3) || ((uintptr_t)out & 1)) return CP25_ERR_INVAL;
  const int64_t n_tok = (int64_t)F * Hp * Wp;
  if ((int64_t)Hp * Wp > 0x7fffffff || n_tok > 0x7fffffff) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(plucker_tokens_kernel, dim3((unsigned)n_tok), dim3(256), 0, stream, w2c, intrinsics,
                     (unsigned short*)out, Hp, Wp);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}
