// Pixel path kernels (gfx950): antialiased resize + centre crop on uint8 frames, uint8 -> VAE clip and VAE clip ->
// uint8. Memory-bound code behind cp25_resize_crop_u8 / cp25_u8_to_clip / cp25_clip_to_u8 (include/cp25.h).
// Strides are in elements of the tensor's own type, so each kernel serves planar and channels-last layouts.
#include "cp25_common.h"

namespace {

// ------------------------------------------------------------------------------------------- resize + crop
// A workgroup owns an RZ_TH x RZ_TW tile of the crop window, all C channels. For in/out <= 4 the source rows the
// tile's outputs touch span at most 4 (T - 1) + 2 * 4 + 1 = 4 T + 5 (start = int(center - support + 0.5) and
// end = int(center + support + 0.5) of outputs T - 1 apart), which sizes the LDS tiles below.
constexpr int RZ_TH = 8, RZ_TW = 32, RZ_THREADS = 256, RZ_MAXTAPS = 9, RZ_MAXC = 4;
constexpr int RZ_SR = 4 * RZ_TH + 5;        // source rows per tile
constexpr int RZ_SC = 4 * RZ_TW + 5;        // source columns per tile
constexpr int RZ_RUN = (RZ_SC + 3 + 3) / 4 * 4;   // LDS bytes of one staged row of one channel (+ <= 3 alignment bytes)
constexpr int RZ_ORUN = RZ_TW + 4;          // LDS bytes of one output row of one channel (+ <= 3 alignment bytes)
static_assert(RZ_THREADS == 8 * RZ_TW, "thread = (column of the tile, one of 8 row groups)");
static_assert(RZ_TH * RZ_MAXC * RZ_ORUN <= RZ_SR * RZ_MAXC * RZ_RUN, "the output tile reuses the source tile's LDS");

// How a row of pixels lies in memory: a run is a stretch of contiguous bytes copied with dword accesses.
enum { RZ_PLANAR = 0,    // x stride 1: one run per (row, channel)
       RZ_CLAST = 1,     // c stride 1, x stride C: one run per row, channels interleaved
       RZ_GATHER = 2 };  // anything else: byte by byte

struct RzParams {
  const uint8_t* src;
  uint8_t* dst;  // the crop window's first pixel
  int64_t ssn, ssc, ssy, ssx, dsn, dsc, dsy, dsx;
  const int* ys; const int* yc; const float* yw;
  const int* xs; const int* xc; const float* xw;
  int ytaps, xtaps, C, Hin, Win, top, left, th, tw, tiles_x, tiles_y, smode, dmode;
};

__device__ __forceinline__ int lowbits(const void* p) { return (int)(reinterpret_cast<uintptr_t>(p) & 3); }

__global__ __launch_bounds__(RZ_THREADS) void resize_crop_u8_kernel(const RzParams p) {
  __shared__ __attribute__((aligned(16))) uint8_t s_src[RZ_SR * RZ_MAXC * RZ_RUN];
  __shared__ float s_h[RZ_SR * RZ_MAXC * RZ_TW];
  const int tid = threadIdx.x, C = p.C;
  int b = blockIdx.x;
  const int tx = b % p.tiles_x;
  b /= p.tiles_x;
  const int ty = b % p.tiles_y, n = b / p.tiles_y;
  const int oy0 = ty * RZ_TH, ox0 = tx * RZ_TW;  // inside the window
  const int nth = min(RZ_TH, p.th - oy0), ntw = min(RZ_TW, p.tw - ox0);
  const int ry0 = p.top + oy0, rx0 = p.left + ox0;  // inside the resized extent (table rows)
  // source rectangle of the tile, clamped to the frame and to the LDS tile
  const int ylo = min(max(p.ys[ry0], 0), p.Hin - 1), xlo = min(max(p.xs[rx0], 0), p.Win - 1);
  const int nrows = min(max(min(p.ys[ry0 + nth - 1] + p.yc[ry0 + nth - 1], p.Hin) - ylo, 0), RZ_SR);
  const int ncols = min(max(min(p.xs[rx0 + ntw - 1] + p.xc[rx0 + ntw - 1], p.Win) - xlo, 0), RZ_SC);
  const uint8_t* sf = p.src + (int64_t)n * p.ssn;

  // 1) stage the source bytes. A run lands in LDS at the byte offset (address & 3) of its global address, so that
  //    aligned dwords of HBM are aligned dwords of LDS; dwords that straddle a run's end go byte by byte.
  if (p.smode == RZ_GATHER) {
    for (int i = tid; i < nrows * C * ncols; i += RZ_THREADS) {
      const int x = i % ncols, rc = i / ncols, c = rc % C, r = rc / C;
      s_src[rc * RZ_RUN + x] = sf[c * p.ssc + (int64_t)(ylo + r) * p.ssy + (int64_t)(xlo + x) * p.ssx];
    }
  } else {
    const bool pl = p.smode == RZ_PLANAR;
    const int nruns = pl ? nrows * C : nrows, runlen = pl ? ncols : ncols * C;
    const int pitch = pl ? RZ_RUN : RZ_MAXC * RZ_RUN, dwpr = (runlen + 6) / 4;  // dwords a run can touch (<= pitch / 4)
    for (int i = tid; i < nruns * dwpr; i += RZ_THREADS) {
      const int run = i / dwpr, k = i - run * dwpr;
      const uint8_t* g = pl ? sf + (run % C) * p.ssc + (int64_t)(ylo + run / C) * p.ssy + xlo
                            : sf + (int64_t)(ylo + run) * p.ssy + (int64_t)xlo * C;
      const int lo = 4 * k - lowbits(g);  // this dword's first byte, relative to the run
      if (lo >= runlen) continue;
      uint8_t* l = s_src + run * pitch + 4 * k;
      if (lo >= 0 && lo + 4 <= runlen) {
        *reinterpret_cast<uint32_t*>(l) = *reinterpret_cast<const uint32_t*>(g + lo);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (lo + e >= 0 && lo + e < runlen) l[e] = g[lo + e];
      }
    }
  }
  __syncthreads();

  // 2) horizontal pass: thread = (output column lx, row group); the column's weights stay in registers
  const int lx = tid & (RZ_TW - 1), grp = tid / RZ_TW;
  float wx[RZ_MAXTAPS];
  int xs0 = 0, xcnt = 0;
  if (lx < ntw) {
    const int rx = rx0 + lx;
    xs0 = p.xs[rx] - xlo;
    xcnt = min(p.xc[rx], p.xtaps);
#pragma unroll
    for (int j = 0; j < RZ_MAXTAPS; ++j) wx[j] = j < xcnt ? p.xw[(int64_t)rx * p.xtaps + j] : 0.f;
    for (int rc = grp; rc < nrows * C; rc += RZ_THREADS / RZ_TW) {
      const int r = rc / C, c = rc - r * C;
      const uint8_t* row;
      int es = 1;
      if (p.smode == RZ_PLANAR) {
        row = s_src + rc * RZ_RUN + lowbits(sf + c * p.ssc + (int64_t)(ylo + r) * p.ssy + xlo);
      } else if (p.smode == RZ_CLAST) {
        row = s_src + r * (RZ_MAXC * RZ_RUN) + lowbits(sf + (int64_t)(ylo + r) * p.ssy + (int64_t)xlo * C) + c;
        es = C;
      } else {
        row = s_src + rc * RZ_RUN;
      }
      float h = 0.f;
#pragma unroll
      for (int j = 0; j < RZ_MAXTAPS; ++j) {  // ascending x; taps in [count, taps) carry weight 0
        if (j >= p.xtaps) break;
        const int xi = xs0 + j;
        if ((unsigned)xi < (unsigned)ncols) h = fmaf(wx[j], (float)row[xi * es], h);
      }
      s_h[rc * RZ_TW + lx] = h;
    }
  }
  __syncthreads();

  // 3) vertical pass from the fp32 tile, round half even, clamp; bytes go to LDS (run layouts) or straight out
  uint8_t* df = p.dst + (int64_t)n * p.dsn;
  if (lx < ntw) {
    for (int oc = grp; oc < nth * C; oc += RZ_THREADS / RZ_TW) {
      const int oy = oc / C, c = oc - oy * C, ry = ry0 + oy;
      const int ys0 = p.ys[ry] - ylo, ycnt = min(min(p.yc[ry], p.ytaps), RZ_MAXTAPS);
      float v = 0.f;
      for (int j = 0; j < ycnt; ++j) {  // ascending y
        const int yi = ys0 + j;
        if ((unsigned)yi < (unsigned)nrows) v = fmaf(p.yw[(int64_t)ry * p.ytaps + j], s_h[(yi * C + c) * RZ_TW + lx], v);
      }
      const uint8_t u = (uint8_t)(int)fminf(fmaxf(rintf(v), 0.f), 255.f);
      if (p.dmode == RZ_PLANAR) {
        s_src[oc * RZ_ORUN + lowbits(df + c * p.dsc + (int64_t)(oy0 + oy) * p.dsy + ox0) + lx] = u;
      } else if (p.dmode == RZ_CLAST) {
        s_src[oy * (RZ_MAXC * RZ_ORUN) + lowbits(df + (int64_t)(oy0 + oy) * p.dsy + (int64_t)ox0 * C) + lx * C + c] = u;
      } else {
        df[c * p.dsc + (int64_t)(oy0 + oy) * p.dsy + (int64_t)(ox0 + lx) * p.dsx] = u;
      }
    }
  }
  if (p.dmode == RZ_GATHER) return;
  __syncthreads();

  // 4) write the window's bytes: whole dwords inside a run, bytes at its ragged ends; nothing outside the window
  {
    const bool pl = p.dmode == RZ_PLANAR;
    const int nruns = pl ? nth * C : nth, runlen = pl ? ntw : ntw * C;
    const int pitch = pl ? RZ_ORUN : RZ_MAXC * RZ_ORUN, dwpr = (runlen + 6) / 4;
    for (int i = tid; i < nruns * dwpr; i += RZ_THREADS) {
      const int run = i / dwpr, k = i - run * dwpr;
      uint8_t* g = pl ? df + (run % C) * p.dsc + (int64_t)(oy0 + run / C) * p.dsy + ox0
                      : df + (int64_t)(oy0 + run) * p.dsy + (int64_t)ox0 * C;
      const int lo = 4 * k - lowbits(g);
      if (lo >= runlen) continue;
      const uint8_t* l = s_src + run * pitch + 4 * k;
      if (lo >= 0 && lo + 4 <= runlen) {
        *reinterpret_cast<uint32_t*>(g + lo) = *reinterpret_cast<const uint32_t*>(l);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (lo + e >= 0 && lo + e < runlen) g[lo + e] = l[e];
      }
    }
  }
}

int layout_mode(int C, int64_t sc, int64_t sx) {
  if (sx == 1) return RZ_PLANAR;
  if (sc == 1 && sx == C) return RZ_CLAST;
  return RZ_GATHER;
}

// ------------------------------------------------------------------------------------------- uint8 <-> clip
constexpr int PX_THREADS = 256;

// one thread per pixel: C strided bytes in, 16 bf16 channels (32 B, two 16-B stores) out
__global__ __launch_bounds__(PX_THREADS) void u8_to_clip_kernel(const uint8_t* __restrict__ src, int64_t sc, int64_t st,
                                                                int64_t sy, int64_t sx, int C, int H, int W,
                                                                unsigned short* __restrict__ dst, int64_t npix) {
  const int64_t i = (int64_t)blockIdx.x * PX_THREADS + threadIdx.x;
  if (i >= npix) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const int64_t t = i / ((int64_t)W * H);
  const uint8_t* s = src + t * st + (int64_t)y * sy + (int64_t)x * sx;
  unsigned short o[16];
#pragma unroll
  for (int c = 0; c < 16; ++c)  // bf16(u) / 127.5 -> bf16, - 1.0 -> bf16: the two roundings of the torch expression
    o[c] = c < C ? f2bf(rbf((float)s[c * sc] / 127.5f) - 1.0f) : (unsigned short)0;
  u32x4 lo4, hi4;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    lo4[e] = (unsigned)o[2 * e] | ((unsigned)o[2 * e + 1] << 16);
    hi4[e] = (unsigned)o[8 + 2 * e] | ((unsigned)o[8 + 2 * e + 1] << 16);
  }
  u32x4* d = reinterpret_cast<u32x4*>(dst + i * 16);
  d[0] = lo4;
  d[1] = hi4;
}

// one thread per pixel: C strided bf16 in, C strided bytes out
__global__ __launch_bounds__(PX_THREADS) void clip_to_u8_kernel(const unsigned short* __restrict__ src, int64_t st,
                                                                int64_t sy, int64_t sx, int64_t sc, int C, int H, int W,
                                                                uint8_t* __restrict__ dst, int64_t dt, int64_t dy,
                                                                int64_t dx, int64_t dc, int64_t npix) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * PX_THREADS + threadIdx.x;
  if (i >= npix) return;
  const int x = (int)(i % W), y = (int)((i / W) % H);
  const int64_t t = i / ((int64_t)W * H);
  const unsigned short* s = src + t * st + (int64_t)y * sy + (int64_t)x * sx;
  uint8_t* d = dst + t * dt + (int64_t)y * dy + (int64_t)x * dx;
  for (int c = 0; c < C; ++c) {
    const float f = fminf(fmaxf((bf2f(s[c * sc]) + 1.0f) / 2.0f, 0.f), 1.f);
    d[c * dc] = (uint8_t)(int)(f * 255.0f);  // truncation
  }
}

bool strides_ok(const int64_t* s, int n) {
  for (int i = 0; i < n; ++i)
    if (s[i] < 0) return false;
  return true;
}

}  // namespace

extern "C" {

int cp25_resize_crop_u8(const void* src, const int64_t* src_strides, int N, int C, int Hin, int Win, void* dst,
                        const int64_t* dst_strides, const int32_t* y_start, const int32_t* y_count, const float* y_w,
                        int y_taps, const int32_t* x_start, const int32_t* x_count, const float* x_w, int x_taps, int rh,
                        int rw, int top, int left, int th, int tw, hipStream_t stream) {
  if (!src || !dst || !src_strides || !dst_strides || !y_start || !y_count || !y_w || !x_start || !x_count || !x_w)
    return CP25_ERR_INVAL;
  if (N < 1 || C < 1 || C > RZ_MAXC || Hin < 1 || Win < 1 || rh < 1 || rw < 1) return CP25_ERR_INVAL;
  if ((int64_t)Hin > 4 * (int64_t)rh || (int64_t)Win > 4 * (int64_t)rw) return CP25_ERR_INVAL;  // in/out <= 4 per axis
  if (y_taps < 1 || y_taps > RZ_MAXTAPS || x_taps < 1 || x_taps > RZ_MAXTAPS) return CP25_ERR_INVAL;
  if (top < 0 || left < 0 || th < 1 || tw < 1 || (int64_t)top + th > rh || (int64_t)left + tw > rw) return CP25_ERR_INVAL;
  if (!strides_ok(src_strides, 4) || !strides_ok(dst_strides, 4)) return CP25_ERR_INVAL;
  RzParams p;
  p.src = static_cast<const uint8_t*>(src);
  p.dst = static_cast<uint8_t*>(dst);
  p.ssn = src_strides[0]; p.ssc = src_strides[1]; p.ssy = src_strides[2]; p.ssx = src_strides[3];
  p.dsn = dst_strides[0]; p.dsc = dst_strides[1]; p.dsy = dst_strides[2]; p.dsx = dst_strides[3];
  p.ys = y_start; p.yc = y_count; p.yw = y_w; p.xs = x_start; p.xc = x_count; p.xw = x_w;
  p.ytaps = y_taps; p.xtaps = x_taps; p.C = C; p.Hin = Hin; p.Win = Win;
  p.top = top; p.left = left; p.th = th; p.tw = tw;
  p.tiles_x = (int)cdiv(tw, RZ_TW);
  p.tiles_y = (int)cdiv(th, RZ_TH);
  p.smode = layout_mode(C, p.ssc, p.ssx);
  p.dmode = layout_mode(C, p.dsc, p.dsx);
  const int64_t blocks = (int64_t)N * p.tiles_x * p.tiles_y;
  if (blocks > 0x7fffffffLL) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(resize_crop_u8_kernel, dim3((unsigned)blocks), dim3(RZ_THREADS), 0, stream, p);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

int cp25_u8_to_clip(const void* src, const int64_t* src_strides, int C, int T, int H, int W, void* dst,
                    hipStream_t stream) {
  if (!src || !dst || !src_strides || C < 1 || C > 16 || T < 1 || H < 1 || W < 1) return CP25_ERR_INVAL;
  if (!strides_ok(src_strides, 4) || (reinterpret_cast<uintptr_t>(dst) & 15)) return CP25_ERR_INVAL;
  const int64_t npix = (int64_t)T * H * W, blocks = cdiv(npix, PX_THREADS);
  if (blocks > 0x7fffffffLL) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(u8_to_clip_kernel, dim3((unsigned)blocks), dim3(PX_THREADS), 0, stream,
                     static_cast<const uint8_t*>(src), src_strides[0], src_strides[1], src_strides[2], src_strides[3],
                     C, H, W, static_cast<unsigned short*>(dst), npix);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

int cp25_clip_to_u8(const void* src, const int64_t* src_strides, int T, int H, int W, int C, void* dst,
                    const int64_t* dst_strides, hipStream_t stream) {
  if (!src || !dst || !src_strides || !dst_strides || C < 1 || C > 4 || T < 1 || H < 1 || W < 1) return CP25_ERR_INVAL;
  if (!strides_ok(src_strides, 4) || !strides_ok(dst_strides, 4)) return CP25_ERR_INVAL;
  const int64_t npix = (int64_t)T * H * W, blocks = cdiv(npix, PX_THREADS);
  if (blocks > 0x7fffffffLL) return CP25_ERR_INVAL;
  hipLaunchKernelGGL(clip_to_u8_kernel, dim3((unsigned)blocks), dim3(PX_THREADS), 0, stream,
                     static_cast<const unsigned short*>(src), src_strides[0], src_strides[1], src_strides[2],
                     src_strides[3], C, H, W, static_cast<uint8_t*>(dst), dst_strides[0], dst_strides[1], dst_strides[2],
                     dst_strides[3], npix);
  CP25_LAUNCH_CHECK();
  return CP25_OK;
}

}  // extern "C"
