// Where does an LDS-DMA piece (buffer_load_dwordx4 ... lds) land when M0 holds an LDS byte address past 64 KiB?
// gfx950 has 160 KiB of LDS per CU; this probe answers whether the DMA's destination base (M0) reaches all of it.
// One wave fills 147 456 B of LDS with a marker, moves one 1 KiB piece (lane l: 16 B, each word = 0x11110000 + word
// index) to LDS byte address M0 = dst, and copies the LDS out. The host prints where the piece's words were found.
//   hipcc --offload-arch=gfx950 -O2 tools/lab/lds_dma_probe.hip -o tools/lab/lds_dma_probe && tools/lab/lds_dma_probe
#include <hip/hip_runtime.h>

#include <cstdio>
#include <vector>

constexpr int kLds = 147456;
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const char* lds_char_ptr;

__global__ void __launch_bounds__(64, 1) probe(const unsigned* src, unsigned* out, unsigned dst) {
  __shared__ __attribute__((aligned(16))) char smem[kLds];
  unsigned* w = reinterpret_cast<unsigned*>(smem);
  for (int i = threadIdx.x; i < kLds / 4; i += 64) w[i] = 0xEEEEEEEEu;
  __syncthreads();
  const uint64_t p = (uint64_t)src;
  const u32x4 rs = {(unsigned)p, (unsigned)(p >> 32) & 0xffffu, 1024u, 0x00020000u};
  const unsigned m0 = (unsigned)(uintptr_t)(lds_char_ptr)smem + dst;
  const int off = 16 * (int)threadIdx.x;
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 4\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_waitcnt vmcnt(0)"
               ::"s"(m0), "v"(off), "s"(rs) : "memory");
  __syncthreads();
  for (int i = threadIdx.x; i < kLds / 4; i += 64) out[i] = w[i];
}

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main() {
  std::vector<unsigned> h(256), o(kLds / 4);
  for (int i = 0; i < 256; ++i) h[i] = 0x11110000u + i;
  unsigned *src, *out;
  CK(hipMalloc(&src, 1024));
  CK(hipMalloc(&out, kLds));
  CK(hipMemcpy(src, h.data(), 1024, hipMemcpyHostToDevice));
  const unsigned dsts[] = {4096u, 61440u, 65536u + 4096u, 131072u + 4096u, (unsigned)kLds - 1024u};
  for (unsigned dst : dsts) {
    hipLaunchKernelGGL(probe, dim3(1), dim3(64), 0, 0, src, out, dst);
    CK(hipDeviceSynchronize());
    CK(hipMemcpy(o.data(), out, kLds, hipMemcpyDeviceToHost));
    int first = -1, n = 0, inorder = 0;
    for (int i = 0; i < kLds / 4; ++i)
      if (o[i] != 0xEEEEEEEEu) {
        if (first < 0) first = i;
        inorder += o[i] == 0x11110000u + (unsigned)(i - first);
        ++n;
      }
    printf("M0 = LDS byte %6u: %d words changed, first at byte %d (%s), %d in order\n", dst, n, first * 4,
           first * 4 == (int)dst ? "where M0 points" : "ELSEWHERE", inorder);
  }
  return 0;
}
