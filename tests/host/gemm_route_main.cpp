// Stand-alone driver of csrc/gemm_route.h (no HIP): reads queries from stdin, prints what the header plans.
//   plan M N K epilogue cus   ->  <packed plan> <workspace bytes at the plan's split>
//   runs nk S                 ->  begin:len of each of the S runs over nk K-tiles, space-separated
//   ws M N K split            ->  <workspace bytes>
// tests/test_gemm_route_cpu.py builds it with g++ (also under ASan + UBSan) and compares it with libcp25.so.
#include <cstdio>
#include <cstring>

#include "gemm_route.h"

int main() {
  char op[16];
  while (std::scanf("%15s", op) == 1) {
    if (!std::strcmp(op, "plan")) {
      int M, N, K, epi, cus;
      if (std::scanf("%d %d %d %d %d", &M, &N, &K, &epi, &cus) != 5) return 2;
      const cp25gemm::GemmPlan p = cp25gemm::gemm_plan(M, N, K, epi, cus);
      std::printf("%d %lld\n", cp25gemm::pack_plan(p), (long long)cp25gemm::workspace_bytes_of(M, N, K, p.split));
    } else if (!std::strcmp(op, "runs")) {
      int nk, S;
      if (std::scanf("%d %d", &nk, &S) != 2 || S < 1) return 2;
      for (int r = 0; r < S; ++r)
        std::printf("%d:%d%c", cp25gemm::run_begin(nk, S, r), cp25gemm::run_len(nk, S, r), r + 1 < S ? ' ' : '\n');
    } else if (!std::strcmp(op, "ws")) {
      int M, N, K, S;
      if (std::scanf("%d %d %d %d", &M, &N, &K, &S) != 4) return 2;
      std::printf("%lld\n", (long long)cp25gemm::workspace_bytes_of(M, N, K, S));
    } else {
      return 2;
    }
  }
  return 0;
}
