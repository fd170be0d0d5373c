// csrc/attn_route.h compiled alone by a host compiler (no HIP), for tests/test_attn_route_cpu.py. Answers queries read
// from stdin, one per line, as libcp25.so answers them on a 256-CU device:
//   name <self form> <cross form> <Lk> <softmax_scale> <q bound> <k bound> <prescaled> <fp8>   -> cp25_attn_kernel
//   plan <self form> <B> <H> <Lq> <Lk>          -> cp25_attn_plan and cp25_attn_tail_workspace_bytes, space-separated
// (floats in any strtod form, rounded to float as a C caller's would be). Every plan query also walks the tail plans of
// its shape at the three workgroup heights and aborts on a plan that breaks plan_tail's contract.
#include <cstdio>
#include <cstdlib>

#include "attn_route.h"

using namespace cp25attn;

constexpr int64_t kCus = 256;
// the attn_fwd_wq forms attn_wide.hip builds (wq_kernel): 320 and 384 rows, fixed shift
constexpr unsigned kWideBuilt = wide_bit(320, 0) | wide_bit(384, 0);

#define REQUIRE(cond)                                                              \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      std::fprintf(stderr, "%s:%d: %s: line '%s'\n", __FILE__, __LINE__, #cond, line); \
      std::exit(1);                                                                \
    }                                                                              \
  } while (0)

// plan_tail's contract: at most kMaxTailSegs segments of >= 2 splits, disjoint, covering exactly the last nwg % cus
// tiles in order, each inside one (b, h); ws_need the largest segment's partials
static void walk_tail(int B, int H, int Lq, int Lk, int qblk, const char* line) {
  TailSeg seg[kMaxTailSegs];
  size_t need = 12345;
  double saved = -1.0;
  const int n = plan_tail(B, H, Lq, Lk, qblk, kCus, seg, &need, &saved);
  REQUIRE(n >= 0 && n <= kMaxTailSegs);
  if (n == 0) {
    REQUIRE(need == 0 && saved == 0.0);
    return;
  }
  const int64_t nqb = ceil_div(Lq, qblk), nwg = nqb * B * H;
  int64_t t = nwg - nwg % kCus;
  size_t largest = 0;
  REQUIRE(t < nwg && saved > 0.0);
  for (int i = 0; i < n; ++i) {
    const TailSeg& g = seg[i];
    REQUIRE(g.s >= 2 && g.s <= 8 && g.s <= ceil_div(Lk, kKBlk) && g.nblk >= 1);
    REQUIRE(g.bh >= 0 && g.bh < B * H && g.qb_lo >= 0 && g.qb_lo + g.nblk <= nqb);
    REQUIRE((int64_t)g.bh * nqb + g.qb_lo == t);  // starts where the previous one (or the whole rounds) ended
    t += g.nblk;
    const int64_t rows = std::min<int64_t>(Lq, (int64_t)(g.qb_lo + g.nblk) * qblk) - (int64_t)g.qb_lo * qblk;
    REQUIRE(rows > 0);
    largest = std::max(largest, (size_t)g.s * rows * (kD + 1) * 4);
  }
  REQUIRE(t == nwg);
  REQUIRE(need == largest);
}

int main() {
  char line[256], sc[64], qb[64], kb[64];
  while (std::fgets(line, sizeof line, stdin)) {
    int self_form, cross_form, Lk, prescaled, fp8, B, H, Lq;
    if (std::sscanf(line, "name %d %d %d %63s %63s %63s %d %d", &self_form, &cross_form, &Lk, sc, qb, kb, &prescaled,
                    &fp8) == 8) {
      const float scale = (float)std::strtod(sc, nullptr);
      const AttnQuery q{Lk, prescaled != 0, prescaled ? 1.f : scale * 1.4426950408889634f,
                        (float)std::strtod(qb, nullptr), (float)std::strtod(kb, nullptr), fp8, prescaled == 2, false, 1,
                        self_form, cross_form, kWideBuilt};
      const AttnRoute r = attn_route(q);
      const char* name = attn_route_name(r);
      REQUIRE(name != nullptr);
      REQUIRE(r.threads == (r.family == AttnFamily::wq ? kWqThreads : kThreads));
      REQUIRE((r.rows == kQBlk) == (r.family != AttnFamily::wq));
      std::printf("%s\n", name);
    } else if (std::sscanf(line, "plan %d %d %d %d %d", &self_form, &B, &H, &Lq, &Lk) == 5) {
      std::printf("%d %zu\n", plan_split(B, H, Lq, Lk, kQBlk, kCus),
                  tail_workspace_bytes(B, H, Lq, Lk, self_form, kCus));
      for (int qblk : {256, 320, 384}) walk_tail(B, H, Lq, Lk, qblk, line);
    } else {
      REQUIRE(!"a query");
    }
  }
  return 0;
}
