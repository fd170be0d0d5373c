// The host-side decisions of an attention launch, once: which kernel, which softmax mode, how many query rows per
// workgroup (attn_route), what that kernel is called (attn_route_name), and how the last partial round and the key
// range are split (plan_tail, plan_split). Plain C++17 with no HIP in it, so a host compiler alone builds and tests it
// (tests/host/attn_route_main.cpp); the CU count is a parameter. attn_fwd.hip's launch and cp25_attn_kernel both take
// their route from here, so the name reported is the kernel that runs. A new route is one branch of attn_route, one row
// of kRouteNames and one case of the kernel lookup in attn_fwd.hip.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace cp25attn {

constexpr int kD = 128;          // head dim
constexpr int kQBlk = 256;       // query rows per workgroup of attn_fwd_m16 / attn_fwd_f8 (8 waves x 32 rows)
constexpr int kKBlk = 64;        // keys per tile
constexpr int kThreads = 512;    // attn_fwd_m16 / attn_fwd_f8: 8 waves
constexpr int kWqThreads = 256;  // attn_fwd_wq: 4 waves, one per SIMD
// Softmax-shift ranges (log2 units). A term is 2^(s - shift) <= 2^kTop, so a row sum is <= Lk 2^96 and O = sum P v is
// <= Lk 2^96 max|v|: inside fp32 (2^128) while max|v| Lk < 2^32, e.g. |v| < 2.6e4 at config 4's Lk = 163 800 (the
// DiT's v is a bf16 projection of a normalised row, orders of magnitude smaller; checked at the top of the window
// over 163 840 keys with |v| ~ 400 by tests/test_attn_m16_gpu.py::test_m16_zero_shift_top_of_window_long_keys). The
// kernels' contract guard poisons a row whose sum overflows. bf16 P has the fp32 exponent range.
constexpr float kTop = 96.f;        // zero / fixed shift: largest exponent a term may reach
constexpr float kMaxBound = 98.f;   // fixed shift: largest score bound b (smallest row-max term 2^(96 - 2 b) >= 2^-100)
constexpr float kPDrop = 60.f;      // fixed shift (round 6): rows shift by floor(min(b_row + 60, 126 - b_row)), so
                                    // P <= 2^-59 where b_row <= 33 and P <= 2^(2 b_row - 125) past it, the row's
                                    // largest term >= 2^-126. Small P runs the power-limited loop faster (P <= 2 vs
                                    // 2^17: -0.8 %; 2^-59 vs 2: -0.7 %, profiles/r6/shift_power/)
constexpr float kGateFixed = 110.f; // gated pair: a block whose data-tight bound is <= 110 runs the fixed shift, whose
                                    // rows then keep P <= 2^(2 * 110 - 125) = 2^95 (inside the zero-shift window's 2^96)
constexpr float kTopF8 = 60.f;      // fp8 Q K^T form: P = exp2(S) unshifted for bound products up to this
constexpr float kLazy = 24.f;       // online max: rescale only when a row max exceeds the shift by more (P <= 2^24)
// fp8 P.V: the e4m3 rounding of q and k (each element within 2^-4 relative) gives |q8| |k8| <= 1.13 |q| |k|, and the
// e5m2 window [2^-15, 2^15] holds a term of every row while 1.13 qb kb <= 30 (shift 1.13 qb kb - 15 <= 15)
constexpr double kF8Round = 1.13;
constexpr double kF8PvSpan = 30.0;
// Launches of up to 4096 keys are the text cross-attention (own symbols in profiles, the zero shift, the persistent
// form); longer ones the self-attention (whole-bound fixed shift, attn_fwd_wq, tail splits)
constexpr int kCrossMaxKeys = 4096;
// attn_fwd_wq's width under the library's routing: 384 rows, measured -7.4 % per launch against attn_fwd_m16 at the
// metric launch (320: -5.0 %) and -8.8 % at a CP = 8 rank's 13 640 x 109 120 (320: -5.5 %); up to 8192 keys 320 rows,
// which at config 5's L = 4800 measured -15 % against -6 % for 384 (its 480 shorter workgroups fill the second round
// better than 416 longer ones). profiles/r13/attn_wide/SUMMARY.md.
constexpr int kWq320MaxKeys = 8192;

constexpr int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---- the route ----

enum class AttnFamily { m16, wq, f8 };
enum class AttnKind { self, cross };

// bit of one attn_fwd_wq form (rows 320 / 384, mode 0 / 1) in AttnQuery::wide_built; 0: no such form
constexpr unsigned wide_bit(int rows, int mode) {
  return (rows == 320 || rows == 384) && (mode == 0 || mode == 1) ? 1u << (2 * (rows == 384) + mode) : 0u;
}

// What a route depends on, and nothing else
struct AttnQuery {
  int Lk;
  bool prescaled;      // q rows carry softmax_scale * log2 e
  float scale_log2;    // softmax_scale * log2 e (read only where q is not prescaled)
  float q_norm_bound, k_norm_bound;  // 0: unknown
  int fp8;             // 0 bf16; 1 Q K^T on e4m3 q / k; 2 also P.V on e5m2 P and e4m3 v
  bool has_kslots;     // the measured key bound in device memory (cp25_attn_fwd_prescaled_kslots)
  bool has_qnorm;      // q normalised in the kernel (cp25_attn_fwd_prescaled_qnorm)
  int n_split;
  int self_form;       // cp25_attn_self_select: 0 attn_fwd_m16 everywhere, 1 the library's width, 320 / 384 forced
  int cross_form;      // cp25_attn_cross_select: 1 the persistent form where it applies, 0 one workgroup per block
  unsigned wide_built; // wide_bit(rows, mode) of every attn_fwd_wq form the library holds
};

struct AttnRoute {
  AttnFamily family;
  AttnKind kind;
  bool prescaled;   // (f8: always)
  int mode;         // m16 / wq softmax shift: 0 fixed, 1 zero, 2 online max (f8: 0; the gated pair: 2, below)
  bool gated;       // m16: the same grid twice, kGate 1 in the fixed mode, then kGate 2 in the online mode
  bool persistent;  // m16 cross: one workgroup per CU over runs of blocks
  int f8;           // attn_fwd_f8's kF8: 0 none, 1 Q K^T, 3 Q K^T and P.V
  int rows;         // query rows per workgroup: 256, or attn_fwd_wq's 320 / 384
  int threads;
};

// query rows per workgroup of attn_fwd_wq under this form for a launch it supports, or 0: none
inline int wide_rows_of(int self_form, int Lk) {
  if (self_form == 0 || Lk <= kCrossMaxKeys) return 0;
  return self_form == 1 ? (Lk > kWq320MaxKeys ? 384 : 320) : self_form;
}

// The softmax-shift mode from the bounds (their product in log2 units; |q_row| <= q_norm_bound): 1 zero shift
// (pre-scaled q, product <= 96), 0 fixed per-row shift (product <= 98), 2 online max (larger or unknown). Long-key
// launches (round 6): a product <= kGateFixed (110) takes the fixed mode, whose rows then shift by their whole bound to
// b_row 63 (P <= 2) and by floor(126 - b_row) past it (P <= 2^95): small P, measured 0.8 % faster than the zero shift
// at the metric launch, the same cycles at a higher power-limited clock (profiles/r6/shift_power/). Short-key launches
// keep the zero shift (the persistent cross-attention has no fixed mode).
// The gated pair (k-norm slots given) runs where these weight bounds alone would leave the launch on the online max
// (long keys: past kGateFixed; short keys: past the zero-shift window). It is tested before fp8, which no launch
// combines with k-norm slots.
// The persistent form runs unsplit cross-attention launches in the zero-shift and online modes with >= 2 key tiles
// (its Q path has no normalisation). attn_fwd_wq runs prescaled, ungated bf16 long-key launches in a mode it is built
// for (the fixed shift: the mode of every long-key launch with usable bounds), bit-identical per row to attn_fwd_m16.
inline AttnRoute attn_route(const AttnQuery& q) {
  const bool cross = q.Lk <= kCrossMaxKeys;
  const double bb = (double)q.q_norm_bound * q.k_norm_bound * (q.prescaled ? 1.0 : q.scale_log2);
  int mode;
  if (!(q.q_norm_bound > 0.f && q.k_norm_bound > 0.f)) mode = 2;
  else if (!cross && bb <= kGateFixed) mode = 0;
  else if (bb > kMaxBound) mode = 2;
  else mode = q.prescaled && bb <= kTop ? 1 : 0;

  AttnRoute r{AttnFamily::m16, cross ? AttnKind::cross : AttnKind::self, q.prescaled, mode, false, false, 0, kQBlk,
              kThreads};
  if (q.prescaled && q.has_kslots && (cross ? mode != 1 : mode == 2)) {
    r.gated = true;
    r.mode = 2;
  } else if (q.fp8 != 0) {
    r.family = AttnFamily::f8;
    r.prescaled = true;
    r.mode = 0;
    r.f8 = q.fp8 == 2 ? 3 : 1;
  } else if (q.cross_form == 1 && cross && q.n_split == 1 && !q.has_qnorm && mode != 0 &&
             ceil_div(q.Lk, kKBlk) >= 2) {
    r.persistent = true;
  } else if (q.prescaled && mode != 2) {
    const int rows = wide_rows_of(q.self_form, q.Lk);
    if (rows && (q.wide_built & wide_bit(rows, mode))) {
      r.family = AttnFamily::wq;
      r.rows = rows;
      r.threads = kWqThreads;
    }
  }
  return r;
}

// Every route attn_route can return, with the name cp25_attn_kernel reports for it
struct AttnRouteName { AttnFamily family; AttnKind kind; bool prescaled; int mode; bool gated, persistent; int f8, rows;
                       const char* name; };
constexpr AttnRouteName kRouteNames[] = {
    // family, kind, prescaled, mode, gated, persistent, f8, rows
    {AttnFamily::m16, AttnKind::self, false, 0, false, false, 0, 256, "attn_fwd_m16<self, fixed shift>"},
    {AttnFamily::m16, AttnKind::self, false, 2, false, false, 0, 256, "attn_fwd_m16<self, online max>"},
    {AttnFamily::m16, AttnKind::self, true, 0, false, false, 0, 256, "attn_fwd_m16<self, prescaled, fixed shift>"},
    {AttnFamily::m16, AttnKind::self, true, 1, false, false, 0, 256, "attn_fwd_m16<self, prescaled, zero shift>"},
    {AttnFamily::m16, AttnKind::self, true, 2, false, false, 0, 256, "attn_fwd_m16<self, prescaled, online max>"},
    {AttnFamily::m16, AttnKind::cross, false, 0, false, false, 0, 256, "attn_fwd_m16<cross, fixed shift>"},
    {AttnFamily::m16, AttnKind::cross, false, 2, false, false, 0, 256, "attn_fwd_m16<cross, online max>"},
    {AttnFamily::m16, AttnKind::cross, true, 0, false, false, 0, 256, "attn_fwd_m16<cross, prescaled, fixed shift>"},
    {AttnFamily::m16, AttnKind::cross, true, 1, false, false, 0, 256, "attn_fwd_m16<cross, prescaled, zero shift>"},
    {AttnFamily::m16, AttnKind::cross, true, 2, false, false, 0, 256, "attn_fwd_m16<cross, prescaled, online max>"},
    {AttnFamily::m16, AttnKind::self, true, 2, true, false, 0, 256,
     "attn_fwd_m16<self, prescaled, gated fixed shift | online max>"},
    {AttnFamily::m16, AttnKind::cross, true, 2, true, false, 0, 256,
     "attn_fwd_m16<cross, prescaled, gated fixed shift | online max>"},
    {AttnFamily::m16, AttnKind::cross, false, 2, false, true, 0, 256, "attn_fwd_m16<cross, online max, persistent>"},
    {AttnFamily::m16, AttnKind::cross, true, 1, false, true, 0, 256,
     "attn_fwd_m16<cross, prescaled, zero shift, persistent>"},
    {AttnFamily::m16, AttnKind::cross, true, 2, false, true, 0, 256,
     "attn_fwd_m16<cross, prescaled, online max, persistent>"},
    {AttnFamily::wq, AttnKind::self, true, 0, false, false, 0, 320,
     "attn_fwd_wq<self, prescaled, 320 rows, fixed shift>"},
    {AttnFamily::wq, AttnKind::self, true, 1, false, false, 0, 320,
     "attn_fwd_wq<self, prescaled, 320 rows, zero shift>"},
    {AttnFamily::wq, AttnKind::self, true, 0, false, false, 0, 384,
     "attn_fwd_wq<self, prescaled, 384 rows, fixed shift>"},
    {AttnFamily::wq, AttnKind::self, true, 1, false, false, 0, 384,
     "attn_fwd_wq<self, prescaled, 384 rows, zero shift>"},
    {AttnFamily::f8, AttnKind::self, true, 0, false, false, 1, 256, "attn_fwd_f8<self, fp8 Q K^T>"},
    {AttnFamily::f8, AttnKind::cross, true, 0, false, false, 1, 256, "attn_fwd_f8<cross, fp8 Q K^T>"},
    {AttnFamily::f8, AttnKind::self, true, 0, false, false, 3, 256, "attn_fwd_f8<self, fp8 Q K^T + fp8 P.V>"},
    {AttnFamily::f8, AttnKind::cross, true, 0, false, false, 3, 256, "attn_fwd_f8<cross, fp8 Q K^T + fp8 P.V>"},
};

// the static name of a route (nullptr: not a route attn_route returns)
inline const char* attn_route_name(const AttnRoute& r) {
  for (const AttnRouteName& n : kRouteNames)
    if (n.family == r.family && n.kind == r.kind && n.prescaled == r.prescaled && n.mode == r.mode &&
        n.gated == r.gated && n.persistent == r.persistent && n.f8 == r.f8 && n.rows == r.rows)
      return n.name;
  return nullptr;
}

// ---- the planners ----

// Work-balance model for the key-range split: the kernel holds one workgroup per CU (2 waves/SIMD), every
// workgroup's time is ~ its key tiles + a fixed ~44 tiles, and workgroups run in ceil(nwg / CUs) rounds; a split
// adds the fp32 partial write + merge traffic (~1 tile of time per 9 MB at HBM rate). The fixed cost is fitted to
// MI355X measurements (tools/bench_cp_chunks.py: B 2, H 16, Lq 13640, Lk 109120 ran 21.9 ms unsplit vs 23.0 ms at
// split 4; H 4: 6.24 vs 6.14 ms): shorter workgroups lose the lock-step K/V streaming through the XCD's L2 that
// long ones keep. Picks the split with the least modelled time.
// Cost of one split launch in tile-times (a workgroup's prologue / epilogue ~ 44 tiles; the fp32 partials' write,
// read and merge at ~9 MB per tile-time): the plan's model.
inline double split_cost(int64_t nwg, int64_t ntiles, int s, int64_t rows, int64_t cus) {
  const int64_t tps = ceil_div(ntiles, s);
  double cost = (double)ceil_div(nwg * s, cus) * (double)(tps + 44);
  if (s > 1) cost += (2.0 * s + 0.5) * (double)rows * kD * 4 / 9.0e6;
  return cost;
}

// Tail split of an unsplit self-attention launch. With nwg workgroups of equal length on cus CUs the last round runs
// r = nwg % cus of them and leaves the other CUs idle for a whole workgroup time (the metric launch: 13 664 = 53 x 256
// + 96, 1.2 % of the launch; a CP = 8 lane: 864 = 3 x 256 + 96, 11 %). The main launch then covers the first nwg - r
// tiles (whole rounds) and the last r query blocks run as key-range splits (per (b, h) segment, s splits each chosen
// to fill one round) with their partials merged, which shortens the tail round to ~1/s of a workgroup. TailSeg lists
// the segments; returns their count (0: no tail split), the largest segment's workspace in *ws_need.
struct TailSeg { int bh, qb_lo, nblk, s; };
constexpr int kMaxTailSegs = 4;
inline int plan_tail(int B, int H, int Lq, int Lk, int qblk, int64_t cus, TailSeg* seg, size_t* ws_need,
                     double* saved) {
  const int64_t nqb = ceil_div(Lq, qblk), ntiles = ceil_div(Lk, kKBlk);
  const int64_t nwg = nqb * B * H;
  const int64_t r = nwg % cus;
  *ws_need = 0;
  if (saved) *saved = 0.0;
  if (r == 0 || nwg < cus || Lk <= kCrossMaxKeys) return 0;
  int n = 0;
  double cost = 0.0;
  size_t need = 0;
  for (int64_t t = nwg - r; t < nwg;) {  // tiles in (b, h) > query block order
    const int bh = (int)(t / nqb), qb = (int)(t % nqb);
    const int nblk = (int)std::min<int64_t>(nqb - qb, nwg - t);
    if (n == kMaxTailSegs) return 0;
    const int64_t rows = std::min<int64_t>(Lq, (int64_t)(qb + nblk) * qblk) - (int64_t)qb * qblk;
    int s = 1;
    for (int c = 2; c <= 8 && c <= ntiles; ++c) {  // the most splits that still fit one round
      const int64_t tps = ceil_div(ntiles, c);
      if (ceil_div(ntiles, tps) == c && (int64_t)nblk * c <= cus) s = c;
    }
    if (s == 1 && qblk != kQBlk) {
      // attn_fwd_wq (round 13): a segment too long for one round of splits (the metric launch's last round is 160
      // workgroups of one (b, h) at either width) runs as the split count whose rounds of shorter workgroups cost the
      // least (160 x 3 = 480 workgroups: two rounds of a third each). attn_fwd_m16's launches keep the one-round rule,
      // so their plans, and with them which rows are merged partials, are what they were.
      double best = 1e300;
      for (int c = 2; c <= 8 && c <= ntiles; ++c) {
        const int64_t tps = ceil_div(ntiles, c);
        if (ceil_div(ntiles, tps) != c) continue;
        const double cc = split_cost(nblk, ntiles, c, rows, cus);
        if (cc < best) { best = cc; s = c; }
      }
    }
    if (s == 1) return 0;
    seg[n++] = TailSeg{bh, qb, nblk, s};
    cost += split_cost(nblk, ntiles, s, rows, cus) + 8.0;  // + launch overhead of the split and merge kernels
    need = std::max<size_t>(need, (size_t)s * rows * (kD + 1) * sizeof(float));
    t += nblk;
  }
  const double unsplit = (double)(ntiles + 44);  // the tail round as one round of whole workgroups
  if (cost >= 0.9 * unsplit) return 0;
  // the multi-round segments above: only where the model recovers at least 0.5 % of the launch
  if (qblk != kQBlk && unsplit - cost < 0.005 * (double)ceil_div(nwg, cus) * unsplit) return 0;
  *ws_need = need;
  if (saved) *saved = unsplit - cost;
  return n;
}

inline int plan_split(int B, int H, int Lq, int Lk, int qblk, int64_t cus) {
  const int64_t nqb = ceil_div(Lq, qblk), ntiles = ceil_div(Lk, kKBlk);
  const int64_t nwg = nqb * B * H;
  const int64_t rows = (int64_t)B * H * Lq;
  int best = 1;
  double best_cost = 1e300;
  for (int s = 1; s <= 8 && s <= ntiles; ++s) {
    const int64_t tps = ceil_div(ntiles, s);
    if (ceil_div(ntiles, tps) != s) continue;  // every split must own at least one tile
    double cost = split_cost(nwg, ntiles, s, rows, cus);
    if (s == 1) {  // unsplit launches may run their last round as a tail split (plan_tail)
      TailSeg seg[kMaxTailSegs];
      size_t need;
      double saved;
      if (plan_tail(B, H, Lq, Lk, qblk, cus, seg, &need, &saved) > 0) cost -= saved;
    }
    if (cost < best_cost * 0.995) { best_cost = cost; best = s; }
  }
  return best;
}

// Workspace that lets an unsplit launch of this shape run its tail split. The shape alone does not say which kernel
// the launch takes (that needs the bounds): enough for attn_fwd_m16's blocks and for attn_fwd_wq's under self_form.
inline size_t tail_workspace_bytes(int B, int H, int Lq, int Lk, int self_form, int64_t cus) {
  TailSeg seg[kMaxTailSegs];
  size_t need = 0, best = 0;
  for (int qblk : {kQBlk, wide_rows_of(self_form, Lk)})
    if (qblk > 0 && plan_tail(B, H, Lq, Lk, qblk, cus, seg, &need, nullptr) > 0) best = std::max(best, need);
  return best;
}

}  // namespace cp25attn
