// K1 dispatch plan, host side: the variant ids the shipping library
// dispatches, the small-tile table, the geometry constants and shape
// predicates the plan shares with the kernels, the stream-K decomposition and
// the tile / row-split / split-K / stream-K cost model with its memo.
// Pure C++ - no HIP - so the library (ntm_validation.hip), the kernel headers
// and a CPU-only test program share it. Functions a kernel header also offers
// to device code carry NTM_HD. plan_search reads nothing but its argument.
#pragma once

#include <cstddef>

#if defined(__HIPCC__)
#define NTM_HD __host__ __device__
#else
#define NTM_HD
#endif

namespace ntm {
namespace k1 {

// K1 variants of the shipping library (the numbering of
// ops.kernels.GEMM_VARIANTS; what each build is: ntm_validation.hip).
enum Variant : int {
  kPlan = 0,  // the default dispatch: plan() below
  kPingpong8b = 4, kPingpong8c = 5, kPingpong8cm = 22, kPingpong8o = 25,
  kTile128 = 15, kTile256x128 = 16, kTile160 = 17, kTile256x160 = 18,
  kTile160x128 = 23, kTile128x160 = 24, kTile128x256 = 26,
  kPp192x256 = 27, kPp256x192 = 28,
  kDma4kD3 = 39,
  kPingpong8s = 49, kPp192x256s = 54, kPp256x192s = 55,  // stream-K
};

// Geometry the plan shares with the kernels: the 256x256x64 tile of the 8-wave
// kernels (gemm_bf16.hpp BM / BN / BK), the K tile split-K slices are rounded
// to (gemm_bf16_t128.hpp TK) and the stream-K workspace (gemm_bf16_sk.hpp).
constexpr int kBM = 256, kBN = 256, kBK = 64;
constexpr int kSplitKTile = 64;
constexpr size_t kPartialBytes = (size_t)kBM * kBN * 4;  // one fp32 256x256 partial
constexpr size_t kCounterBytes = 4096;                   // counter block at the workspace start
// error word (last of the counter block): 0, or the first XCD-placement
// violation a combiner saw: 0x80000000 | mode << 28 | tile << 8 | mine << 4 | other
constexpr int kErrWord = (int)(kCounterBytes / 4) - 1;
constexpr int kMaxSlices = 8;

// pingpong8o's shape rule (gemm_bf16_pp6.hpp)
NTM_HD inline bool shape_ok6(int M, int N, int K) {
  return M > 0 && N > 0 && (M % kBM) == 0 && (N % kBN) == 0 && (K % (2 * kBK)) == 0 && K >= 4 * kBK;
}

// stream-K's (gemm_bf16_sk.hpp, gemm_bf16_skh.hpp)
NTM_HD inline bool shape_ok_sk(int M, int N, int K) {
  return M > 0 && N > 0 && (N % 8) == 0 && K >= 2 * kBK && (K % 8) == 0;
}

inline size_t sk_ws_bytes(int G) { return kCounterBytes + (size_t)G * 2 * kPartialBytes; }

// Split-K over S slices of kc = ceil(K / S) rounded up to 64 (the last slice
// may be shorter): gemm_bf16_t128.hpp launch_gemm_bf16_tile_ws_splitk.
inline int splitk_kc(int K, int S) {
  return ((K + S - 1) / S + kSplitKTile - 1) / kSplitKTile * kSplitKTile;
}
inline int splitk_slices(int K, int S) { const int kc = splitk_kc(K, S); return (K + kc - 1) / kc; }

// Tiles, pairs and the whole-tile prefix for (M, N, K) in TM x TN tiles on
// `cus` CUs (SkArgs of gemm_bf16_sk.hpp carries the same five fields).
// Two-round mode (S = 0; kTwoRound builds only): more tiles than CUs, not a
// multiple of them.
// Split mode (S >= 2, gemm_bf16_sks_kernel): every XCD's tiles fit its CUs at
// least twice over, so each tile is cut into S equal K slices and every slice
// runs at once on its own CU (one round, slices at the same K offsets in
// lockstep); S = the most slices that fit, at most kMaxSlices and one pair each.
struct SkShape {
  int G, D, Tp, ntiles, S;  // as SkArgs; S = split mode's K slices per tile, else 0
};

template <int TM, int TN, bool kTwoRound>
NTM_HD inline bool sk_decompose(int M, int N, int K, int cus, SkShape& s) {
  // one 4-byte counter per workgroup slot (or per tile) in the kCounterBytes block
  if (M <= 0 || N <= 0 || K <= 0 || cus < 8 || (cus % 8) != 0 || cus + 8 > kErrWord)
    return false;
  s.ntiles = ((M + TM - 1) / TM) * ((N + TN - 1) / TN);
  s.G = cus;
  s.Tp = (K + 2 * kBK - 1) / (2 * kBK);
  s.D = 0;
  s.S = 0;
  if (s.ntiles <= s.G) {
    const int per_xcd = (s.ntiles + 7) / 8, W = s.G / 8;
    int S = W / per_xcd;
    if (S > kMaxSlices) S = kMaxSlices;
    if (S > s.Tp) S = s.Tp;
    if (S < 2) return false;
    s.S = S;
    return true;
  }
  if (!kTwoRound || (s.ntiles % s.G) == 0) return false;
  s.D = (s.ntiles / s.G - 1) * s.G;
  return true;
}

// Measured on MI355X (tools/gemm_check.py, random bf16, median of 7 rounds,
// profiles/r1_pp3/): 8192^3: 5 1567 TF, 4 1530; 4096^3: 5 1479, 4 1435; then
// variant 5 without s_setprio +1.3-1.7 % (profiles/r1_pp3_knobs) and with the
// LDS-staged epilogue (profiles/r1_epilogue, r1_round7): 8192^3 1623-1635 TF
// vs hipBLASLt 1632-1648, 4096^3 1536 vs 1532-1544 (same processes).
// Variants 4 and 5 pass tools/race_screen.py (bitwise-stable under HBM noise).
// Default: 5 when K % 128 == 0, else 4 (both need K % 64 == 0, K >= 128).
// 25 = pingpong8o, the persistent build of 5 whose C stores overlap the next
// tile's K loop (gemm_bf16_pp6.hpp): the plan runs it in place of 5 when the
// 256x256 part has more tiles than CUs (a CU then crosses a tile boundary) and
// K >= 256. Measured in one process against 5 (tools/gemm_check.py, medians of
// 13 rounds, profiles/r3_k1o/): 8192^3 1634 vs 1622 TF/s (+0.8 %), 5120^3
// 1394 vs 1374 (+1.5 %), 8192x8192x6144 1611 vs 1590 (+1.3 %).
constexpr int kDefaultVariant = kPingpong8c;
constexpr int kPersistentVariant = kPingpong8o;
// K1-fp8 runs the persistent overlap kernel with f8f6f4 MFMAs on VGPR
// accumulators (gemm_bf16_pp6.hpp F8, experimental fp8 knob 30 until round 4)
// on whole 256x256 tiles, one round or more: +0.8 to +3.0 % over the fp8
// pingpong8c at 4096^3, 8192^3, 8192x8192x4096, 8192x4096x8192 and
// 4096x8192x8192 on each of 3 boxes (profiles/r4_fp8/, r4_ab/); bitwise equal.
// With the spread boundary stores too (ntm_validation.hip kPp6Spread; fp8 knob
// 31): another +1.3 to +2.0 % at 8192^3 and +2.6 to +4.4 % at 8192x8192x4096
// over knob 30 on each of 3 boxes (profiles/r4_ab/fp8_spread_*), never below it.
constexpr bool kFp8Persistent = true;
// pingpong8om (variant 47, the persistent overlap kernel on ragged C) measured
// no better than pingpong8cm under the plan (round 4, profiles/r4_om/), so the
// plan never runs it; it lives in libntm_experimental.so (round 5 hygiene).

// Tile-shape plan of the default dispatch: the smallest predicted time
// rounds(tiles) x tile_area / efficiency over 256 CUs, where the efficiencies
// are each kernel's full-chip rate relative to the 256x256 kernel. The plan
// may split C by rows: the top rows on the 256x256 kernel in whole rounds, the
// rest in a second launch on a small tile, so a partial last round of big
// tiles becomes a full round of small ones (6144^3: 3 rounds of 256x256 ->
// 2 rounds + one of 256x128). Alone it picks 128x128 at 2048^3, 160x160 at
// 2560^3 and 3200^3, 256x128 at 2816^3 and 4096x2048x4096, and 256x256 at
// 3072^3, 4096^3 and 8192^3.
// Efficiencies (round 2, wave-specialised 128x128 / 256x128 / 160x160):
// 0.60 / 0.78 at 8192^3 (989 / 1306 vs 1654 TF/s, profiles/r2_ws/policy_ws1.log,
// interleaved in one process); 160x160 at its full-chip rate at 5120^3 (4 full
// rounds). 256x160 (4-wave) is priced from a full round of it against one of
// 256x256 at 4096x2560x4096 (1121 vs 1146 TF/s, r1_t160/policy_plan.log), not
// from its 8192x5120 rate (0.72): at 0.72 the plan split 5120^3 and
// 8192x5120x4096 onto it and lost 2-3 %. 160x128 / 128x160 (0.70): 1160 /
// 1170 TF/s on 8 full rounds (5120x8192x4096 / 8192x5120x4096,
// profiles/r2_tiles/); they fill a round where the square tiles leave CUs idle
// (5624x752x5880: 216 tiles of 160x128 vs 180 of 160x160, 677 vs 616 TF/s).
// 128x256 (round 3, hipBLASLt's MT128x256 on 4672x1472x6696,
// profiles/r2_tiles/hipblaslt_kernels_stats.csv): 2 % above 256x128 on full
// rounds (8192x8192x4096 / 4096x8192x4096 / 8192x4096x4096: 1300 / 1289 / 1282
// vs 1279 / 1258 / 1253 TF/s, profiles/r3_tiles/), so 0.80 against 0.78; it
// wastes fewer edge rows where M is ragged and N a multiple of 256.
// 192x256 / 256x192 (round 5, `pp`: gemm_bf16_pp3h.hpp, the 8-wave ping-pong
// with one 64-row half; hipBLASLt's MT256x192 / MT192x256 on ragged one-round C,
// profiles/r5_h192/): one round of them took 0.88-0.96 of the time of
// pingpong8cm's round of 256x256 tiles on 7 ragged shapes, for 0.75 of the work
// per CU - eff 0.78-0.85, priced at 0.82. One-round tiles, like 160x128.
// They serve all of C in one launch only: as the rest part after whole rounds
// of 256x256 tiles they tied the old plan at best and lost 22-24 % at
// 5120x5120x128 / 256; below K = 1024 they lost 17-21 % to pingpong8cm
// (7400x1224x616, 4392x2184x544), where loading the A / B panels for 31 % more
// tiles dominates (profiles/r5_h192/plan_ab_*.log).
// (the CU count the rounds are priced over is the launch's own: PlanQuery::cus)
// The table is the one source of tile geometry: the dispatch derives the
// kernels' template arguments from tm / tn (ntm_validation.hip with_ws_tile).
struct SmallTile {
  int variant, tm, tn;
  double eff;
  bool masked;     // wave-specialised kernel: any M, N % 4, K % 8 (edge tiles / K tail masked)
  bool one_round;  // only where its tiles fit in one round of 256 CUs
  bool splitk;     // a split-K candidate (the split model was fitted without 128x256)
  double ragged;   // measured / modelled time of one round on ragged C (stream-K pricing only)
  bool pp = false;  // 8-wave ping-pong tile (gemm_bf16_pp3h.hpp): N % 8, bf16 only
};
// 160x128 / 128x160 are one-round tiles: filling a round the square tiles
// leave part-idle they win 2-16 % (5624x752x5880, 4072x1240x3784, the rest
// parts of 4608^3 / 6144^3); over 2+ rounds, in place of the 256x256 kernel's
// one partial round, they lost 3-22 % (3000^3, 1344x6216x4848, 1616x6208x6504;
// profiles/r2_tiles/plan_ab_*.log) - there the big kernel's partial round runs
// faster per tile than the full-chip rate the model prices.
// `ragged`: one round of the tile on C with an edge tile row / column or K % 128
// != 0 took 1.1-1.5x the modelled time on MI355X (20 one-round shapes,
// profiles/r4_sks/split_sweep.log; exact shapes were within 0.93-1.02x). Only
// the stream-K choice uses it: the tile choice itself was tuned with the model.
constexpr SmallTile kSmallTiles[] = {{kTile128, 128, 128, 0.60, true, false, true, 1.13},
                                     {kTile256x128, 256, 128, 0.78, true, false, true, 1.0},
                                     {kTile160, 160, 160, 0.72, true, false, true, 1.17},
                                     {kTile160x128, 160, 128, 0.70, true, true, true, 1.37},
                                     {kTile128x160, 128, 160, 0.70, true, true, true, 1.37},
                                     {kTile128x256, 128, 256, 0.80, true, false, false, 1.30},
                                     {kTile256x160, 256, 160, 0.61, false, false, false, 1.0},
                                     {kPp192x256, 192, 256, 0.82, true, true, false, 1.0, true},
                                     {kPp256x192, 256, 192, 0.82, true, true, false, 1.0, true}};
constexpr int kNumSmallTiles = (int)(sizeof(kSmallTiles) / sizeof(kSmallTiles[0]));
// the table entry of a variant (variant 0 in the result: not a small tile)
constexpr SmallTile small_tile(int variant) {
  for (const SmallTile& st : kSmallTiles)
    if (st.variant == variant) return st;
  return SmallTile{0, 0, 0, 0.0, false, false, false, 0.0};
}
constexpr int kPpMinK = 1024;
constexpr double kSplitPenalty = 0.25;  // a second launch, in 128x128-tile-round units

struct K1Plan {
  int top_rows;      // rows [0, top_rows) on top_variant; -1 = no plan tiles (M,N,K)
  int top_variant;   // 5 / 4 (the 256x256 kernel) or a kSmallTiles variant
  int rest_variant;  // rows [top_rows, M) on a kSmallTiles variant
  int splits = 1;    // > 1: all of C on top_variant (masked tile), split-K in that many slices
  bool sk = false;   // all of C on the stream-K kernel (top_variant 49 / 54 / 55)
  // a split-K search's predicted unsplit / stream-K seconds (ntm_k1_plan_times)
  double unsplit_s = 0.0, sk_s = 0.0;
  bool feasible() const { return top_rows >= 0; }
};

// Split-K time model (seconds), fitted on MI355X (tools/experiments/splitk_check.py, 14
// shapes x 3 tiles x up to 6 slice counts, profiles/r2_splitk/): a round of
// tm x tn tiles over kc costs 2 tm tn kc / (kPerCU eff); the fp32 partials cost
// kRedFixed + slices M N 4 / kRedBW (the partial stores in the tile epilogue +
// the reduction kernel's reads; an effective rate, not HBM's). Its picks are
// within 3.3 % of the fastest measured split on every fitted shape. A split plan
// must beat the unsplit one by kSplitKMargin.
// Round 5 (profiles/r5_margin/): the model leaves out per-launch fixed costs on
// both sides, so on small C the unsplit plan is about as optimistic as the
// split one, and the 1.1 margin kept C unsplit where a split with long slices
// ran 10-25 % faster. A split whose slices keep >= kLongSliceK of K needs only
// kSplitKMarginLong against the unsplit plan. Short slices keep 1.1 (at 1.03,
// three slices of 464 / 621 K lost 22-28 %), and so does any split against a
// stream-K plan (at 1.03, 256x128 / 2 replaced stream-K split mode on 14
// shapes and lost on 10, by up to 8 %).
constexpr double kPerCU = 1650e12 / 256.0;  // the 256x256 kernel's per-CU bf16 rate
constexpr double kRedFixed = 2e-6;
constexpr double kRedBW = 2e12;
constexpr double kSplitKMargin = 1.1;
constexpr double kSplitKMarginLong = 1.03;
constexpr int kLongSliceK = 1024;
// K1-fp8 (K in bf16-sized pairs of e4m3): the same rule from slices of >= 1152
// pairs (profiles/r5_margin/fp8_seed*: of 52 changed shapes on three seeds, the
// three that lost 15-20 % had slices of 1000-1036 pairs, 1024 / 1088 after
// rounding to the K tile; from 1152 on, 43 of 49 ran faster, median 1.13)
constexpr int kLongSliceKFp8 = 1152;
constexpr int kMaxSplits = 16;

// Host-only A/B knobs of the plan, at their shipping defaults. Every one is
// part of PlanQuery, so of the memo key.
struct PlanKnobs {
  // tools/pp_plan_ab.py: the 192-wide tiles on all of C / stream-K split mode on them
  bool pp = true, pp_split = true;
  // tools/margin_ab.py: the long-slice margin and threshold the plan uses
  // (margin <= 0 / min_k < 0: the shipping values; margin 1.1 = round 4's plan)
  double splitk_margin = 0.0;
  int splitk_min_k = -1;
  // false keeps K1-fp8's split-K at 1.1 everywhere (round 4's fp8 plan)
  bool splitk_fp8_long = true;
  // Split-K candidates with slices of >= kLongSliceK are priced against the
  // ragged-scaled unsplit time that stream-K already uses (profiles/r5_margin/):
  // 146 changed plans on seeds 12 / 13 - long slices 95 of 129 faster, geo-mean
  // 1.045; short ones lost up to 37 % - then fresh seed 14: 46 of 55 faster,
  // median 1.04, worst 0.875. bf16 only (not measured on K1-fp8).
  bool splitk_ragged = true;
  bool operator==(const PlanKnobs& o) const {
    return pp == o.pp && pp_split == o.pp_split && splitk_margin == o.splitk_margin &&
           splitk_min_k == o.splitk_min_k && splitk_fp8_long == o.splitk_fp8_long &&
           splitk_ragged == o.splitk_ragged;
  }
  double long_margin() const { return splitk_margin > 0.0 ? splitk_margin : kSplitKMarginLong; }
  int long_k() const { return splitk_min_k >= 0 ? splitk_min_k : kLongSliceK; }
};

// Everything the search reads: the memo key. cus = the CUs the launches run on
// (256 on MI355X in SPX mode; fewer in a DPX / CPX partition): stream-K's
// decomposition must be the launch's own. fp8: K in bf16-sized pairs of e4m3.
struct PlanQuery {
  int M, N, K, cus;
  bool splitk, fp8;
  PlanKnobs knobs;
  bool operator==(const PlanQuery& o) const {
    return M == o.M && N == o.N && K == o.K && cus == o.cus && splitk == o.splitk &&
           fp8 == o.fp8 && knobs == o.knobs;
  }
  unsigned hash() const {
    const unsigned pp = (knobs.pp ? 1u : 0u) | (knobs.pp_split ? 2u : 0u) | (knobs.splitk_ragged ? 4u : 0u);
    const unsigned h = ((unsigned)M * 2654435761u) ^ ((unsigned)N * 40503u) ^ ((unsigned)K * 97u) ^
                       ((unsigned)cus << 3) ^ (splitk ? 0x55u : 0u) ^ (fp8 ? 0xAAu : 0u) ^ (pp << 8);
    return h ^ (h >> 8) ^ (h >> 16);
  }
};

// Stream-K ("pingpong8s", gemm_bf16_sk.hpp; needs the caller's workspace, so
// only in the split-K plan). Time model, from its stamps (profiles/r4_sk/
// sk_stamps.log): the K loop runs 5 % slower per K-tile pair than the
// data-parallel kernel's (two K offsets per XCD instead of one), over
// ntiles / G tiles per CU, plus ~30 us per workgroup for the fix-ups, the
// extra C store and the imbalance between 2- and 3-segment workgroups. It is
// within +-5 % of the measured time on 29 of 30 shapes (profiles/r4_sk/
// plan_calibration.log). The unsplit plan's model leaves out per-tile fixed
// costs, so it is optimistic; stream-K is chosen whenever its predicted time is
// below the unsplit plan's (4 of 41 random shapes: measured +1 to +12 %).
// Split mode (at most half a round of tiles, S K slices each): ceil(Tp / S)
// pairs per CU plus the fix-up terms below, priced against the unsplit plan
// scaled by SmallTile::ragged (profiles/r4_sks: 6 of 15 sweep shapes, +9 to
// +39 % over the small tile).
// split mode on the 192-wide ping-pong tiles (gemm_bf16_skh.hpp): a tile of
// them costs kPpTileTime of a 256x256 tile over the same K (0.75 of the work at
// the 0.82 efficiency the plan prices them at); its partials are 0.75 the size
constexpr double kPpTileTime = 0.75 / 0.82;
constexpr double kSkLoopFactor = 1.05;
constexpr double kSkFixed = 30e-6;
constexpr double kSkMargin = 1.0;
// split mode (at most half a round of tiles, gemm_bf16_sks_kernel): the K loop
// of ceil(Tp / S) pairs at the data-parallel rate, plus the fix-up. Every one of
// the P = tiles x S slices writes a 256 KiB partial (the write phase grows with
// P) and each combiner reads S of them (grows with S): fitted over 16 measured
// shapes, S = 2..8, P = 128..256, rms 4 us (profiles/r4_sks, r4_tiles).
constexpr double kSkSplitFixed = -18e-6;
constexpr double kSkSplitPerPartial = 0.15e-6;
constexpr double kSkSplitPerSlice = 3.4e-6;
constexpr double kSkSplitMinFixup = 8e-6;

// The plan: C split by rows into a top part and a rest part, each on one tile
// kernel in its own launch (either part may be empty). The top part runs the
// 256x256 kernel or a small tile, the rest a small tile; the smallest
// predicted time wins. Mixed small tiles fill whole rounds where one tile
// shape cannot: 3200^3 = 1920 rows of 160x160 (240 tiles) + 1280 rows of
// 128x128 (250 tiles), two full rounds instead of 1.56 rounds of 160x160
// (977 vs 924 TF/s, hipBLASLt 948: profiles/r2_ws/split_3200.log).
// Ties: fewer launches, then more rows on the 256x256 kernel, then (one
// launch) less of C covered by tiles (edge waste): in one round, 128x160 beat 160x128 (equal
// modelled cost) wherever it had fewer tiles, by 2-13 % (8008x536x2896: 252 vs
// 255 tiles, 34.8 vs 39.4 us; 4152x1096x16056, 1456x2696x10744), and tied
// where the counts were equal (profiles/r4_tiles).
// fp8 (K1-fp8's plan): K counted in bf16-sized pairs of e4m3 values (a K-tile
// costs the same cycles in both dtypes); only the tiles with an fp8 build - the
// 256x256 kernel and the wave-specialised ones - and no split-K.
inline K1Plan plan_search(const PlanQuery& q) {
  const int M = q.M, N = q.N, K = q.K;
  const bool splitk = q.splitk, fp8 = q.fp8;
  const PlanKnobs& knobs = q.knobs;
  const double kCUs = (double)q.cus;
  auto rounds = [&](double tiles) { return tiles <= 0 ? 0.0 : __builtin_ceil(tiles / kCUs); };
  const double inf = 1e300;
  // the 256x256 kernel on whole tiles: pingpong8c (K % 128). K % 128 != 0 goes
  // to the masked build's partial-K path (22), measured faster than pingpong8b
  // (8192x8192x8000: 1634 vs 1472 TF/s, profiles/r2_ws/ktail_pp2_vs_cm.log); the
  // pingpong8b clause below only matters if that build ever cannot serve a shape
  const bool big_masked_ok = N % 8 == 0 && K % 8 == 0;
  const bool big_ok = N % 256 == 0 && K >= 128 &&
                      (K % 128 == 0 || (K % 64 == 0 && !big_masked_ok));
  const int big_variant = K % 128 == 0 ? kDefaultVariant : kPingpong8b;
  K1Plan best{-1, kTile128, kTile128};
  double best_cost = inf;
  int best_launches = 3, best_big_rows = -1;
  double best_cover = inf;
  if (M <= 0 || N <= 0 || K <= 0) return best;
  auto small_ok = [&](const SmallTile& st, int rows) {  // masked: any M, N % 4, K % 8
    if (fp8 && (!st.masked || st.pp)) return false;
    if (st.pp) return knobs.pp && N % 8 == 0 && K % 8 == 0 && K >= kPpMinK;
    if (st.masked) return N % 4 == 0 && K % 8 == 0;
    return rows % st.tm == 0 && N % st.tn == 0 && K % 128 == 0 && K >= 128;
  };
  auto small_cost = [&](const SmallTile& st, int rows) {  // edge tiles cost a whole tile
    const double tiles = (double)((rows + st.tm - 1) / st.tm) * ((N + st.tn - 1) / st.tn);
    if (st.one_round && tiles > kCUs) return inf;
    return rounds(tiles) * (st.tm * st.tn / 16384.0) / st.eff;
  };
  // top candidates: index -1 = the 256x256 kernel, else kSmallTiles[t]
  // the 256x256 kernel on ragged C: variant 22 (masked edge tiles, N % 8, K % 8)
  for (int t = -1; t < kNumSmallTiles; ++t) {
    const int tm = t < 0 ? 256 : kSmallTiles[t].tm;
    if (t < 0 && !big_ok && !big_masked_ok) continue;
    if (t >= 0 && !small_ok(kSmallTiles[t], kSmallTiles[t].tm)) continue;
    const bool masked = t >= 0 ? kSmallTiles[t].masked : big_masked_ok;
    for (int m1 = tm; m1 < M + (masked ? tm : 1); m1 += tm) {
      if (m1 > M) m1 = M;  // masked kernel: the whole of C, last tile row partial
      const bool big_exact = t < 0 && big_ok && m1 % 256 == 0;
      if (t < 0 && !big_exact && !big_masked_ok) continue;
      const double top = t < 0 ? rounds((double)((m1 + 255) / 256) * ((N + 255) / 256)) * 4.0
                               : small_cost(kSmallTiles[t], m1);
      const int rest = M - m1;
      for (int r = 0; r < kNumSmallTiles; ++r) {
        if (rest > 0 && (kSmallTiles[r].pp || !small_ok(kSmallTiles[r], rest))) continue;
        if (rest == 0 && r > 0) break;  // no rest part: one candidate is enough
        const double cost = top + (rest > 0 ? small_cost(kSmallTiles[r], rest) + kSplitPenalty : 0.0);
        if (cost >= inf) continue;  // a one-round tile over more than one round
        // one-round tiles: all of C, or the rest after the 256x256 kernel's rounds
        if (rest > 0 && t >= 0 && (kSmallTiles[t].one_round || kSmallTiles[r].one_round))
          continue;
        const int launches = rest > 0 ? 2 : 1;
        const int big_rows = t < 0 ? m1 : 0;
        auto cover = [&](int tmc, int tnc, int rows) {  // elements of C the tiles span
          return rows <= 0 ? 0.0 : (double)((rows + tmc - 1) / tmc) * ((N + tnc - 1) / tnc) * tmc * tnc;
        };
        const double cov = (t < 0 ? cover(256, 256, m1) : cover(tm, kSmallTiles[t].tn, m1)) +
                           (rest > 0 ? cover(kSmallTiles[r].tm, kSmallTiles[r].tn, rest) : 0.0);
        const bool better = cost < best_cost - 1e-9 ||
                            (cost <= best_cost + 1e-9 &&
                             (launches < best_launches ||
                              (launches == best_launches &&
                               (big_rows > best_big_rows ||
                                (big_rows == best_big_rows && launches == 1 && cov < best_cover)))));
        if (better) {
          best_cost = cost;
          best_launches = launches;
          best_big_rows = big_rows;
          best_cover = cov;
          best = K1Plan{m1, t < 0 ? (big_exact ? big_variant : kPingpong8cm) : kSmallTiles[t].variant,
                        rest > 0 ? kSmallTiles[r].variant : (t < 0 ? kTile128 : kSmallTiles[t].variant)};
        }
      }
    }
  }
  // whole 256x256 tiles over more than one round: the persistent build
  // (K1-fp8: from one round on, K in bf16-sized pairs)
  if (!fp8 && best.feasible() && best.top_variant == kDefaultVariant && K >= 256 &&
      (double)(best.top_rows / 256) * (N / 256) > kCUs)
    best.top_variant = kPersistentVariant;
  if (fp8 && kFp8Persistent && best.feasible() && best.top_variant == kDefaultVariant &&
      shape_ok6(best.top_rows, N, K))
    best.top_variant = kPersistentVariant;
  if (!splitk || !best.feasible()) return best;
  // Split-K: C too small to fill 256 CUs with a long K (e.g. 280x6352x7568: 80
  // tiles of 160x160 -> 3 slices of 240 tiles, 631 vs 321 TF/s unsplit).
  const double unit_s = 2.0 * 16384.0 * K / kPerCU;  // cost units -> seconds
  const double unsplit = best_cost * unit_s;
  double best_t = inf;        // the fastest split-K candidate so far
  double sk_bar = inf;        // a split-K plan must also beat a chosen stream-K plan
  K1Plan split = best;
  // Stream-K: a partial last round of 256x256 tiles spread over every CU, or
  // split mode (at most half a round of tiles) on the 256x256 or the 192-wide
  // tiles; the fastest predicted candidate is priced against the unsplit plan
  SkShape sk;
  double debug_unsplit_s = unsplit, debug_sk_s = 0.0;
  double t_sk = 0.0;
  int sk_variant = 0;
  auto split_mode_s = [&](const SkShape& a, double tile_s, double partial_scale) {
    // one slice of ceil(Tp / S) pairs per CU, one round, plus the fix-up
    const double pairs = (double)((a.Tp + a.S - 1) / a.S);
    const double fixup = kSkSplitFixed + kSkSplitPerPartial * partial_scale * a.ntiles * a.S +
                         kSkSplitPerSlice * a.S;
    return pairs / a.Tp * tile_s + (fixup > kSkSplitMinFixup ? fixup : kSkSplitMinFixup);
  };
  if (!fp8 && shape_ok_sk(M, N, K)) {
    if (sk_decompose<kBM, kBN, true>(M, N, K, (int)kCUs, sk)) {
      const double tile_s = 4.0 * unit_s * (2.0 * sk.Tp * kBK / K);  // one 256x256 tile, K in pairs
      t_sk = sk.S >= 2 ? split_mode_s(sk, tile_s, 1.0)
                       : kSkLoopFactor * ((double)sk.ntiles / kCUs) * tile_s + kSkFixed;
      sk_variant = kPingpong8s;
    }
    if (knobs.pp_split && K >= kPpMinK) {
      for (int gi = 0; gi < 2; ++gi) {
        SkShape sh;
        const bool ok = gi == 0 ? sk_decompose<192, 256, false>(M, N, K, (int)kCUs, sh)
                                : sk_decompose<256, 192, false>(M, N, K, (int)kCUs, sh);
        // S = 2 (the head / tail protocol) only: at S >= 3 it replaced a small tile
        // on 4 random shapes and lost on 3 (0.88-0.98, profiles/r5_skh/pp_ab_random200.log)
        if (!ok || sh.S != 2) continue;
        const double tile_s = kPpTileTime * 4.0 * unit_s * (2.0 * sh.Tp * kBK / K);
        const double t = split_mode_s(sh, tile_s, 0.75);
        if (sk_variant == 0 || t < t_sk) {
          t_sk = t;
          sk_variant = gi == 0 ? kPp192x256s : kPp256x192s;
        }
      }
    }
  }
  // a single launch of one small tile in one round on ragged C runs slower
  // than the model (SmallTile::ragged): stream-K is priced against the
  // measured-ish time (and split-K too, with PlanKnobs::splitk_ragged)
  double unsplit_ragged = unsplit;
  if (best.top_rows == M && best.top_variant == best.rest_variant)
    for (const SmallTile& st : kSmallTiles)
      if (st.variant == best.top_variant &&
          (double)((M + st.tm - 1) / st.tm) * ((N + st.tn - 1) / st.tn) <= kCUs &&
          (M % st.tm != 0 || N % st.tn != 0 || K % 128 != 0))
        // rows of A / B at least 64-byte aligned (K % 32 == 0): a third of it
        // (4704, 6240, 10720: 1.00-1.16 where 16 / 32-byte rows gave 1.1-1.5)
        // and 16-byte rows (K % 16 == 8) at least 1.25 (128x128 1.26 / 1.27,
        // 160x160 1.11 / 1.35 measured)
        unsplit_ragged *= K % 32 == 0   ? 1.0 + (st.ragged - 1.0) * 0.4
                          : K % 16 == 8 ? (st.ragged > 1.0 && st.ragged < 1.25 ? 1.25 : st.ragged)
                                        : st.ragged;
  if (sk_variant != 0) {
    debug_sk_s = t_sk;
    const double unsplit_vs_sk = unsplit_ragged;
    debug_unsplit_s = unsplit_vs_sk;
    if (t_sk * kSkMargin < unsplit_vs_sk) {
      split = K1Plan{M, sk_variant, sk_variant, 1};
      split.sk = true;
      sk_bar = t_sk * kSkMargin / kSplitKMargin;
    }
  }
  for (const SmallTile& st : kSmallTiles) {
    if (!st.masked || !st.splitk || !small_ok(st, M)) continue;
    const double tiles = (double)((M + st.tm - 1) / st.tm) * ((N + st.tn - 1) / st.tn);
    for (int sp = 2; sp <= kMaxSplits; ++sp) {
      const int slices = splitk_slices(K, sp);
      if (slices != sp) continue;  // the same slicing as a smaller sp
      if (st.one_round && tiles * slices > kCUs) break;
      const double kc = splitk_kc(K, sp);
      const double t = rounds(tiles * slices) * 2.0 * st.tm * st.tn * kc / (kPerCU * st.eff) +
                       kRedFixed + (double)slices * M * N * 4.0 / kRedBW;
      const int long_k = fp8 ? (knobs.splitk_min_k >= 0 ? knobs.splitk_min_k : kLongSliceKFp8)
                             : knobs.long_k();
      const double margin = (!fp8 || knobs.splitk_fp8_long) && kc >= long_k
                                ? knobs.long_margin() : kSplitKMargin;
      const double vs = knobs.splitk_ragged && !fp8 && kc >= knobs.long_k() ? unsplit_ragged : unsplit;
      if (t < best_t && t * margin < vs && t < sk_bar) {
        best_t = t;
        split = K1Plan{M, st.variant, st.variant, slices};
      }
    }
  }
  split.unsplit_s = debug_unsplit_s;
  split.sk_s = debug_sk_s;
  return split;
}

// The plan is an exhaustive search over tiles and row splits: 3-25 us of host
// time per shape, paid on every default-dispatch call until round 5 (twice in
// ntm_gemm_bf16_ex). For C of a few microseconds that made the launch
// host-bound (6712x280x368: 18.3 us per call against 8.0 for its own tile,
// profiles/r5_h192/small_shapes_sweep.log). Plans are memoised per host thread
// in a small direct-mapped table keyed by the query, which is everything the
// search reads.
constexpr int kPlanCacheSlots = 256;

inline K1Plan plan(const PlanQuery& q) {
  struct Entry {
    PlanQuery key;
    K1Plan plan;
    bool valid;
  };
  static thread_local Entry cache[kPlanCacheSlots] = {};
  Entry& e = cache[q.hash() % kPlanCacheSlots];
  if (e.valid && e.key == q) return e.plan;
  const K1Plan p = plan_search(q);
  e = Entry{q, p, true};
  return p;
}

}  // namespace k1
}  // namespace ntm
