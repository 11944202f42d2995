// C ABI over the MI355X validation kernels (K1 GEMM, K2 HBM stream,
// K3 fill/reference/verify, K4 HBM pattern test, K5 per-CU compute sweep,
// K6 host-link check, K7 MX block-scaled matrix check, K8 per-XCD sweep,
// K9 atomics and cross-XCD hand-off check, K10 fp64 / fp32 / fp16 / int8 / sparse
// matrix-core check, K11 MX quantise / dequantise, K12 wave data paths and special functions).
// Built for gfx950 only into
//   nvidia_terraform_modules_amd/ops/libntm_validation.so   (Python, ctypes)
//   validation/build/amdgpu-validate                        (Job entrypoint)
// Every entry point is stream-ordered, allocation-free and sync-free, so it
// can be captured in a hipGraph (playbook §6 Guideline 9).
//
// Only the kernels the default dispatch can select are instantiated here
// (pingpong8c / pingpong8b 256x256, the six tile shapes and split-K, K1-fp8 on
// the 256x256 kernel and the wave-specialised tiles, K2, K3).
// The non-default K1 builds, schedule knobs and diagnostics live in
// ntm_experimental.hip -> libntm_experimental.so (tests and tools only).
#include "ntm/atomics.hpp"
#include "ntm/attn.hpp"
#include "ntm/aux_kernels.hpp"
#include "ntm/cu_sweep.hpp"
#include "ntm/gemm_bf16_pp2.hpp"
#include "ntm/gemm_bf16_pp3.hpp"
#include "ntm/gemm_bf16_pp3h.hpp"
#include "ntm/gemm_bf16_pp6.hpp"
#include "ntm/gemm_bf16_sk.hpp"
#include "ntm/gemm_bf16_skh.hpp"
#include "ntm/gemm_bf16_t128.hpp"
#include "ntm/gemm_fp8.hpp"
#include "ntm/gemm_w4k.hpp"
#include "ntm/hbm_pattern.hpp"
#include "ntm/host_link.hpp"
#include "ntm/mcore.hpp"
#include "ntm/mx_gemm.hpp"
#include "ntm/mxq.hpp"
#include "ntm/pda.hpp"
#include "ntm/wave_paths.hpp"
#include "ntm/xcd_sweep.hpp"

#include "ntm/abi.h"  // NTM_API and the prototype of every export below

namespace {
inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline unsigned stream_grid(size_t work_items, unsigned block) {
  // memory-bound: min(work / block, 256 CUs x 8 blocks)
  size_t g = (work_items + block - 1) / block;
  if (g > 2048) g = 2048;
  if (g == 0) g = 1;
  return (unsigned)g;
}
}  // namespace

NTM_API const char* ntm_version() { return "ntm-validation 0.1.0 gfx950"; }

NTM_API int ntm_gemm_shape_ok(int M, int N, int K) {
  return ntm::gemm::shape_ok(M, N, K) ? 1 : 0;
}

namespace k1 = ntm::k1;

// K1 variants in this (shipping) library (k1_plan.hpp Variant, the numbering of
// ops.kernels.GEMM_VARIANTS): 4 = pingpong8b, the 8-wave 256x256
// kernel with the balanced 8/4/8/4 LDS read schedule (gemm_bf16_pp2.hpp; K %
// 64); 5 = pingpong8c, the same schedule with parity-alternating B buffers, a
// uniform tail-free K loop and the LDS-staged nontemporal epilogue
// (gemm_bf16_pp3.hpp; K % 128); 15 / 16 / 17 / 23 / 24 / 18 = 128x128 /
// 256x128 / 160x160 / 160x128 / 128x160 / 256x160 tiles (gemm_bf16_t128.hpp):
// all but the last on the wave-specialised 8-wave kernel (masked: any M, N % 4,
// K % 8), 256x160 on the 4-wave one (whole tiles, K % 128; its accumulators +
// one fragment set do not fit 256 registers at two waves per SIMD).
// 25 = pingpong8o, the persistent build of 5 whose C stores overlap the next
// tile's K loop (gemm_bf16_pp6.hpp).
// 0 = default: the plan (k1_plan.hpp: the cost model, its measurements, its
// memo and its A/B knobs). Variants 1-3 and 6-14 (the first ping-pong,
// the 4-wave 128x128-per-wave kernel, the persistent kernel, the 32-MFMA
// segment schedules, epilogue knobs) are experimental: libntm_experimental.so.
// Boundary stores of the shipping build spread over the 7 phases the quadrants
// allow (gemm_bf16_pp6.hpp SPREAD, "pingpong8od"), round 4: median over 3
// boxes vs hipBLASLt 8192^3 0.998 (plain 0.996), 8192x8192x4096 1.008
// (0.992), 5120^3 1.022 (1.009), 8192x8192x6144 1.005 (0.998); never below
// the plain build on any box (profiles/r4_ab/). Bitwise equal; race screen
// clean (profiles/r4_race/).
constexpr bool kPp6Spread = true;

// The plan's host-only A/B knobs (k1_plan.hpp PlanKnobs; process-wide).
static k1::PlanKnobs g_knobs;
// tools/pp_plan_ab.py: bit 0 = the 192-wide tiles on all of C, bit 1 =
// stream-K split mode on them (3 = the shipping plan)
NTM_API void ntm_set_plan_pp_tiles(int on) {
  g_knobs.pp = (on & 1) != 0;
  g_knobs.pp_split = (on & 2) != 0;
}
// tools/margin_ab.py: margin <= 0 / long_k < 0: the shipping values;
// fp8_long = 0 keeps K1-fp8's split-K at 1.1 everywhere
NTM_API void ntm_set_plan_splitk(double margin, int long_k, int fp8_long) {
  g_knobs.splitk_margin = margin > 0.0 ? margin : 0.0;
  g_knobs.splitk_min_k = long_k >= 0 ? long_k : -1;
  g_knobs.splitk_fp8_long = fp8_long != 0;
}
NTM_API void ntm_set_plan_splitk_ragged(int on) { g_knobs.splitk_ragged = on != 0; }

// The memoised plan for the CUs the launches below run on (device_cus()).
inline k1::PlanQuery query(int M, int N, int K, bool splitk, bool fp8) {
  return k1::PlanQuery{M, N, K, ntm::gemm6::device_cus(), splitk, fp8, g_knobs};
}
inline k1::K1Plan plan_k1(int M, int N, int K, bool splitk = false, bool fp8 = false) {
  return k1::plan(query(M, N, K, splitk, fp8));
}
// A feasible plan to the out-pointers of the ntm_k1*_plan* entry points
// (splits: the split-K ones only).
inline int put_plan(const k1::K1Plan& pl, int* top_rows, int* top_variant, int* rest_variant,
                    int* splits = nullptr) {
  if (!pl.feasible()) return (int)hipErrorInvalidValue;
  *top_rows = pl.top_rows;
  *top_variant = pl.top_variant;
  *rest_variant = pl.rest_variant;
  if (splits) *splits = pl.splits;
  return 0;
}

// The counted vmcnt phase P (0..3) of the 192-wide ping-pong build <ah, bh>
// waits for (Geo::vmc, gemm_bf16_pp3h.hpp; 128 / 128 is pingpong8c's 10): host
// only, for the CPU model of the DMA schedule (tests/test_pp3h_schedule_model.py).
NTM_API int ntm_pp3h_vmcnt(int ah, int bh, int phase) {
  using namespace ntm::gemm3h;
  if (phase < 0 || phase > 3) return -1;
  int v[4];
  auto fill = [&](auto geo) {
    using G = decltype(geo);
    v[0] = G::vmc(0), v[1] = G::vmc(1), v[2] = G::vmc(2), v[3] = G::vmc(3);
  };
  if (ah == 64 && bh == 128) fill(Geo<64, 128>{});
  else if (ah == 128 && bh == 64) fill(Geo<128, 64>{});
  else if (ah == 96 && bh == 128) fill(Geo<96, 128>{});
  else if (ah == 128 && bh == 128) fill(Geo<128, 128>{});
  else return -1;
  return v[phase];
}

// The split-K plan's predicted seconds for (M, N, K): the best unsplit plan and
// stream-K (0 when it does not serve the shape). Host only; tools.
NTM_API int ntm_k1_plan_times(int M, int N, int K, double* unsplit_s, double* sk_s) {
  if (!unsplit_s || !sk_s) return (int)hipErrorInvalidValue;
  const k1::K1Plan pl = plan_k1(M, N, K, true);
  if (!pl.feasible()) return (int)hipErrorInvalidValue;
  *unsplit_s = pl.unsplit_s;
  *sk_s = pl.sk_s;
  return 0;
}

// The default dispatch's plan for (M, N, K) (host only; tests and tools).
NTM_API int ntm_k1_plan(int M, int N, int K, int* top_rows, int* top_variant, int* rest_variant) {
  if (M <= 0 || N <= 0 || K <= 0 || !top_rows || !top_variant || !rest_variant)
    return (int)hipErrorInvalidValue;
  return put_plan(plan_k1(M, N, K), top_rows, top_variant, rest_variant);
}

// The same with split-K allowed (a workspace of ntm_splitk_ws_bytes(M, N, K,
// *splits) bytes when *splits > 1): the plan ntm_gemm_bf16_ex runs.
NTM_API int ntm_k1_plan_splitk(int M, int N, int K, int* top_rows, int* top_variant,
                               int* rest_variant, int* splits) {
  if (M <= 0 || N <= 0 || K <= 0 || !top_rows || !top_variant || !rest_variant || !splits)
    return (int)hipErrorInvalidValue;
  return put_plan(plan_k1(M, N, K, true), top_rows, top_variant, rest_variant, splits);
}

// The wave-specialised tiles (15-17, 23, 24, 26: the masked, non-ping-pong
// entries of k1::kSmallTiles): f(<tm / 32>, <tn / 32>) as integral constants,
// the template arguments of the gemm_bf16_t128.hpp launchers, from the table
// entry of `variant`; hipErrorInvalidValue for any other variant.
template <int I = 0, typename F>
inline int with_ws_tile(int variant, F&& f) {
  if constexpr (I < k1::kNumSmallTiles) {
    constexpr k1::SmallTile st = k1::kSmallTiles[I];
    if constexpr (st.masked && !st.pp) {
      if (variant == st.variant)
        return (int)f(std::integral_constant<int, st.tm / 32>{},
                      std::integral_constant<int, st.tn / 32>{});
    }
    return with_ws_tile<I + 1>(variant, f);
  }
  return (int)hipErrorInvalidValue;
}
// the tiles with a launcher of their own: the table entry is the launched shape
static_assert(k1::small_tile(k1::kTile256x160).tm == ntm::gemmt::Cfg<8, 5>::TM &&
              k1::small_tile(k1::kTile256x160).tn == ntm::gemmt::Cfg<8, 5>::TN);
static_assert(k1::small_tile(k1::kPp192x256).tm == ntm::gemm3h::Geo<64, 128>::TM &&
              k1::small_tile(k1::kPp192x256).tn == ntm::gemm3h::Geo<64, 128>::TN);
static_assert(k1::small_tile(k1::kPp256x192).tm == ntm::gemm3h::Geo<128, 64>::TM &&
              k1::small_tile(k1::kPp256x192).tn == ntm::gemm3h::Geo<128, 64>::TN);

NTM_API int ntm_gemm_bf16_variant(int variant, const void* A, const void* B,
                                  void* C, int M, int N, int K, int lda,
                                  int ldb, int ldc, void* stream) {
  if (variant == k1::kPlan) {
    const k1::K1Plan pl = plan_k1(M, N, K);
    if (!pl.feasible()) return (int)hipErrorInvalidValue;  // nothing launched
    if (pl.top_rows < M) {
      const int rc = ntm_gemm_bf16_variant(pl.top_variant, A, B, C, pl.top_rows, N, K, lda, ldb,
                                           ldc, stream);
      if (rc != 0) return rc;
      return ntm_gemm_bf16_variant(pl.rest_variant, (const __bf16*)A + (size_t)pl.top_rows * lda,
                                   B, (__bf16*)C + (size_t)pl.top_rows * ldc, M - pl.top_rows, N,
                                   K, lda, ldb, ldc, stream);
    }
    variant = pl.top_variant;
  }
  const ntm::gemm::GemmArgs a = ntm::gemm::make_args(A, B, C, M, N, K, lda, ldb, ldc);
  switch (variant) {
    case k1::kPingpong8b: return (int)ntm::gemm2::launch_gemm_bf16_pp2(a, S(stream));
    case k1::kPingpong8c: return (int)ntm::gemm3::launch_gemm_bf16_pp3(a, S(stream));
    // persistent pingpong8c with overlapped C stores (needs lda / ldb / ldc % 8,
    // K >= 256; otherwise the same tiles on pingpong8c)
    case k1::kPingpong8o:
      if (!ntm::gemm6::shape_ok6(M, N, K) || (lda % 8) || (ldb % 8) || (ldc % 8))
        return (int)ntm::gemm3::launch_gemm_bf16_pp3(a, S(stream));
      return (int)ntm::gemm6::launch_gemm_bf16_pp6<1, 0, kPp6Spread>(a, S(stream));
    // gemm_bf16_t128.hpp: 256x160 on the 4-wave tile kernel
    case k1::kTile256x160: return (int)ntm::gemmt::launch_gemm_bf16_tile<8, 5>(a, S(stream));
    // 256x256 on ragged C: clamped loads, masked LDS-staged stores
    case k1::kPingpong8cm: return (int)ntm::gemm3::launch_gemm_bf16_pp3_masked(a, S(stream));
    // 192x256 / 256x192 on the same ping-pong (gemm_bf16_pp3h.hpp): ragged C, one round
    case k1::kPp192x256: return (int)ntm::gemm3h::launch_gemm_bf16_pp3h<64, 128>(a, S(stream));
    case k1::kPp256x192: return (int)ntm::gemm3h::launch_gemm_bf16_pp3h<128, 64>(a, S(stream));
    // dma4k_d3 (gemm_w4k.hpp): 4 waves x 128x128 per wave on 256x256 tiles, a DMA
    // piece every 3 slots. Not on the plan: under the power limit it trades places
    // with pingpong8o box by box (-3 % .. +1.8 %, profiles/r6_w4kh), so bench.py
    // measures both on the box it runs on and times the faster (select_k1).
    case k1::kDma4kD3: return (int)ntm::w4k::launch_gemm_bf16_w4k<3>(a, S(stream));
    // the tiles of the wave-specialised kernel (4 DMA-producer + 4 MFMA-consumer
    // waves); anything else is experimental: libntm_experimental.so
    default:
      return with_ws_tile(variant, [&](auto mt, auto nt) {
        return ntm::gemmt::launch_gemm_bf16_tile_ws<decltype(mt)::value, decltype(nt)::value>(
            a, S(stream));
      });
  }
}

// Split-K on a wave-specialised tile (15-17, 23, 24, 26): `splits` K-slices, fp32 partials
// in the caller's workspace ws (ntm_splitk_ws_bytes; stream-ordered, reused once
// this call's reduction has run), then one reduction kernel writes C.
NTM_API size_t ntm_splitk_ws_bytes(int M, int N, int K, int splits) {
  if (M <= 0 || N <= 0 || K <= 0 || splits < 1) return 0;
  return sizeof(float) * (size_t)ntm::gemmt::splitk_slices(K, splits) * M * N;
}

NTM_API int ntm_gemm_bf16_splitk(int variant, int splits, const void* A, const void* B, void* C,
                                 int M, int N, int K, int lda, int ldb, int ldc, void* ws,
                                 size_t ws_bytes, void* stream) {
  if (splits < 1 || !ws || ws_bytes < ntm_splitk_ws_bytes(M, N, K, splits))
    return (int)hipErrorInvalidValue;
  const ntm::gemm::GemmArgs a = ntm::gemm::make_args(A, B, C, M, N, K, lda, ldb, ldc);
  return with_ws_tile(variant, [&](auto mt, auto nt) {
    return ntm::gemmt::launch_gemm_bf16_tile_ws_splitk<decltype(mt)::value, decltype(nt)::value>(
        a, splits, (float*)ws, S(stream));
  });
}

// Stream-K on the 256x256 kernel ("pingpong8s", gemm_bf16_sk.hpp): the last two
// rounds of tiles dealt out as K-tile pairs over every CU, fp32 partials of the
// split tiles in ws. ntm_sk_ws_bytes = 0: stream-K does not serve (M, N, K) on
// this device (the tile count is a multiple of the CUs, or at most one round).
// Index (in 4-byte words) of the stream-K workspace's XCD-placement error word
// (gemm_bf16_sk.hpp kErrWord): nonzero after a launch in which some part of a
// split tile ran on a different XCD than the part that combined it.
NTM_API int ntm_sk_error_word_index() { return ntm::gemmsk::kErrWord; }
// Fault injection for that check (tests, the Job's self-check): nonzero makes the
// head / slice 0 of every split tile claim XCC_ID ^ v, so every stream-K launch
// after this call sets the error word. Process-wide; 0 = off.
NTM_API void ntm_set_sk_fault_inject(int v) { ntm::gemmsk::sk_fault_inject() = (unsigned)v; }

// The CU count the plan and the persistent / stream-K launches use, and a test
// override of it (0 = the device's own; host only: a CPU test of the plan on
// partition sizes other than 256 - never set it around real launches).
NTM_API int ntm_plan_cus() { return ntm::gemm6::device_cus(); }
NTM_API void ntm_set_cus_override(int cus) { ntm::gemm6::cu_override() = cus > 0 ? cus : 0; }

NTM_API size_t ntm_sk_ws_bytes(int M, int N, int K) {
  ntm::gemmsk::SkArgs s;
  if (!ntm::gemmsk::shape_ok_sk(M, N, K) ||
      !ntm::gemmsk::sk_decompose(M, N, K, ntm::gemm6::pp6_grid(1 << 30), s))
    return 0;
  return ntm::gemmsk::sk_ws_bytes(s.G);
}

NTM_API int ntm_gemm_bf16_sk(const void* A, const void* B, void* C, int M, int N, int K, int lda,
                             int ldb, int ldc, void* ws, size_t ws_bytes, void* stream) {
  const ntm::gemm::GemmArgs a = ntm::gemm::make_args(A, B, C, M, N, K, lda, ldb, ldc);
  return (int)ntm::gemmsk::launch_gemm_bf16_sk(a, ntm::gemm6::pp6_grid(1 << 30), ws, ws_bytes,
                                               S(stream));
}

// Split mode on the 192-wide tiles (variant 54: 192x256, 55: 256x192;
// gemm_bf16_skh.hpp) with a stream-K workspace of ntm_skh_ws_bytes bytes (0:
// split mode on that tile does not serve (M, N, K) on this device).
NTM_API size_t ntm_skh_ws_bytes(int variant, int M, int N, int K) {
  ntm::gemmsk::SkArgs s;
  const int cus = ntm::gemm6::pp6_grid(1 << 30);
  if (!ntm::gemmsk::shape_ok_sk(M, N, K)) return 0;
  const bool ok = variant == k1::kPp192x256s   ? ntm::gemmskh::sk_decompose_h<192, 256>(M, N, K, cus, s)
                  : variant == k1::kPp256x192s ? ntm::gemmskh::sk_decompose_h<256, 192>(M, N, K, cus, s)
                                               : false;
  return ok ? ntm::gemmsk::sk_ws_bytes(s.G) : 0;
}

// `fault`: this launch's own fault-injection value (the Job runs one thread per
// GPU and corrupts only the last GPU's launch; -1 = the process-wide
// ntm_set_sk_fault_inject value).
NTM_API int ntm_gemm_bf16_skh_ex(int variant, const void* A, const void* B, void* C, int M, int N,
                                 int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes,
                                 int fault, void* stream) {
  const ntm::gemm::GemmArgs a = ntm::gemm::make_args(A, B, C, M, N, K, lda, ldb, ldc);
  const int cus = ntm::gemm6::pp6_grid(1 << 30);
  if (variant == k1::kPp192x256s)
    return (int)ntm::gemmskh::launch_gemm_bf16_skh<64, 128>(a, cus, ws, ws_bytes, S(stream), fault);
  if (variant == k1::kPp256x192s)
    return (int)ntm::gemmskh::launch_gemm_bf16_skh<128, 64>(a, cus, ws, ws_bytes, S(stream), fault);
  return (int)hipErrorInvalidValue;
}

// The same with the process-wide fault-injection value (launch_gemm_bf16_skh's
// default, fault = -1).
NTM_API int ntm_gemm_bf16_skh(int variant, const void* A, const void* B, void* C, int M, int N,
                              int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes,
                              void* stream) {
  return ntm_gemm_bf16_skh_ex(variant, A, B, C, M, N, K, lda, ldb, ldc, ws, ws_bytes, -1, stream);
}

// The default dispatch with split-K allowed: ws (ws_bytes) is the caller's
// workspace; when the split-K plan needs more than ws_bytes (or ws is null) the
// unsplit plan runs instead.
NTM_API int ntm_gemm_bf16_ex(const void* A, const void* B, void* C, int M, int N, int K, int lda,
                             int ldb, int ldc, void* ws, size_t ws_bytes, void* stream) {
  if (ws) {
    const k1::K1Plan pl = plan_k1(M, N, K, true);
    if (pl.feasible() && pl.splits > 1 && ws_bytes >= ntm_splitk_ws_bytes(M, N, K, pl.splits))
      return ntm_gemm_bf16_splitk(pl.top_variant, pl.splits, A, B, C, M, N, K, lda, ldb, ldc, ws,
                                  ws_bytes, stream);
    // stream-K: this entry takes any caller workspace, so it zeroes the counter
    // block first (a caller that keeps a zeroed workspace per stream calls
    // ntm_gemm_bf16_sk directly and saves that dispatch)
    if (pl.feasible() && pl.sk && pl.top_variant == k1::kPingpong8s &&
        ws_bytes >= ntm_sk_ws_bytes(M, N, K) &&
        hipMemsetAsync(ws, 0, ntm::gemmsk::kCounterBytes, S(stream)) == hipSuccess &&
        ntm_gemm_bf16_sk(A, B, C, M, N, K, lda, ldb, ldc, ws, ws_bytes, stream) == 0)
      return 0;
    if (pl.feasible() && pl.sk && pl.top_variant != k1::kPingpong8s &&
        ws_bytes >= ntm_skh_ws_bytes(pl.top_variant, M, N, K) &&
        ntm_skh_ws_bytes(pl.top_variant, M, N, K) > 0 &&
        hipMemsetAsync(ws, 0, ntm::gemmsk::kCounterBytes, S(stream)) == hipSuccess &&
        ntm_gemm_bf16_skh(pl.top_variant, A, B, C, M, N, K, lda, ldb, ldc, ws, ws_bytes, stream) == 0)
      return 0;
  }
  return ntm_gemm_bf16_variant(0, A, B, C, M, N, K, lda, ldb, ldc, stream);
}

// K1-fp8: C (bf16) = A (e4m3) * B (e4m3)^T, fp32 accumulation. Variant 5 / 22:
// the 256x256 kernel (gemm_fp8.hpp; exact, masked and partial-K builds picked by
// shape); 15 / 16 / 17 / 23 / 24 / 26: the wave-specialised tiles with the fp8
// consumer (gemm_bf16_t128.hpp); 0: the plan (plan_k1 in fp8 mode: tile shape
// and row split priced exactly as for bf16).
NTM_API int ntm_gemm_fp8_variant(int variant, const void* A, const void* B, void* C, int M, int N,
                                 int K, int lda, int ldb, int ldc, void* stream) {
  if (!ntm::fp8::shape_ok(M, N, K)) return (int)hipErrorInvalidValue;
  if (variant == k1::kPlan) {
    const k1::K1Plan pl = plan_k1(M, N, K / 2, false, true);
    if (!pl.feasible()) return (int)hipErrorInvalidValue;  // nothing launched
    if (pl.top_rows < M) {
      const int rc = ntm_gemm_fp8_variant(pl.top_variant, A, B, C, pl.top_rows, N, K, lda, ldb,
                                          ldc, stream);
      if (rc != 0) return rc;
      return ntm_gemm_fp8_variant(pl.rest_variant, (const char*)A + (size_t)pl.top_rows * lda, B,
                                  (__bf16*)C + (size_t)pl.top_rows * ldc, M - pl.top_rows, N, K,
                                  lda, ldb, ldc, stream);
    }
    variant = pl.top_variant;
  }
  __bf16* c = (__bf16*)C;
  switch (variant) {
    case k1::kPingpong8c:
    case k1::kPingpong8cm:
      return (int)ntm::fp8::launch_gemm_fp8(A, B, c, M, N, K, lda, ldb, ldc, S(stream));
    // the persistent overlap build (whole 256x256 tiles, K % 256, K >= 512;
    // otherwise the same tiles on pingpong8c)
    case k1::kPingpong8o:
      if (ntm::gemm6::fp8_pp6_ok(M, N, K, lda, ldb, ldc))
        return (int)ntm::gemm6::launch_gemm_fp8_pp6<kPp6Spread>(A, B, c, M, N, K, lda, ldb, ldc,
                                                               S(stream));
      return (int)ntm::fp8::launch_gemm_fp8(A, B, c, M, N, K, lda, ldb, ldc, S(stream));
    default:
      return with_ws_tile(variant, [&](auto mt, auto nt) {
        return ntm::gemmt::launch_gemm_fp8_tile_ws<decltype(mt)::value, decltype(nt)::value>(
            A, B, c, M, N, K, lda, ldb, ldc, S(stream));
      });
  }
}

NTM_API int ntm_k1_fp8_plan(int M, int N, int K, int* top_rows, int* top_variant,
                            int* rest_variant) {
  if (!ntm::fp8::shape_ok(M, N, K) || !top_rows || !top_variant || !rest_variant)
    return (int)hipErrorInvalidValue;
  return put_plan(plan_k1(M, N, K / 2, false, true), top_rows, top_variant, rest_variant);
}

NTM_API int ntm_gemm_fp8(const void* A, const void* B, void* C, int M, int N, int K, int lda,
                         int ldb, int ldc, void* stream) {
  return ntm_gemm_fp8_variant(0, A, B, C, M, N, K, lda, ldb, ldc, stream);
}

// K1-fp8 split-K on a wave-specialised tile (15-17, 23, 24, 26): `splits` slices of
// the K-tile range, fp32 partials in ws (ntm_fp8_splitk_ws_bytes), one reduction.
NTM_API size_t ntm_fp8_splitk_ws_bytes(int M, int N, int K, int splits) {
  return ntm_splitk_ws_bytes(M, N, K / 2, splits);
}

NTM_API int ntm_gemm_fp8_splitk(int variant, int splits, const void* A, const void* B, void* C,
                                int M, int N, int K, int lda, int ldb, int ldc, void* ws,
                                size_t ws_bytes, void* stream) {
  if (!ntm::fp8::shape_ok(M, N, K) || splits < 1 || !ws ||
      ws_bytes < ntm_fp8_splitk_ws_bytes(M, N, K, splits))
    return (int)hipErrorInvalidValue;
  return with_ws_tile(variant, [&](auto mt, auto nt) {
    return ntm::gemmt::launch_gemm_fp8_tile_ws_splitk<decltype(mt)::value, decltype(nt)::value>(
        A, B, (__bf16*)C, M, N, K, lda, ldb, ldc, splits, (float*)ws, S(stream));
  });
}

// K1-fp8's plan with split-K allowed (what ntm_gemm_fp8_ex runs when given a
// workspace of ntm_fp8_splitk_ws_bytes(M, N, K, *splits) bytes).
NTM_API int ntm_k1_fp8_plan_splitk(int M, int N, int K, int* top_rows, int* top_variant,
                                   int* rest_variant, int* splits) {
  if (!ntm::fp8::shape_ok(M, N, K) || !top_rows || !top_variant || !rest_variant || !splits)
    return (int)hipErrorInvalidValue;
  return put_plan(plan_k1(M, N, K / 2, true, true), top_rows, top_variant, rest_variant, splits);
}

NTM_API int ntm_gemm_fp8_ex(const void* A, const void* B, void* C, int M, int N, int K, int lda,
                            int ldb, int ldc, void* ws, size_t ws_bytes, void* stream) {
  if (ws && ntm::fp8::shape_ok(M, N, K)) {
    const k1::K1Plan pl = plan_k1(M, N, K / 2, true, true);
    if (pl.feasible() && pl.splits > 1 && ws_bytes >= ntm_fp8_splitk_ws_bytes(M, N, K, pl.splits))
      return ntm_gemm_fp8_splitk(pl.top_variant, pl.splits, A, B, C, M, N, K, lda, ldb, ldc, ws,
                                 ws_bytes, stream);
  }
  return ntm_gemm_fp8_variant(0, A, B, C, M, N, K, lda, ldb, ldc, stream);
}

NTM_API int ntm_gemm_fp8_shape_ok(int M, int N, int K) {
  return ntm::fp8::shape_ok(M, N, K) ? 1 : 0;
}

NTM_API int ntm_gemm_bf16(const void* A, const void* B, void* C, int M, int N,
                          int K, int lda, int ldb, int ldc, void* stream) {
  return ntm_gemm_bf16_variant(0, A, B, C, M, N, K, lda, ldb, ldc, stream);
}

// K1 with the fused ABFT row checksum (default 8-wave kernel): rowsum[m] (fp32, M
// entries) must be zeroed by the caller on `stream` before the call.
NTM_API int ntm_gemm_bf16_rowsum(const void* A, const void* B, void* C,
                                 float* rowsum, int M, int N, int K, int lda,
                                 int ldb, int ldc, void* stream) {
  if (!rowsum) return (int)hipErrorInvalidValue;
  ntm::gemm::GemmArgs a = ntm::gemm::make_args(A, B, C, M, N, K, lda, ldb, ldc);
  a.rowsum = rowsum;
  return ntm::gemm3::shape_ok3(M, N, K) ? (int)ntm::gemm3::launch_gemm_bf16_pp3(a, S(stream))
                                        : (int)ntm::gemm2::launch_gemm_bf16_pp2(a, S(stream));
}

// K1-fp8 with the fused ABFT row checksum: the 256x256 fp8 build with kRowSum
// (exact shapes: M, N, K % 256); rowsum zeroed by the caller on `stream`.
NTM_API int ntm_gemm_fp8_rowsum(const void* A, const void* B, void* C, float* rowsum, int M,
                                int N, int K, int lda, int ldb, int ldc, void* stream) {
  if (!rowsum || !ntm::fp8::shape_exact(M, N, K) || lda < K || ldb < K || ldc < N ||
      (lda % 16) || (ldb % 16) || (ldc % 8))
    return (int)hipErrorInvalidValue;
  // byte image: two e4m3 per bf16 slot (gemm_fp8.hpp)
  ntm::gemm::GemmArgs a = ntm::gemm::make_args(A, B, C, M, N, K / 2, lda / 2, ldb / 2, ldc);
  a.rowsum = rowsum;
  using ntm::gemm3::gemm_bf16_pp3_kernel;
  using ntm::gemm3::kEpiDefault;
  hipLaunchKernelGGL((gemm_bf16_pp3_kernel<true, ntm::gemm::kGroupM, false, kEpiDefault, 0, 3>),
                     dim3((unsigned)((M / ntm::gemm::BM) * (N / ntm::gemm::BN))),
                     dim3(ntm::gemm::kThreads), 0, S(stream), a);
  return (int)hipGetLastError();
}

namespace {
template <typename T>
int abft_check_t(const void* A, const void* B, const void* C, const float* rowsum, int M, int N,
                 int K, int lda, int ldb, int ldc, double* scratch, void* result,
                 hipStream_t stream) {
  if (M <= 0 || N <= 0 || K <= 0 || !rowsum || !scratch || !result)
    return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(scratch, 0, sizeof(double) * (size_t)K, stream);
  if (e != hipSuccess) return (int)e;
  e = hipMemsetAsync(result, 0, sizeof(ntm::aux::AbftResult), stream);
  if (e != hipSuccess) return (int)e;
  // ~2048 column blocks x row chunks: enough parallelism for 256 CUs
  const int kb = (K + 255) / 256;
  int chunks = (2048 + kb - 1) / kb;
  if (chunks > N) chunks = N;
  const int rpc = (N + chunks - 1) / chunks;
  chunks = (N + rpc - 1) / rpc;
  hipLaunchKernelGGL(ntm::aux::abft_colsum_kernel<T>, dim3(kb, chunks), dim3(256), 0, stream,
                     (const T*)B, N, K, ldb, rpc, scratch);
  hipLaunchKernelGGL(ntm::aux::abft_row_check_kernel<T>, dim3(M), dim3(256), 0, stream,
                     (const T*)A, lda, (const __bf16*)C, ldc, rowsum, scratch, N, K,
                     (ntm::aux::AbftResult*)result);
  return (int)hipGetLastError();
}
}  // namespace

// ABFT check of K1-fp8's C = A B^T (e4m3 operands) against its fused rowsum.
NTM_API int ntm_abft_check_fp8(const void* A, const void* B, const void* C, const float* rowsum,
                               int M, int N, int K, int lda, int ldb, int ldc, double* scratch,
                               void* result, void* stream) {
  return abft_check_t<uint8_t>(A, B, C, rowsum, M, N, K, lda, ldb, ldc, scratch, result,
                               S(stream));
}

// ABFT check of C = A B^T against the fused rowsum. scratch: K doubles;
// result: ntm::aux::AbftResult (both zeroed here, stream-ordered).
NTM_API int ntm_abft_check(const void* A, const void* B, const void* C,
                           const float* rowsum, int M, int N, int K, int lda,
                           int ldb, int ldc, double* scratch, void* result,
                           void* stream) {
  return abft_check_t<__bf16>(A, B, C, rowsum, M, N, K, lda, ldb, ldc, scratch, result,
                              S(stream));
}

NTM_API int ntm_abft_result_bytes() {
  return (int)sizeof(ntm::aux::AbftResult);
}

NTM_API int ntm_fill_uniform_bf16(void* out, size_t n, unsigned long long seed,
                                  float scale, void* stream) {
  if (n == 0) return 0;
  const unsigned grid = stream_grid((n + 7) / 8, 256);
  hipLaunchKernelGGL(ntm::aux::fill_uniform_bf16_kernel, dim3(grid), dim3(256),
                     0, S(stream), (__bf16*)out, n, (uint64_t)seed, scale);
  return (int)hipGetLastError();
}

NTM_API int ntm_ref_gemm_f32(const void* A, const void* B, float* C, int M,
                             int N, int K, int lda, int ldb, int ldc,
                             void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return (int)hipErrorInvalidValue;
  dim3 grid((N + ntm::aux::kRefTile - 1) / ntm::aux::kRefTile,
            (M + ntm::aux::kRefTile - 1) / ntm::aux::kRefTile);
  hipLaunchKernelGGL(ntm::aux::ref_gemm_f32_kernel<__bf16>, grid, dim3(256), 0,
                     S(stream), (const __bf16*)A, (const __bf16*)B, C, M, N, K,
                     lda, ldb, ldc);
  return (int)hipGetLastError();
}

// K3 for K1-fp8: e4m3 operands (uniform [-1, 1) rounded RNE) and the fp32
// FMA reference over their exact values.
NTM_API int ntm_fill_uniform_e4m3(void* out, size_t n, unsigned long long seed, float scale,
                                  void* stream) {
  if (n == 0) return 0;
  const unsigned grid = stream_grid((n + 15) / 16, 256);
  hipLaunchKernelGGL(ntm::aux::fill_uniform_e4m3_kernel, dim3(grid), dim3(256), 0, S(stream),
                     (uint8_t*)out, n, (uint64_t)seed, scale);
  return (int)hipGetLastError();
}

NTM_API int ntm_ref_gemm_f32_e4m3(const void* A, const void* B, float* C, int M, int N, int K,
                                  int lda, int ldb, int ldc, void* stream) {
  if (M <= 0 || N <= 0 || K <= 0) return (int)hipErrorInvalidValue;
  dim3 grid((N + ntm::aux::kRefTile - 1) / ntm::aux::kRefTile,
            (M + ntm::aux::kRefTile - 1) / ntm::aux::kRefTile);
  hipLaunchKernelGGL(ntm::aux::ref_gemm_f32_kernel<uint8_t>, grid, dim3(256), 0, S(stream),
                     (const uint8_t*)A, (const uint8_t*)B, C, M, N, K, lda, ldb, ldc);
  return (int)hipGetLastError();
}

// result: device pointer to a zeroed ntm::aux::VerifyResult (32 bytes)
NTM_API int ntm_verify_bf16(const void* C, const float* R, size_t n,
                            float atol, float rtol, void* result,
                            void* stream) {
  const unsigned grid = stream_grid(n, 256);
  hipLaunchKernelGGL(ntm::aux::verify_bf16_kernel, dim3(grid), dim3(256), 0,
                     S(stream), (const __bf16*)C, R, n, atol, rtol,
                     (ntm::aux::VerifyResult*)result);
  return (int)hipGetLastError();
}

// Clock probe (aux_kernels.hpp clock_probe_kernel): grid blocks of 4 waves,
// out = 2 u64 per wave (shader cycles, 100 MHz ticks), sink = 1 float.
NTM_API int ntm_clock_probe(int grid, int iters, void* out, float* sink, void* stream) {
  if (grid <= 0 || iters <= 0 || !out || !sink) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(ntm::aux::clock_probe_kernel, dim3(grid), dim3(256), 0, S(stream), iters,
                     7u, (unsigned long long*)out, sink);
  return (int)hipGetLastError();
}

// GEMM clock: the shipping pingpong8o build with a start / end
// s_memtime + s_memrealtime stamp per workgroup (gemm_bf16_pp6.hpp STAMP 1).
// Whole 256x256 tiles, more tiles than CUs; stamps = ntm_gemm_bf16_clock_words()
// u64 per workgroup (start / end shader clock and real time, XCC_ID, HW_ID;
// ntm_gemm_bf16_clock_grid workgroups). C is the real product.
NTM_API int ntm_gemm_bf16_clock_words() { return ntm::gemm6::kClockStampWords; }

NTM_API int ntm_gemm_bf16_clock_grid(int M, int N) {
  if (M <= 0 || N <= 0 || M % 256 || N % 256) return 0;
  return ntm::gemm6::pp6_grid((M / 256) * (N / 256));
}

NTM_API int ntm_gemm_bf16_clock(const void* A, const void* B, void* C, int M, int N, int K,
                                int lda, int ldb, int ldc, void* stamps, void* stream) {
  if (!stamps) return (int)hipErrorInvalidValue;
  ntm::gemm::GemmArgs a = ntm::gemm::make_args(A, B, C, M, N, K, lda, ldb, ldc);
  a.stamps = (unsigned long long*)stamps;
  return (int)ntm::gemm6::launch_gemm_bf16_pp6<1, 1, kPp6Spread>(a, S(stream));
}

NTM_API int ntm_verify_result_bytes() {
  return (int)sizeof(ntm::aux::VerifyResult);
}

// K2 entry points. unroll in {2,4,8,16} selects the block-tiled kernels
// (policy bit0 = nontemporal loads, bit1 = nontemporal stores, bit2 (copy
// only) = software-pipelined; grid 0 = one block per tile, no grid-stride
// loop: the hardware dispatcher keeps every CU's wave slots full);
// unroll 1 selects the first grid-stride kernel (2048 x 256, nt), kept as
// the sweep baseline. Defaults measured by tools/hbm_sweep.py on MI355X.
namespace {
template <int U>
int copy_u(const void* src, void* dst, size_t n4, int policy, unsigned grid,
           hipStream_t s) {
  using namespace ntm::aux;
  const auto* a = (const ntm::f32x4*)src;
  auto* b = (ntm::f32x4*)dst;
  switch (policy) {
    case 0: hipLaunchKernelGGL((stream_copy_tiled_kernel<U, 0, 0>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 1: hipLaunchKernelGGL((stream_copy_tiled_kernel<U, 1, 0>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 2: hipLaunchKernelGGL((stream_copy_tiled_kernel<U, 0, 1>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 3: hipLaunchKernelGGL((stream_copy_tiled_kernel<U, 1, 1>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 4: hipLaunchKernelGGL((stream_copy_pipe_kernel<U, 0, 0>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 5: hipLaunchKernelGGL((stream_copy_pipe_kernel<U, 1, 0>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 6: hipLaunchKernelGGL((stream_copy_pipe_kernel<U, 0, 1>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 7: hipLaunchKernelGGL((stream_copy_pipe_kernel<U, 1, 1>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 9: hipLaunchKernelGGL((stream_copy_chunk_kernel<U, 1, 0>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 11: hipLaunchKernelGGL((stream_copy_chunk_kernel<U, 1, 1>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 8: hipLaunchKernelGGL((stream_copy_chunk_kernel<U, 0, 0>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    case 10: hipLaunchKernelGGL((stream_copy_chunk_kernel<U, 0, 1>), dim3(grid), dim3(256), 0, s, a, b, n4); break;
    default: return (int)hipErrorInvalidValue;
  }
  return (int)hipGetLastError();
}
template <int U>
int read_u(const void* src, size_t n4, float* sink, int policy, unsigned grid,
           hipStream_t s) {
  using namespace ntm::aux;
  const auto* a = (const ntm::f32x4*)src;
  if (policy & 1)
    hipLaunchKernelGGL((stream_read_tiled_kernel<U, 1>), dim3(grid), dim3(256), 0, s, a, n4, sink);
  else
    hipLaunchKernelGGL((stream_read_tiled_kernel<U, 0>), dim3(grid), dim3(256), 0, s, a, n4, sink);
  return (int)hipGetLastError();
}
unsigned tiled_grid(size_t n4, int unroll, int grid) {
  if (grid > 0) return (unsigned)grid;
  const size_t tiles = n4 / (256 * (size_t)unroll);
  return (unsigned)(tiles < 1 ? 1 : (tiles > 0x7fffffffu ? 0x7fffffffu : tiles));
}
}  // namespace

NTM_API int ntm_stream_copy_ex(const void* src, void* dst, size_t bytes,
                               int unroll, int policy, int grid, void* stream) {
  if (bytes % 16 || grid < 0) return (int)hipErrorInvalidValue;
  const size_t n4 = bytes / 16;
  if (unroll == 1) {
    hipLaunchKernelGGL(ntm::aux::stream_copy_kernel, dim3(2048), dim3(256), 0,
                       S(stream), (const ntm::f32x4*)src, (ntm::f32x4*)dst, n4);
    return (int)hipGetLastError();
  }
  const unsigned g = tiled_grid(n4, unroll, grid);
  switch (unroll) {
    case 2: return copy_u<2>(src, dst, n4, policy, g, S(stream));
    case 4: return copy_u<4>(src, dst, n4, policy, g, S(stream));
    case 8: return copy_u<8>(src, dst, n4, policy, g, S(stream));
    case 16: return copy_u<16>(src, dst, n4, policy, g, S(stream));
    default: return (int)hipErrorInvalidValue;
  }
}

NTM_API int ntm_stream_read_ex(const void* src, size_t bytes, float* sink,
                               int unroll, int policy, int grid, void* stream) {
  if (bytes % 16 || grid < 0) return (int)hipErrorInvalidValue;
  const size_t n4 = bytes / 16;
  if (unroll == 1) {
    hipLaunchKernelGGL(ntm::aux::stream_read_kernel, dim3(2048), dim3(256), 0,
                       S(stream), (const ntm::f32x4*)src, n4, sink);
    return (int)hipGetLastError();
  }
  const unsigned g = tiled_grid(n4, unroll, grid);
  switch (unroll) {
    case 2: return read_u<2>(src, n4, sink, policy, g, S(stream));
    case 4: return read_u<4>(src, n4, sink, policy, g, S(stream));
    case 8: return read_u<8>(src, n4, sink, policy, g, S(stream));
    case 16: return read_u<16>(src, n4, sink, policy, g, S(stream));
    default: return (int)hipErrorInvalidValue;
  }
}

// Tuned defaults (= ops.kernels.STREAM_COPY_CONFIG / STREAM_READ_CONFIG).
// Copy: 2 float4 per lane, nontemporal load + store, one 8 KiB tile per block
// (grid 0): 6.37 TB/s at 2 GiB, 6.05 at 4 GiB against 5.81 / 5.41 for the
// earlier (8, 7, 512) grid-stride pipeline (interleaved, profiles/r2_k2/).
// Read 7.1 TB/s on two MI355X boxes.
NTM_API int ntm_stream_copy(const void* src, void* dst, size_t bytes,
                            void* stream) {
  return ntm_stream_copy_ex(src, dst, bytes, 2, 7, 0, stream);
}

NTM_API int ntm_stream_read(const void* src, size_t bytes, float* sink,
                            void* stream) {
  return ntm_stream_read_ex(src, bytes, sink, 8, 1, 1024, stream);
}

// K4: HBM pattern test (hbm_pattern.hpp). One block per tile (4 KiB for the
// write, 8 KiB like the tuned K2 copy for the verify kernels). `result` is one ntm::hbm::PatternResult the caller has
// initialised (zero, first_bad_offset all ones); the kernels only add to it, so
// one record can collect a whole step. Offsets in it are logical: base_bytes +
// the offset in this buffer. invert_after: store the complement of the expected
// pattern behind the compare (moving inversions).
namespace {
template <int PAT>
void pattern_write_p(void* ptr, size_t n4, uint64_t base_w, uint64_t seed, uint32_t inv,
                     hipStream_t s) {
  using namespace ntm::hbm;
  const unsigned g = tiled_grid(n4, kWriteUnroll, 0);
  hipLaunchKernelGGL((hbm_pattern_write_kernel<PAT, kWriteUnroll>), dim3(g), dim3(256), 0, s,
                     (u32x4*)ptr, n4, base_w, seed, inv);
}
template <int PAT, bool INV>
void pattern_verify_p(void* ptr, size_t n4, uint64_t base_w, uint64_t seed, uint32_t inv,
                      void* result, hipStream_t s) {
  using namespace ntm::hbm;
  const unsigned g = tiled_grid(n4, kVerifyUnroll, 0);
  hipLaunchKernelGGL((hbm_pattern_verify_kernel<PAT, kVerifyUnroll, INV>), dim3(g), dim3(256), 0,
                     s, (u32x4*)ptr, n4, base_w, seed, inv, (PatternResult*)result);
}
bool pattern_args_ok(const void* ptr, size_t bytes, unsigned long long base_bytes, int pattern) {
  return ptr && (uintptr_t)ptr % 16 == 0 && bytes % 16 == 0 && base_bytes % 16 == 0 &&
         (pattern == ntm::hbm::kPatternAddr || pattern == ntm::hbm::kPatternHash);
}
}  // namespace

NTM_API int ntm_hbm_pattern_result_bytes() { return (int)sizeof(ntm::hbm::PatternResult); }

NTM_API int ntm_hbm_pattern_write(void* ptr, size_t bytes, unsigned long long base_bytes,
                                  int pattern, unsigned long long seed, int invert,
                                  void* stream) {
  if (!pattern_args_ok(ptr, bytes, base_bytes, pattern)) return (int)hipErrorInvalidValue;
  if (bytes == 0) return 0;
  const uint32_t inv = invert ? ~0u : 0u;
  if (pattern == ntm::hbm::kPatternAddr)
    pattern_write_p<ntm::hbm::kPatternAddr>(ptr, bytes / 16, base_bytes / 4, seed, inv, S(stream));
  else
    pattern_write_p<ntm::hbm::kPatternHash>(ptr, bytes / 16, base_bytes / 4, seed, inv, S(stream));
  return (int)hipGetLastError();
}

NTM_API int ntm_hbm_pattern_verify(void* ptr, size_t bytes, unsigned long long base_bytes,
                                   int pattern, unsigned long long seed, int invert,
                                   int invert_after, void* result, void* stream) {
  if (!pattern_args_ok(ptr, bytes, base_bytes, pattern) || !result || (uintptr_t)result % 64)
    return (int)hipErrorInvalidValue;
  if (bytes == 0) return 0;
  const uint32_t inv = invert ? ~0u : 0u;
  const size_t n4 = bytes / 16;
  const uint64_t bw = base_bytes / 4;
  using namespace ntm::hbm;
  if (pattern == kPatternAddr) {
    if (invert_after) pattern_verify_p<kPatternAddr, true>(ptr, n4, bw, seed, inv, result, S(stream));
    else pattern_verify_p<kPatternAddr, false>(ptr, n4, bw, seed, inv, result, S(stream));
  } else {
    if (invert_after) pattern_verify_p<kPatternHash, true>(ptr, n4, bw, seed, inv, result, S(stream));
    else pattern_verify_p<kPatternHash, false>(ptr, n4, bw, seed, inv, result, S(stream));
  }
  return (int)hipGetLastError();
}

// K5: per-CU compute sweep (cu_sweep.hpp; record, decode, expected tables and
// aggregation in cu_sweep_plan.hpp). ntm_cu_sweep_launch is one launch:
// `records` (device, grid * 64 bytes) is zeroed and filled, `expected` (device)
// holds ntm_cu_sweep_expected(iters, seed). fault_key = ~0u: no injection.
// The decode / expected / summarize entry points are host-only: no GPU needed.
NTM_API int ntm_cu_sweep_record_bytes() { return (int)sizeof(ntm::cus::Record); }

NTM_API size_t ntm_cu_sweep_expected_bytes(int iters) {
  return iters >= 1 && iters <= ntm::cus::kMaxIters ? ntm::cus::expected_bytes(iters) : 0;
}

NTM_API int ntm_cu_sweep_expected(int iters, unsigned seed, void* out, size_t out_bytes) {
  if (!out || iters < 1 || iters > ntm::cus::kMaxIters || out_bytes < ntm::cus::expected_bytes(iters))
    return (int)hipErrorInvalidValue;
  ntm::cus::make_expected((uint32_t*)out, iters, seed);
  return 0;
}

// The LDS fill pattern of round `round`: words first .. first + count.
NTM_API int ntm_cu_sweep_lds_words(unsigned seed, unsigned round, unsigned first, unsigned count,
                                   unsigned* out) {
  if (!out) return (int)hipErrorInvalidValue;
  const uint32_t rs = ntm::cus::round_seed(seed, round);
  for (unsigned i = 0; i < count; ++i) out[i] = ntm::cus::lds_word(first + i, rs);
  return 0;
}

// The device's per-block LDS maximum (the default lds_bytes), 0 on an error.
NTM_API int ntm_cu_sweep_max_lds_bytes(int device) {
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return v / 16 * 16;
}

NTM_API int ntm_cu_sweep_launch(void* records, const void* expected, unsigned grid, int iters,
                                size_t lds_bytes, unsigned seed, unsigned fault_key,
                                int fault_subtest, void* stream) {
  if ((uintptr_t)records % 8 || (uintptr_t)expected % 8) return (int)hipErrorInvalidValue;
  return (int)ntm::cus::launch_cu_sweep((ntm::cus::Record*)records, (const uint32_t*)expected, grid,
                                        iters, lds_bytes, seed, fault_key, fault_subtest, S(stream));
}

// out[0..5] = xcc, se, sh, cu, simd, packed key
NTM_API void ntm_cu_sweep_decode(unsigned hw_id, unsigned xcc_id, unsigned* out) {
  const ntm::cus::CuId id = ntm::cus::decode(hw_id, xcc_id);
  out[0] = id.xcc, out[1] = id.se, out[2] = id.sh, out[3] = id.cu, out[4] = id.simd;
  out[5] = ntm::cus::cu_key(hw_id, xcc_id);
}

// Aggregates n host records of `launches` launches on a device of `cus` CUs
// into a JSON object (cu_sweep_plan.hpp summary_json). Returns the JSON's
// length; it is written (NUL-terminated) only when it fits in `cap`.
NTM_API size_t ntm_cu_sweep_summarize(const void* records, size_t n, unsigned cus, unsigned launches,
                                      int gpu, char* json, size_t cap) {
  ntm::cus::Sweep sweep;
  std::vector<ntm::cus::Record> recs(n);
  if (n) std::memcpy(recs.data(), records, n * sizeof(ntm::cus::Record));
  sweep.add(recs.data(), n);
  ntm::cus::Summary s = sweep.summary(cus);
  s.launches = launches;
  const std::string j = ntm::cus::summary_json(gpu, s);
  if (json && j.size() < cap) std::memcpy(json, j.c_str(), j.size() + 1);
  return j.size();
}

// K6: host-link (PCIe) check (host_link.hpp; host side in host_link_plan.hpp).
// `host` is pinned, device-mapped host memory (hipHostMalloc, hipHostRegister,
// a pinned torch tensor): each entry point resolves it with
// hipHostGetDevicePointer and returns hipErrorInvalidValue for memory that is
// not mapped, a size or base that is no 16-byte multiple, or an unknown
// pattern. blocks <= 0: ntm_host_link_default_blocks(pull). The _ex entry points
// take the sweep's knobs (unroll 1 / 2 / 4 / 8, nt = nontemporal accesses;
// tools/host_link_rates.py); the plain ones run the measured defaults.
namespace {
namespace hl = ntm::hostlink;

// The device's view of [host, host + bytes), or null when either end is not mapped.
void* mapped(const void* host, size_t bytes) {
  void *d0 = nullptr, *d1 = nullptr;
  if (!host || bytes == 0) return nullptr;
  if (hipHostGetDevicePointer(&d0, const_cast<void*>(host), 0) != hipSuccess ||
      hipHostGetDevicePointer(&d1, (char*)const_cast<void*>(host) + (bytes - 1), 0) != hipSuccess ||
      !d0 || (char*)d1 - (char*)d0 != (ptrdiff_t)(bytes - 1)) {
    (void)hipGetLastError();
    return nullptr;
  }
  return d0;
}
bool link_args_ok(const void* host, size_t bytes, unsigned long long base_bytes, int pattern,
                  int blocks) {
  return host && (uintptr_t)host % 16 == 0 && bytes % 16 == 0 && base_bytes % 16 == 0 &&
         blocks <= hl::kMaxBlocks &&
         (pattern == ntm::hbm::kPatternAddr || pattern == ntm::hbm::kPatternHash);
}
inline unsigned link_grid(int blocks, bool pull) {
  return (unsigned)(blocks > 0 ? blocks : pull ? hl::kPullBlocks : hl::kPushBlocks);
}

template <int PAT, int U, bool NT>
void push_launch(void* d, size_t n4, uint64_t bw, uint64_t seed, uint32_t inv, unsigned g,
                 hipStream_t s) {
  hipLaunchKernelGGL((hl::host_link_push_kernel<PAT, U, NT>), dim3(g), dim3(256), 0, s,
                     (hl::u32x4*)d, n4, bw, seed, inv);
}
template <int PAT, int U, bool NT>
void pull_launch(const void* d, size_t n4, uint64_t bw, uint64_t seed, uint32_t inv, void* dst,
                 void* result, unsigned g, hipStream_t s) {
  if (dst)
    hipLaunchKernelGGL((hl::host_link_pull_kernel<PAT, U, true, NT>), dim3(g), dim3(256), 0, s,
                       (const hl::u32x4*)d, n4, bw, seed, inv, (hl::u32x4*)dst,
                       (hl::PatternResult*)result);
  else
    hipLaunchKernelGGL((hl::host_link_pull_kernel<PAT, U, false, NT>), dim3(g), dim3(256), 0, s,
                       (const hl::u32x4*)d, n4, bw, seed, inv, (hl::u32x4*)nullptr,
                       (hl::PatternResult*)result);
}
// f(<PAT>, <U>, <NT>) as integral constants; false for knobs outside the sweep
template <typename F>
bool with_link_knobs(int pattern, int unroll, int nt, F&& f) {
  auto pat = [&](auto u, auto n) {
    if (pattern == ntm::hbm::kPatternAddr) f(std::integral_constant<int, ntm::hbm::kPatternAddr>{}, u, n);
    else f(std::integral_constant<int, ntm::hbm::kPatternHash>{}, u, n);
  };
  auto un = [&](auto n) -> bool {
    switch (unroll) {
      case 1: pat(std::integral_constant<int, 1>{}, n); return true;
      case 2: pat(std::integral_constant<int, 2>{}, n); return true;
      case 4: pat(std::integral_constant<int, 4>{}, n); return true;
      case 8: pat(std::integral_constant<int, 8>{}, n); return true;
      default: return false;
    }
  };
  return nt ? un(std::true_type{}) : un(std::false_type{});
}
}  // namespace

// blocks of the push (pull != 0: pull) kernel when the caller passes blocks <= 0
NTM_API int ntm_host_link_default_blocks(int pull) { return pull ? hl::kPullBlocks : hl::kPushBlocks; }
// bytes one block moves per loop trip in the default push (pull != 0: pull) build
NTM_API int ntm_host_link_tile_bytes(int pull) {
  return 256 * 16 * (pull ? hl::kPullUnroll : hl::kPushUnroll);
}

NTM_API int ntm_host_link_push_ex(void* host, size_t bytes, unsigned long long base_bytes,
                                  int pattern, unsigned long long seed, int invert, int blocks,
                                  int unroll, int nt, void* stream) {
  if (!link_args_ok(host, bytes, base_bytes, pattern, blocks)) return (int)hipErrorInvalidValue;
  if (bytes == 0) return 0;
  void* d = mapped(host, bytes);
  if (!d) return (int)hipErrorInvalidValue;
  const uint32_t inv = invert ? ~0u : 0u;
  const bool ok = with_link_knobs(pattern, unroll, nt, [&](auto p, auto u, auto n) {
    push_launch<decltype(p)::value, decltype(u)::value, decltype(n)::value>(
        d, bytes / 16, base_bytes / 4, seed, inv, link_grid(blocks, false), S(stream));
  });
  return ok ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

NTM_API int ntm_host_link_push(void* host, size_t bytes, unsigned long long base_bytes,
                               int pattern, unsigned long long seed, int invert, int blocks,
                               void* stream) {
  return ntm_host_link_push_ex(host, bytes, base_bytes, pattern, seed, invert, blocks,
                               hl::kPushUnroll, hl::kPushNontemporal, stream);
}

// `result`: one initialised ntm::hbm::PatternResult in device memory (as for
// ntm_hbm_pattern_verify); `dst`: null, or `bytes` of HBM that receive what was read.
NTM_API int ntm_host_link_pull_ex(const void* host, size_t bytes, unsigned long long base_bytes,
                                  int pattern, unsigned long long seed, int invert, void* dst,
                                  int blocks, int unroll, int nt, void* result, void* stream) {
  if (!link_args_ok(host, bytes, base_bytes, pattern, blocks) || !result ||
      (uintptr_t)result % 64 || (uintptr_t)dst % 16)
    return (int)hipErrorInvalidValue;
  if (bytes == 0) return 0;
  const void* d = mapped(host, bytes);
  if (!d) return (int)hipErrorInvalidValue;
  const uint32_t inv = invert ? ~0u : 0u;
  const bool ok = with_link_knobs(pattern, unroll, nt, [&](auto p, auto u, auto n) {
    pull_launch<decltype(p)::value, decltype(u)::value, decltype(n)::value>(
        d, bytes / 16, base_bytes / 4, seed, inv, dst, result, link_grid(blocks, true), S(stream));
  });
  return ok ? (int)hipGetLastError() : (int)hipErrorInvalidValue;
}

NTM_API int ntm_host_link_pull(const void* host, size_t bytes, unsigned long long base_bytes,
                               int pattern, unsigned long long seed, int invert, void* dst,
                               int blocks, void* result, void* stream) {
  return ntm_host_link_pull_ex(host, bytes, base_bytes, pattern, seed, invert, dst, blocks,
                               hl::kPullUnroll, hl::kPullNontemporal, result, stream);
}

// `host`: nslots slots of 64 bytes (host_link_plan.hpp chase_fill); `out`: 3 u64 of
// device memory (final index, wall_clock64 ticks, hops done).
NTM_API int ntm_host_link_chase(const void* host, unsigned long long nslots,
                                unsigned long long start, unsigned hops, void* out, void* stream) {
  if (!host || (uintptr_t)host % 8 || nslots == 0 || nslots > (1ull << 32) || start >= nslots ||
      hops == 0 || !out || (uintptr_t)out % 8)
    return (int)hipErrorInvalidValue;
  const void* d = mapped(host, (size_t)nslots * hl::kChaseSlotBytes);
  if (!d) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(hl::host_link_chase_kernel, dim3(1), dim3(64), 0, S(stream),
                     (const unsigned long long*)d, nslots, start, hops, (unsigned long long*)out);
  return (int)hipGetLastError();
}

// wall_clock64() ticks per millisecond on `device` (0 on an error).
NTM_API int ntm_host_link_clock_khz(int device) {
  int v = 0;
  if (hipDeviceGetAttribute(&v, hipDeviceAttributeWallClockRate, device) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  return v;
}

// K7: MX block-scaled matrix check (mx_gemm.hpp; host side in mx_plan.hpp).
// fmt: 0 e4m3, 1 e5m2, 2 e2m3, 3 e3m2, 4 e2m1 for both operands; A / B row-major
// packed (K * bits / 8 bytes per row, 16-byte aligned), SA[M][K/32] / SB[N][K/32]
// E8M0 bytes, C fp32 [M][N]. M, N and K must be multiples of 128: anything
// else returns hipErrorInvalidValue and launches nothing.
NTM_API int ntm_mx_shape_ok(int M, int N, int K) { return ntm::mx::shape_ok(M, N, K) ? 1 : 0; }

NTM_API int ntm_mx_gemm(int fmt, const void* A, const void* B, const void* SA, const void* SB,
                        void* C, int M, int N, int K, void* stream) {
  return (int)ntm::mx::launch_mx_gemm(fmt, A, B, SA, SB, (float*)C, M, N, K, S(stream));
}

// The same product without the matrix cores (mx_ref_kernel).
NTM_API int ntm_mx_reference(int fmt, const void* A, const void* B, const void* SA, const void* SB,
                             void* C, int M, int N, int K, void* stream) {
  return (int)ntm::mx::launch_mx_reference(fmt, A, B, SA, SB, (float*)C, M, N, K, S(stream));
}

// Bitwise compare of n 32-bit words; `out`: one initialised ntm::mx::Mismatch
// (24 bytes: count, first index = all ones, expected, got) in device memory.
NTM_API int ntm_mx_compare(const void* expected, const void* got, size_t n, void* out, void* stream) {
  return (int)ntm::mx::launch_mx_compare(expected, got, n, out, S(stream));
}
NTM_API int ntm_mx_mismatch_bytes() { return (int)sizeof(ntm::mx::Mismatch); }

// K8: per-XCD sweep (xcd_sweep.hpp; record, aggregation and verdict in
// xcd_sweep_plan.hpp). The read launch takes a buffer of xcds * slice_bytes that
// ntm_hbm_pattern_write filled from logical byte 0, `heads` (device,
// ntm_xcd_sweep_heads_bytes(), zeroed here) and `records` (device, grid * 64
// bytes, every one written). slow_xcd = -1: no injection.
NTM_API int ntm_xcd_sweep_record_bytes() { return (int)sizeof(ntm::xcs::Record); }
NTM_API int ntm_xcd_sweep_heads_bytes() { return (int)ntm::xcs::kHeadsBytes; }
NTM_API int ntm_xcd_sweep_tile_bytes() { return (int)ntm::xcs::kTileBytes; }
NTM_API int ntm_xcd_sweep_mfma_per_batch() { return (int)ntm::xcs::kMfmaPerBatch; }
// 1 when the rate rule judges the cell, 0 when it is reported only
NTM_API int ntm_xcd_sweep_gated(int level, int mode) { return ntm::xcs::gated(level, mode) ? 1 : 0; }

NTM_API int ntm_xcd_sweep_read_launch(const void* buf, size_t slice_bytes, unsigned xcds,
                                      unsigned xcd_mask, unsigned passes, int pattern,
                                      unsigned long long seed, unsigned grid, int slow_xcd,
                                      unsigned slow_factor, void* heads, void* records, void* stream) {
  return (int)ntm::xcs::launch_xcd_read(buf, slice_bytes, xcds, xcd_mask, passes, pattern, seed, grid,
                                        slow_xcd, slow_factor, (uint32_t*)heads,
                                        (ntm::xcs::Record*)records, S(stream));
}

NTM_API int ntm_xcd_sweep_mfma_launch(unsigned grid, unsigned batches, unsigned seed, unsigned xcds,
                                      unsigned xcd_mask, int slow_xcd, unsigned slow_factor,
                                      void* records, float* sink, void* stream) {
  return (int)ntm::xcs::launch_xcd_mfma(grid, batches, seed, xcds, xcd_mask, slow_xcd, slow_factor,
                                        (ntm::xcs::Record*)records, sink, S(stream));
}

// Host-only. Aggregates n host records (one launch, or launches with disjoint
// masks concatenated) per XCD into a JSON object (xcd_sweep_plan.hpp
// summary_json). level / mode: the plan's ids; expected_tiles: what every XCD in
// `mask` must have pulled (0 = not checked). Returns the JSON's length; it is
// written (NUL-terminated) only when it fits in `cap`.
NTM_API size_t ntm_xcd_sweep_summarize(const void* records, size_t n, int level, int mode, unsigned xcds,
                                       unsigned mask, unsigned long long expected_tiles, double ratio,
                                       int gpu, char* json, size_t cap) {
  if (level < 0 || level >= ntm::xcs::kLevels || mode < 0 || mode >= ntm::xcs::kModes) return 0;
  std::vector<ntm::xcs::Record> recs(n);
  if (n) std::memcpy(recs.data(), records, n * sizeof(ntm::xcs::Record));
  const std::string j = ntm::xcs::summary_json(
      ntm::xcs::summarize(recs.data(), n, level, mode, xcds, mask, expected_tiles, ratio, gpu));
  if (json && j.size() < cap) std::memcpy(json, j.c_str(), j.size() + 1);
  return j.size();
}

// K9: atomics and cross-XCD hand-off check (atomics.hpp; ops, operands, bounds, records
// and verdicts in atomics_plan.hpp). rmw: `table` is slots x ntm_atomics_slot_bytes(op)
// device bytes, initialised here; the reference launch fills a second table with no
// atomic. tickets: `counters` (ntm_atomics_counter_bytes(heads)) and `claim`
// (ntm_atomics_ticket_claim_bytes) are initialised here. handoff: `slabs` hold round - 1
// (ntm_atomics_handoff_init, or the round before), `counters` one line per episode,
// `records` grid x 96 bytes, every one written. inject_gid / inject_wg = ~0u: none.
namespace atm = ntm::atm;
NTM_API int ntm_atomics_ops() { return atm::kOps; }
NTM_API const char* ntm_atomics_op_name(int op) { return atm::op_name(op); }
NTM_API int ntm_atomics_slot_bytes(int op) { return op >= 0 && op < atm::kOps ? (int)atm::slot_bytes(op) : 0; }
NTM_API int ntm_atomics_record_bytes() { return (int)sizeof(atm::Record); }
NTM_API int ntm_atomics_exact(int op, unsigned long long adds_per_slot, unsigned long long max_abs) {
  return atm::atomics_exact(op, adds_per_slot, max_abs) ? 1 : 0;
}
NTM_API int ntm_atomics_rmw_shape_ok(int op, unsigned long long slots, unsigned grid, unsigned iters,
                                     unsigned long long max_abs) {
  return atm::rmw_shape_ok(op, slots, grid, iters, max_abs) ? 1 : 0;
}
// Host-only: the expected table, slots x slot_bytes(op), into `out`. 0 = written.
NTM_API int ntm_atomics_expected(int op, unsigned long long slots, unsigned long long total, unsigned long long seed,
                                 unsigned long long max_abs, void* out) {
  if (op < 0 || op >= atm::kOps || !slots || !out || (atm::is_float(op) && !max_abs)) return 1;
  for (unsigned long long s = 0; s < slots; ++s) {
    const uint64_t v = atm::expected_slot(op, s, slots, total, seed, atm::is_float(op) ? max_abs : 1);
    if (atm::slot_bytes(op) == 8) ((uint64_t*)out)[s] = v;
    else ((uint32_t*)out)[s] = (uint32_t)v;
  }
  return 0;
}
NTM_API int ntm_atomics_rmw_launch(int op, void* table, unsigned long long slots, unsigned grid, unsigned iters,
                                   unsigned long long seed, unsigned long long max_abs, void* stream) {
  return (int)atm::launch_rmw(op, table, slots, grid, iters, seed, max_abs, S(stream));
}
NTM_API int ntm_atomics_rmw_reference_launch(int op, void* table, unsigned long long slots, unsigned grid,
                                             unsigned iters, unsigned long long seed, unsigned long long max_abs,
                                             void* stream) {
  return (int)atm::launch_rmw_reference(op, table, slots, grid, iters, seed, max_abs, S(stream));
}
NTM_API size_t ntm_atomics_ticket_claim_bytes(unsigned heads, unsigned grid, unsigned iters) {
  return atm::ticket_shape_ok(heads, grid, iters) ? (size_t)(heads * atm::tickets_per_head(heads, grid, iters) * 4) : 0;
}
NTM_API size_t ntm_atomics_counter_bytes(unsigned counters) { return (size_t)counters * atm::kLineWords * 4; }
NTM_API int ntm_atomics_ticket_launch(void* counters, void* claim, unsigned heads, unsigned grid, unsigned iters,
                                      unsigned inject_gid, void* stream) {
  return (int)atm::launch_tickets((uint32_t*)counters, (uint32_t*)claim, heads, grid, iters, inject_gid, S(stream));
}
NTM_API size_t ntm_atomics_handoff_slab_bytes(unsigned episodes, unsigned episode_size) {
  return atm::handoff_shape_ok(episodes, episode_size) ? atm::handoff_slab_bytes(episodes, episode_size) : 0;
}
NTM_API int ntm_atomics_handoff_init(void* slabs, unsigned episodes, unsigned episode_size, unsigned long long seed,
                                     unsigned round, void* stream) {
  return (int)atm::launch_handoff_init(slabs, episodes, episode_size, seed, round, S(stream));
}
NTM_API int ntm_atomics_handoff_launch(void* slabs, void* counters, void* records, unsigned episodes,
                                       unsigned episode_size, unsigned long long seed, unsigned round,
                                       unsigned inject_wg, void* stream) {
  return (int)atm::launch_handoff(slabs, (uint32_t*)counters, (atm::Record*)records, episodes, episode_size, seed,
                                  round, inject_wg, S(stream));
}

// Host-only verdicts as JSON (atomics_plan.hpp). Each returns the JSON's length; it is
// written (NUL-terminated) only when it fits in `cap`. 0 = arguments refused.
namespace {
size_t put_json(const std::string& j, char* json, size_t cap) {
  if (json && j.size() < cap) std::memcpy(json, j.c_str(), j.size() + 1);
  return j.size();
}
}  // namespace
NTM_API size_t ntm_atomics_summarize_rmw(int op, const void* got, const void* expected, unsigned long long slots,
                                         int gpu, char* json, size_t cap) {
  if (op < 0 || op >= atm::kOps || !got || !expected) return 0;
  return put_json(atm::rmw_json(atm::summarize_rmw(op, got, expected, slots, gpu)), json, cap);
}
NTM_API size_t ntm_atomics_summarize_tickets(const void* counters, const void* claim, unsigned heads, unsigned grid,
                                             unsigned iters, int gpu, char* json, size_t cap) {
  if (!counters || !claim || !atm::ticket_shape_ok(heads, grid, iters)) return 0;
  return put_json(atm::ticket_json(atm::summarize_tickets((const uint32_t*)counters, (const uint32_t*)claim, heads,
                                                          atm::tickets_per_head(heads, grid, iters),
                                                          grid * atm::kThreads, iters, gpu)),
                  json, cap);
}
NTM_API size_t ntm_atomics_summarize_handoff(const void* records, size_t n, unsigned episodes, unsigned episode_size,
                                             unsigned xcds, unsigned launches, int gpu, char* json, size_t cap) {
  if (!atm::handoff_shape_ok(episodes, episode_size) || xcds < 1 || launches < 1) return 0;
  std::vector<atm::Record> recs(n);
  if (n) std::memcpy(recs.data(), records, n * sizeof(atm::Record));
  return put_json(atm::handoff_json(atm::summarize_handoff(recs.data(), n, episodes, episode_size, xcds, launches, gpu)),
                  json, cap);
}

// K10: matrix-core check of the formats K1 and K7 never issue (mcore.hpp; formats,
// generators, bound and messages in mcore_plan.hpp). fmt: 0 f64, 1 f32, 2 f16, 3 i8,
// 4 sp_bf16, 5 sp_i8. A is [M][K] elements, or for a sparse format Ac [M][K/2] with AI
// [M][K/4] index bytes (ignored otherwise); B is [N][K]; C is [M][N] fp64 / fp32 / int32.
// A bad format, shape or pointer returns hipErrorInvalidValue and launches nothing.
NTM_API int ntm_mcore_gemm(int fmt, const void* A, const void* AI, const void* B, void* C, int M, int N, int K,
                           void* stream) {
  return (int)ntm::mc::launch_mcore(false, fmt, A, AI, B, C, M, N, K, S(stream));
}
NTM_API int ntm_mcore_reference(int fmt, const void* A, const void* AI, const void* B, void* C, int M, int N, int K,
                                void* stream) {
  return (int)ntm::mc::launch_mcore(true, fmt, A, AI, B, C, M, N, K, S(stream));
}
// `out`: ntm_mcore_mismatch_bytes() of device memory holding {0, ~0, 0, 0} as 64-bit words.
NTM_API int ntm_mcore_compare(const void* expected, const void* got, size_t n, int word_bytes, void* out,
                              void* stream) {
  return (int)ntm::mc::launch_mcore_compare(expected, got, n, word_bytes, out, S(stream));
}
NTM_API int ntm_mcore_mismatch_bytes() { return (int)sizeof(ntm::mc::Mismatch); }

// K11: MX quantise / dequantise on the device with the scaled-conversion instructions
// (mxq.hpp; rules, generators and messages in mxq_plan.hpp). fmt as K7; dtype 0 fp32,
// 1 bf16; x / y are [R][ldx] elements of it, packed [R][K * bits / 8] and scales [R][K / 32]
// as ntm_mx_gemm takes them; rounding 0 = nearest even, 1 = stochastic (e2m1 and e4m3 only,
// the random word of element i = row * K + k is hash32(seed, 11, i)). ntm_mxq_cvt is the
// element-level form: it reads the scale bytes instead of choosing them. The
// ntm_mxq_reference_* twins use integer arithmetic only. K % 32 != 0, ldx < K, a bad format,
// dtype or rounding mode, a null pointer, packed not 16-byte or scales not 4-byte aligned
// return hipErrorInvalidValue and launch nothing.
NTM_API int ntm_mxq_shape_ok(int R, int K, int ldx) { return ntm::mxq::shape_ok(R, K, ldx) ? 1 : 0; }
NTM_API int ntm_mxq_quantize(int fmt, int src_dtype, const void* x, void* packed, void* scales, int R, int K, int ldx,
                             int rounding, unsigned long long seed, void* stream) {
  return (int)ntm::mxq::launch_quantize(false, false, fmt, src_dtype, x, packed, scales, R, K, ldx, rounding, seed, S(stream));
}
NTM_API int ntm_mxq_dequantize(int fmt, int dst_dtype, const void* packed, const void* scales, void* y, int R, int K,
                               int ldx, void* stream) {
  return (int)ntm::mxq::launch_dequantize(false, fmt, dst_dtype, packed, scales, y, R, K, ldx, S(stream));
}
NTM_API int ntm_mxq_cvt(int fmt, int src_dtype, const void* x, const void* scales, void* packed, int R, int K, int ldx,
                        int rounding, unsigned long long seed, void* stream) {
  return (int)ntm::mxq::launch_quantize(false, true, fmt, src_dtype, x, packed, const_cast<void*>(scales), R, K, ldx, rounding, seed, S(stream));
}
NTM_API int ntm_mxq_reference_quantize(int fmt, int src_dtype, const void* x, void* packed, void* scales, int R, int K,
                                       int ldx, void* stream) {
  return (int)ntm::mxq::launch_quantize(true, false, fmt, src_dtype, x, packed, scales, R, K, ldx, 0, 0, S(stream));
}
NTM_API int ntm_mxq_reference_dequantize(int fmt, int dst_dtype, const void* packed, const void* scales, void* y, int R,
                                         int K, int ldx, void* stream) {
  return (int)ntm::mxq::launch_dequantize(true, fmt, dst_dtype, packed, scales, y, R, K, ldx, S(stream));
}
NTM_API int ntm_mxq_reference_cvt(int fmt, int src_dtype, const void* x, const void* scales, void* packed, int R, int K,
                                  int ldx, void* stream) {
  return (int)ntm::mxq::launch_quantize(true, true, fmt, src_dtype, x, packed, const_cast<void*>(scales), R, K, ldx, 0, 0, S(stream));
}

// K12: wave data-path and special-function check (wave_paths.hpp; op list, maps, generators,
// records and messages in wave_paths_plan.hpp). `reference` != 0 runs the kernel that uses none
// of the instructions under test. Buffers are 32-bit words, 4-byte aligned (a transposed-read
// image 16-byte aligned); a null or misaligned pointer, a bad op / form / family id or a bad
// shape returns hipErrorInvalidValue and launches nothing.
//   ntm_wave_lane      ops op_first .. op_first + op_count - 1 of the lane list on x[n], y[n]
//                      (n a multiple of 256; each 64 words are one wave) -> out[k * n + i]
//   ntm_wave_tr_read   one workgroup reads an image of rows x stride bytes through the
//                      bits-wide transposed read -> out[ntm_wave_tr_out_words()]
//   ntm_wave_sfu       y[i] = the instruction op on x[i]
//   ntm_wave_sfu_distance  largest ordered-integer distance of y[i] from [lo[i], hi[i]], its
//                      index, the count beyond `bound` and the first such index -> out (16 bytes,
//                      initialised max 0 / all ones / 0 / all ones)
//   ntm_wave_sfu_locate  the second launch behind an inconsistent digest: the first of `grid`
//                      workgroups that runs on the CU cu_key (on_key != 0; else on any other CU)
//                      sets *claim (zeroed by the caller), stores the instruction's words on
//                      x[n] to y and fills *record
//   ntm_wave_valu      op 0: out[table * n + i] = bitop3(a, b, c) for the 256 tables; op 1:
//                      out[i] = bf16(a[i]) | bf16(b[i]) << 16
//   ntm_wave_sweep     the per-CU form: `grid` workgroups each run the whole family against
//                      `expected` and leave one Record (layout of `in`: wave_paths.hpp)
NTM_API int ntm_wave_lane_ops() { return ntm::wave::kLaneOps; }
NTM_API int ntm_wave_record_bytes() { return (int)sizeof(ntm::wave::Record); }
NTM_API int ntm_wave_lane(int reference, int op_first, int op_count, const void* x, const void* y, void* out, size_t n,
                          void* stream) {
  return (int)ntm::wave::launch_lane(reference != 0, op_first, op_count, x, y, out, n, S(stream));
}
NTM_API int ntm_wave_tr_out_words(int bits, int rows, int stride) {
  ntm::wave::TrShape s;
  return ntm::wave::tr_shape(bits, rows, stride, &s) ? (int)ntm::wave::tr_out_words(s) : 0;
}
NTM_API int ntm_wave_tr_read(int reference, int bits, const void* image, int rows, int stride, void* out, void* stream) {
  return (int)ntm::wave::launch_tr_read(reference != 0, bits, image, rows, stride, out, S(stream));
}
NTM_API int ntm_wave_sfu(int op, const void* x, void* y, size_t n, void* stream) {
  return (int)ntm::wave::launch_sfu(op, x, y, n, S(stream));
}
NTM_API int ntm_wave_sfu_distance(const void* y, const void* lo, const void* hi, size_t n, unsigned bound, void* out,
                                  void* stream) {
  return (int)ntm::wave::launch_sfu_distance(y, lo, hi, n, bound, out, S(stream));
}
NTM_API int ntm_wave_sfu_locate(int op, const void* x, unsigned n, unsigned cu_key, int on_key, void* claim, void* y,
                                void* record, int grid, unsigned fault_key, unsigned fault_index, void* stream) {
  return (int)ntm::wave::launch_sfu_locate(op, x, n, cu_key, on_key, claim, y, record, grid, fault_key, fault_index, S(stream));
}
NTM_API int ntm_wave_valu(int reference, int op, const void* a, const void* b, const void* c, void* out, size_t n,
                          void* stream) {
  return (int)ntm::wave::launch_valu(reference != 0, op, a, b, c, out, n, S(stream));
}
NTM_API int ntm_wave_sweep(int family, const void* in, size_t in_words, const unsigned* layout, const void* expected,
                           void* records, int grid, unsigned fault_wg, unsigned fault_index, void* stream) {
  return (int)ntm::wave::launch_sweep(family, in, in_words, layout, expected, records, grid, fault_wg, fault_index, S(stream));
}

// K13: fused attention forward (attn.hpp; shapes, the arithmetic contract, exact inputs and
// messages in attn_plan.hpp). Q [B][Hq][Sq][128], K and V [B][Hkv][Sk][128], O like Q, all
// contiguous bf16 and 16-byte aligned; m, l [B][Hq][Sq] fp32 and table (ntm_attn_table_bytes:
// raw HW_ID and XCC_ID per workgroup) may be null. ntm_attn_reference is the kernel without
// matrix or cross-lane instructions; each of its outputs may be null: O (bf16), O32 (the fp32
// quotient before the pack), absum (sum p |v| / l), m, l. ntm_attn_compare counts the 4-byte
// words that differ into a K7 mismatch record. A bad shape (Hq % Hkv, Sk > 65536, causal with
// Sk < Sq), a scale that is not positive, a null or misaligned pointer return
// hipErrorInvalidValue and launch nothing.
NTM_API int ntm_attn_shape_ok(int B, int Hq, int Hkv, int Sq, int Sk, int causal) {
  return ntm::attn::shape_ok(B, Hq, Hkv, Sq, Sk, causal) ? 1 : 0;
}
NTM_API size_t ntm_attn_table_bytes(int B, int Hq, int Sq) {
  return B > 0 && Hq > 0 && Sq > 0 ? (size_t)ntm::attn::grid(B, Hq, Sq) * ntm::attn::kTableWords * 4 : 0;
}
NTM_API int ntm_attn_lds_bytes() { return ntm::attn::kLdsBytes; }
NTM_API int ntm_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* m, float* l, unsigned* table, int B,
                         int Hq, int Hkv, int Sq, int Sk, int causal, float scale_log2, void* stream) {
  return (int)ntm::attn::launch_attn_fwd(Q, K, V, O, m, l, table, B, Hq, Hkv, Sq, Sk, causal, scale_log2, S(stream));
}
NTM_API int ntm_attn_reference(const void* Q, const void* K, const void* V, void* O, float* O32, float* absum, float* m,
                               float* l, int B, int Hq, int Hkv, int Sq, int Sk, int causal, float scale_log2,
                               void* stream) {
  return (int)ntm::attn::launch_attn_reference(Q, K, V, O, O32, absum, m, l, B, Hq, Hkv, Sq, Sk, causal, scale_log2,
                                               S(stream));
}
NTM_API int ntm_attn_compare(const void* expected, const void* got, size_t n, void* out, void* stream) {
  return (int)ntm::attn::launch_attn_compare(expected, got, n, out, S(stream));
}
NTM_API int ntm_attn_mismatch_bytes() { return (int)sizeof(ntm::mx::Mismatch); }

// K14: paged-KV decode attention (pda.hpp; shapes, the split plan and the arithmetic contract in
// pda_plan.hpp). Q and O [B][Hq][T][128], the K and V pools [pages][Hkv][16][128], all contiguous
// bf16 and 16-byte aligned; block_table [B][max_pages] and seq_lens [B] int32 on the device;
// workspace of ntm_pda_workspace_bytes, 16-byte aligned; m, l [B][Hq][T] fp32 and table
// (ntm_pda_table_bytes: raw HW_ID and XCC_ID per split workgroup) may be null. Two launches on
// the stream: the split kernel, then the combine. A bad shape (Hq % Hkv, T > 4, Hq / Hkv * T > 32,
// splits outside 1 .. 64, max_pages > 4096), a scale that is not positive, a null or misaligned
// pointer return hipErrorInvalidValue and launch nothing. The reference is ntm_attn_reference on
// the gathered keys of one sequence, the compare ntm_attn_compare.
NTM_API int ntm_pda_shape_ok(int B, int Hq, int Hkv, int T, int max_pages, int pages, int splits) {
  return ntm::pda::shape_ok(B, Hq, Hkv, T, max_pages, pages, splits) ? 1 : 0;
}
NTM_API size_t ntm_pda_workspace_bytes(int B, int Hkv, int splits) { return ntm::pda::workspace_bytes(B, Hkv, splits); }
NTM_API size_t ntm_pda_table_bytes(int B, int Hkv, int splits) { return ntm::pda::table_bytes(B, Hkv, splits); }
NTM_API int ntm_pda_lds_bytes() { return ntm::pda::kLdsBytes; }
NTM_API int ntm_pda_default_splits(int B, int Hkv, int max_len, int cus) { return ntm::pda::pda_splits(B, Hkv, max_len, cus); }
NTM_API int ntm_pda_fwd(const void* Q, const void* Kpool, const void* Vpool, const int* block_table, const int* seq_lens,
                        void* O, float* m, float* l, void* workspace, unsigned* table, int B, int Hq, int Hkv, int T,
                        int max_pages, int pages, int splits, float scale_log2, void* stream) {
  return (int)ntm::pda::launch_pda_fwd(Q, Kpool, Vpool, block_table, seq_lens, O, m, l, workspace, table, B, Hq, Hkv, T,
                                       max_pages, pages, splits, scale_log2, S(stream));
}
