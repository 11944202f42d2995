// amdgpu-validate: what the checks found and how it is reported (host-only C++17, no
// HIP include).
//
// One small struct per check; GpuResult is their composition. An opt-in check's
// struct carries its own `failures`, its JSON fragment (json(): `,"key":value...`,
// appended to the GPU's object) and its Prometheus metrics (prometheus()). The
// top-level writers at the end stitch them in a fixed order: report_json(),
// prometheus_text() and termination_message(). tests/test_validate_report.py runs
// them in a stand-alone sanitized program on synthetic results.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "ntm/atomics_plan.hpp"
#include "ntm/attn_plan.hpp"
#include "ntm/cu_sweep_plan.hpp"
#include "ntm/host_link_plan.hpp"
#include "ntm/mcore_plan.hpp"
#include "ntm/mxq_plan.hpp"
#include "ntm/pda_plan.hpp"
#include "ntm/wave_paths_plan.hpp"
#include "ntm/xcd_sweep_plan.hpp"

#include "json.hpp"
#include "options.hpp"

namespace ntm::job {

struct GpuResult;
using Gpus = std::vector<GpuResult>;

constexpr unsigned long long kNotRun = ~0ull;  // a count that no check has written yet

inline std::string count_or_null(unsigned long long v) {
  return v == kNotRun ? std::string("null") : std::to_string(v);
}

inline std::string jstrs(const std::vector<std::string>& v) {
  std::string s = "[";
  for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + jstr(v[i]);
  return s + "]";
}

// K1: the bf16 GEMM against the fp32 reference, and the build with the fused ABFT row checksum
struct K1Result {
  double ms = 0, tflops = 0;
  unsigned long long bad = kNotRun;
  float max_err = NAN;
  unsigned long long abft_bad_acc = kNotRun, abft_bad_store = kNotRun;
  float abft_max_rel_acc = NAN;
  double abft_tflops = 0;
  std::string json() const {
    return ",\"gemm_ms\":" + jnum(ms) + ",\"gemm_tflops\":" + jnum(tflops) +
           ",\"gemm_wrong\":" + count_or_null(bad) + ",\"gemm_max_abs_err\":" + jnum(max_err) +
           ",\"abft_tflops\":" + jnum(abft_tflops) + ",\"abft_bad_rows\":" +
           (abft_bad_acc == kNotRun ? std::string("null") : std::to_string(abft_bad_acc + abft_bad_store)) +
           ",\"abft_max_rel_err\":" + jnum(abft_max_rel_acc);
  }
};

// K1-fp8: the same schedule on e4m3 operands
struct Fp8Result {
  double ms = 0, tflops = 0;
  unsigned long long bad = kNotRun;       // stays ~0 when --no-fp8
  float max_err = NAN;
  unsigned long long abft_bad = kNotRun;  // rows failing the fp8 fused checksum (~0: not run)
  std::string json() const {
    return ",\"gemm_fp8_tflops\":" + jnum(tflops) + ",\"gemm_fp8_wrong\":" + count_or_null(bad) +
           ",\"gemm_fp8_max_abs_err\":" + jnum(max_err) +
           ",\"gemm_fp8_abft_bad_rows\":" + count_or_null(abft_bad);
  }
};

// stream-K split mode self-check (kSkM x kSkN x kSkK on a 192-wide tile)
struct SkResult {
  int variant = 0;                     // 54 / 55 (0: not served on this device)
  unsigned long long bad = kNotRun;    // elements off the fp32 reference (~0: not run)
  unsigned word = 0;                   // the workspace's XCD-placement error word
  double ms = 0;
  std::string json() const {
    return ",\"sk_split_variant\":" + std::to_string(variant) + ",\"sk_split_wrong\":" + count_or_null(bad) +
           ",\"sk_xcc_error\":" + std::to_string(word) + ",\"sk_split_ms\":" + jnum(ms);
  }
};

// K2: HBM stream copy / read
struct K2Result {
  double copy_gbps = 0, read_gbps = 0;
  bool copy_ok = false;
  std::string json() const {
    return ",\"hbm_copy_GBps\":" + jnum(copy_gbps) + ",\"hbm_read_GBps\":" + jnum(read_gbps);
  }
};

// K4 (only with --hbm-test-gb)
struct HbmTestResult {
  bool ran = false;
  double gb = 0, requested_gb = 0;
  unsigned long long bad_words = 0, bad_bits = 0;
  double write_gbps = 0, verify_gbps = 0, seconds = 0, alloc_s = 0, free_s = 0;
  std::string steps;                  // JSON array of per-step seconds
  std::vector<std::string> failures;  // empty = clean
  std::string json() const {
    if (!ran) return "";
    return ",\"hbm_test_gb\":" + jnum(gb) + ",\"hbm_test_requested_gb\":" + jnum(requested_gb) +
           ",\"hbm_test_bad_words\":" + std::to_string(bad_words) +
           ",\"hbm_test_bad_bits\":" + std::to_string(bad_bits) +
           ",\"hbm_test_write_GBps\":" + jnum(write_gbps) + ",\"hbm_test_verify_GBps\":" + jnum(verify_gbps) +
           ",\"hbm_test_s\":" + jnum(seconds) + ",\"hbm_test_alloc_s\":" + jnum(alloc_s) +
           ",\"hbm_test_free_s\":" + jnum(free_s) +
           ",\"hbm_test_steps\":" + (steps.empty() ? std::string("[]") : steps);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K5 (only with --cu-sweep)
struct CuSweepResult {
  bool ran = false;
  ntm::cus::Summary sum;
  int lds_bytes = 0;
  double seconds = 0;
  std::vector<std::string> failures;  // empty = clean
  std::string json() const {
    if (!ran) return "";
    return ",\"cu_sweep_cus\":" + std::to_string(sum.cus) +
           ",\"cu_sweep_cus_covered\":" + std::to_string(sum.cus_covered) +
           ",\"cu_sweep_simds_covered\":" + std::to_string(sum.simds_covered) +
           ",\"cu_sweep_launches\":" + std::to_string(sum.launches) +
           ",\"cu_sweep_bad_cus\":" + ntm::cus::bad_cus_json(sum) +
           ",\"cu_sweep_lds_bytes\":" + std::to_string(lds_bytes) + ",\"cu_sweep_s\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K6 (only with --host-link-mib)
struct HostLinkResult {
  bool ran = false;
  long mib = 0;
  double h2d_gbps = 0, d2h_gbps = 0;            // pull / push kernels
  double h2d_copy_gbps = 0, d2h_copy_gbps = 0;  // hipMemcpyAsync
  double duplex_gbps = 0, latency_us = 0;
  unsigned long long bad_words = 0, bad_bits = 0;
  ntm::hostlink::LinkState pcie;
  double seconds = 0, pin_s = 0, xfer_s = 0, free_s = 0;
  std::vector<std::string> failures;  // empty = clean
  // per direction, the faster of kernel and hipMemcpyAsync (a degraded link caps both)
  double h2d_best() const { return std::max(h2d_gbps, h2d_copy_gbps); }
  double d2h_best() const { return std::max(d2h_gbps, d2h_copy_gbps); }
  std::string json() const {
    if (!ran) return "";
    return ",\"host_link_mib\":" + std::to_string(mib) +
           ",\"host_link_h2d_GBps\":" + jnum(h2d_gbps) + ",\"host_link_d2h_GBps\":" + jnum(d2h_gbps) +
           ",\"host_link_h2d_copy_GBps\":" + jnum(h2d_copy_gbps) +
           ",\"host_link_d2h_copy_GBps\":" + jnum(d2h_copy_gbps) +
           ",\"host_link_duplex_GBps\":" + jnum(duplex_gbps) +
           ",\"host_link_read_latency_us\":" + jnum(latency_us) +
           ",\"host_link_bad_words\":" + std::to_string(bad_words) +
           ",\"host_link_bad_bits\":" + std::to_string(bad_bits) +
           ",\"host_link_pcie\":" + ntm::hostlink::link_json(pcie) +
           ",\"host_link_s\":" + jnum(seconds) + ",\"host_link_pin_s\":" + jnum(pin_s) +
           ",\"host_link_transfer_s\":" + jnum(xfer_s) + ",\"host_link_free_s\":" + jnum(free_s);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K7 (only with --mx-check)
struct MxResult {
  bool ran = false;
  std::vector<std::string> formats;  // formats whose every step compared clean
  unsigned long long bad_elements = 0;
  double fp4_tflops = 0, seconds = 0;
  int scale_spread = 0;
  std::vector<std::string> failures;  // empty = clean
  std::string json() const {
    if (!ran) return "";
    return ",\"mx_formats\":" + jstrs(formats) + ",\"mx_bad_elements\":" + std::to_string(bad_elements) +
           ",\"mx_fp4_tflops\":" + jnum(fp4_tflops) + ",\"mx_scale_spread\":" + std::to_string(scale_spread) +
           ",\"mx_s\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K8: one level and mode of the per-XCD sweep
struct XcdCell {
  ntm::xcs::Summary sum;
  uint32_t passes = 0;       // read: passes over the slice; mfma: batches per wave
  uint64_t min_span_ticks = 0, max_span_ticks = 0;  // over the XCDs that timed something
  bool gated = false;        // the rate rule judges this cell (ntm::xcs::gated)
};

// K8 (only with --xcd-sweep)
struct XcdSweepResult {
  bool ran = false;
  uint32_t xcds = 0;
  long mib = 0;              // --xcd-sweep-mib and --xcd-ratio as the sweep ran them
  double ratio = 0;
  std::vector<XcdCell> cells;   // one per level and mode that ran
  std::vector<std::string> failures;
  double seconds = 0;
  std::string json() const {
    if (!ran) return "";
    namespace xs = ntm::xcs;
    std::string js = ",\"xcd_sweep_xcds\":" + std::to_string(xcds) + ",\"xcd_sweep_mib\":" + std::to_string(mib) +
                     ",\"xcd_sweep_ratio\":" + jnum(ratio);
    std::string slow = "[", bad = "[", rule;
    for (auto& c : cells) {
      const std::string k = std::string(",\"xcd_sweep_") + xs::level_name(c.sum.level) + "_" +
                            xs::mode_name(c.sum.mode);
      js += k + "_rate\":" + xs::rates_json(c.sum) + k + "_clock_ghz\":" + xs::clocks_json(c.sum) +
            k + "_min_over_median\":" + jnum(c.sum.min_over_median) +
            k + "_median\":" + jnum(c.sum.median_rate) +
            k + "_passes\":" + std::to_string(c.passes) +
            k + "_span_us\":[" + jnum((double)c.min_span_ticks * 0.01) + "," +
            jnum((double)c.max_span_ticks * 0.01) + "]" +
            k + "_gated\":" + jbool(c.gated);
      const std::string at = std::string(",\"level\":") + jstr(xs::level_name(c.sum.level)) +
                             ",\"mode\":" + jstr(xs::mode_name(c.sum.mode)) + "}";
      for (uint32_t x : c.sum.slow) slow += std::string(slow.size() > 1 ? "," : "") + "{\"xcd\":" + std::to_string(x) + at;
      for (uint32_t x : c.sum.bad) bad += std::string(bad.size() > 1 ? "," : "") + "{\"xcd\":" + std::to_string(x) + at;
      if (c.gated && !c.sum.rule_ran) rule = c.sum.rule_skipped;
    }
    return js + ",\"xcd_sweep_slow\":" + slow + "],\"xcd_sweep_bad\":" + bad + "]" +
           ",\"xcd_sweep_rule_skipped\":" + jstr(rule) + ",\"xcd_sweep_failures\":" + jstrs(failures) +
           ",\"xcd_sweep_s\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K9: one op of the atomics check
struct AtomicsOpRow {
  int op = 0;
  unsigned long long bad = 0;  // slots that differ from the reference table
  double gops = 0;             // 1e9 atomic operations per second, reported only
};

// K9 (only with NTM_ATOMICS_CHECK=1)
struct AtomicsResult {
  bool ran = false;
  std::vector<AtomicsOpRow> ops;
  unsigned long long ticket_bad = 0, handoff_bad_words = 0, handoff_stale_words = 0;
  double episodes_per_s = 0;
  uint32_t xcds = 0, xcd_pairs_covered = 0;
  std::vector<uint8_t> pairs;  // kMaxXcds x kMaxXcds, [writer][reader]
  double seconds = 0;
  std::vector<std::string> failures;  // empty = clean
  std::string json() const {
    if (!ran) return "";
    std::string names = "[", per_op, m = "[";
    for (size_t i = 0; i < ops.size(); ++i) {
      const std::string n = ntm::atm::op_name(ops[i].op);
      names += (i ? "," : "") + jstr(n);
      per_op += ",\"atomics_" + n + "_bad\":" + std::to_string(ops[i].bad) + ",\"atomics_" + n + "_gops\":" +
                jnum(ops[i].gops);
    }
    for (uint32_t w = 0; w < xcds && !pairs.empty(); ++w) {
      m += w ? ",[" : "[";
      for (uint32_t x = 0; x < xcds; ++x)
        m += (x ? "," : "") + std::to_string((int)pairs[(size_t)w * ntm::atm::kMaxXcds + x]);
      m += "]";
    }
    return ",\"atomics_ops\":" + names + "]" + per_op + ",\"atomics_ticket_bad\":" + std::to_string(ticket_bad) +
           ",\"atomics_handoff_bad_words\":" + std::to_string(handoff_bad_words) +
           ",\"atomics_handoff_stale_words\":" + std::to_string(handoff_stale_words) +
           ",\"atomics_handoff_episodes_per_s\":" + jnum(episodes_per_s) +
           ",\"atomics_xcd_pairs_covered\":" + std::to_string(xcd_pairs_covered) +
           ",\"atomics_xcd_pairs\":" + m + "]" + ",\"atomics_seconds\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K10 (only with NTM_MCORE_CHECK=1)
struct McoreResult {
  bool ran = false;
  unsigned long long bad[ntm::mc::kFormats] = {};  // result words that differ, decode sweep and dense runs
  double f64_tflops = 0, i8_tops = 0;              // the verified 4096^3 products, reported only
  double seconds = 0;
  std::vector<std::string> failures;  // empty = clean
  double rate(int fmt) const { return fmt == ntm::mc::kF64 ? f64_tflops : i8_tops; }
  std::string json() const {
    if (!ran) return "";
    std::string names = "[", per;
    for (int f = 0; f < ntm::mc::kFormats; ++f) {
      const std::string n = ntm::mc::format_name(f);
      names += (f ? "," : "") + jstr(n);
      per += ",\"mcore_" + n + "_bad\":" + std::to_string(bad[f]);
    }
    return ",\"mcore_formats\":" + names + "]" + per + ",\"mcore_f64_tflops\":" + jnum(f64_tflops) +
           ",\"mcore_i8_tops\":" + jnum(i8_tops) + ",\"mcore_seconds\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K11 (only with NTM_MXQ_CHECK=1)
struct MxqResult {
  bool ran = false;
  // 32-bit words that differ, per format: conversion sweeps down / up, block quantise (packed
  // and scale bytes), end to end (e2m1, e2m3 and e4m3 only)
  unsigned long long bad_down[ntm::mx::kFormats] = {}, bad_up[ntm::mx::kFormats] = {},
                     bad_block[ntm::mx::kFormats] = {}, bad_e2e[ntm::mx::kFormats] = {};
  double quantize_gbps = 0;  // fp32 -> e2m1, 8192 x 8192, bytes read + written; reported only
  double seconds = 0;
  std::vector<std::string> failures;  // empty = clean
  unsigned long long bad(int f) const { return bad_down[f] + bad_up[f] + bad_block[f] + bad_e2e[f]; }
  std::string json() const {
    if (!ran) return "";
    std::string names = "[", per;
    for (int f = 0; f < ntm::mx::kFormats; ++f) {
      const std::string n = ntm::mx::format_name(f);
      names += (f ? "," : "") + jstr(n);
      per += ",\"mxq_" + n + "_down_bad\":" + std::to_string(bad_down[f]) + ",\"mxq_" + n +
             "_up_bad\":" + std::to_string(bad_up[f]) + ",\"mxq_" + n + "_block_bad\":" + std::to_string(bad_block[f]) +
             ",\"mxq_" + n + "_e2e_bad\":" + std::to_string(bad_e2e[f]);
    }
    return ",\"mxq_formats\":" + names + "]" + per + ",\"mxq_quantize_GBps\":" + jnum(quantize_gbps) +
           ",\"mxq_seconds\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K12 (only with NTM_WAVE_CHECK=1)
struct WaveResult {
  bool ran = false;
  uint32_t cus = 0, cus_covered = 0;  // CUs that ran every family
  // result words that differ from the reference kernels' tables, over all workgroups
  unsigned long long lane_bad = 0, ldstr_bad = 0, valu_bad = 0;
  unsigned long long sfu_inconsistent = 0;  // (workgroup, instruction) digests off the majority's
  uint32_t sfu_max_d[ntm::wave::kSfuOps] = {}, sfu_max_x[ntm::wave::kSfuOps] = {};  // largest distance, its input
  unsigned long long sfu_beyond = 0;        // results beyond a recorded bound
  double seconds = 0;
  std::vector<std::string> failures;  // empty = clean
  std::string json() const {
    if (!ran) return "";
    std::string d = "{";
    for (int op = 0; op < ntm::wave::kSfuOps; ++op)
      d += std::string(op ? "," : "") + jstr(ntm::wave::sfu_name(op)) + ":{\"d\":" + std::to_string(sfu_max_d[op]) +
           ",\"input\":" + jstr(ntm::wave::hex32(sfu_max_x[op])) + ",\"judged\":" +
           (ntm::wave::kSfuBound[op] != ntm::wave::kSfuNoBound ? "true" : "false") + "}";
    return ",\"wave_lane_bad\":" + std::to_string(lane_bad) + ",\"wave_ldstr_bad\":" + std::to_string(ldstr_bad) +
           ",\"wave_valu_bad\":" + std::to_string(valu_bad) + ",\"wave_sfu_inconsistent\":" +
           std::to_string(sfu_inconsistent) + ",\"wave_sfu_max_distance\":" + d + "}" + ",\"wave_sfu_beyond_bound\":" +
           std::to_string(sfu_beyond) + ",\"wave_cus_covered\":" + std::to_string(cus_covered) +
           ",\"wave_seconds\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K13 (only with NTM_ATTN_CHECK=1)
struct AttnResult {
  bool ran = false;
  unsigned long long exact_bad = 0;  // 4-byte words of O, m, l that differ from the reference kernel's
  unsigned long long dense_bad = 0;  // elements beyond 2^-7 a + 2^-20
  float dense_worst = 0;             // largest error / a of the dense sub-test
  uint32_t cus = 0, cus_covered = 0, launches = 0;  // exact launches, and the CUs their tables showed
  double tflops = 0;                 // B 4, Hq 32, Hkv 8, S 4096, causal; reported only
  double seconds = 0;
  std::vector<std::string> failures;  // empty = clean
  std::string json() const {
    if (!ran) return "";
    return ",\"attn_exact_bad\":" + std::to_string(exact_bad) + ",\"attn_dense_bad\":" + std::to_string(dense_bad) +
           ",\"attn_dense_worst_err_over_a\":" + jnum(dense_worst) + ",\"attn_cus_covered\":" +
           std::to_string(cus_covered) + ",\"attn_launches\":" + std::to_string(launches) + ",\"attn_tflops\":" +
           jnum(tflops) + ",\"attn_seconds\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

// K14 (only with NTM_PDA_CHECK=1)
struct PdaResult {
  bool ran = false;
  unsigned long long exact_bad = 0;  // 4-byte words of O, m, l that differ from the reference kernel's
  unsigned long long dense_bad = 0;  // elements beyond 2^-7 a + 2^-20
  float dense_worst = 0;             // largest error / a of the dense sub-test
  uint32_t cus = 0, cus_covered = 0, launches = 0;  // exact launches, and the CUs their tables showed
  uint32_t splits = 0;               // the default S of the timed shape on this device
  double kv_gbps = 0;                // B 32, Hq 32, Hkv 8, T 1, len 8192: K and V bytes / time; reported only
  double seconds = 0;
  std::vector<std::string> failures;  // empty = clean
  std::string json() const {
    if (!ran) return "";
    return ",\"pda_exact_bad\":" + std::to_string(exact_bad) + ",\"pda_dense_bad\":" + std::to_string(dense_bad) +
           ",\"pda_dense_worst_err_over_a\":" + jnum(dense_worst) + ",\"pda_cus_covered\":" +
           std::to_string(cus_covered) + ",\"pda_launches\":" + std::to_string(launches) + ",\"pda_splits\":" +
           std::to_string(splits) + ",\"pda_kv_gbps\":" + jnum(kv_gbps) + ",\"pda_seconds\":" + jnum(seconds);
  }
  static void prometheus(std::ostream& p, const Gpus& res);
};

struct GpuResult {
  int device = -1;
  std::string name, arch;
  double total_gb = 0, free_gb = 0;
  double t_init = 0, t_gemm = 0, t_hbm = 0;  // wall clock; t_hbm is stamped after the opt-in checks
  K1Result k1;
  SkResult sk;
  Fp8Result fp8;
  K2Result k2;
  HbmTestResult hbm_test;
  CuSweepResult cu_sweep;
  HostLinkResult host_link;
  MxResult mx;
  XcdSweepResult xcd;
  AtomicsResult atomics;
  McoreResult mcore;
  MxqResult mxq;
  WaveResult wave;
  AttnResult attn;
  PdaResult pda;
};

// ------------------------------------------------------------ per-GPU verdicts
// Every failure one GPU's results amount to under `o`, in the order the report lists them.
inline std::vector<std::string> gpu_failures(const GpuResult& r, const Opts& o) {
  std::vector<std::string> out;
  const std::string d = "gpu" + std::to_string(r.device) + ": ";
  if (r.k1.bad != 0) out.push_back(d + "GEMM verification failed (" + std::to_string(r.k1.bad) + " elements)");
  if (r.sk.variant && r.sk.word != 0) {
    char w[16];
    std::snprintf(w, sizeof w, "0x%08x", r.sk.word);
    out.push_back(d + "stream-K split mode: a split tile's parts ran on different XCDs (error word " + w +
                  "); its C is not trusted");
  }
  if (r.sk.variant && r.sk.bad != 0)
    out.push_back(d + "stream-K split-mode GEMM verification failed (" + std::to_string(r.sk.bad) + " elements)");
  if (r.k1.abft_bad_acc != 0 || r.k1.abft_bad_store != 0)
    out.push_back(d + "GEMM ABFT checksum failed (" + std::to_string(r.k1.abft_bad_acc) + " accumulator / " +
                  std::to_string(r.k1.abft_bad_store) + " stored rows)");
  if (o.tflops_floor > 0 && r.k1.tflops < o.tflops_floor)
    out.push_back(d + "GEMM " + jnum(r.k1.tflops) + " TFLOP/s below floor " + jnum(o.tflops_floor));
  if (o.fp8 && r.fp8.bad != 0)
    out.push_back(d + "fp8 GEMM verification failed (" +
                  (r.fp8.bad == kNotRun ? std::string("not run: --size must be a multiple of 256")
                                        : std::to_string(r.fp8.bad) + " elements") + ")");
  if (o.fp8 && r.fp8.abft_bad != 0 && r.fp8.abft_bad != kNotRun)
    out.push_back(d + "fp8 GEMM ABFT checksum failed (" + std::to_string(r.fp8.abft_bad) + " rows)");
  if (o.fp8 && o.fp8_tflops_floor > 0 && r.fp8.tflops < o.fp8_tflops_floor)
    out.push_back(d + "fp8 GEMM " + jnum(r.fp8.tflops) + " TFLOP/s below floor " + jnum(o.fp8_tflops_floor));
  if (o.min_hbm_gb > 0 && r.total_gb < o.min_hbm_gb)
    out.push_back(d + "HBM " + jnum(r.total_gb) + " GB below " + jnum(o.min_hbm_gb) + " GB");
  if (!r.k2.copy_ok) out.push_back(d + "HBM copy mismatch");
  for (const auto* v : {&r.hbm_test.failures, &r.cu_sweep.failures, &r.host_link.failures, &r.mx.failures,
                        &r.xcd.failures, &r.atomics.failures, &r.mcore.failures, &r.mxq.failures, &r.wave.failures,
                        &r.attn.failures, &r.pda.failures})
    out.insert(out.end(), v->begin(), v->end());
  if (o.hbm_floor_gbps > 0 && r.k2.copy_gbps < o.hbm_floor_gbps)
    out.push_back(d + "HBM copy " + jnum(r.k2.copy_gbps) + " GB/s below floor");
  return out;
}

// ------------------------------------------------------------ collectives, host
struct CollRow {
  const char* dtype;
  size_t bytes;
  double us, algbw, busbw;
  unsigned long long bad;
};

inline std::string coll_json(const std::vector<CollRow>& rows) {
  std::string s = "[";
  for (size_t i = 0; i < rows.size(); ++i) {
    const auto& r = rows[i];
    s += (i ? "," : "") + std::string("{\"dtype\":\"") + r.dtype + "\",\"bytes\":" +
         std::to_string(r.bytes) +
         ",\"time_us\":" + jnum(r.us) + ",\"algbw_GBps\":" + jnum(r.algbw) +
         ",\"busbw_GBps\":" + jnum(r.busbw) + ",\"wrong\":" + std::to_string(r.bad) + "}";
  }
  return s + "]";
}

// peak busbw of the bf16 rows (the floors gate the interconnect, not a size)
inline double peak_busbw(const std::vector<CollRow>& rows) {
  double m = 0;
  for (auto& r : rows)
    if (std::strncmp(r.dtype, "bf16", 4) == 0 && std::isfinite(r.busbw)) m = std::max(m, r.busbw);
  return m;
}

// C3: the per-link xGMI pull matrix
struct P2pResult {
  int n = 0;
  std::vector<double> gbps;  // n x n, row = destination (puller), NAN on the diagonal
  unsigned long long bad_pairs = 0;
  double min_gbps = 0;
  std::string json() const {
    std::string js = "[";
    for (int d = 0; d < n; ++d) {
      js += d ? ",[" : "[";
      for (int s2 = 0; s2 < n; ++s2) js += (s2 ? "," : "") + jnum(gbps[(size_t)d * n + s2]);
      js += "]";
    }
    return js + "]";
  }
};

// --xgmi-tune: what the mini-sweep chose (and its table) for the JSON report.
struct XgmiTune {
  bool ran = false;
  int nblk = 0;
  size_t one_shot_max = 0;
  double seconds = 0;
  std::string table = "[]";
};

// MI355X host preparation as the pod sees it (the node-prep DaemonSet of
// modules/amd-gpu-stack, or the EKS pre-bootstrap user data, sets it up):
// automatic NUMA balancing off (a host-wide sysctl, readable in any
// container), RLIMIT_MEMLOCK unlimited for this process (inherited from
// containerd's LimitMEMLOCK; RCCL pins host memory) and iommu=pt on the
// kernel command line (xGMI / PCIe peer DMA).
struct HostPrep {
  int numa_balancing = -1;  // -1: unreadable
  bool memlock_unlimited = false;
  bool iommu_pt = false;
};

// ------------------------------------------------------------ the whole run
struct Report {
  Opts o;
  std::string node;        // NODE_NAME (downward API in the module's Job), "" when unset
  std::vector<int> devs;   // the HIP device of each entry of `gpus`
  Gpus gpus;
  std::vector<CollRow> rccl_rows, xgmi_rows;
  XgmiTune xtune;
  P2pResult p2p;
  HostPrep hp;
  double t_start = 0, t_hip = 0, t_rccl = 0, t_end = 0;  // wall clock, epoch seconds
  std::vector<std::string> failures;
  std::string push_status;  // only with --pushgateway

  bool passed() const { return failures.empty(); }
  double gemm_tflops_aggregate() const {
    double agg = 0;
    for (auto& r : gpus) agg += r.k1.tflops;
    return agg;
  }
  // the largest busbw of any row (the metric and the termination message; the floors use peak_busbw)
  static double peak_any(const std::vector<CollRow>& rows) {
    double m = 0;
    for (auto& c : rows) m = std::max(m, c.busbw);
    return m;
  }
};

// ------------------------------------------------------------ Prometheus
// One per-GPU gauge: HELP (when there is one) and TYPE once, then one sample for every
// GPU for which `ran` holds.
template <class Ran, class Value>
void gauge(std::ostream& p, const Gpus& res, const std::string& name, const char* help, Ran ran, Value value) {
  if (help) p << "# HELP " << name << " " << help << "\n";
  p << "# TYPE " << name << " gauge\n";
  for (auto& r : res)
    if (ran(r)) p << name << "{gpu=\"" << r.device << "\"} " << value(r) << "\n";
}

inline bool every_gpu(const GpuResult&) { return true; }

inline void HbmTestResult::prometheus(std::ostream& p, const Gpus& res) {
  auto ran = [](const GpuResult& r) { return r.hbm_test.ran; };
  gauge(p, res, "amdgpu_validate_hbm_test_gb", "HBM written, read back and compared by the pattern test.", ran,
        [](const GpuResult& r) { return jnum(r.hbm_test.gb); });
  gauge(p, res, "amdgpu_validate_hbm_test_bad_words", "8-byte words the pattern test read back wrong.", ran,
        [](const GpuResult& r) { return r.hbm_test.bad_words; });
}

inline void CuSweepResult::prometheus(std::ostream& p, const Gpus& res) {
  auto ran = [](const GpuResult& r) { return r.cu_sweep.ran; };
  gauge(p, res, "amdgpu_validate_cu_sweep_cus_covered", "Compute units that ran a workgroup of the CU sweep.", ran,
        [](const GpuResult& r) { return r.cu_sweep.sum.cus_covered; });
  gauge(p, res, "amdgpu_validate_cu_sweep_bad_cus", "Compute units with a wrong known-answer result.", ran,
        [](const GpuResult& r) { return r.cu_sweep.sum.bad_cus.size(); });
}

inline void HostLinkResult::prometheus(std::ostream& p, const Gpus& res) {
  auto ran = [](const GpuResult& r) { return r.host_link.ran; };
  gauge(p, res, "amdgpu_validate_host_link_h2d_gbps",
        "Host-to-device rate over the host link (faster of kernel and hipMemcpyAsync).", ran,
        [](const GpuResult& r) { return jnum(r.host_link.h2d_best()); });
  gauge(p, res, "amdgpu_validate_host_link_d2h_gbps",
        "Device-to-host rate over the host link (faster of kernel and hipMemcpyAsync).", ran,
        [](const GpuResult& r) { return jnum(r.host_link.d2h_best()); });
  gauge(p, res, "amdgpu_validate_host_link_bad_words", "8-byte words that crossed the host link wrong.", ran,
        [](const GpuResult& r) { return r.host_link.bad_words; });
}

inline void MxResult::prometheus(std::ostream& p, const Gpus& res) {
  auto ran = [](const GpuResult& r) { return r.mx.ran; };
  gauge(p, res, "amdgpu_validate_mx_formats", "MX element formats whose every step compared clean (of 5).", ran,
        [](const GpuResult& r) { return r.mx.formats.size(); });
  gauge(p, res, "amdgpu_validate_mx_bad_elements",
        "Elements of the MX block-scaled GEMMs that differ bitwise from the exact answer.", ran,
        [](const GpuResult& r) { return r.mx.bad_elements; });
  gauge(p, res, "amdgpu_validate_mx_fp4_tflops", "TFLOP/s of the dense MXFP4 (e2m1) GEMM.", ran,
        [](const GpuResult& r) { return jnum(r.mx.fp4_tflops); });
  gauge(p, res, "amdgpu_validate_mx_scale_spread",
        "Scale spread W (k-block scale exponents base .. base + W) of the dense e2m1 run.", ran,
        [](const GpuResult& r) { return r.mx.scale_spread; });
  gauge(p, res, "amdgpu_validate_mx_s", "Seconds the MX check took.", ran,
        [](const GpuResult& r) { return jnum(r.mx.seconds); });
}

// one sample per XCD, level and mode: labels of its own, so no gauge()
inline void XcdSweepResult::prometheus(std::ostream& p, const Gpus& res) {
  for (int clock = 0; clock < 2; ++clock) {
    const char* name = clock ? "amdgpu_validate_xcd_clock_ghz" : "amdgpu_validate_xcd_rate";
    p << "# HELP " << name
      << (clock ? " Shader clock of one XCD during a level and mode of the XCD sweep.\n"
                : " Rate of one XCD in the XCD sweep: GB/s read and verified, GMFMA/s at level mfma.\n")
      << "# TYPE " << name << " gauge\n";
    for (auto& r : res)
      for (auto& c : r.xcd.cells)
        for (auto& row : c.sum.rows)
          p << name << "{gpu=\"" << r.device << "\",xcd=\"" << row.xcd << "\",level=\""
            << ntm::xcs::level_name(c.sum.level) << "\",mode=\"" << ntm::xcs::mode_name(c.sum.mode)
            << "\"} " << jnum(clock ? row.clock_ghz : row.rate) << "\n";
  }
}

// the rate per op carries an op label, so no gauge() for it
inline void AtomicsResult::prometheus(std::ostream& p, const Gpus& res) {
  auto ran = [](const GpuResult& r) { return r.atomics.ran; };
  gauge(p, res, "amdgpu_validate_atomics_bad_slots", "Table slots of the atomics check that differ from the reference.",
        ran, [](const GpuResult& r) {
          unsigned long long n = 0;
          for (auto& o : r.atomics.ops) n += o.bad;
          return n;
        });
  p << "# HELP amdgpu_validate_atomics_gops Atomic operations per second of one op, in 1e9.\n"
    << "# TYPE amdgpu_validate_atomics_gops gauge\n";
  for (auto& r : res)
    for (auto& o : r.atomics.ops)
      p << "amdgpu_validate_atomics_gops{gpu=\"" << r.device << "\",op=\"" << ntm::atm::op_name(o.op) << "\"} "
        << jnum(o.gops) << "\n";
  gauge(p, res, "amdgpu_validate_atomics_ticket_bad", "Tickets missing, duplicate or invalid, and counters off.", ran,
        [](const GpuResult& r) { return r.atomics.ticket_bad; });
  gauge(p, res, "amdgpu_validate_atomics_handoff_bad_words", "16-byte words a hand-off's reader found wrong.", ran,
        [](const GpuResult& r) { return r.atomics.handoff_bad_words; });
  gauge(p, res, "amdgpu_validate_atomics_handoff_stale_words", "Of them, words that held last round's pattern.", ran,
        [](const GpuResult& r) { return r.atomics.handoff_stale_words; });
  gauge(p, res, "amdgpu_validate_atomics_handoff_episodes_per_s", "Hand-off episodes per second.", ran,
        [](const GpuResult& r) { return jnum(r.atomics.episodes_per_s); });
  gauge(p, res, "amdgpu_validate_atomics_xcd_pairs_covered", "Ordered writer -> reader XCD pairs a hand-off checked.", ran,
        [](const GpuResult& r) { return r.atomics.xcd_pairs_covered; });
  gauge(p, res, "amdgpu_validate_atomics_seconds", "Seconds the atomics check took.", ran,
        [](const GpuResult& r) { return jnum(r.atomics.seconds); });
}

// both gauges carry a format label, so no gauge() for them
inline void McoreResult::prometheus(std::ostream& p, const Gpus& res) {
  p << "# HELP amdgpu_validate_mcore_bad Result words of the matrix-core check that differ from the exact answer.\n"
    << "# TYPE amdgpu_validate_mcore_bad gauge\n";
  for (auto& r : res)
    for (int f = 0; r.mcore.ran && f < ntm::mc::kFormats; ++f)
      p << "amdgpu_validate_mcore_bad{gpu=\"" << r.device << "\",format=\"" << ntm::mc::format_name(f) << "\"} "
        << r.mcore.bad[f] << "\n";
  p << "# HELP amdgpu_validate_mcore_rate Verified 4096^3 product, 1e12 operations per second (reported only).\n"
    << "# TYPE amdgpu_validate_mcore_rate gauge\n";
  for (auto& r : res)
    for (int f : {ntm::mc::kF64, ntm::mc::kI8})
      if (r.mcore.ran)
        p << "amdgpu_validate_mcore_rate{gpu=\"" << r.device << "\",format=\"" << ntm::mc::format_name(f) << "\"} "
          << jnum(r.mcore.rate(f)) << "\n";
}

inline void MxqResult::prometheus(std::ostream& p, const Gpus& res) {
  p << "# HELP amdgpu_validate_mxq_bad Words of the MX quantise check that differ from the reference kernels.\n"
    << "# TYPE amdgpu_validate_mxq_bad gauge\n";
  for (auto& r : res)
    for (int f = 0; r.mxq.ran && f < ntm::mx::kFormats; ++f)
      p << "amdgpu_validate_mxq_bad{gpu=\"" << r.device << "\",format=\"" << ntm::mx::format_name(f) << "\"} "
        << r.mxq.bad(f) << "\n";
  auto ran = [](const GpuResult& r) { return r.mxq.ran; };
  gauge(p, res, "amdgpu_validate_mxq_quantize_gbps",
        "fp32 to MXFP4 quantise of 8192 x 8192, GB/s of bytes read and written (reported only).", ran,
        [](const GpuResult& r) { return jnum(r.mxq.quantize_gbps); });
  gauge(p, res, "amdgpu_validate_mxq_seconds", "Seconds the MX quantise check took.", ran,
        [](const GpuResult& r) { return jnum(r.mxq.seconds); });
}

inline void WaveResult::prometheus(std::ostream& p, const Gpus& res) {
  p << "# HELP amdgpu_validate_wave_bad Results of the wave data-path check that differ from the reference kernels.\n"
    << "# TYPE amdgpu_validate_wave_bad gauge\n";
  for (auto& r : res) {
    if (!r.wave.ran) continue;
    const unsigned long long bad[ntm::wave::kFamilies] = {r.wave.lane_bad, r.wave.ldstr_bad,
                                                          r.wave.sfu_inconsistent + r.wave.sfu_beyond, r.wave.valu_bad};
    for (int f = 0; f < ntm::wave::kFamilies; ++f)
      p << "amdgpu_validate_wave_bad{gpu=\"" << r.device << "\",family=\"" << ntm::wave::family_name(f) << "\"} " << bad[f]
        << "\n";
  }
  gauge(p, res, "amdgpu_validate_wave_seconds", "Seconds the wave data-path check took.",
        [](const GpuResult& r) { return r.wave.ran; }, [](const GpuResult& r) { return jnum(r.wave.seconds); });
}

inline void AttnResult::prometheus(std::ostream& p, const Gpus& res) {
  auto ran = [](const GpuResult& r) { return r.attn.ran; };
  gauge(p, res, "amdgpu_validate_attn_bad",
        "Results of the fused attention check that differ from the reference kernel or lie beyond the tolerance.", ran,
        [](const GpuResult& r) { return r.attn.exact_bad + r.attn.dense_bad; });
  gauge(p, res, "amdgpu_validate_attn_tflops", "TFLOP/s of the causal 4 x 32 x 4096 x 4096 attention (reported only).", ran,
        [](const GpuResult& r) { return jnum(r.attn.tflops); });
  gauge(p, res, "amdgpu_validate_attn_seconds", "Seconds the fused attention check took.", ran,
        [](const GpuResult& r) { return jnum(r.attn.seconds); });
}

inline void PdaResult::prometheus(std::ostream& p, const Gpus& res) {
  auto ran = [](const GpuResult& r) { return r.pda.ran; };
  gauge(p, res, "amdgpu_validate_pda_bad",
        "Results of the paged-KV decode attention check that differ from the reference kernel or lie beyond the tolerance.",
        ran, [](const GpuResult& r) { return r.pda.exact_bad + r.pda.dense_bad; });
  gauge(p, res, "amdgpu_validate_pda_kv_gbps", "GB/s of K and V read by the 32 x 8192-key paged decode pass (reported only).",
        ran, [](const GpuResult& r) { return jnum(r.pda.kv_gbps); });
  gauge(p, res, "amdgpu_validate_pda_seconds", "Seconds the paged-KV decode attention check took.", ran,
        [](const GpuResult& r) { return jnum(r.pda.seconds); });
}

// node-exporter textfile-collector format (--prom-out) and Pushgateway body
// (--pushgateway); labels carry the device index.
inline std::string prometheus_text(const Report& R) {
  const Opts& o = R.o;
  std::ostringstream p;
  p << "# HELP amdgpu_validate_passed 1 if every validation check passed.\n"
    << "# TYPE amdgpu_validate_passed gauge\n"
    << "amdgpu_validate_passed" << (R.node.empty() ? "" : "{node=" + jstr(R.node) + "}") << " "
    << (R.passed() ? 1 : 0) << "\n"
    << "# TYPE amdgpu_validate_seconds gauge\n"
    << "amdgpu_validate_seconds " << jnum(R.t_end - R.t_start) << "\n";
  gauge(p, R.gpus, "amdgpu_validate_gemm_tflops", nullptr, every_gpu,
        [](const GpuResult& r) { return jnum(r.k1.tflops); });
  if (o.fp8)
    gauge(p, R.gpus, "amdgpu_validate_gemm_fp8_tflops", nullptr, every_gpu,
          [](const GpuResult& r) { return jnum(r.fp8.tflops); });
  gauge(p, R.gpus, "amdgpu_validate_hbm_copy_gbps", nullptr, every_gpu,
        [](const GpuResult& r) { return jnum(r.k2.copy_gbps); });
  gauge(p, R.gpus, "amdgpu_validate_hbm_total_gb", nullptr, every_gpu,
        [](const GpuResult& r) { return jnum(r.total_gb); });
  if (o.hbm_test_gb != 0) HbmTestResult::prometheus(p, R.gpus);
  if (o.cu_sweep) CuSweepResult::prometheus(p, R.gpus);
  if (o.host_link_mib > 0) HostLinkResult::prometheus(p, R.gpus);
  if (o.xcd_sweep) XcdSweepResult::prometheus(p, R.gpus);
  if (o.mx_check) MxResult::prometheus(p, R.gpus);
  if (o.atomics_check) AtomicsResult::prometheus(p, R.gpus);
  if (o.mcore_check) McoreResult::prometheus(p, R.gpus);
  if (o.mxq_check) MxqResult::prometheus(p, R.gpus);
  if (o.wave_check) WaveResult::prometheus(p, R.gpus);
  if (o.attn_check) AttnResult::prometheus(p, R.gpus);
  if (o.pda_check) PdaResult::prometheus(p, R.gpus);
  if (!R.rccl_rows.empty() || !R.xgmi_rows.empty())
    p << "# TYPE amdgpu_validate_allreduce_busbw_gbps gauge\n"
      << "amdgpu_validate_allreduce_busbw_gbps{impl=\"rccl\"} " << jnum(Report::peak_any(R.rccl_rows)) << "\n"
      << "amdgpu_validate_allreduce_busbw_gbps{impl=\"xgmi\"} " << jnum(Report::peak_any(R.xgmi_rows)) << "\n";
  if (R.p2p.n > 0) {
    p << "# HELP amdgpu_validate_xgmi_p2p_gbps Pull bandwidth dst <- src over one xGMI link.\n"
      << "# TYPE amdgpu_validate_xgmi_p2p_gbps gauge\n";
    for (int d = 0; d < R.p2p.n; ++d)
      for (int s2 = 0; s2 < R.p2p.n; ++s2)
        if (std::isfinite(R.p2p.gbps[(size_t)d * R.p2p.n + s2]))
          p << "amdgpu_validate_xgmi_p2p_gbps{dst=\"" << R.devs[d] << "\",src=\"" << R.devs[s2]
            << "\"} " << jnum(R.p2p.gbps[(size_t)d * R.p2p.n + s2]) << "\n";
  }
  return p.str();
}

// ------------------------------------------------------------ the JSON document
inline std::string report_json(const Report& R) {
  const Opts& o = R.o;
  std::string js = "{";
  js += "\"tool\":\"amdgpu-validate\",\"passed\":" + std::string(jbool(R.passed()));
  if (!R.node.empty()) js += ",\"node\":" + jstr(R.node);
  js += ",\"n_gpus\":" + std::to_string(R.gpus.size()) + ",\"gemm_size\":" + std::to_string(o.size);
  js += ",\"gemm_tflops_aggregate\":" + jnum(R.gemm_tflops_aggregate());
  js += ",\"gpus\":[";
  for (size_t i = 0; i < R.gpus.size(); ++i) {
    const auto& r = R.gpus[i];
    js += (i ? "," : "") + std::string("{\"device\":") + std::to_string(r.device) +
          ",\"name\":" + jstr(r.name) + ",\"arch\":" + jstr(r.arch) + ",\"hbm_total_gb\":" + jnum(r.total_gb) +
          r.k1.json() + r.fp8.json() + r.sk.json() + r.k2.json() + r.hbm_test.json() + r.cu_sweep.json() +
          r.host_link.json() + r.mx.json() + r.xcd.json() + r.atomics.json() + r.mcore.json() + r.mxq.json() + r.wave.json() +
          r.attn.json() + r.pda.json() + "}";
  }
  js += "],\"rccl_allreduce\":" + coll_json(R.rccl_rows);
  js += ",\"xgmi_allreduce_bf16\":" + coll_json(R.xgmi_rows);
  js += ",\"xgmi_simulated_ranks\":" + std::to_string(o.xgmi_sim);
  js += ",\"xgmi_nblk\":" + std::to_string(R.xtune.nblk ? R.xtune.nblk : o.xgmi_nblk) +
        ",\"xgmi_one_shot_max_bytes\":" +
        std::to_string(R.xtune.nblk ? (long)R.xtune.one_shot_max : o.xgmi_one_shot_max);
  js += ",\"xgmi_tune\":{\"ran\":" + std::string(jbool(R.xtune.ran)) +
        ",\"seconds\":" + jnum(R.xtune.seconds) + ",\"table\":" + R.xtune.table + "}";
  js += ",\"rccl_peak_busbw_bf16_GBps\":" + jnum(peak_busbw(R.rccl_rows)) +
        ",\"xgmi_peak_busbw_bf16_GBps\":" + jnum(peak_busbw(R.xgmi_rows));
  js += ",\"host_prep\":{\"numa_balancing\":" + std::to_string(R.hp.numa_balancing) +
        ",\"memlock_unlimited\":" + jbool(R.hp.memlock_unlimited) +
        ",\"iommu_pt\":" + jbool(R.hp.iommu_pt) + "}";
  js += ",\"xgmi_p2p_GBps\":" + R.p2p.json() + ",\"xgmi_p2p_min_GBps\":" +
        (R.p2p.n > 0 ? jnum(R.p2p.min_gbps) : std::string("null")) +
        ",\"xgmi_p2p_bad_pairs\":" + std::to_string(R.p2p.bad_pairs);
  double t_gemm = R.t_hip, t_hbm = R.t_hip;
  for (auto& r : R.gpus) { t_gemm = std::max(t_gemm, r.t_gemm); t_hbm = std::max(t_hbm, r.t_hbm); }
  js += ",\"phases_s\":{\"process_start_to_hip_init\":" + jnum(R.t_hip - R.t_start) +
        ",\"gemm_done\":" + jnum(t_gemm - R.t_start) + ",\"hbm_done\":" + jnum(t_hbm - R.t_start) +
        ",\"rccl_done\":" + jnum(R.t_rccl - R.t_start) + ",\"end\":" + jnum(R.t_end - R.t_start) + "}";
  js += ",\"start_epoch_s\":" + jnum(R.t_start) + ",\"end_epoch_s\":" + jnum(R.t_end);
  js += ",\"failures\":" + jstrs(R.failures);
  if (!o.pushgateway.empty()) js += ",\"pushgateway\":" + jstr(R.push_status);
  return js + "}";
}

// Kubernetes surfaces this as the pod's termination message (truncated at
// 4 KiB): the one-line verdict an operator sees first. Failures are cut to 200
// characters each and no further one starts past 3500 bytes, so the whole stays
// under the cap.
inline std::string termination_message(const Report& R) {
  std::string t = "{\"passed\":" + std::string(jbool(R.passed())) +
                  (R.node.empty() ? std::string() : ",\"node\":" + jstr(R.node)) +
                  ",\"n_gpus\":" + std::to_string(R.gpus.size()) +
                  ",\"gemm_tflops_aggregate\":" + jnum(R.gemm_tflops_aggregate()) +
                  ",\"rccl_peak_busbw_GBps\":" + jnum(Report::peak_any(R.rccl_rows)) +
                  ",\"seconds\":" + jnum(R.t_end - R.t_start);
  if (R.o.xcd_sweep) {  // the lowest min / median of a gated cell over all GPUs
    double worst = 1e300;
    for (auto& r : R.gpus)
      for (auto& c : r.xcd.cells)
        if (c.gated) worst = std::min(worst, c.sum.min_over_median);
    t += ",\"xcd_sweep_min_over_median\":" + (worst < 1e300 ? jnum(worst) : std::string("null"));
  }
  t += ",\"failures\":[";
  for (size_t i = 0; i < R.failures.size() && t.size() < 3500; ++i)
    t += (i ? "," : "") + jstr(R.failures[i].substr(0, 200));
  return t + "]}";
}

}  // namespace ntm::job
