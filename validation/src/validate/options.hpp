// amdgpu-validate: the command line (host-only C++17, no HIP include).
//
// Opts, ONE flag table, parse(), usage() and the range checks. A new flag is a
// field of Opts, a row of kFlags and a line of usage(); a bound on it goes into
// range_ok(). tests/test_validate_options.py runs this header in a stand-alone
// sanitized program and checks flag -> field for every row.
#pragma once

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <variant>

#include "ntm/abi.h"  // NTM_XGMI_MAX_RANKS
#include "ntm/cu_sweep_plan.hpp"
#include "ntm/mx_plan.hpp"

namespace ntm::job {

struct Opts {
  int gpus = 0;  // 0 = all visible
  int size = 8192;
  int iters = 50;
  double tflops_floor = 0;
  double min_hbm_gb = 0;
  double hbm_floor_gbps = 0;
  double hbm_test_gb = 0;       // K4: 0 = off, < 0 = all free HBM minus the headroom
  int hbm_test_passes = 1;
  bool cu_sweep = false;        // K5: off unless asked for
  int cu_sweep_iters = 16;      // rounds per workgroup (profiles/cu_sweep/README.md)
  long host_link_mib = 0;       // K6: 0 = off; MiB of pinned host memory per GPU
  double host_link_floor_gbps = 0;  // per direction, 0 = report only
  bool mx_check = false;        // K7: off unless asked for
  int mx_size = 4096;           // M = N = K of the dense e2m1 run (a multiple of 128)
  double mx_tflops_floor = 0;   // 0 = report only
  bool xcd_sweep = false;       // K8: off unless asked for
  long xcd_sweep_mib = 256;     // MiB per XCD of the hbm level
  bool atomics_check = false;   // K9: env NTM_ATOMICS_CHECK=1 (no flag yet: validate/README.md)
  bool mcore_check = false;     // K10: env NTM_MCORE_CHECK=1 (no flag yet: validate/README.md)
  bool mxq_check = false;       // K11: env NTM_MXQ_CHECK=1 (no flag yet: validate/README.md)
  bool wave_check = false;      // K12: env NTM_WAVE_CHECK=1 (no flag yet: validate/README.md)
  bool attn_check = false;      // K13: env NTM_ATTN_CHECK=1 (no flag yet: validate/README.md)
  bool pda_check = false;       // K14: env NTM_PDA_CHECK=1 (no flag yet: validate/README.md)
  double xcd_ratio = 0;         // fail an XCD below ratio x its card's median; 0 = report only
  long allreduce_max_mib = 8192;  // 8 GiB, capped by free HBM
  bool xgmi = true;
  int xgmi_sim = 0;             // C2 with N simulated ranks on GPU 0 (one-GPU test path)
  int rccl = -1;                // C1: -1 auto (n > 1), 0 off, 1 on (--rccl: at n = 1 too)
  double settle_s = 0.1;        // untimed clock-settle pre-warm before each timed GEMM loop
  bool fp8 = true;              // K1-fp8 check of the e4m3 MX-scaled matrix path
  double fp8_tflops_floor = 0;
  bool p2p = true;              // C3: per-link xGMI pull matrix (n > 1)
  bool p2p_loopback = false;    // C3 code path on one GPU (pair 0 <- 0), for tests
  long p2p_mib = 256;
  double p2p_floor_gbps = 0;
  double rccl_busbw_floor_gbps = 0;  // C1: peak bf16 busbw floor (0 = off; busbw is 0 at n = 1)
  double xgmi_busbw_floor_gbps = 0;  // C2: the same for the hand-written all-reduce
  int xgmi_nblk = 64;                // C2 blocks per rank (bench.py sweeps it at N > 1)
  long xgmi_one_shot_max = 256 << 10;  // C2: messages <= this take the one-shot kernel
  bool xgmi_tune = false;            // C2: mini-sweep nblk x cutoff first, then run the best
  bool require_host_prep = false;    // fail unless numa_balancing = 0 and memlock unlimited
  bool require_iommu_pt = false;     // ... and the kernel booted with iommu=pt
  bool describe_sweep = false;       // print the C1/C2 size lists + busbw factors, no GPU
  bool json = true;
  std::string out;
  std::string termination_log;  // k8s terminationMessagePath (<= 4 KiB summary)
  std::string prom_out;         // Prometheus textfile-collector metrics
  std::string fault;            // fault injection: corrupt_gemm | corrupt_abft | corrupt_hbm | ...
  std::string pushgateway;      // http://host[:port][/prefix] of a Prometheus Pushgateway
};

inline void usage() {
  std::fprintf(stderr,
               "usage: amdgpu-validate [--gpus N] [--size 8192] [--iters 50]\n"
               "       [--tflops-floor TF] [--min-hbm-gb GB] [--hbm-floor-gbps GBps]\n"
               "       [--hbm-test-gb GB] [--hbm-test-passes P]\n"
               "       [--cu-sweep] [--cu-sweep-iters N]\n"
               "       [--host-link-mib MiB] [--host-link-floor-gbps GBps]\n"
               "       [--mx-check] [--mx-size S] [--mx-tflops-floor TF]\n"
               "       [--xcd-sweep] [--xcd-sweep-mib MiB] [--xcd-ratio R]\n"
               "       [--allreduce-max-mib MiB] [--rccl | --no-rccl] [--no-xgmi] [--xgmi-sim N]\n"
               "       [--settle-s S] [--no-fp8] [--fp8-tflops-floor TF]\n"
               "       [--no-p2p] [--p2p-mib MiB] [--p2p-floor-gbps GBps] [--p2p-loopback]\n"
               "       [--rccl-busbw-floor-gbps GBps] [--xgmi-busbw-floor-gbps GBps]\n"
               "       [--xgmi-nblk N] [--xgmi-one-shot-max BYTES] [--xgmi-tune]\n"
               "       [--require-host-prep] [--require-iommu-pt] [--describe-sweep]\n"
               "       [--json] [--out FILE]\n"
               "       [--termination-log FILE] [--prom-out FILE] [--fault-inject KIND]\n"
               "       [--pushgateway http://host:port]\n"
               "fault-inject (also env NTM_FAULT_INJECT): corrupt_gemm | corrupt_abft |\n"
               "       corrupt_fp8 | corrupt_fp8_abft | corrupt_p2p | corrupt_allreduce |\n"
               "       corrupt_hbm | bad_cu | corrupt_host_link | corrupt_mx | slow_xcd | corrupt_xcd | sk_xcc - corrupts the LAST GPU's data (sk_xcc: its stream-K\n"
               "       launch claims a wrong XCD; corrupt_hbm: one bit of the pattern test's\n"
               "       last chunk, needs --hbm-test-gb) to prove detection\n"
               "hbm-test-gb: K4, write / read back / compare an address pattern and a hash\n"
               "       pattern over GB (1e9 bytes) of each GPU's HBM; 0 = off (default), -1 = all\n"
               "       free HBM minus max(2 GiB, 2 %%); hbm-test-passes: repeat it P times\n"
               "cu-sweep: K5, known-answer LDS / VALU / MFMA sub-tests on every CU (4 workgroups\n"
               "       per CU and launch, up to 8 launches until every CU ran one); a failure\n"
               "       names xcd, se, sh, cu and simd; cu-sweep-iters: rounds per workgroup\n"
               "       (default 16). fault-inject bad_cu (needs --cu-sweep): the workgroups on one\n"
               "       CU of the LAST GPU flip one bit of a computed value\n"
               "host-link-mib: K6, the GPU writes a hash pattern into MiB of pinned host memory,\n"
               "       reads it back over the host link (PCIe) and compares on the device; also\n"
               "       both at once, hipMemcpyAsync both ways and the read latency; 0 = off\n"
               "       (default). host-link-floor-gbps: fail when a direction's faster path (kernel or\n"
               "       hipMemcpyAsync) is below GBps (0 = report only). fault-inject corrupt_host_link\n"
               "       (needs --host-link-mib): the host flips one bit of the LAST GPU's pinned buffer\n"
               "mx-check: K7, block-scaled GEMMs on the scaled f8f6f4 matrix instruction with real\n"
               "       E8M0 scales: a decode sweep of e4m3 / e5m2 / e2m3 / e3m2 / e2m1 against the\n"
               "       host's integer table, dense e2m3 (K = 512) and dense e2m1 (mx-size^3,\n"
               "       default 4096, a multiple of 128) against a reference kernel without matrix\n"
               "       cores, every element compared bitwise, then a timed e2m1 loop;\n"
               "       mx-tflops-floor: fail when that loop is below TF (0 = report only).\n"
               "       fault-inject corrupt_mx (needs --mx-check): one bit of one element of the LAST\n"
               "       GPU's dense e2m1 result is flipped before the compare\n"
               "xcd-sweep: K8, every XCD reads its own slice of a hash-pattern buffer through a work\n"
               "       queue of its own, compares every word and is timed against its own stamps:\n"
               "       alone and all together, at 1 MiB (l2), 16 MiB (mall) and xcd-sweep-mib (hbm,\n"
               "       default 256) per XCD, plus a bf16 MFMA clock probe. Wrong data, a lost tile or\n"
               "       a missing CU fail; xcd-ratio R (0 <= R < 1, default 0 = report only) also fails\n"
               "       an XCD whose rate is below R x the median of its card's XCDs (mall / together\n"
               "       and hbm / together are reported, not judged). fault-inject\n"
               "       slow_xcd / corrupt_xcd (need --xcd-sweep): XCD 5 of the LAST GPU (XCD 0 on a\n"
               "       partitioned device) runs at a quarter of its rate / one bit of XCD 3's hbm\n"
               "       slice is flipped after the fill\n");
}

// What a flag does with its destination: kTrue / kFalse set a bool, kConst stores
// `constant` into an int; the others take the next argument as their value.
enum class Kind { kTrue, kFalse, kConst, kInt, kLong, kDouble, kString };

struct Flag {
  const char* name;
  Kind kind;
  std::variant<bool Opts::*, int Opts::*, long Opts::*, double Opts::*, std::string Opts::*> dest;
  int constant = 0;
};

inline const Flag kFlags[] = {
    {"--gpus", Kind::kInt, &Opts::gpus},
    {"--size", Kind::kInt, &Opts::size},
    {"--iters", Kind::kInt, &Opts::iters},
    {"--tflops-floor", Kind::kDouble, &Opts::tflops_floor},
    {"--min-hbm-gb", Kind::kDouble, &Opts::min_hbm_gb},
    {"--hbm-floor-gbps", Kind::kDouble, &Opts::hbm_floor_gbps},
    {"--hbm-test-gb", Kind::kDouble, &Opts::hbm_test_gb},
    {"--hbm-test-passes", Kind::kInt, &Opts::hbm_test_passes},
    {"--cu-sweep", Kind::kTrue, &Opts::cu_sweep},
    {"--cu-sweep-iters", Kind::kInt, &Opts::cu_sweep_iters},
    {"--host-link-mib", Kind::kLong, &Opts::host_link_mib},
    {"--host-link-floor-gbps", Kind::kDouble, &Opts::host_link_floor_gbps},
    {"--mx-check", Kind::kTrue, &Opts::mx_check},
    {"--mx-size", Kind::kInt, &Opts::mx_size},
    {"--mx-tflops-floor", Kind::kDouble, &Opts::mx_tflops_floor},
    {"--xcd-sweep", Kind::kTrue, &Opts::xcd_sweep},
    {"--xcd-sweep-mib", Kind::kLong, &Opts::xcd_sweep_mib},
    {"--xcd-ratio", Kind::kDouble, &Opts::xcd_ratio},
    {"--allreduce-max-mib", Kind::kLong, &Opts::allreduce_max_mib},
    {"--rccl", Kind::kConst, &Opts::rccl, 1},
    {"--no-rccl", Kind::kConst, &Opts::rccl, 0},
    {"--no-xgmi", Kind::kFalse, &Opts::xgmi},
    {"--xgmi-sim", Kind::kInt, &Opts::xgmi_sim},
    {"--settle-s", Kind::kDouble, &Opts::settle_s},
    {"--no-fp8", Kind::kFalse, &Opts::fp8},
    {"--fp8-tflops-floor", Kind::kDouble, &Opts::fp8_tflops_floor},
    {"--no-p2p", Kind::kFalse, &Opts::p2p},
    {"--p2p-mib", Kind::kLong, &Opts::p2p_mib},
    {"--p2p-floor-gbps", Kind::kDouble, &Opts::p2p_floor_gbps},
    {"--p2p-loopback", Kind::kTrue, &Opts::p2p_loopback},
    {"--rccl-busbw-floor-gbps", Kind::kDouble, &Opts::rccl_busbw_floor_gbps},
    {"--xgmi-busbw-floor-gbps", Kind::kDouble, &Opts::xgmi_busbw_floor_gbps},
    {"--xgmi-nblk", Kind::kInt, &Opts::xgmi_nblk},
    {"--xgmi-one-shot-max", Kind::kLong, &Opts::xgmi_one_shot_max},
    {"--xgmi-tune", Kind::kTrue, &Opts::xgmi_tune},
    {"--require-host-prep", Kind::kTrue, &Opts::require_host_prep},
    {"--require-iommu-pt", Kind::kTrue, &Opts::require_iommu_pt},
    {"--describe-sweep", Kind::kTrue, &Opts::describe_sweep},
    {"--json", Kind::kTrue, &Opts::json},  // the only output format: accepted, changes nothing
    {"--out", Kind::kString, &Opts::out},
    {"--termination-log", Kind::kString, &Opts::termination_log},
    {"--prom-out", Kind::kString, &Opts::prom_out},
    {"--fault-inject", Kind::kString, &Opts::fault},
    {"--pushgateway", Kind::kString, &Opts::pushgateway},
};

// the bounds every run must meet; parse() fails (exit status 2 after usage()) outside them
inline bool range_ok(const Opts& o) {
  return o.size > 0 && o.iters > 0 && o.p2p_mib > 0 && o.allreduce_max_mib > 0 &&
         o.xgmi_sim >= 0 && o.xgmi_sim <= NTM_XGMI_MAX_RANKS && o.settle_s >= 0 &&
         o.hbm_test_passes >= 1 && std::isfinite(o.hbm_test_gb) && o.cu_sweep_iters >= 1 &&
         o.cu_sweep_iters <= ntm::cus::kMaxIters && o.host_link_mib >= 0 &&
         o.host_link_mib <= (1l << 20) && o.host_link_floor_gbps >= 0 &&
         ntm::mx::shape_ok(o.mx_size, o.mx_size, o.mx_size) && o.mx_size <= 16384 &&
         o.mx_tflops_floor >= 0 && o.xcd_sweep_mib >= 1 && o.xcd_sweep_mib <= 4096 &&
         o.xcd_ratio >= 0 && o.xcd_ratio < 1;
}

// the C2 knobs have a message of their own (no usage text), also exit status 2
inline bool xgmi_knobs_ok(const Opts& o) {
  if (o.xgmi_nblk >= 1 && o.xgmi_nblk <= 1024 && o.xgmi_one_shot_max >= 0) return true;
  std::fprintf(stderr, "--xgmi-nblk must be in 1..1024, --xgmi-one-shot-max >= 0\n");
  return false;
}

inline bool parse(int argc, char** argv, Opts& o) {
  for (int i = 1; i < argc; ++i) {
    const char* a = argv[i];
    if (!std::strcmp(a, "-h") || !std::strcmp(a, "--help")) {
      usage();
      std::exit(0);
    }
    const Flag* f = nullptr;
    for (const Flag& k : kFlags)
      if (!std::strcmp(a, k.name)) f = &k;
    if (!f) {
      std::fprintf(stderr, "unknown argument %s\n", a);
      return false;
    }
    const char* v = nullptr;
    if (f->kind >= Kind::kInt) {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "missing value for %s\n", a);
        return false;
      }
      v = argv[++i];
    }
    switch (f->kind) {
      case Kind::kTrue: o.*std::get<bool Opts::*>(f->dest) = true; break;
      case Kind::kFalse: o.*std::get<bool Opts::*>(f->dest) = false; break;
      case Kind::kConst: o.*std::get<int Opts::*>(f->dest) = f->constant; break;
      case Kind::kInt: o.*std::get<int Opts::*>(f->dest) = std::atoi(v); break;
      case Kind::kLong: o.*std::get<long Opts::*>(f->dest) = std::atol(v); break;
      case Kind::kDouble: o.*std::get<double Opts::*>(f->dest) = std::atof(v); break;
      case Kind::kString: o.*std::get<std::string Opts::*>(f->dest) = v; break;
    }
  }
  return range_ok(o);
}

}  // namespace ntm::job
