// amdgpu-validate: the post-provision validation Job entrypoint.
//
// Runs on the MI355X GPUs granted to the Kubernetes Job (amd.com/gpu: N) and
// proves them usable, replacing the NVIDIA GPU Operator's CUDA validator
// (reference: helm_release.gpu_operator, /root/reference/eks/main.tf:185-203):
//
//   K1  hand-written bf16 MFMA GEMM per GPU (TFLOP/s + full verification
//       against an independent fp32 reference kernel)
//   K2  HBM stream copy bandwidth + capacity check (288 GB class)
//   K4  HBM pattern test over (up to) all free HBM, off by default
//       (--hbm-test-gb; ntm/hbm_pattern.hpp)
//   K5  per-CU compute sweep that names a bad CU, off by default
//       (--cu-sweep; ntm/cu_sweep.hpp)
//   K6  host-link (PCIe) check: verified transfers both ways through pinned
//       host memory, rate and read latency, off by default
//       (--host-link-mib; ntm/host_link.hpp)
//   K7  MX block-scaled matrix check: MXFP8 / MXFP6 / MXFP4 GEMMs with real
//       E8M0 scales, every element compared bitwise, off by default
//       (--mx-check; ntm/mx_gemm.hpp)
//   K8  per-XCD sweep that names a slow or wrong XCD, off by default
//       (--xcd-sweep; ntm/xcd_sweep.hpp)
//   C1  RCCL all-reduce sweep over xGMI (ncclCommInitAll, one process owns
//       all GPUs; every element checked)
//   C2  hand-written two-shot all-reduce over peer-mapped xGMI, vs RCCL
//
// One process, one host thread per GPU for K1/K2; no Python, no PyTorch - the
// container is small and starts fast (time-to-GPU-ready). Prints ONE JSON
// document; exit 0 = all checks passed, 1 = a check failed, 2 = environment
// error (no GPUs, not gfx950, HIP/RCCL error).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <netdb.h>
#include <sys/resource.h>
#include <sys/socket.h>
#include <unistd.h>

#include "ntm/common.hpp"
#include "ntm/cu_sweep_plan.hpp"
#include "ntm/hbm_test_plan.hpp"
#include "ntm/host_link_plan.hpp"
#include "ntm/mx_plan.hpp"
#include "ntm/xcd_sweep_plan.hpp"

namespace ntm {
namespace xgmi {
constexpr int kMaxRanks = 8;  // = ntm/xgmi_allreduce.hpp (kernels live in its .hip)
}
}  // namespace ntm

// C ABI of ntm_validation.hip / xgmi_allreduce.hip (linked into this binary)
extern "C" {
int ntm_gemm_bf16(const void*, const void*, void*, int, int, int, int, int, int, void*);
int ntm_gemm_shape_ok(int, int, int);
int ntm_gemm_fp8(const void*, const void*, void*, int, int, int, int, int, int, void*);
int ntm_gemm_fp8_shape_ok(int, int, int);
int ntm_fill_uniform_e4m3(void*, size_t, unsigned long long, float, void*);
int ntm_ref_gemm_f32_e4m3(const void*, const void*, float*, int, int, int, int, int, int, void*);
int ntm_fill_uniform_bf16(void*, size_t, unsigned long long, float, void*);
int ntm_ref_gemm_f32(const void*, const void*, float*, int, int, int, int, int, int, void*);
int ntm_verify_bf16(const void*, const float*, size_t, float, float, void*, void*);
int ntm_verify_result_bytes();
int ntm_stream_copy(const void*, void*, size_t, void*);
int ntm_stream_read(const void*, size_t, float*, void*);
int ntm_gemm_bf16_rowsum(const void*, const void*, void*, float*, int, int, int, int, int, int,
                         void*);
int ntm_abft_check(const void*, const void*, const void*, const float*, int, int, int, int, int,
                   int, double*, void*, void*);
int ntm_abft_result_bytes();
int ntm_gemm_fp8_rowsum(const void*, const void*, void*, float*, int, int, int, int, int, int,
                        void*);
int ntm_abft_check_fp8(const void*, const void*, const void*, const float*, int, int, int, int,
                       int, int, double*, void*, void*);
int ntm_xgmi_allreduce_bf16(const void* const*, void* const*, unsigned* const*, int, int,
                            int, int, size_t, unsigned, unsigned*, int, void*);
size_t ntm_xgmi_signal_bytes(int);
int ntm_k1_plan_splitk(int, int, int, int*, int*, int*, int*);
size_t ntm_skh_ws_bytes(int, int, int, int);
int ntm_gemm_bf16_skh_ex(int, const void*, const void*, void*, int, int, int, int, int, int, void*,
                         size_t, int, void*);
int ntm_sk_error_word_index();
int ntm_hbm_pattern_write(void*, size_t, unsigned long long, int, unsigned long long, int, void*);
int ntm_hbm_pattern_verify(void*, size_t, unsigned long long, int, unsigned long long, int, int,
                           void*, void*);
int ntm_hbm_pattern_result_bytes();
int ntm_cu_sweep_launch(void*, const void*, unsigned, int, size_t, unsigned, unsigned, int, void*);
int ntm_cu_sweep_max_lds_bytes(int);
int ntm_host_link_push(void*, size_t, unsigned long long, int, unsigned long long, int, int, void*);
int ntm_host_link_pull(const void*, size_t, unsigned long long, int, unsigned long long, int, void*,
                       int, void*, void*);
int ntm_host_link_chase(const void*, unsigned long long, unsigned long long, unsigned, void*, void*);
int ntm_host_link_clock_khz(int);
int ntm_mx_gemm(int, const void*, const void*, const void*, const void*, void*, int, int, int, void*);
int ntm_mx_reference(int, const void*, const void*, const void*, const void*, void*, int, int, int,
                     void*);
int ntm_mx_compare(const void*, const void*, size_t, void*, void*);
int ntm_xcd_sweep_read_launch(const void*, size_t, unsigned, unsigned, unsigned, int, unsigned long long,
                              unsigned, int, unsigned, void*, void*, void*);
int ntm_xcd_sweep_mfma_launch(unsigned, unsigned, unsigned, unsigned, unsigned, int, unsigned, void*,
                              float*, void*);
}

namespace {

using Clock = std::chrono::steady_clock;

double wall_now() {
  return std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch())
      .count();
}

double process_start_epoch() {
  std::ifstream st("/proc/self/stat"), up("/proc/uptime");
  std::string s((std::istreambuf_iterator<char>(st)), std::istreambuf_iterator<char>());
  double uptime = 0;
  up >> uptime;
  const size_t rp = s.rfind(')');
  if (rp == std::string::npos || uptime <= 0) return wall_now();
  std::istringstream rest(s.substr(rp + 2));
  std::string tok;
  long long start_ticks = 0;
  for (int i = 0; i < 20 && rest >> tok; ++i)
    if (i == 19) start_ticks = std::atoll(tok.c_str());
  const long hz = sysconf(_SC_CLK_TCK);
  return wall_now() - uptime + (double)start_ticks / (double)hz;
}

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

void usage() {
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

bool parse(int argc, char** argv, Opts& o) {
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    auto next = [&](const char* name) -> const char* {
      if (i + 1 >= argc) {
        std::fprintf(stderr, "missing value for %s\n", name);
        return nullptr;
      }
      return argv[++i];
    };
    const char* v = nullptr;
    if (a == "--gpus") { if (!(v = next("--gpus"))) return false; o.gpus = std::atoi(v); }
    else if (a == "--size") { if (!(v = next("--size"))) return false; o.size = std::atoi(v); }
    else if (a == "--iters") { if (!(v = next("--iters"))) return false; o.iters = std::atoi(v); }
    else if (a == "--tflops-floor") { if (!(v = next(a.c_str()))) return false; o.tflops_floor = std::atof(v); }
    else if (a == "--min-hbm-gb") { if (!(v = next(a.c_str()))) return false; o.min_hbm_gb = std::atof(v); }
    else if (a == "--hbm-floor-gbps") { if (!(v = next(a.c_str()))) return false; o.hbm_floor_gbps = std::atof(v); }
    else if (a == "--hbm-test-gb") { if (!(v = next(a.c_str()))) return false; o.hbm_test_gb = std::atof(v); }
    else if (a == "--cu-sweep") o.cu_sweep = true;
    else if (a == "--cu-sweep-iters") { if (!(v = next(a.c_str()))) return false; o.cu_sweep_iters = std::atoi(v); }
    else if (a == "--host-link-mib") { if (!(v = next(a.c_str()))) return false; o.host_link_mib = std::atol(v); }
    else if (a == "--mx-check") o.mx_check = true;
    else if (a == "--mx-size") { if (!(v = next(a.c_str()))) return false; o.mx_size = std::atoi(v); }
    else if (a == "--mx-tflops-floor") { if (!(v = next(a.c_str()))) return false; o.mx_tflops_floor = std::atof(v); }
    else if (a == "--xcd-sweep") o.xcd_sweep = true;
    else if (a == "--xcd-sweep-mib") { if (!(v = next(a.c_str()))) return false; o.xcd_sweep_mib = std::atol(v); }
    else if (a == "--xcd-ratio") { if (!(v = next(a.c_str()))) return false; o.xcd_ratio = std::atof(v); }
    else if (a == "--host-link-floor-gbps") { if (!(v = next(a.c_str()))) return false; o.host_link_floor_gbps = std::atof(v); }
    else if (a == "--hbm-test-passes") { if (!(v = next(a.c_str()))) return false; o.hbm_test_passes = std::atoi(v); }
    else if (a == "--allreduce-max-mib") { if (!(v = next(a.c_str()))) return false; o.allreduce_max_mib = std::atol(v); }
    else if (a == "--no-xgmi") o.xgmi = false;
    else if (a == "--no-rccl") o.rccl = 0;
    else if (a == "--rccl") o.rccl = 1;
    else if (a == "--xgmi-sim") { if (!(v = next(a.c_str()))) return false; o.xgmi_sim = std::atoi(v); }
    else if (a == "--settle-s") { if (!(v = next(a.c_str()))) return false; o.settle_s = std::atof(v); }
    else if (a == "--no-fp8") o.fp8 = false;
    else if (a == "--no-p2p") o.p2p = false;
    else if (a == "--p2p-loopback") o.p2p_loopback = true;
    else if (a == "--p2p-mib") { if (!(v = next(a.c_str()))) return false; o.p2p_mib = std::atol(v); }
    else if (a == "--p2p-floor-gbps") { if (!(v = next(a.c_str()))) return false; o.p2p_floor_gbps = std::atof(v); }
    else if (a == "--rccl-busbw-floor-gbps") { if (!(v = next(a.c_str()))) return false; o.rccl_busbw_floor_gbps = std::atof(v); }
    else if (a == "--xgmi-busbw-floor-gbps") { if (!(v = next(a.c_str()))) return false; o.xgmi_busbw_floor_gbps = std::atof(v); }
    else if (a == "--xgmi-nblk") { if (!(v = next(a.c_str()))) return false; o.xgmi_nblk = std::atoi(v); }
    else if (a == "--xgmi-one-shot-max") { if (!(v = next(a.c_str()))) return false; o.xgmi_one_shot_max = std::atol(v); }
    else if (a == "--xgmi-tune") o.xgmi_tune = true;
    else if (a == "--require-host-prep") o.require_host_prep = true;
    else if (a == "--require-iommu-pt") o.require_iommu_pt = true;
    else if (a == "--describe-sweep") o.describe_sweep = true;
    else if (a == "--fp8-tflops-floor") { if (!(v = next(a.c_str()))) return false; o.fp8_tflops_floor = std::atof(v); }
    else if (a == "--json") o.json = true;
    else if (a == "--out") { if (!(v = next("--out"))) return false; o.out = v; }
    else if (a == "--termination-log") { if (!(v = next(a.c_str()))) return false; o.termination_log = v; }
    else if (a == "--prom-out") { if (!(v = next(a.c_str()))) return false; o.prom_out = v; }
    else if (a == "--fault-inject") { if (!(v = next(a.c_str()))) return false; o.fault = v; }
    else if (a == "--pushgateway") { if (!(v = next(a.c_str()))) return false; o.pushgateway = v; }
    else if (a == "-h" || a == "--help") { usage(); std::exit(0); }
    else { std::fprintf(stderr, "unknown argument %s\n", a.c_str()); return false; }
  }
  return o.size > 0 && o.iters > 0 && o.p2p_mib > 0 && o.allreduce_max_mib > 0 &&
         o.xgmi_sim >= 0 && o.xgmi_sim <= ntm::xgmi::kMaxRanks && o.settle_s >= 0 &&
         o.hbm_test_passes >= 1 && std::isfinite(o.hbm_test_gb) && o.cu_sweep_iters >= 1 &&
         o.cu_sweep_iters <= ntm::cus::kMaxIters && o.host_link_mib >= 0 &&
         o.host_link_mib <= (1l << 20) && o.host_link_floor_gbps >= 0 &&
         ntm::mx::shape_ok(o.mx_size, o.mx_size, o.mx_size) && o.mx_size <= 16384 &&
         o.mx_tflops_floor >= 0 && o.xcd_sweep_mib >= 1 && o.xcd_sweep_mib <= 4096 &&
         o.xcd_ratio >= 0 && o.xcd_ratio < 1;
}

// ------------------------------------------------------------ JSON helpers
std::string jnum(double v) {
  if (!std::isfinite(v)) return "null";
  char b[64];
  std::snprintf(b, sizeof b, "%.15g", v);
  return b;
}
std::string jstr(const std::string& s) {
  std::string o = "\"";
  for (char c : s) {
    if (c == '"' || c == '\\') o += '\\';
    if ((unsigned char)c < 0x20) continue;
    o += c;
  }
  return o + "\"";
}

std::mutex g_fail_mu;
std::vector<std::string> g_failures;
void fail(const std::string& why) {
  std::lock_guard<std::mutex> l(g_fail_mu);
  g_failures.push_back(why);
}

#define CK(expr)                                                              \
  do {                                                                        \
    hipError_t _e = (hipError_t)(expr);                                       \
    if (_e != hipSuccess) {                                                   \
      fail(std::string("HIP error ") + hipGetErrorString(_e) + " at " #expr); \
      return false;                                                           \
    }                                                                         \
  } while (0)

// ------------------------------------------------- pattern kernels (C1/C2)
// rank r contributes 2^(i%4) * (r+1): every partial sum is exact in bf16 for
// n <= 8 ranks, so the result is checked element by element, exactly.
// (exact in fp32 too). T = uint16_t holds bf16 bits, T = float holds fp32.
template <typename T>
__device__ __forceinline__ T to_elem(float v) {
  if constexpr (sizeof(T) == 2) return ntm::f32_to_bf16_bits(v);
  else return v;
}
template <typename T>
__device__ __forceinline__ float from_elem(T v) {
  if constexpr (sizeof(T) == 2) return ntm::bf16_bits_to_f32(v);
  else return v;
}

template <typename T>
__global__ void fill_pattern(T* x, size_t n, int rank) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    x[i] = to_elem<T>((float)(1u << (i & 3)) * (float)(rank + 1));
}

template <typename T>
__global__ void check_pattern(const T* x, size_t n, int nranks,
                              unsigned long long* bad) {
  unsigned long long b = 0;
  const float s = (float)(nranks * (nranks + 1) / 2);
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n;
       i += (size_t)gridDim.x * blockDim.x)
    b += from_elem<T>(x[i]) != (float)(1u << (i & 3)) * s;
  if (b) atomicAdd(bad, b);
}

// -------------------------------------------------------------- per GPU
// K8: one level and mode of the per-XCD sweep
struct XcdCell {
  ntm::xcs::Summary sum;
  uint32_t passes = 0;       // read: passes over the slice; mfma: batches per wave
  uint64_t min_span_ticks = 0, max_span_ticks = 0;  // over the XCDs that timed something
  bool gated = false;        // the rate rule judges this cell (ntm::xcs::gated)
};

struct GpuResult {
  int device = -1;
  std::string name, arch;
  double total_gb = 0, free_gb = 0;
  double gemm_ms = 0, gemm_tflops = 0;
  unsigned long long gemm_bad = ~0ull;
  float gemm_max_err = NAN;
  unsigned long long abft_bad_acc = ~0ull, abft_bad_store = ~0ull;
  float abft_max_rel_acc = NAN;
  double abft_tflops = 0;
  double fp8_ms = 0, fp8_tflops = 0;
  unsigned long long fp8_bad = ~0ull;  // stays ~0 when --no-fp8
  float fp8_max_err = NAN;
  unsigned long long fp8_abft_bad = ~0ull;  // rows failing the fp8 fused checksum (~0: not run)
  // stream-K split mode self-check (kSkM x kSkN x kSkK on a 192-wide tile)
  int sk_variant = 0;                    // 54 / 55 (0: not served on this device)
  unsigned long long sk_bad = ~0ull;     // elements off the fp32 reference (~0: not run)
  unsigned sk_word = 0;                  // the workspace's XCD-placement error word
  double sk_ms = 0;
  double hbm_copy_gbps = 0, hbm_read_gbps = 0;
  bool hbm_copy_ok = false;
  double t_init = 0, t_gemm = 0, t_hbm = 0;
  // K4 (only with --hbm-test-gb)
  bool hbm_test_ran = false;
  double hbm_test_gb = 0, hbm_test_requested_gb = 0;
  unsigned long long hbm_test_bad_words = 0, hbm_test_bad_bits = 0;
  double hbm_test_write_gbps = 0, hbm_test_verify_gbps = 0, hbm_test_s = 0;
  double hbm_test_alloc_s = 0, hbm_test_free_s = 0;
  std::string hbm_test_steps;    // JSON array of per-step seconds
  std::string hbm_test_failure;  // empty = clean
  // K5 (only with --cu-sweep)
  bool cu_sweep_ran = false;
  ntm::cus::Summary cu_sweep;
  int cu_sweep_lds_bytes = 0;
  double cu_sweep_s = 0;
  std::string cu_sweep_failure;  // empty = clean
  // K6 (only with --host-link-mib)
  bool host_link_ran = false;
  long host_link_mib = 0;
  double host_link_h2d_gbps = 0, host_link_d2h_gbps = 0;            // pull / push kernels
  double host_link_h2d_copy_gbps = 0, host_link_d2h_copy_gbps = 0;  // hipMemcpyAsync
  double host_link_duplex_gbps = 0, host_link_latency_us = 0;
  unsigned long long host_link_bad_words = 0, host_link_bad_bits = 0;
  ntm::hostlink::LinkState host_link_pcie;
  double host_link_s = 0, host_link_pin_s = 0, host_link_xfer_s = 0, host_link_free_s = 0;
  std::vector<std::string> host_link_failures;  // empty = clean
  // K7 (only with --mx-check)
  bool mx_ran = false;
  std::vector<std::string> mx_formats;  // formats whose every step compared clean
  unsigned long long mx_bad_elements = 0;
  double mx_fp4_tflops = 0, mx_s = 0;
  int mx_scale_spread = 0;
  std::vector<std::string> mx_failures;  // empty = clean
  // K8 (only with --xcd-sweep)
  bool xcd_ran = false;
  uint32_t xcd_xcds = 0;
  std::vector<XcdCell> xcd_cells;   // one per level and mode that ran
  std::vector<std::string> xcd_failures;
  double xcd_s = 0;
};

// The split-mode self-check shape: 48 x 5 of 192x256 tiles, half a round on
// 256 CUs, so each tile is cut into K slices combined through the workspace (the
// ragged shape round 5 moved from 0.82-0.89 to 1.03 of hipBLASLt).
constexpr int kSkM = 4152, kSkN = 1096, kSkK = 16056;

bool run_sk_check(int dev, bool last, const Opts& o, hipStream_t s, void* V, GpuResult& r) {
  int top = 0, tv = 0, rest = 0, sp = 0;
  int variant = 0;
  if (ntm_k1_plan_splitk(kSkM, kSkN, kSkK, &top, &tv, &rest, &sp) == 0 &&
      (tv == 54 || tv == 55) && ntm_skh_ws_bytes(tv, kSkM, kSkN, kSkK) > 0)
    variant = tv;  // what the default dispatch runs for this shape
  for (int v : {54, 55})
    if (!variant && ntm_skh_ws_bytes(v, kSkM, kSkN, kSkK) > 0) variant = v;
  if (!variant) return true;  // a partition with other CU counts: not served, not run
  r.sk_variant = variant;
  const size_t ea = (size_t)kSkM * kSkK, eb = (size_t)kSkN * kSkK, ec = (size_t)kSkM * kSkN;
  const size_t wsb = ntm_skh_ws_bytes(variant, kSkM, kSkN, kSkK);
  void *A, *B, *C, *W;
  float* R;
  CK(hipMalloc(&A, ea * 2));
  CK(hipMalloc(&B, eb * 2));
  CK(hipMalloc(&C, ec * 2));
  CK(hipMalloc(&R, ec * 4));
  CK(hipMalloc(&W, wsb));
  CK(hipMemsetAsync(W, 0, wsb, s));  // counters zero on entry (each launch leaves them zero)
  CK(ntm_fill_uniform_bf16(A, ea, 5000 + 2 * dev, 1.0f, s));
  CK(ntm_fill_uniform_bf16(B, eb, 5001 + 2 * dev, 1.0f, s));
  const int fault = (last && o.fault == "sk_xcc") ? 1 : 0;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipEventRecord(e0, s));
  CK(ntm_gemm_bf16_skh_ex(variant, A, B, C, kSkM, kSkN, kSkK, kSkK, kSkK, kSkN, W, wsb, fault, s));
  CK(hipEventRecord(e1, s));
  CK(ntm_ref_gemm_f32(A, B, R, kSkM, kSkN, kSkK, kSkK, kSkK, kSkN, s));
  CK(hipMemsetAsync(V, 0, 64, s));
  const float atol = 1e-3f + 4.0f * std::sqrt((float)kSkK) * std::ldexp(1.0f, -20);
  CK(ntm_verify_bf16(C, R, ec, atol, std::ldexp(1.0f, -7), V, s));
  unsigned char vr[64];
  CK(hipMemcpyAsync(vr, V, ntm_verify_result_bytes(), hipMemcpyDeviceToHost, s));
  CK(hipMemcpyAsync(&r.sk_word, (unsigned*)W + ntm_sk_error_word_index(), 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  std::memcpy(&r.sk_bad, vr, 8);
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  r.sk_ms = ms;
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  CK(hipFree(A));
  CK(hipFree(B));
  CK(hipFree(C));
  CK(hipFree(R));
  CK(hipFree(W));
  return true;
}

// ---- K4: HBM pattern test (ntm/hbm_pattern.hpp, plan in ntm/hbm_test_plan.hpp).
// Allocates the plan's chunks (a failed hipMalloc ends the list), then per pass:
// write ADDR / verify + invert in place / verify inverted / write HASH (seed =
// pass) / verify. Every chunk of a step is enqueued back to back; the one error
// record is read once per step. The first step that finds a bad word ends the test.
bool run_hbm_test(int dev, bool last, const Opts& o, hipStream_t s, GpuResult& r) {
  namespace hb = ntm::hbm;
  const auto t_begin = Clock::now();
  auto since = [](Clock::time_point t0) {
    return std::chrono::duration<double>(Clock::now() - t0).count();
  };
  size_t fre = 0, tot = 0;
  CK(hipMemGetInfo(&fre, &tot));
  const hb::TestPlan plan = hb::make_test_plan(fre, o.hbm_test_gb);
  r.hbm_test_ran = true;
  r.hbm_test_requested_gb = plan.requested_bytes / 1e9;
  struct Chunk { void* p; size_t bytes; unsigned long long base; };
  std::vector<Chunk> chunks;
  unsigned long long tested = 0;
  for (uint64_t c : plan.chunks) {
    void* p = nullptr;
    if (hipMalloc(&p, c) != hipSuccess) {
      (void)hipGetLastError();  // out of memory here shortens the test, it is no HIP failure
      break;
    }
    chunks.push_back({p, (size_t)c, tested});
    tested += c;
  }
  r.hbm_test_alloc_s = since(t_begin);
  r.hbm_test_gb = tested / 1e9;
  if (chunks.empty()) {
    if (!plan.chunks.empty()) r.hbm_test_failure = "gpu" + std::to_string(dev) + ": HBM pattern test: no chunk of " + std::to_string(plan.chunks[0]) + " bytes could be allocated";
    else r.hbm_test_failure = "gpu" + std::to_string(dev) + ": HBM pattern test: no free HBM beyond the headroom";
    r.hbm_test_s = since(t_begin);
    return true;
  }
  hb::PatternResult* dres;
  CK(hipMalloc(&dres, sizeof(hb::PatternResult)));
  hb::PatternResult hres, init;
  hb::pattern_result_init(init);
  double t_write = 0, t_verify = 0;
  unsigned long long b_write = 0, b_verify = 0;
  std::string steps = "[";
  bool injected = false;
  // one step: kind 0 = write, 1 = verify, 2 = verify + invert in place
  auto step = [&](const char* name, int kind, int pattern, unsigned long long seed, int invert) -> bool {
    const auto t0 = Clock::now();
    if (kind) CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s));
    for (auto& c : chunks) {
      if (kind == 0) CK(ntm_hbm_pattern_write(c.p, c.bytes, c.base, pattern, seed, invert, s));
      else CK(ntm_hbm_pattern_verify(c.p, c.bytes, c.base, pattern, seed, invert, kind == 2, dres, s));
    }
    if (kind) CK(hipMemcpyAsync(&hres, dres, sizeof hres, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    const double dt = since(t0);
    steps += std::string(steps.size() > 1 ? "," : "") + "{\"step\":" + jstr(name) + ",\"s\":" + jnum(dt) + "}";
    if (kind == 0) { t_write += dt; b_write += tested; }
    if (kind == 1) { t_verify += dt; b_verify += tested; }
    if (kind && hres.bad_words) {
      r.hbm_test_bad_words = hres.bad_words;
      r.hbm_test_bad_bits = hres.bad_bits_or;
      r.hbm_test_failure = hb::failure_message(dev, name, hres);
    }
    return true;
  };
  for (int pass = 0; pass < o.hbm_test_passes && r.hbm_test_failure.empty(); ++pass) {
    if (!step("addr write", 0, hb::kPatternAddr, 0, 0)) return false;
    if (last && o.fault == "corrupt_hbm" && !injected) {  // flip one bit in the last chunk
      injected = true;
      const Chunk& c = chunks.back();
      uint32_t* w = (uint32_t*)((char*)c.p + ((c.bytes / 2) & ~(size_t)15) + 4);
      uint32_t h;
      CK(hipMemcpy(&h, w, 4, hipMemcpyDeviceToHost));
      h ^= 1u << 13;
      CK(hipMemcpy(w, &h, 4, hipMemcpyHostToDevice));
    }
    if (!step("addr verify+invert", 2, hb::kPatternAddr, 0, 0)) return false;
    if (!r.hbm_test_failure.empty()) break;
    if (!step("addr inverted verify", 1, hb::kPatternAddr, 0, 1)) return false;
    if (!r.hbm_test_failure.empty()) break;
    if (!step("hash write", 0, hb::kPatternHash, (unsigned long long)pass, 0)) return false;
    if (!step("hash verify", 1, hb::kPatternHash, (unsigned long long)pass, 0)) return false;
  }
  r.hbm_test_steps = steps + "]";
  if (t_write > 0) r.hbm_test_write_gbps = b_write / t_write / 1e9;
  if (t_verify > 0) r.hbm_test_verify_gbps = b_verify / t_verify / 1e9;
  const auto t_free = Clock::now();
  CK(hipFree(dres));
  for (auto& c : chunks) CK(hipFree(c.p));
  r.hbm_test_free_s = since(t_free);
  r.hbm_test_s = since(t_begin);
  return true;
}

// ---- K5: per-CU compute sweep (ntm/cu_sweep.hpp, host side in ntm/cu_sweep_plan.hpp).
// Launches of 4 workgroups per CU until every CU ran one, at most kMaxLaunches: a CU
// that never ran fails the check. bad_cu: a clean launch learns the CU keys, then the
// sweep runs with the middle key of the sorted list as the CU that flips a bit.
bool run_cu_sweep(int dev, bool last, const Opts& o, hipStream_t s, GpuResult& r) {
  namespace cu = ntm::cus;
  const auto t_begin = Clock::now();
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  const uint32_t cus = (uint32_t)prop.multiProcessorCount;
  const unsigned grid = cu::kGridPerCu * cus;
  const int lds = ntm_cu_sweep_max_lds_bytes(dev);
  r.cu_sweep_ran = true;
  r.cu_sweep_lds_bytes = lds;
  if (lds < 16 || cus == 0) {
    r.cu_sweep_failure = "gpu" + std::to_string(dev) + ": CU sweep: cannot read the device's LDS size or CU count";
    return true;
  }
  const int iters = o.cu_sweep_iters;
  std::vector<uint32_t> table(cu::expected_bytes(iters) / 4);
  void *dexp = nullptr, *drec = nullptr;
  CK(hipMalloc(&dexp, table.size() * 4));
  CK(hipMalloc(&drec, (size_t)grid * sizeof(cu::Record)));
  uint32_t fault_key = cu::kFaultOff;
  bool hip_ok = true;
  auto launch = [&](int l, std::vector<cu::Record>& recs) -> bool {
    // a new seed per launch: new tables, so repeated launches do not repeat the data
    cu::make_expected(table.data(), iters, (uint32_t)l);
    recs.resize(grid);
    hip_ok = hipMemcpyAsync(dexp, table.data(), table.size() * 4, hipMemcpyHostToDevice, s) == hipSuccess &&
             ntm_cu_sweep_launch(drec, dexp, grid, iters, (size_t)lds, (unsigned)l, fault_key,
                                 cu::kSubBf16, s) == 0 &&
             hipMemcpyAsync(recs.data(), drec, recs.size() * sizeof(cu::Record), hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
    return hip_ok;
  };
  if (last && o.fault == "bad_cu") {
    cu::Sweep probe;
    std::vector<cu::Record> recs;
    if (launch(0, recs)) {
      probe.add(recs.data(), recs.size());
      const std::vector<uint32_t> keys = probe.keys();  // sorted
      if (!keys.empty()) fault_key = keys[keys.size() / 2];
    }
  }
  cu::Sweep sweep;
  if (hip_ok) cu::coverage_loop(cus, cu::kMaxLaunches, launch, sweep);
  if (!hip_ok) {
    fail("gpu" + std::to_string(dev) + ": CU sweep: HIP error " + hipGetErrorString(hipGetLastError()));
    return false;
  }
  r.cu_sweep = sweep.summary(cus);
  r.cu_sweep_failure = cu::failure_message(dev, r.cu_sweep);
  CK(hipFree(dexp));
  CK(hipFree(drec));
  r.cu_sweep_s = std::chrono::duration<double>(Clock::now() - t_begin).count();
  return true;
}

// ---- K6: host-link (PCIe) check (ntm/host_link.hpp, host side in ntm/host_link_plan.hpp).
// One pinned buffer and one HBM buffer of --host-link-mib: push the HASH pattern
// (device->host), pull and verify on the device (host->device), both at once on
// two streams over the two halves, hipMemcpyAsync both ways on the same buffers
// (the path frameworks use: the reference for the kernels' rate), then the
// pointer chase. Rates are medians of 3, timed with events. The healthy path does
// no CPU work on the data; on a mismatch the host re-checks the pinned buffer to
// say which direction went wrong. corrupt_host_link: the host flips one bit of
// the pinned buffer between push and pull.
bool run_host_link(int dev, bool last, const Opts& o, hipStream_t s, GpuResult& r) {
  namespace hl = ntm::hostlink;
  namespace hb = ntm::hbm;
  const auto t_begin = Clock::now();
  auto since = [](Clock::time_point t0) {
    return std::chrono::duration<double>(Clock::now() - t0).count();
  };
  auto median3 = [](double a, double b, double c) {
    return std::max(std::min(a, b), std::min(std::max(a, b), c));
  };
  const std::string d = "gpu" + std::to_string(dev) + ": ";
  const size_t bytes = (size_t)o.host_link_mib << 20;
  const size_t half = bytes / 2;  // a multiple of 16: bytes is a multiple of 1 MiB
  constexpr int kPat = hb::kPatternHash;
  const unsigned long long seed = 0x4B36ull + (unsigned)dev;
  r.host_link_ran = true;
  r.host_link_mib = o.host_link_mib;
  char bus[32] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof bus, dev) != hipSuccess) {
    (void)hipGetLastError();
    bus[0] = 0;
  }
  void *hbuf = nullptr, *dbuf = nullptr;
  if (hipHostMalloc(&hbuf, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();  // no pinned memory (RLIMIT_MEMLOCK, host RAM): a verdict, no HIP failure
    r.host_link_failures.push_back(d + "host link: cannot pin " + std::to_string(o.host_link_mib) +
                                   " MiB of host memory");
    r.host_link_s = since(t_begin);
    return true;
  }
  r.host_link_pin_s = since(t_begin);
  const auto t_xfer = Clock::now();
  hb::PatternResult *dres = nullptr, hres, init;
  unsigned long long* dchase = nullptr;
  hb::pattern_result_init(init);
  CK(hipMalloc(&dbuf, bytes));
  CK(hipMalloc(&dres, sizeof(hb::PatternResult)));
  CK(hipMalloc(&dchase, 3 * sizeof(unsigned long long)));
  hipStream_t s2;
  hipEvent_t e0, e1;
  CK(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float ms = 0;
  double t[3];
  // device->host; the link state is read while the last push is in flight (AMD GPUs
  // drop the link speed at idle)
  for (int i = 0; i < 3; ++i) {
    CK(hipEventRecord(e0, s));
    CK(ntm_host_link_push(hbuf, bytes, 0, kPat, seed, 0, 0, s));
    CK(hipEventRecord(e1, s));
    if (i == 2 && bus[0]) r.host_link_pcie = hl::read_link_state("/sys", bus);
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    t[i] = ms;
  }
  r.host_link_d2h_gbps = bytes / (median3(t[0], t[1], t[2]) * 1e-3) / 1e9;
  if (last && o.fault == "corrupt_host_link")
    ((uint32_t*)hbuf)[((bytes / 2) & ~(size_t)15) / 4 + 1] ^= 1u << 13;
  // host->device, compared on the device; the first pull that finds a bad word ends the stage
  bool clean = true;
  int pulls = 0;
  for (int i = 0; i < 3 && clean; ++i) {
    CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s));
    CK(hipEventRecord(e0, s));
    CK(ntm_host_link_pull(hbuf, bytes, 0, kPat, seed, 0, nullptr, 0, dres, s));
    CK(hipEventRecord(e1, s));
    CK(hipMemcpyAsync(&hres, dres, sizeof hres, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    CK(hipEventElapsedTime(&ms, e0, e1));
    t[pulls++] = ms;
    if (hres.bad_words) {
      clean = false;
      r.host_link_bad_words = hres.bad_words;
      r.host_link_bad_bits = hres.bad_bits_or;
      // which direction: is the pinned buffer itself wrong?
      hb::PatternResult host_res;
      const bool host_bad = hl::host_check(hbuf, bytes, 0, kPat, seed, false, host_res) != 0;
      r.host_link_failures.push_back(
          hl::data_failure_message(dev, host_bad ? hl::kDirPush : hl::kDirPull, host_bad ? host_res : hres));
    }
  }
  // a stage cut short reports its first pull
  r.host_link_h2d_gbps = bytes / ((pulls == 3 ? median3(t[0], t[1], t[2]) : t[0]) * 1e-3) / 1e9;
  if (clean) {
    // duplex: push into the first half, pull from the second, wall time of both
    CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s2));
    CK(hipStreamSynchronize(s2));
    for (int i = 0; i < 3; ++i) {
      CK(hipStreamSynchronize(s));
      const auto t0 = Clock::now();
      CK(ntm_host_link_push(hbuf, half, 0, kPat, seed, 0, 0, s));
      CK(ntm_host_link_pull((char*)hbuf + half, half, half, kPat, seed, 0, nullptr, 0, dres, s2));
      CK(hipStreamSynchronize(s));
      CK(hipStreamSynchronize(s2));
      t[i] = since(t0) * 1e3;
    }
    r.host_link_duplex_gbps = 2.0 * half / (median3(t[0], t[1], t[2]) * 1e-3) / 1e9;
    CK(hipMemcpy(&hres, dres, sizeof hres, hipMemcpyDeviceToHost));
    if (hres.bad_words) {
      r.host_link_bad_words = hres.bad_words;
      r.host_link_bad_bits = hres.bad_bits_or;
      r.host_link_failures.push_back(hl::data_failure_message(dev, "duplex host->device read", hres));
    }
    // hipMemcpyAsync on the same buffers, both ways
    for (int dir = 0; dir < 2; ++dir) {
      for (int i = 0; i < 3; ++i) {
        CK(hipEventRecord(e0, s));
        if (dir == 0) CK(hipMemcpyAsync(dbuf, hbuf, bytes, hipMemcpyHostToDevice, s));
        else CK(hipMemcpyAsync(hbuf, dbuf, bytes, hipMemcpyDeviceToHost, s));
        CK(hipEventRecord(e1, s));
        CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
        t[i] = ms;
      }
      (dir == 0 ? r.host_link_h2d_copy_gbps : r.host_link_d2h_copy_gbps) =
          bytes / (median3(t[0], t[1], t[2]) * 1e-3) / 1e9;
    }
    // read round trip: 4096 dependent loads through a 1024-slot cycle in host memory
    const size_t chase_bytes = (size_t)hl::kChaseSlots * hl::kChaseSlotBytes;
    const int khz = ntm_host_link_clock_khz(dev);
    if (bytes >= chase_bytes && khz > 0) {
      const std::vector<uint32_t> next = hl::chase_permutation(hl::kChaseSlots, seed);
      hl::chase_fill(hbuf, next);
      unsigned long long out[3] = {0, 0, 0};
      CK(ntm_host_link_chase(hbuf, hl::kChaseSlots, 0, hl::kChaseHops, dchase, s));
      CK(hipMemcpyAsync(out, dchase, sizeof out, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      const uint32_t want = hl::chase_walk(next, 0, hl::kChaseHops);
      if (out[0] != want || out[2] != hl::kChaseHops)
        r.host_link_failures.push_back(d + "host link chase ended at slot " + std::to_string(out[0]) +
                                       " after " + std::to_string(out[2]) + " hops, expected slot " +
                                       std::to_string(want) + " after " + std::to_string(hl::kChaseHops));
      else
        r.host_link_latency_us = (double)out[1] / khz * 1e3 / hl::kChaseHops;
    }
    // the floor: per direction, on the faster of kernel and hipMemcpyAsync (a degraded link caps both)
    if (o.host_link_floor_gbps > 0) {
      const double h2d = std::max(r.host_link_h2d_gbps, r.host_link_h2d_copy_gbps);
      const double d2h = std::max(r.host_link_d2h_gbps, r.host_link_d2h_copy_gbps);
      if (h2d < o.host_link_floor_gbps)
        r.host_link_failures.push_back(
            hl::rate_failure_message(dev, "host->device", h2d, o.host_link_floor_gbps, r.host_link_pcie));
      if (d2h < o.host_link_floor_gbps)
        r.host_link_failures.push_back(
            hl::rate_failure_message(dev, "device->host", d2h, o.host_link_floor_gbps, r.host_link_pcie));
    }
  }
  r.host_link_xfer_s = since(t_xfer);
  const auto t_free = Clock::now();
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  CK(hipStreamDestroy(s2));
  CK(hipFree(dchase));
  CK(hipFree(dres));
  CK(hipFree(dbuf));
  CK(hipHostFree(hbuf));
  r.host_link_free_s = since(t_free);
  r.host_link_s = since(t_begin);
  return true;
}

// ---- K7: MX block-scaled matrix check (ntm/mx_gemm.hpp, host side in ntm/mx_plan.hpp).
// Every answer is exact and every compare bitwise:
//   1. the decode sweep of all five formats, 256 x 128 x 128, one non-zero per row of A,
//      all 15 windows of A scale bytes 0 .. 254, against the host's integer table;
//   2. dense e2m3, mx-size x mx-size x 512, and
//   3. dense e2m1, mx-size^3, both with non-unit scales of the largest spread W <= 3
//      the bound allows, against mx_ref_kernel (no matrix core);
//   4. the e2m1 product timed: the settle of the other GEMM stages, then o.iters launches.
// corrupt_mx: one bit of one element of the dense e2m1 result is flipped before the compare.
bool run_mx_check(int dev, bool last, const Opts& o, hipStream_t s, GpuResult& r) {
  namespace mx = ntm::mx;
  const auto t_begin = Clock::now();
  r.mx_ran = true;
  const int S = o.mx_size;
  mx::Mismatch init, got;
  mx::mismatch_init(init);
  mx::Mismatch* dres = nullptr;
  CK(hipMalloc(&dres, sizeof init));
  bool fmt_clean[mx::kFormats] = {true, true, true, true, true};
  unsigned char *dA = nullptr, *dB = nullptr, *dSA = nullptr, *dSB = nullptr;
  float *dC = nullptr, *dE = nullptr;
  // One product: upload, run the GEMM, get the expected bits (host table or reference
  // kernel), compare on the device. The buffers stay allocated for the timed loop.
  auto product = [&](const mx::Inputs& in, const char* mode, bool host_table, bool inject) -> bool {
    const size_t nc = (size_t)in.M * in.N;
    CK(hipMalloc(&dA, in.a.size()));
    CK(hipMalloc(&dB, in.b.size()));
    CK(hipMalloc(&dSA, in.sa.size()));
    CK(hipMalloc(&dSB, in.sb.size()));
    CK(hipMalloc(&dC, nc * 4));
    CK(hipMalloc(&dE, nc * 4));
    CK(hipMemcpyAsync(dA, in.a.data(), in.a.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dB, in.b.data(), in.b.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dSA, in.sa.data(), in.sa.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dSB, in.sb.data(), in.sb.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(dC, 0xFF, nc * 4, s));
    CK(ntm_mx_gemm(in.fmt, dA, dB, dSA, dSB, dC, in.M, in.N, in.K, s));
    std::vector<uint32_t> bits;
    if (host_table) {
      if (!mx::host_reference(in, bits)) {
        fail("mx host reference: scale spread too wide");
        return false;
      }
      CK(hipMemcpyAsync(dE, bits.data(), nc * 4, hipMemcpyHostToDevice, s));
    } else {
      CK(ntm_mx_reference(in.fmt, dA, dB, dSA, dSB, dE, in.M, in.N, in.K, s));
    }
    if (inject) {
      uint32_t w;
      float* at = dC + (nc / 2 + 5);
      CK(hipMemcpyAsync(&w, at, 4, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      w ^= 1u << 3;
      CK(hipMemcpyAsync(at, &w, 4, hipMemcpyHostToDevice, s));
    }
    CK(ntm_mx_compare(dE, dC, nc, dres, s));
    CK(hipMemcpyAsync(&got, dres, sizeof got, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (got.count) {
      r.mx_bad_elements += got.count;
      fmt_clean[in.fmt] = false;
      // one line per format and mode: the first failing product names the element
      const std::string head = "gpu" + std::to_string(dev) + ": mx " + mx::format_name(in.fmt) + " " + mode + ":";
      bool seen = false;
      for (auto& f : r.mx_failures) seen = seen || f.compare(0, head.size(), head) == 0;
      if (!seen) r.mx_failures.push_back(mx::failure_message(dev, in.fmt, mode, got, in.N));
    }
    return true;
  };
  auto release = [&]() -> bool {
    CK(hipFree(dA));
    CK(hipFree(dB));
    CK(hipFree(dSA));
    CK(hipFree(dSB));
    CK(hipFree(dC));
    CK(hipFree(dE));
    dA = dB = dSA = dSB = nullptr;
    dC = dE = nullptr;
    return true;
  };
  for (int fmt = 0; fmt < mx::kFormats; ++fmt)
    for (int w = 0; w < mx::kDecodeWindows; ++w) {
      if (!product(mx::make_decode(fmt, 256, 128, 128, w), "decode", true, false)) return false;
      if (!release()) return false;
    }
  const unsigned long long seed = 0x4B37ull + (unsigned)dev;
  const int w6 = mx::dense_max_spread(mx::kFmtE2M3, 512);
  if (w6 >= 0) {
    if (!product(mx::make_dense(mx::kFmtE2M3, S, S, 512, seed, w6), "dense", false, false)) return false;
    if (!release()) return false;
  }
  const int w4 = mx::dense_max_spread(mx::kFmtE2M1, S);
  if (w4 < 0) {
    r.mx_failures.push_back("gpu" + std::to_string(dev) + ": mx e2m1 dense: no exact scale spread at size " +
                            std::to_string(S));
    fmt_clean[mx::kFmtE2M1] = false;
  } else {
    r.mx_scale_spread = w4;
    if (!product(mx::make_dense(mx::kFmtE2M1, S, S, S, seed, w4), "dense", false,
                 last && o.fault == "corrupt_mx"))
      return false;
    // timed: the buffers of the dense e2m1 product are still in place
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    const auto t0 = Clock::now();
    do {
      for (int i = 0; i < 8; ++i) CK(ntm_mx_gemm(mx::kFmtE2M1, dA, dB, dSA, dSB, dC, S, S, S, s));
      CK(hipStreamSynchronize(s));
    } while (std::chrono::duration<double>(Clock::now() - t0).count() < o.settle_s);
    CK(hipEventRecord(e0, s));
    for (int i = 0; i < o.iters; ++i) CK(ntm_mx_gemm(mx::kFmtE2M1, dA, dB, dSA, dSB, dC, S, S, S, s));
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    float ms = 0;
    CK(hipEventElapsedTime(&ms, e0, e1));
    r.mx_fp4_tflops = 2.0 * S * (double)S * S / (ms / o.iters * 1e-3) / 1e12;
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    if (!release()) return false;
    if (o.mx_tflops_floor > 0 && r.mx_fp4_tflops < o.mx_tflops_floor)
      r.mx_failures.push_back("gpu" + std::to_string(dev) + ": mx e2m1 GEMM " + jnum(r.mx_fp4_tflops) +
                              " TFLOP/s below floor " + jnum(o.mx_tflops_floor));
  }
  CK(hipFree(dres));
  for (int fmt = 0; fmt < mx::kFormats; ++fmt)
    if (fmt_clean[fmt]) r.mx_formats.push_back(mx::format_name(fmt));
  r.mx_s = std::chrono::duration<double>(Clock::now() - t_begin).count();
  return true;
}

// ---- K8: per-XCD sweep (ntm/xcd_sweep.hpp, host side in ntm/xcd_sweep_plan.hpp).
// One buffer of xcds x xcd-sweep-mib, filled once with K4's hash pattern; the l2 and
// mall levels read its first xcds x 1 MiB / 16 MiB (the pattern depends on the position
// alone). Per level: mode alone (one launch per XCD) and together (one launch). Every
// cell runs once untimed with a first guess of the passes, which warms it up and sizes
// the passes for spans of at least 100 us, then once for the record. slow_xcd and
// corrupt_xcd act on the LAST GPU.
bool run_xcd_sweep(int dev, bool last, const Opts& o, hipStream_t s, GpuResult& r) {
  namespace xs = ntm::xcs;
  const auto t_begin = Clock::now();
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  const uint32_t xcds = std::min<uint32_t>(xs::xcds_expected((uint32_t)prop.multiProcessorCount), xs::kMaxXcds);
  const std::string head = "gpu" + std::to_string(dev) + ": XCD sweep: ";
  r.xcd_ran = true;
  r.xcd_xcds = xcds;
  if (xcds < 1) {
    r.xcd_failures.push_back(head + "the device reports " + std::to_string(prop.multiProcessorCount) +
                             " CUs, fewer than one XCD");
    return true;
  }
  const uint32_t hbm_mib = (uint32_t)o.xcd_sweep_mib;
  const size_t bytes = (size_t)xcds * hbm_mib << 20;
  const uint32_t grid = xs::grid_of(xcds, xs::kWgPerCu), mfma_grid = xs::grid_of(xcds, 1);
  const uint32_t all = xs::full_mask(xcds);
  const unsigned long long seed = 0x4B38ull + (unsigned)dev;
  const int slow_xcd = last && o.fault == "slow_xcd" ? (xcds > 5 ? 5 : 0) : xs::kSlowOff;
  const uint32_t slow_factor = slow_xcd == xs::kSlowOff ? 1 : 4;
  void *buf = nullptr, *heads = nullptr, *drec = nullptr, *sink = nullptr;
  CK(hipMalloc(&buf, bytes));
  CK(hipMalloc(&heads, xs::kHeadsBytes));
  CK(hipMalloc(&drec, (size_t)grid * sizeof(xs::Record)));
  CK(hipMalloc(&sink, 256));
  CK(ntm_hbm_pattern_write(buf, bytes, 0, ntm::hbm::kPatternHash, seed, 0, s));
  CK(hipStreamSynchronize(s));

  bool hip_ok = true;
  std::vector<xs::Record> one;
  // one launch; its records are appended to `recs`
  auto launch = [&](int level, uint32_t mask, uint32_t passes, std::vector<xs::Record>& recs) {
    const bool mfma = level == xs::kLevelMfma;
    const uint32_t g = mfma ? mfma_grid : grid;
    one.resize(g);
    const int rc = mfma ? ntm_xcd_sweep_mfma_launch(g, passes, 7u, xcds, mask, slow_xcd, slow_factor, drec,
                                                    (float*)sink, s)
                        : ntm_xcd_sweep_read_launch(buf, (size_t)xs::level_mib(level, hbm_mib) << 20, xcds,
                                                    mask, passes, ntm::hbm::kPatternHash, seed, g, slow_xcd,
                                                    slow_factor, heads, drec, s);
    hip_ok = hip_ok && rc == 0 &&
             hipMemcpyAsync(one.data(), drec, one.size() * sizeof(xs::Record), hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipStreamSynchronize(s) == hipSuccess;
    if (hip_ok) recs.insert(recs.end(), one.begin(), one.end());
    return hip_ok;
  };
  auto run_cell = [&](int level, int mode, uint32_t passes, double ratio) {
    std::vector<xs::Record> recs;
    if (mode == xs::kModeAlone) {
      for (uint32_t x = 0; x < xcds && hip_ok; ++x) launch(level, 1u << x, passes, recs);
    } else {
      launch(level, all, passes, recs);
    }
    const uint64_t expected =
        level == xs::kLevelMfma ? 0 : xs::expected_tiles((uint64_t)xs::level_mib(level, hbm_mib) << 20, passes);
    XcdCell c;
    c.passes = passes;
    c.sum = xs::summarize(recs.data(), recs.size(), level, mode, xcds, all, expected, ratio, dev);
    c.min_span_ticks = xs::min_timed_span(c.sum);
    for (auto& row : c.sum.rows) c.max_span_ticks = std::max(c.max_span_ticks, row.span_ticks);
    return c;
  };
  for (int level = 0; level < xs::kLevels && hip_ok; ++level) {
    if (level == xs::kLevelHbm && last && o.fault == "corrupt_xcd") {
      // one bit of a word in the middle of XCD 3's hbm slice (the last XCD's on a smaller device)
      const size_t off = ((size_t)std::min<uint32_t>(3, xcds - 1) * hbm_mib << 20) + ((size_t)hbm_mib << 19) + 40;
      uint32_t w = 0;
      CK(hipMemcpy(&w, (char*)buf + off, 4, hipMemcpyDeviceToHost));
      w ^= 1u << 9;
      CK(hipMemcpy((char*)buf + off, &w, 4, hipMemcpyHostToDevice));
    }
    for (int mode = 0; mode < xs::kModes && hip_ok; ++mode) {
      if (level == xs::kLevelMfma && mode == xs::kModeAlone) continue;  // the clock probe loads every XCD at once
      const uint32_t first = level == xs::kLevelL2 ? 64 : level == xs::kLevelMall ? 4 : level == xs::kLevelHbm ? 1 : 16;
      XcdCell c = run_cell(level, mode, first, 0);
      uint32_t passes = first;
      for (int attempt = 0; attempt < 2 && hip_ok; ++attempt) {
        // sized from the XCDs that pulled tiles; one that ran nothing fails on its own
        passes = xs::passes_for_min_span(passes, c.min_span_ticks);
        if (level == xs::kLevelMfma) passes = std::min(passes, xs::kMaxMfmaBatches);
        while (level != xs::kLevelMfma && passes > 1 &&
               !xs::passes_ok((uint64_t)xs::level_mib(level, hbm_mib) << 20, passes))
          passes /= 2;
        c = run_cell(level, mode, passes, xs::gated(level, mode) ? o.xcd_ratio : 0);
        if (c.min_span_ticks == 0 || c.min_span_ticks >= xs::kMinSpanTicks) break;
      }
      c.gated = xs::gated(level, mode);
      if (!hip_ok) break;
      for (auto& f : c.sum.failures) r.xcd_failures.push_back(f);
      r.xcd_cells.push_back(std::move(c));
    }
  }
  if (!hip_ok) {
    fail(head + "HIP error " + hipGetErrorString(hipGetLastError()));
    return false;
  }
  CK(hipFree(buf));
  CK(hipFree(heads));
  CK(hipFree(drec));
  CK(hipFree(sink));
  r.xcd_s = std::chrono::duration<double>(Clock::now() - t_begin).count();
  return true;
}

bool run_gpu(int dev, bool last, const Opts& o, GpuResult& r) {
  r.device = dev;
  CK(hipSetDevice(dev));
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  r.name = prop.name;
  r.arch = prop.gcnArchName;
  if (r.arch.find("gfx950") == std::string::npos) {
    fail("device " + std::to_string(dev) + " is " + r.arch + ", not gfx950 (MI355X)");
    return false;
  }
  size_t fre = 0, tot = 0;
  CK(hipMemGetInfo(&fre, &tot));
  r.total_gb = tot / 1e9;
  r.free_gb = fre / 1e9;
  hipStream_t s;
  CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  r.t_init = wall_now();

  // ---- K1
  const int n = o.size;
  if (!ntm_gemm_shape_ok(n, n, n)) {
    fail("--size must be a multiple of 256 (>= 256)");
    return false;
  }
  const size_t e = (size_t)n * n;
  void *A, *B, *C, *V;
  float* R;
  CK(hipMalloc(&A, e * 2));
  CK(hipMalloc(&B, e * 2));
  CK(hipMalloc(&C, e * 2));
  CK(hipMalloc(&R, e * 4));
  CK(hipMalloc(&V, 64));
  CK(ntm_fill_uniform_bf16(A, e, 1000 + 2 * dev, 1.0f, s));
  CK(ntm_fill_uniform_bf16(B, e, 1001 + 2 * dev, 1.0f, s));
  CK(ntm_gemm_bf16(A, B, C, n, n, n, n, n, n, s));  // warm-up + verified result
  if (last && o.fault == "corrupt_gemm") {  // flip one output element's exponent
    uint16_t h;
    CK(hipMemcpyAsync(&h, (uint16_t*)C + 4321, 2, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    h ^= 0x0100;
    CK(hipMemcpyAsync((uint16_t*)C + 4321, &h, 2, hipMemcpyHostToDevice, s));
  }
  CK(ntm_ref_gemm_f32(A, B, R, n, n, n, n, n, n, s));
  CK(hipMemsetAsync(V, 0, 64, s));
  const float atol = 1e-3f + 4.0f * std::sqrt((float)n) * std::ldexp(1.0f, -20);
  CK(ntm_verify_bf16(C, R, e, atol, std::ldexp(1.0f, -7), V, s));
  unsigned char vr[64];
  CK(hipMemcpyAsync(vr, V, ntm_verify_result_bytes(), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  std::memcpy(&r.gemm_bad, vr, 8);
  std::memcpy(&r.gemm_max_err, vr + 8, 4);
  CK(hipFree(R));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  // Untimed clock-settle pre-warm: a cold MI355X runs the first launches at boost
  // clock, overshoots its power limit a few ms in and throttles, and needs ~25 ms
  // of sustained load to settle (profiles/r2_bench/). Timing 5 launches after a
  // cold start measures that transient, not the kernel.
  auto settle = [&](auto&& launch) -> bool {
    const auto t0 = Clock::now();
    do {
      for (int i = 0; i < 8; ++i) CK(launch());
      CK(hipStreamSynchronize(s));
    } while (std::chrono::duration<double>(Clock::now() - t0).count() < o.settle_s);
    return true;
  };
  if (!settle([&] { return ntm_gemm_bf16(A, B, C, n, n, n, n, n, n, s); })) return false;
  CK(hipEventRecord(e0, s));
  for (int i = 0; i < o.iters; ++i) CK(ntm_gemm_bf16(A, B, C, n, n, n, n, n, n, s));
  CK(hipEventRecord(e1, s));
  CK(hipEventSynchronize(e1));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  r.gemm_ms = ms / o.iters;
  r.gemm_tflops = 2.0 * n * (double)n * n / (r.gemm_ms * 1e-3) / 1e12;

  // ---- K1 + fused ABFT row checksum, checked in O(n^2) (every launch of a
  // long-running health check can afford this; the fp32 reference cannot)
  {
    float* rowsum;
    double* scratch;
    void* ab;
    CK(hipMalloc(&rowsum, sizeof(float) * n));
    CK(hipMalloc(&scratch, sizeof(double) * n));
    CK(hipMalloc(&ab, 64));
    const int it = std::max(1, o.iters / 5);
    CK(hipEventRecord(e0, s));
    for (int i = 0; i < it; ++i) {
      CK(hipMemsetAsync(rowsum, 0, sizeof(float) * n, s));
      CK(ntm_gemm_bf16_rowsum(A, B, C, rowsum, n, n, n, n, n, n, s));
    }
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    r.abft_tflops = 2.0 * n * (double)n * n / (ms / it * 1e-3) / 1e12;
    if (last && o.fault == "corrupt_abft") {
      const float bump = 64.0f;
      float v;
      CK(hipMemcpyAsync(&v, rowsum + 7, 4, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      v += bump;
      CK(hipMemcpyAsync(rowsum + 7, &v, 4, hipMemcpyHostToDevice, s));
    }
    CK(ntm_abft_check(A, B, C, rowsum, n, n, n, n, n, n, scratch, ab, s));
    unsigned char abr[64];
    CK(hipMemcpyAsync(abr, ab, ntm_abft_result_bytes(), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    std::memcpy(&r.abft_bad_acc, abr, 8);
    std::memcpy(&r.abft_bad_store, abr + 8, 8);
    unsigned bits;
    std::memcpy(&bits, abr + 16, 4);
    std::memcpy(&r.abft_max_rel_acc, &bits, 4);
    CK(hipFree(rowsum));
    CK(hipFree(scratch));
    CK(hipFree(ab));
  }
  CK(hipFree(A));
  CK(hipFree(B));

  // ---- stream-K split mode on a 192-wide tile: the one K1 path
  // whose correctness rests on a placement invariant (every part of a split tile
  // on one XCD, gemm_bf16_sk.hpp) - checked against the fp32 reference, and the
  // kernel's own placement error word must stay zero. fault "sk_xcc" makes the
  // last GPU's launch claim a wrong XCC and must fail the Job.
  if (!run_sk_check(dev, last, o, s, V, r)) return false;

  // ---- K1-fp8: the same schedule on e4m3 operands (MX-scaled MFMA, unit
  // scales), checked element-wise against the fp32 reference of the e4m3 values
  if (o.fp8 && ntm_gemm_fp8_shape_ok(n, n, n)) {
    void *A8, *B8;
    CK(hipMalloc(&A8, e));
    CK(hipMalloc(&B8, e));
    CK(hipMalloc(&R, e * 4));
    CK(ntm_fill_uniform_e4m3(A8, e, 3000 + 2 * dev, 1.0f, s));
    CK(ntm_fill_uniform_e4m3(B8, e, 3001 + 2 * dev, 1.0f, s));
    CK(ntm_gemm_fp8(A8, B8, C, n, n, n, n, n, n, s));
    if (last && o.fault == "corrupt_fp8") {
      uint16_t h;
      CK(hipMemcpyAsync(&h, (uint16_t*)C + 777, 2, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      h ^= 0x0100;
      CK(hipMemcpyAsync((uint16_t*)C + 777, &h, 2, hipMemcpyHostToDevice, s));
    }
    CK(ntm_ref_gemm_f32_e4m3(A8, B8, R, n, n, n, n, n, n, s));
    CK(hipMemsetAsync(V, 0, 64, s));
    CK(ntm_verify_bf16(C, R, e, atol, std::ldexp(1.0f, -7), V, s));
    CK(hipMemcpyAsync(vr, V, ntm_verify_result_bytes(), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    std::memcpy(&r.fp8_bad, vr, 8);
    std::memcpy(&r.fp8_max_err, vr + 8, 4);
    CK(hipFree(R));
    if (!settle([&] { return ntm_gemm_fp8(A8, B8, C, n, n, n, n, n, n, s); })) return false;
    CK(hipEventRecord(e0, s));
    for (int i = 0; i < o.iters; ++i) CK(ntm_gemm_fp8(A8, B8, C, n, n, n, n, n, n, s));
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    r.fp8_ms = ms / o.iters;
    r.fp8_tflops = 2.0 * n * (double)n * n / (r.fp8_ms * 1e-3) / 1e12;
    if (n % 256 == 0) {
      // the fp8 build with the fused ABFT row checksum, checked in O(n^2)
      float* rowsum;
      double* scratch;
      void* ab;
      CK(hipMalloc(&rowsum, sizeof(float) * n));
      CK(hipMalloc(&scratch, sizeof(double) * n));
      CK(hipMalloc(&ab, 64));
      CK(hipMemsetAsync(rowsum, 0, sizeof(float) * n, s));
      CK(ntm_gemm_fp8_rowsum(A8, B8, C, rowsum, n, n, n, n, n, n, s));
      if (last && o.fault == "corrupt_fp8_abft") {
        uint16_t h;
        CK(hipMemcpyAsync(&h, (uint16_t*)C + 4242, 2, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        h ^= 0x4000;  // exponent bit: a large stored-output error
        CK(hipMemcpyAsync((uint16_t*)C + 4242, &h, 2, hipMemcpyHostToDevice, s));
      }
      CK(ntm_abft_check_fp8(A8, B8, C, rowsum, n, n, n, n, n, n, scratch, ab, s));
      unsigned char abr[64];
      CK(hipMemcpyAsync(abr, ab, ntm_abft_result_bytes(), hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      unsigned long long bad_acc, bad_store;
      std::memcpy(&bad_acc, abr, 8);
      std::memcpy(&bad_store, abr + 8, 8);
      r.fp8_abft_bad = bad_acc + bad_store;
      CK(hipFree(rowsum));
      CK(hipFree(scratch));
      CK(hipFree(ab));
    }
    CK(hipFree(A8));
    CK(hipFree(B8));
  }
  CK(hipFree(C));
  CK(hipFree(V));
  r.t_gemm = wall_now();

  // ---- K2: 2 GiB float4 copy
  const size_t hb = std::min<size_t>((size_t)2 << 30, fre / 4) / 16 * 16;
  void *src, *dst;
  CK(hipMalloc(&src, hb));
  CK(hipMalloc(&dst, hb));
  CK(ntm_fill_uniform_bf16(src, hb / 2, 77 + dev, 1.0f, s));
  CK(ntm_stream_copy(src, dst, hb, s));
  CK(hipEventRecord(e0, s));
  for (int i = 0; i < 10; ++i) CK(ntm_stream_copy(src, dst, hb, s));
  CK(hipEventRecord(e1, s));
  CK(hipEventSynchronize(e1));
  CK(hipEventElapsedTime(&ms, e0, e1));
  r.hbm_copy_gbps = 2.0 * hb * 10 / (ms * 1e-3) / 1e9;
  {
    float* sink;
    CK(hipMalloc(&sink, sizeof(float) * 8192));
    CK(ntm_stream_read(src, hb, sink, s));
    CK(hipEventRecord(e0, s));
    for (int i = 0; i < 10; ++i) CK(ntm_stream_read(src, hb, sink, s));
    CK(hipEventRecord(e1, s));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms, e0, e1));
    r.hbm_read_gbps = (double)hb * 10 / (ms * 1e-3) / 1e9;
    CK(hipFree(sink));
  }
  {  // byte-exact copy check on a sample window (first + last 16 MiB)
    const size_t w = std::min<size_t>(hb, 16u << 20);
    std::vector<unsigned char> h0(w), h1(w);
    bool ok = true;
    for (size_t off : {(size_t)0, hb - w}) {
      CK(hipMemcpy(h0.data(), (char*)src + off, w, hipMemcpyDeviceToHost));
      CK(hipMemcpy(h1.data(), (char*)dst + off, w, hipMemcpyDeviceToHost));
      ok = ok && std::memcmp(h0.data(), h1.data(), w) == 0;
    }
    r.hbm_copy_ok = ok;
  }
  CK(hipFree(src));
  CK(hipFree(dst));
  if (o.hbm_test_gb != 0 && !run_hbm_test(dev, last, o, s, r)) return false;
  if (o.cu_sweep && !run_cu_sweep(dev, last, o, s, r)) return false;
  if (o.host_link_mib > 0 && !run_host_link(dev, last, o, s, r)) return false;
  if (o.mx_check && !run_mx_check(dev, last, o, s, r)) return false;
  if (o.xcd_sweep && !run_xcd_sweep(dev, last, o, s, r)) return false;
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  CK(hipStreamDestroy(s));
  r.t_hbm = wall_now();
  return true;
}

struct CollRow {
  const char* dtype;
  size_t bytes;
  double us, algbw, busbw;
  unsigned long long bad;
};

double bus_factor(int n) { return n > 1 ? 2.0 * (n - 1) / n : 0.0; }

// C1 message sizes up to maxb: nccl-tests style, 8 B .. max, x4 per step (the
// torch sweep in parallel/collectives.py builds the same list; a CPU test
// pins the two against each other through --describe-sweep)
std::vector<size_t> rccl_sizes(size_t maxb) {
  std::vector<size_t> v;
  for (size_t b = 8; b <= maxb; b *= 4) v.push_back(b);
  return v;
}

// C2 message sizes: the C1 sizes from 512 B that split into 8-element chunks
// per rank, so every C2 row pairs with a C1 row (bench.py builds the same list)
std::vector<size_t> xgmi_sizes(size_t maxb, int n) {
  std::vector<size_t> v;
  for (const size_t b : rccl_sizes(maxb))
    if (b >= 512 && (b / 2) % (8 * (size_t)n) == 0) v.push_back(b);
  return v;
}

// Largest sweep message: --allreduce-max-mib, capped at 40 % of the smallest
// free HBM over `devs` and rounded down to a power of two (the sweep doubles).
size_t sweep_cap(const std::vector<int>& devs, size_t want, int buffers_per_dev) {
  size_t mn = SIZE_MAX;
  for (int d : devs) {
    size_t fre = 0, tot = 0;
    if (hipSetDevice(d) != hipSuccess || hipMemGetInfo(&fre, &tot) != hipSuccess) return 0;
    mn = std::min(mn, fre);
  }
  const size_t cap = (size_t)(0.4 * (double)mn) / (size_t)buffers_per_dev;
  size_t b = 8;
  while (b * 2 <= std::min(want, cap)) b *= 2;
  return b;
}

// C1: RCCL all-reduce sweep, single process owning all devices
// (ncclCommInitAll). Runs at n = 1 too - a one-rank communicator: busbw factor
// 0, result still checked element by element - so the path the 8-GPU node
// uses has executed before it gets there. Every RCCL call is checked, in the
// warm-up and timed loops as well: a failed launch must never turn into a
// fast, wrong bandwidth figure.
bool run_rccl(const std::vector<int>& devs, const Opts& o, std::vector<CollRow>& rows) {
  const int n = (int)devs.size();
  const size_t maxb = sweep_cap(devs, (size_t)o.allreduce_max_mib << 20, 1);
  if (maxb < 8) { fail("RCCL sweep: no free HBM"); return false; }
  std::vector<ncclComm_t> comms(n);
  if (ncclCommInitAll(comms.data(), n, devs.data()) != ncclSuccess) {
    fail("ncclCommInitAll failed");
    return false;
  }
  std::vector<hipStream_t> st(n);
  std::vector<void*> buf(n, nullptr);
  std::vector<unsigned long long*> bad(n, nullptr);
  bool ok = true;
  auto cleanup = [&] {
    for (int i = 0; i < n; ++i) {
      (void)hipSetDevice(devs[i]);
      if (buf[i]) (void)hipFree(buf[i]);
      if (bad[i]) (void)hipFree(bad[i]);
      if (st[i]) (void)hipStreamDestroy(st[i]);
      ncclCommDestroy(comms[i]);
    }
  };
  for (int i = 0; i < n; ++i) {
    st[i] = nullptr;
    if (hipSetDevice(devs[i]) != hipSuccess ||
        hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&buf[i], maxb) != hipSuccess || hipMalloc(&bad[i], 8) != hipSuccess) {
      fail("RCCL sweep: buffer allocation failed");
      cleanup();
      return false;
    }
  }
  // nccl-tests style: 8 B .. max, x4 per step, bf16 then fp32
  for (const bool f32 : {false, true}) {
    for (const size_t bytes : rccl_sizes(maxb)) {
      if (!ok) break;
      const size_t esz = f32 ? 4 : 2;
      const size_t cnt = bytes / esz;
      const ncclDataType_t dt = f32 ? ncclFloat32 : ncclBfloat16;
      auto run_once = [&]() -> bool {
        if (ncclGroupStart() != ncclSuccess) return false;
        bool good = true;
        for (int i = 0; i < n; ++i)
          good = good && ncclAllReduce(buf[i], buf[i], cnt, dt, ncclSum, comms[i], st[i]) == ncclSuccess;
        return (ncclGroupEnd() == ncclSuccess) && good;
      };
      auto sync_all = [&]() -> bool {
        for (int i = 0; i < n; ++i)
          if (hipSetDevice(devs[i]) != hipSuccess || hipStreamSynchronize(st[i]) != hipSuccess)
            return false;
        return true;
      };
      const unsigned blocks = (unsigned)std::min<size_t>(1024, (cnt + 255) / 256);
      for (int i = 0; i < n; ++i) {
        CK(hipSetDevice(devs[i]));
        // fault injection: the last rank contributes the wrong pattern
        const int contrib = (o.fault == "corrupt_allreduce" && i == n - 1) ? i + 1 : i;
        if (f32)
          hipLaunchKernelGGL(fill_pattern<float>, dim3(blocks), dim3(256), 0, st[i], (float*)buf[i], cnt, contrib);
        else
          hipLaunchKernelGGL(fill_pattern<uint16_t>, dim3(blocks), dim3(256), 0, st[i], (uint16_t*)buf[i], cnt, contrib);
        CK(hipGetLastError());
        CK(hipMemsetAsync(bad[i], 0, 8, st[i]));
      }
      if (!run_once()) { fail("ncclAllReduce failed"); ok = false; break; }
      unsigned long long tot_bad = 0;
      for (int i = 0; i < n; ++i) {
        CK(hipSetDevice(devs[i]));
        if (f32)
          hipLaunchKernelGGL(check_pattern<float>, dim3(blocks), dim3(256), 0, st[i], (const float*)buf[i], cnt, n, bad[i]);
        else
          hipLaunchKernelGGL(check_pattern<uint16_t>, dim3(blocks), dim3(256), 0, st[i], (const uint16_t*)buf[i], cnt, n, bad[i]);
        CK(hipGetLastError());
        unsigned long long b = 0;
        CK(hipMemcpyAsync(&b, bad[i], 8, hipMemcpyDeviceToHost, st[i]));
        CK(hipStreamSynchronize(st[i]));
        tot_bad += b;
      }
      // timing: fewer iterations for the multi-GiB messages
      const int iters = bytes >= ((size_t)1 << 30) ? 4 : 10;
      bool run_ok = true;
      for (int w = 0; w < 2 && run_ok; ++w) run_ok = run_once();
      run_ok = run_ok && sync_all();
      const auto t0 = Clock::now();
      for (int it = 0; it < iters && run_ok; ++it) run_ok = run_once();
      run_ok = run_ok && sync_all();
      if (!run_ok) { fail("ncclAllReduce failed in the timed loop"); ok = false; break; }
      const double sec = std::chrono::duration<double>(Clock::now() - t0).count() / iters;
      // one rank: RCCL's in-place all-reduce moves nothing - only the check counts
      const double alg = n > 1 ? bytes / sec / 1e9 : NAN;
      rows.push_back({f32 ? "fp32" : "bf16", bytes, sec * 1e6, alg, n > 1 ? alg * bus_factor(n) : 0.0,
                      tot_bad});
      if (tot_bad) ok = false;
    }
  }
  cleanup();
  if (!ok) fail("RCCL all-reduce failed or produced wrong elements");
  return ok;
}

// C2: hand-written two-shot all-reduce over peer-mapped xGMI.
// C3: per-link xGMI check. For every ordered pair (dst <- src), GPU dst pulls
// --p2p-mib MiB out of GPU src's HBM through the peer mapping with the K2 copy
// kernel, so every read crosses the one dst-src link; timed with events on
// dst, pairs one at a time, then a sample window is compared byte for byte.
// A degraded or miswired link is one cell of this matrix, where a ring
// all-reduce's busbw only shows the slowest ring. --p2p-loopback runs the same
// code on a single GPU as pair 0 <- 0 (a local copy) so the path is testable
// on a one-GPU box.
struct P2pResult {
  int n = 0;
  std::vector<double> gbps;  // n x n, row = destination (puller), NAN on the diagonal
  unsigned long long bad_pairs = 0;
  double min_gbps = 0;
};

bool run_p2p(const std::vector<int>& devs, const Opts& o, P2pResult& r) {
  const int n = o.p2p_loopback ? 1 : (int)devs.size();
  r.n = n;
  r.gbps.assign((size_t)n * n, NAN);
  const size_t bytes = (size_t)o.p2p_mib << 20;
  std::vector<void*> src(n, nullptr), dst(n, nullptr);
  std::vector<hipStream_t> st(n);
  std::vector<hipEvent_t> e0(n), e1(n);
  for (int i = 0; i < n; ++i) {
    CK(hipSetDevice(devs[i]));
    if (!o.p2p_loopback)
      for (int j = 0; j < n; ++j) {
        if (i == j) continue;
        int can = 0;
        CK(hipDeviceCanAccessPeer(&can, devs[i], devs[j]));
        if (!can) {
          fail("no peer access from GPU " + std::to_string(devs[i]) + " to " + std::to_string(devs[j]));
          return false;
        }
        hipError_t e = hipDeviceEnablePeerAccess(devs[j], 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) CK(e);
      }
    CK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
    CK(hipEventCreate(&e0[i]));
    CK(hipEventCreate(&e1[i]));
    CK(hipMalloc(&src[i], bytes));
    CK(hipMalloc(&dst[i], bytes));
    CK(ntm_fill_uniform_bf16(src[i], bytes / 2, 4242 + devs[i], 1.0f, st[i]));
    CK(hipStreamSynchronize(st[i]));
  }
  const size_t w = std::min<size_t>(bytes, 1u << 20);
  std::vector<unsigned char> h0(w), h1(w);
  double mn = INFINITY;
  for (int d = 0; d < n; ++d)
    for (int sidx = 0; sidx < n; ++sidx) {
      if (sidx == d && !o.p2p_loopback) continue;
      CK(hipSetDevice(devs[d]));
      CK(hipMemsetAsync(dst[d], 0, bytes, st[d]));
      CK(ntm_stream_copy(src[sidx], dst[d], bytes, st[d]));  // warm the mapping
      const int iters = 5;
      CK(hipEventRecord(e0[d], st[d]));
      for (int it = 0; it < iters; ++it) CK(ntm_stream_copy(src[sidx], dst[d], bytes, st[d]));
      CK(hipEventRecord(e1[d], st[d]));
      CK(hipEventSynchronize(e1[d]));
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0[d], e1[d]));
      const double g = (double)bytes * iters / (ms * 1e-3) / 1e9;  // bytes over the link
      r.gbps[(size_t)d * n + sidx] = g;
      mn = std::min(mn, g);
      if (d == n - 1 && sidx == (n > 1 ? 0 : d) && o.fault == "corrupt_p2p") {
        unsigned char b = 0x5a;
        CK(hipMemcpy((char*)dst[d] + 4097, &b, 1, hipMemcpyHostToDevice));
      }
      bool same = true;
      for (size_t off : {(size_t)0, bytes - w}) {
        CK(hipMemcpy(h0.data(), (char*)src[sidx] + off, w, hipMemcpyDeviceToHost));
        CK(hipMemcpy(h1.data(), (char*)dst[d] + off, w, hipMemcpyDeviceToHost));
        same = same && std::memcmp(h0.data(), h1.data(), w) == 0;
      }
      if (!same) {
        ++r.bad_pairs;
        fail("xGMI P2P copy GPU " + std::to_string(devs[sidx]) + " -> GPU " +
             std::to_string(devs[d]) + " corrupted data");
      }
      if (o.p2p_floor_gbps > 0 && g < o.p2p_floor_gbps)
        fail("xGMI P2P GPU " + std::to_string(devs[sidx]) + " -> GPU " + std::to_string(devs[d]) +
             " " + jnum(g) + " GB/s below floor " + jnum(o.p2p_floor_gbps));
    }
  r.min_gbps = std::isfinite(mn) ? mn : 0;
  for (int i = 0; i < n; ++i) {
    CK(hipSetDevice(devs[i]));
    CK(hipFree(src[i]));
    CK(hipFree(dst[i]));
    CK(hipEventDestroy(e0[i]));
    CK(hipEventDestroy(e1[i]));
    CK(hipStreamDestroy(st[i]));
  }
  return true;
}

std::string p2p_json(const P2pResult& r) {
  std::string js = "[";
  for (int d = 0; d < r.n; ++d) {
    js += d ? ",[" : "[";
    for (int s2 = 0; s2 < r.n; ++s2) js += (s2 ? "," : "") + jnum(r.gbps[(size_t)d * r.n + s2]);
    js += "]";
  }
  return js + "]";
}

// C2 driver. Real mode: rank i on GPU devs[i] (peer access between all pairs,
// one launch per GPU). Simulated mode (--xgmi-sim N): all N ranks on devs[0]
// in one launch (rank = block / nblk), so the whole protocol - entry barrier,
// reduce-scatter, all-gather, exit barrier, epochs - runs on a one-GPU box
// through this same driver. Sizes: xgmi_sizes (512 B .. min(max, 1 GiB));
// <= --xgmi-one-shot-max (256 KiB) takes the one-shot kernel. The kernel
// synchronises the ranks itself (device-side entry barrier), so the timed
// loop launches back to back with no host sync.
// --xgmi-tune: what the mini-sweep chose (and its table) for the JSON report.
struct XgmiTune {
  bool ran = false;
  int nblk = 0;
  size_t one_shot_max = 0;
  double seconds = 0;
  std::string table = "[]";
};

bool run_xgmi(const std::vector<int>& devs, const Opts& o, std::vector<CollRow>& rows,
              XgmiTune& tune) {
  const bool sim = o.xgmi_sim > 0;
  const int n = sim ? o.xgmi_sim : (int)devs.size();
  if (n < 1 || n > ntm::xgmi::kMaxRanks) return true;
  const int ndev = sim ? 1 : n;                    // devices launching
  auto dev_of = [&](int r) { return sim ? devs[0] : devs[r]; };
  if (!sim)
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        if (i == j) continue;
        int can = 0;
        CK(hipDeviceCanAccessPeer(&can, devs[i], devs[j]));
        if (!can) {
          fail("no peer access between GPUs " + std::to_string(devs[i]) + " and " + std::to_string(devs[j]));
          return false;
        }
        CK(hipSetDevice(devs[i]));
        hipError_t e = hipDeviceEnablePeerAccess(devs[j], 0);
        if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) CK(e);
      }
  // blocks per rank and the one-shot cutoff are knobs (--xgmi-nblk,
  // --xgmi-one-shot-max): bench.py sweeps them at N > 1, so the first 8-GPU
  // run says whether the design or the constant is at fault
  // --xgmi-tune: a mini-sweep (blocks per rank 32..256 x one-/two-shot at
  // 256 KiB, 1 MiB and 64 MiB, a few calls each, well under 2 s at N = 8)
  // picks both before the main sweep, like bench.py's xgmi.tune does at N > 1.
  // One signal area sized for the largest candidate serves every nblk: slots
  // only alias across calls, and epochs only grow.
  constexpr int kTuneNblk[] = {32, 64, 128, 256};
  const int nblk_cap = sim ? 1024 / n : 1024;
  int nblk = std::min(o.xgmi_nblk, nblk_cap);
  size_t one_shot_max = (size_t)std::max(0L, o.xgmi_one_shot_max);
  const int sig_nblk = o.xgmi_tune ? std::max(nblk, std::min(256, nblk_cap)) : nblk;
  std::vector<int> used(devs.begin(), devs.begin() + ndev);
  const size_t maxb = sweep_cap(used, std::min<size_t>((size_t)o.allreduce_max_mib << 20,
                                                       (size_t)1 << 30), sim ? 2 * n : 2);
  std::vector<void*> in(n), out(n);
  std::vector<unsigned*> sig(n);
  std::vector<unsigned*> err(ndev);
  std::vector<unsigned long long*> bad(n);
  std::vector<hipStream_t> st(ndev);
  for (int i = 0; i < ndev; ++i) {
    CK(hipSetDevice(devs[i]));
    CK(hipStreamCreateWithFlags(&st[i], hipStreamNonBlocking));
    CK(hipMalloc(&err[i], 4));
    CK(hipMemset(err[i], 0, 4));
  }
  for (int r = 0; r < n; ++r) {
    CK(hipSetDevice(dev_of(r)));
    CK(hipMalloc(&in[r], maxb));
    CK(hipMalloc(&out[r], maxb));
    CK(hipMalloc(&bad[r], 8));
    CK(hipExtMallocWithFlags((void**)&sig[r], ntm_xgmi_signal_bytes(sig_nblk), hipDeviceMallocUncached));
    CK(hipMemset(sig[r], 0, ntm_xgmi_signal_bytes(sig_nblk)));
  }
  unsigned epoch = 0;
  bool ok = true;
  if (o.xgmi_tune) {
    // time `calls` back-to-back launches at (nb, bytes, one-shot); < 0 on failure
    auto time_point = [&](int nb, size_t bytes, int os, int calls) -> double {
      const size_t cnt = bytes / 2;
      auto launch = [&]() -> bool {
        ++epoch;
        for (int i = 0; i < ndev; ++i)
          if (hipSetDevice(devs[i]) != hipSuccess ||
              ntm_xgmi_allreduce_bf16((const void* const*)in.data(), os ? out.data() : (void* const*)in.data(),
                                      sig.data(), n, sim ? 0 : i, sim ? n : 1, nb, cnt, epoch,
                                      err[i], os, st[i]) != 0)
            return false;
        return true;
      };
      auto sync = [&]() -> bool {
        for (int i = 0; i < ndev; ++i)
          if (hipSetDevice(devs[i]) != hipSuccess || hipStreamSynchronize(st[i]) != hipSuccess)
            return false;
        return true;
      };
      if (!launch() || !sync()) return -1;
      const auto t0 = Clock::now();
      for (int c = 0; c < calls; ++c)
        if (!launch()) return -1;
      if (!sync()) return -1;
      return std::chrono::duration<double>(Clock::now() - t0).count() / calls;
    };
    const auto t_tune = Clock::now();
    std::vector<size_t> tsizes;
    for (const size_t b : {(size_t)256 << 10, (size_t)1 << 20, (size_t)64 << 20})
      if (b <= maxb && (b / 2) % (8 * (size_t)n) == 0) tsizes.push_back(b);
    const size_t cuts[] = {0, (size_t)256 << 10, (size_t)1 << 20};
    double best_t = 1e300;
    std::string tab = "[";
    for (const int nb : kTuneNblk) {
      // no size fits the sweep cap: nothing to time, keep the defaults (nblk 32,
      // the default cutoff) rather than "choosing" cutoff 0 on an empty table
      if (nb > nblk_cap || !ok || tsizes.empty()) continue;
      double t1[3] = {1e300, 1e300, 1e300}, t2[3] = {1e300, 1e300, 1e300};
      for (size_t k = 0; k < tsizes.size() && ok; ++k)
        for (const int os : {1, 2}) {
          if (os == 1 && tsizes[k] > ((size_t)1 << 20)) continue;
          const double t = time_point(nb, tsizes[k], os == 1, 3);
          if (t < 0) { fail("xGMI tune launch failed"); ok = false; break; }
          (os == 1 ? t1 : t2)[k] = t;
          tab += std::string(tab.size() > 1 ? "," : "") + "{\"nblk\":" + std::to_string(nb) +
                 ",\"bytes\":" + std::to_string(tsizes[k]) + ",\"algo\":\"" +
                 (os == 1 ? "1shot" : "2shot") + "\",\"time_us\":" + jnum(t * 1e6) + "}";
        }
      for (const size_t c : cuts) {
        double tot = 0;
        for (size_t k = 0; k < tsizes.size(); ++k) tot += tsizes[k] <= c ? t1[k] : t2[k];
        if (tot < best_t) {
          best_t = tot;
          nblk = nb;
          one_shot_max = c;
        }
      }
    }
    tune.table = tab + "]";
    tune.ran = ok && !tsizes.empty();
    tune.seconds = std::chrono::duration<double>(Clock::now() - t_tune).count();
    for (int i = 0; i < ndev && ok; ++i) {   // a tune call that timed out fails the run
      unsigned e = 0;
      CK(hipSetDevice(devs[i]));
      CK(hipMemcpy(&e, err[i], 4, hipMemcpyDeviceToHost));
      if (e) { fail("xGMI tune: barrier timed out (code " + std::to_string(e) + ")"); ok = false; }
    }
  }
  tune.nblk = nblk;
  tune.one_shot_max = one_shot_max;
  for (const size_t bytes : xgmi_sizes(maxb, n)) {
    if (!ok) break;
    const size_t cnt = bytes / 2;
    const int one_shot = bytes <= one_shot_max ? 1 : 0;
    auto run_once = [&]() -> bool {
      ++epoch;
      for (int i = 0; i < ndev; ++i) {
        if (hipSetDevice(devs[i]) != hipSuccess) return false;
        if (ntm_xgmi_allreduce_bf16((const void* const*)in.data(), out.data(), sig.data(), n,
                                    sim ? 0 : i, sim ? n : 1, nblk, cnt, epoch, err[i],
                                    one_shot, st[i]) != 0)
          return false;
      }
      return true;
    };
    auto sync_all = [&]() -> bool {
      for (int i = 0; i < ndev; ++i)
        if (hipSetDevice(devs[i]) != hipSuccess || hipStreamSynchronize(st[i]) != hipSuccess)
          return false;
      return true;
    };
    auto timed_out = [&]() -> unsigned {
      unsigned worst = 0;
      for (int i = 0; i < ndev; ++i) {
        unsigned e = 0;
        if (hipSetDevice(devs[i]) != hipSuccess ||
            hipMemcpy(&e, err[i], 4, hipMemcpyDeviceToHost) != hipSuccess)
          return ~0u;
        worst = std::max(worst, e);
      }
      return worst;
    };
    for (int r = 0; r < n; ++r) {
      CK(hipSetDevice(dev_of(r)));
      const int contrib = (o.fault == "corrupt_allreduce" && r == n - 1) ? r + 1 : r;
      hipLaunchKernelGGL(fill_pattern<uint16_t>, dim3(1024), dim3(256), 0, st[sim ? 0 : r],
                         (uint16_t*)in[r], cnt, contrib);
      CK(hipGetLastError());
      CK(hipMemsetAsync(bad[r], 0, 8, st[sim ? 0 : r]));
    }
    if (!run_once()) { fail("xGMI all-reduce launch failed"); ok = false; break; }
    if (!sync_all()) { fail("xGMI all-reduce: stream error"); ok = false; break; }
    if (const unsigned e = timed_out()) {
      fail("xGMI all-reduce barrier timed out (code " + std::to_string(e) + ")");
      ok = false;
      break;
    }
    unsigned long long tot_bad = 0;
    for (int r = 0; r < n; ++r) {
      CK(hipSetDevice(dev_of(r)));
      hipStream_t sr = st[sim ? 0 : r];
      hipLaunchKernelGGL(check_pattern<uint16_t>, dim3(1024), dim3(256), 0, sr,
                         (const uint16_t*)out[r], cnt, n, bad[r]);
      CK(hipGetLastError());
      unsigned long long b = 0;
      CK(hipMemcpyAsync(&b, bad[r], 8, hipMemcpyDeviceToHost, sr));
      CK(hipStreamSynchronize(sr));
      tot_bad += b;
    }
    const int iters = 10;
    bool run_ok = run_once() && sync_all();   // warm-up
    const auto t0 = Clock::now();
    for (int it = 0; it < iters && run_ok; ++it) run_ok = run_once();
    run_ok = run_ok && sync_all();
    const double sec = std::chrono::duration<double>(Clock::now() - t0).count() / iters;
    if (!run_ok) { fail("xGMI all-reduce failed in the timed loop"); ok = false; break; }
    if (const unsigned e = timed_out()) {
      fail("xGMI all-reduce barrier timed out in the timed loop (code " + std::to_string(e) + ")");
      ok = false;
      break;
    }
    const double alg = bytes / sec / 1e9;
    rows.push_back({one_shot ? "bf16-1shot" : "bf16", bytes, sec * 1e6, alg, alg * bus_factor(n),
                    tot_bad});
    if (tot_bad) ok = false;
  }
  for (int r = 0; r < n; ++r) {
    (void)hipSetDevice(dev_of(r));
    (void)hipFree(in[r]);
    (void)hipFree(out[r]);
    (void)hipFree(sig[r]);
    (void)hipFree(bad[r]);
  }
  for (int i = 0; i < ndev; ++i) {
    (void)hipSetDevice(devs[i]);
    (void)hipFree(err[i]);
    (void)hipStreamDestroy(st[i]);
  }
  if (!ok) fail("xGMI all-reduce failed or produced wrong elements");
  return ok;
}

std::string coll_json(const std::vector<CollRow>& rows) {
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

// POST `body` (Prometheus text format) to a Pushgateway:
//   <url>/metrics/job/amdgpu_validate/instance/<host>
// Plain HTTP/1.1 over a socket (the image has no curl). Returns "ok" or a
// short error; never fatal - the verdict does not depend on the push.
std::string push_metrics(const std::string& url, const std::string& body) {
  const std::string scheme = "http://";
  if (url.rfind(scheme, 0) != 0) return "error: only http:// URLs";
  std::string rest = url.substr(scheme.size());
  const size_t slash = rest.find('/');
  std::string hostport = rest.substr(0, slash);
  std::string prefix = slash == std::string::npos ? "" : rest.substr(slash);
  while (!prefix.empty() && prefix.back() == '/') prefix.pop_back();
  std::string host = hostport, port = "9091";
  const size_t colon = hostport.rfind(':');
  if (colon != std::string::npos) {
    host = hostport.substr(0, colon);
    port = hostport.substr(colon + 1);
  }
  char me[256] = "unknown";
  gethostname(me, sizeof me - 1);
  const std::string path = prefix + "/metrics/job/amdgpu_validate/instance/" + me;
  addrinfo hints{}, *ai = nullptr;
  hints.ai_family = AF_UNSPEC;
  hints.ai_socktype = SOCK_STREAM;
  if (getaddrinfo(host.c_str(), port.c_str(), &hints, &ai) != 0 || !ai)
    return "error: cannot resolve " + host;
  int fd = -1;
  for (addrinfo* p = ai; p; p = p->ai_next) {
    fd = socket(p->ai_family, p->ai_socktype, p->ai_protocol);
    if (fd < 0) continue;
    timeval tv{10, 0};
    setsockopt(fd, SOL_SOCKET, SO_SNDTIMEO, &tv, sizeof tv);
    setsockopt(fd, SOL_SOCKET, SO_RCVTIMEO, &tv, sizeof tv);
    if (connect(fd, p->ai_addr, p->ai_addrlen) == 0) break;
    close(fd);
    fd = -1;
  }
  freeaddrinfo(ai);
  if (fd < 0) return "error: cannot connect to " + hostport;
  const std::string req = "POST " + path + " HTTP/1.1\r\nHost: " + hostport +
                          "\r\nContent-Type: text/plain; version=0.0.4\r\nContent-Length: " +
                          std::to_string(body.size()) + "\r\nConnection: close\r\n\r\n" + body;
  size_t off = 0;
  while (off < req.size()) {
    const ssize_t w = send(fd, req.data() + off, req.size() - off, MSG_NOSIGNAL);
    if (w <= 0) {
      close(fd);
      return "error: send failed";
    }
    off += (size_t)w;
  }
  char buf[256];
  const ssize_t r = recv(fd, buf, sizeof buf - 1, 0);
  close(fd);
  if (r <= 0) return "error: no response";
  buf[r] = 0;
  const std::string status(buf, strnlen(buf, sizeof buf));
  // "HTTP/1.1 200 OK" / "202 Accepted"
  if (status.size() > 12 && status[9] == '2') return "ok";
  return "error: " + status.substr(0, status.find('\r'));
}

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

HostPrep read_host_prep() {
  HostPrep h;
  std::ifstream nb("/proc/sys/kernel/numa_balancing");
  if (nb) nb >> h.numa_balancing;
  rlimit rl{};
  h.memlock_unlimited = getrlimit(RLIMIT_MEMLOCK, &rl) == 0 && rl.rlim_cur == RLIM_INFINITY;
  std::ifstream cl("/proc/cmdline");
  std::string w;
  while (cl >> w) h.iommu_pt = h.iommu_pt || w == "iommu=pt";
  return h;
}

// peak busbw of the bf16 rows (the floors gate the interconnect, not a size)
double peak_busbw(const std::vector<CollRow>& rows) {
  double m = 0;
  for (auto& r : rows)
    if (std::strncmp(r.dtype, "bf16", 4) == 0 && std::isfinite(r.busbw)) m = std::max(m, r.busbw);
  return m;
}

}  // namespace

int main(int argc, char** argv) {
  const double t_start = process_start_epoch();
  Opts o;
  if (!parse(argc, argv, o)) {
    usage();
    return 2;
  }
  if (o.xgmi_nblk < 1 || o.xgmi_nblk > 1024 || o.xgmi_one_shot_max < 0) {
    std::fprintf(stderr, "--xgmi-nblk must be in 1..1024, --xgmi-one-shot-max >= 0\n");
    return 2;
  }
  if (o.describe_sweep) {
    // host-only: the sweep definitions the GPU paths use, for CPU tests
    const size_t maxb = (size_t)o.allreduce_max_mib << 20;
    auto arr = [](const std::vector<size_t>& v) {
      std::string t = "[";
      for (size_t i = 0; i < v.size(); ++i) t += (i ? "," : "") + std::to_string(v[i]);
      return t + "]";
    };
    std::string t = "{\"rccl_bytes\":" + arr(rccl_sizes(maxb)) + ",\"bus_factor\":[";
    for (int k = 1; k <= 8; ++k) t += (k > 1 ? "," : "") + jnum(bus_factor(k));
    t += "],\"xgmi_bytes\":{";
    for (int k = 1; k <= 8; ++k)
      t += (k > 1 ? ",\"" : "\"") + std::to_string(k) + "\":" + arr(xgmi_sizes(std::min<size_t>(maxb, (size_t)1 << 30), k));
    std::printf("%s}}\n", t.c_str());
    return 0;
  }
  if (o.fault.empty())
    if (const char* f = std::getenv("NTM_FAULT_INJECT")) o.fault = f;
  if ((o.fault == "slow_xcd" || o.fault == "corrupt_xcd") && !o.xcd_sweep) {
    std::fprintf(stderr, "fault-inject %s needs --xcd-sweep\n", o.fault.c_str());
    usage();
    return 2;
  }
  const HostPrep hp = read_host_prep();
  if (o.require_host_prep || o.require_iommu_pt) {
    if (hp.numa_balancing != 0)
      fail("host prep: kernel.numa_balancing = " + std::to_string(hp.numa_balancing) + " (want 0)");
    if (!hp.memlock_unlimited) fail("host prep: RLIMIT_MEMLOCK is not unlimited (containerd LimitMEMLOCK)");
  }
  if (o.require_iommu_pt && !hp.iommu_pt) fail("host prep: iommu=pt missing from /proc/cmdline");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) {
    const char* nn = std::getenv("NODE_NAME");
    std::printf("{\"passed\":false,%s\"failures\":[\"no AMD GPU visible\"]}\n",
                nn ? ("\"node\":" + jstr(nn) + ",").c_str() : "");
    return 2;
  }
  const int n = o.gpus > 0 ? std::min(o.gpus, ndev) : ndev;
  if (o.gpus > ndev) fail("requested " + std::to_string(o.gpus) + " GPUs, " + std::to_string(ndev) + " visible");
  std::vector<int> devs(n);
  for (int i = 0; i < n; ++i) devs[i] = i;
  const double t_hip = wall_now();

  std::vector<GpuResult> res(n);
  std::vector<std::thread> th;
  for (int i = 0; i < n; ++i)
    th.emplace_back([&, i] { run_gpu(devs[i], i == n - 1, o, res[i]); });
  for (auto& t : th) t.join();
  const double t_local = wall_now();

  for (auto& r : res) {
    const std::string d = "gpu" + std::to_string(r.device) + ": ";
    if (r.gemm_bad != 0) fail(d + "GEMM verification failed (" + std::to_string(r.gemm_bad) + " elements)");
    if (r.sk_variant && r.sk_word != 0) {
      char w[16];
      std::snprintf(w, sizeof w, "0x%08x", r.sk_word);
      fail(d + "stream-K split mode: a split tile's parts ran on different XCDs (error word " + w +
           "); its C is not trusted");
    }
    if (r.sk_variant && r.sk_bad != 0)
      fail(d + "stream-K split-mode GEMM verification failed (" + std::to_string(r.sk_bad) +
           " elements)");
    if (r.abft_bad_acc != 0 || r.abft_bad_store != 0)
      fail(d + "GEMM ABFT checksum failed (" + std::to_string(r.abft_bad_acc) + " accumulator / " +
           std::to_string(r.abft_bad_store) + " stored rows)");
    if (o.tflops_floor > 0 && r.gemm_tflops < o.tflops_floor)
      fail(d + "GEMM " + jnum(r.gemm_tflops) + " TFLOP/s below floor " + jnum(o.tflops_floor));
    if (o.fp8 && r.fp8_bad != 0)
      fail(d + "fp8 GEMM verification failed (" +
           (r.fp8_bad == ~0ull ? std::string("not run: --size must be a multiple of 256")
                               : std::to_string(r.fp8_bad) + " elements") + ")");
    if (o.fp8 && r.fp8_abft_bad != 0 && r.fp8_abft_bad != ~0ull)
      fail(d + "fp8 GEMM ABFT checksum failed (" + std::to_string(r.fp8_abft_bad) + " rows)");
    if (o.fp8 && o.fp8_tflops_floor > 0 && r.fp8_tflops < o.fp8_tflops_floor)
      fail(d + "fp8 GEMM " + jnum(r.fp8_tflops) + " TFLOP/s below floor " + jnum(o.fp8_tflops_floor));
    if (o.min_hbm_gb > 0 && r.total_gb < o.min_hbm_gb)
      fail(d + "HBM " + jnum(r.total_gb) + " GB below " + jnum(o.min_hbm_gb) + " GB");
    if (!r.hbm_copy_ok) fail(d + "HBM copy mismatch");
    if (!r.hbm_test_failure.empty()) fail(r.hbm_test_failure);
    if (!r.cu_sweep_failure.empty()) fail(r.cu_sweep_failure);
    for (auto& f : r.host_link_failures) fail(f);
    for (auto& f : r.mx_failures) fail(f);
    for (auto& f : r.xcd_failures) fail(f);
    if (o.hbm_floor_gbps > 0 && r.hbm_copy_gbps < o.hbm_floor_gbps)
      fail(d + "HBM copy " + jnum(r.hbm_copy_gbps) + " GB/s below floor");
  }

  std::vector<CollRow> rccl_rows, xgmi_rows;
  // C1 by default on n > 1; --rccl runs the one-rank communicator on n = 1 (the
  // same code path; its ~2 s RCCL init is not worth paying in a 1-GPU Job)
  if (o.rccl == 1 || (o.rccl < 0 && n > 1)) run_rccl(devs, o, rccl_rows);
  const double t_rccl = wall_now();
  XgmiTune xtune;
  if (o.xgmi && (n > 1 || o.xgmi_sim > 0)) run_xgmi(devs, o, xgmi_rows, xtune);
  P2pResult p2p;
  if (o.p2p && (n > 1 || o.p2p_loopback)) run_p2p(devs, o, p2p);
  const double t_end = wall_now();
  // interconnect gates (0 = off; set from the first 8-GPU measurement)
  const double rccl_peak_bf16 = peak_busbw(rccl_rows), xgmi_peak_bf16 = peak_busbw(xgmi_rows);
  if (o.rccl_busbw_floor_gbps > 0 && !rccl_rows.empty() && rccl_peak_bf16 < o.rccl_busbw_floor_gbps)
    fail("RCCL all-reduce peak bf16 busbw " + jnum(rccl_peak_bf16) + " GB/s below floor " +
         jnum(o.rccl_busbw_floor_gbps));
  if (o.xgmi_busbw_floor_gbps > 0 && !xgmi_rows.empty() && xgmi_peak_bf16 < o.xgmi_busbw_floor_gbps)
    fail("xGMI all-reduce peak bf16 busbw " + jnum(xgmi_peak_bf16) + " GB/s below floor " +
         jnum(o.xgmi_busbw_floor_gbps));

  double agg = 0;
  for (auto& r : res) agg += r.gemm_tflops;
  // node-exporter textfile-collector format (--prom-out) and Pushgateway
  // body (--pushgateway); labels carry the device index.
  double peak_rccl = 0, peak_xgmi = 0;
  for (auto& c : rccl_rows) peak_rccl = std::max(peak_rccl, c.busbw);
  for (auto& c : xgmi_rows) peak_xgmi = std::max(peak_xgmi, c.busbw);
  const bool passed = g_failures.empty();
  // the Kubernetes node this ran on (NODE_NAME from the downward API in the
  // module's Job, one pod per GPU node): every verdict and metric names it
  const char* node_env = std::getenv("NODE_NAME");
  const std::string node = node_env ? node_env : "";
  std::string prom_text;
  {
    std::ostringstream p;
    p << "# HELP amdgpu_validate_passed 1 if every validation check passed.\n"
      << "# TYPE amdgpu_validate_passed gauge\n"
      << "amdgpu_validate_passed" << (node.empty() ? "" : "{node=" + jstr(node) + "}") << " "
      << (passed ? 1 : 0) << "\n"
      << "# TYPE amdgpu_validate_seconds gauge\n"
      << "amdgpu_validate_seconds " << jnum(t_end - t_start) << "\n"
      << "# TYPE amdgpu_validate_gemm_tflops gauge\n";
    for (auto& r : res)
      p << "amdgpu_validate_gemm_tflops{gpu=\"" << r.device << "\"} " << jnum(r.gemm_tflops) << "\n";
    if (o.fp8) {
      p << "# TYPE amdgpu_validate_gemm_fp8_tflops gauge\n";
      for (auto& r : res)
        p << "amdgpu_validate_gemm_fp8_tflops{gpu=\"" << r.device << "\"} " << jnum(r.fp8_tflops) << "\n";
    }
    p << "# TYPE amdgpu_validate_hbm_copy_gbps gauge\n";
    for (auto& r : res)
      p << "amdgpu_validate_hbm_copy_gbps{gpu=\"" << r.device << "\"} " << jnum(r.hbm_copy_gbps) << "\n";
    p << "# TYPE amdgpu_validate_hbm_total_gb gauge\n";
    for (auto& r : res)
      p << "amdgpu_validate_hbm_total_gb{gpu=\"" << r.device << "\"} " << jnum(r.total_gb) << "\n";
    if (o.hbm_test_gb != 0) {
      p << "# HELP amdgpu_validate_hbm_test_gb HBM written, read back and compared by the pattern test.\n"
        << "# TYPE amdgpu_validate_hbm_test_gb gauge\n";
      for (auto& r : res)
        if (r.hbm_test_ran)
          p << "amdgpu_validate_hbm_test_gb{gpu=\"" << r.device << "\"} " << jnum(r.hbm_test_gb) << "\n";
      p << "# HELP amdgpu_validate_hbm_test_bad_words 8-byte words the pattern test read back wrong.\n"
        << "# TYPE amdgpu_validate_hbm_test_bad_words gauge\n";
      for (auto& r : res)
        if (r.hbm_test_ran)
          p << "amdgpu_validate_hbm_test_bad_words{gpu=\"" << r.device << "\"} " << r.hbm_test_bad_words << "\n";
    }
    if (o.cu_sweep) {
      p << "# HELP amdgpu_validate_cu_sweep_cus_covered Compute units that ran a workgroup of the CU sweep.\n"
        << "# TYPE amdgpu_validate_cu_sweep_cus_covered gauge\n";
      for (auto& r : res)
        if (r.cu_sweep_ran)
          p << "amdgpu_validate_cu_sweep_cus_covered{gpu=\"" << r.device << "\"} " << r.cu_sweep.cus_covered << "\n";
      p << "# HELP amdgpu_validate_cu_sweep_bad_cus Compute units with a wrong known-answer result.\n"
        << "# TYPE amdgpu_validate_cu_sweep_bad_cus gauge\n";
      for (auto& r : res)
        if (r.cu_sweep_ran)
          p << "amdgpu_validate_cu_sweep_bad_cus{gpu=\"" << r.device << "\"} " << r.cu_sweep.bad_cus.size() << "\n";
    }
    if (o.host_link_mib > 0) {
      auto gauge = [&](const char* name, const char* help, auto value) {
        p << "# HELP amdgpu_validate_host_link_" << name << " " << help << "\n"
          << "# TYPE amdgpu_validate_host_link_" << name << " gauge\n";
        for (auto& r : res)
          if (r.host_link_ran)
            p << "amdgpu_validate_host_link_" << name << "{gpu=\"" << r.device << "\"} " << value(r) << "\n";
      };
      gauge("h2d_gbps", "Host-to-device rate over the host link (faster of kernel and hipMemcpyAsync).",
            [](const GpuResult& r) { return jnum(std::max(r.host_link_h2d_gbps, r.host_link_h2d_copy_gbps)); });
      gauge("d2h_gbps", "Device-to-host rate over the host link (faster of kernel and hipMemcpyAsync).",
            [](const GpuResult& r) { return jnum(std::max(r.host_link_d2h_gbps, r.host_link_d2h_copy_gbps)); });
      gauge("bad_words", "8-byte words that crossed the host link wrong.",
            [](const GpuResult& r) { return std::to_string(r.host_link_bad_words); });
    }
    if (o.xcd_sweep) {
      for (int clock = 0; clock < 2; ++clock) {
        const char* name = clock ? "amdgpu_validate_xcd_clock_ghz" : "amdgpu_validate_xcd_rate";
        p << "# HELP " << name
          << (clock ? " Shader clock of one XCD during a level and mode of the XCD sweep.\n"
                    : " Rate of one XCD in the XCD sweep: GB/s read and verified, GMFMA/s at level mfma.\n")
          << "# TYPE " << name << " gauge\n";
        for (auto& r : res)
          for (auto& c : r.xcd_cells)
            for (auto& row : c.sum.rows)
              p << name << "{gpu=\"" << r.device << "\",xcd=\"" << row.xcd << "\",level=\""
                << ntm::xcs::level_name(c.sum.level) << "\",mode=\"" << ntm::xcs::mode_name(c.sum.mode)
                << "\"} " << jnum(clock ? row.clock_ghz : row.rate) << "\n";
      }
    }
    if (o.mx_check) {
      auto gauge = [&](const char* name, const char* help, auto value) {
        p << "# HELP amdgpu_validate_mx_" << name << " " << help << "\n"
          << "# TYPE amdgpu_validate_mx_" << name << " gauge\n";
        for (auto& r : res)
          if (r.mx_ran)
            p << "amdgpu_validate_mx_" << name << "{gpu=\"" << r.device << "\"} " << value(r) << "\n";
      };
      gauge("formats", "MX element formats whose every step compared clean (of 5).",
            [](const GpuResult& r) { return std::to_string(r.mx_formats.size()); });
      gauge("bad_elements", "Elements of the MX block-scaled GEMMs that differ bitwise from the exact answer.",
            [](const GpuResult& r) { return std::to_string(r.mx_bad_elements); });
      gauge("fp4_tflops", "TFLOP/s of the dense MXFP4 (e2m1) GEMM.",
            [](const GpuResult& r) { return jnum(r.mx_fp4_tflops); });
      gauge("scale_spread", "Scale spread W (k-block scale exponents base .. base + W) of the dense e2m1 run.",
            [](const GpuResult& r) { return std::to_string(r.mx_scale_spread); });
      gauge("s", "Seconds the MX check took.", [](const GpuResult& r) { return jnum(r.mx_s); });
    }
    if (!rccl_rows.empty() || !xgmi_rows.empty())
      p << "# TYPE amdgpu_validate_allreduce_busbw_gbps gauge\n"
        << "amdgpu_validate_allreduce_busbw_gbps{impl=\"rccl\"} " << jnum(peak_rccl) << "\n"
        << "amdgpu_validate_allreduce_busbw_gbps{impl=\"xgmi\"} " << jnum(peak_xgmi) << "\n";
    if (p2p.n > 0) {
      p << "# HELP amdgpu_validate_xgmi_p2p_gbps Pull bandwidth dst <- src over one xGMI link.\n"
        << "# TYPE amdgpu_validate_xgmi_p2p_gbps gauge\n";
      for (int d = 0; d < p2p.n; ++d)
        for (int s2 = 0; s2 < p2p.n; ++s2)
          if (std::isfinite(p2p.gbps[(size_t)d * p2p.n + s2]))
            p << "amdgpu_validate_xgmi_p2p_gbps{dst=\"" << devs[d] << "\",src=\"" << devs[s2]
              << "\"} " << jnum(p2p.gbps[(size_t)d * p2p.n + s2]) << "\n";
    }
    prom_text = p.str();
  }
  std::string push_status;
  if (!o.pushgateway.empty()) {
    push_status = push_metrics(o.pushgateway, prom_text);
    if (push_status != "ok") std::fprintf(stderr, "amdgpu-validate: pushgateway %s\n", push_status.c_str());
  }
  std::string js = "{";
  js += "\"tool\":\"amdgpu-validate\",\"passed\":" + std::string(g_failures.empty() ? "true" : "false");
  if (!node.empty()) js += ",\"node\":" + jstr(node);
  js += ",\"n_gpus\":" + std::to_string(n) + ",\"gemm_size\":" + std::to_string(o.size);
  js += ",\"gemm_tflops_aggregate\":" + jnum(agg);
  js += ",\"gpus\":[";
  for (int i = 0; i < n; ++i) {
    const auto& r = res[i];
    js += (i ? "," : "") + std::string("{\"device\":") + std::to_string(r.device) +
          ",\"name\":" + jstr(r.name) + ",\"arch\":" + jstr(r.arch) +
          ",\"hbm_total_gb\":" + jnum(r.total_gb) + ",\"gemm_ms\":" + jnum(r.gemm_ms) +
          ",\"gemm_tflops\":" + jnum(r.gemm_tflops) +
          ",\"gemm_wrong\":" + (r.gemm_bad == ~0ull ? std::string("null") : std::to_string(r.gemm_bad)) +
          ",\"gemm_max_abs_err\":" + jnum(r.gemm_max_err) +
          ",\"abft_tflops\":" + jnum(r.abft_tflops) +
          ",\"abft_bad_rows\":" + (r.abft_bad_acc == ~0ull ? std::string("null")
                                     : std::to_string(r.abft_bad_acc + r.abft_bad_store)) +
          ",\"abft_max_rel_err\":" + jnum(r.abft_max_rel_acc) +
          ",\"gemm_fp8_tflops\":" + jnum(r.fp8_tflops) +
          ",\"gemm_fp8_wrong\":" + (r.fp8_bad == ~0ull ? std::string("null") : std::to_string(r.fp8_bad)) +
          ",\"gemm_fp8_max_abs_err\":" + jnum(r.fp8_max_err) +
          ",\"gemm_fp8_abft_bad_rows\":" +
          (r.fp8_abft_bad == ~0ull ? std::string("null") : std::to_string(r.fp8_abft_bad)) +
          ",\"sk_split_variant\":" + std::to_string(r.sk_variant) +
          ",\"sk_split_wrong\":" + (r.sk_bad == ~0ull ? std::string("null") : std::to_string(r.sk_bad)) +
          ",\"sk_xcc_error\":" + std::to_string(r.sk_word) +
          ",\"sk_split_ms\":" + jnum(r.sk_ms) +
          ",\"hbm_copy_GBps\":" + jnum(r.hbm_copy_gbps) +
          ",\"hbm_read_GBps\":" + jnum(r.hbm_read_gbps);
    if (r.hbm_test_ran)
      js += ",\"hbm_test_gb\":" + jnum(r.hbm_test_gb) +
            ",\"hbm_test_requested_gb\":" + jnum(r.hbm_test_requested_gb) +
            ",\"hbm_test_bad_words\":" + std::to_string(r.hbm_test_bad_words) +
            ",\"hbm_test_bad_bits\":" + std::to_string(r.hbm_test_bad_bits) +
            ",\"hbm_test_write_GBps\":" + jnum(r.hbm_test_write_gbps) +
            ",\"hbm_test_verify_GBps\":" + jnum(r.hbm_test_verify_gbps) +
            ",\"hbm_test_s\":" + jnum(r.hbm_test_s) +
            ",\"hbm_test_alloc_s\":" + jnum(r.hbm_test_alloc_s) +
            ",\"hbm_test_free_s\":" + jnum(r.hbm_test_free_s) +
            ",\"hbm_test_steps\":" + (r.hbm_test_steps.empty() ? std::string("[]") : r.hbm_test_steps);
    if (r.cu_sweep_ran)
      js += ",\"cu_sweep_cus\":" + std::to_string(r.cu_sweep.cus) +
            ",\"cu_sweep_cus_covered\":" + std::to_string(r.cu_sweep.cus_covered) +
            ",\"cu_sweep_simds_covered\":" + std::to_string(r.cu_sweep.simds_covered) +
            ",\"cu_sweep_launches\":" + std::to_string(r.cu_sweep.launches) +
            ",\"cu_sweep_bad_cus\":" + ntm::cus::bad_cus_json(r.cu_sweep) +
            ",\"cu_sweep_lds_bytes\":" + std::to_string(r.cu_sweep_lds_bytes) +
            ",\"cu_sweep_s\":" + jnum(r.cu_sweep_s);
    if (r.host_link_ran)
      js += ",\"host_link_mib\":" + std::to_string(r.host_link_mib) +
            ",\"host_link_h2d_GBps\":" + jnum(r.host_link_h2d_gbps) +
            ",\"host_link_d2h_GBps\":" + jnum(r.host_link_d2h_gbps) +
            ",\"host_link_h2d_copy_GBps\":" + jnum(r.host_link_h2d_copy_gbps) +
            ",\"host_link_d2h_copy_GBps\":" + jnum(r.host_link_d2h_copy_gbps) +
            ",\"host_link_duplex_GBps\":" + jnum(r.host_link_duplex_gbps) +
            ",\"host_link_read_latency_us\":" + jnum(r.host_link_latency_us) +
            ",\"host_link_bad_words\":" + std::to_string(r.host_link_bad_words) +
            ",\"host_link_bad_bits\":" + std::to_string(r.host_link_bad_bits) +
            ",\"host_link_pcie\":" + ntm::hostlink::link_json(r.host_link_pcie) +
            ",\"host_link_s\":" + jnum(r.host_link_s) +
            ",\"host_link_pin_s\":" + jnum(r.host_link_pin_s) +
            ",\"host_link_transfer_s\":" + jnum(r.host_link_xfer_s) +
            ",\"host_link_free_s\":" + jnum(r.host_link_free_s);
    if (r.mx_ran) {
      js += ",\"mx_formats\":[";
      for (size_t i = 0; i < r.mx_formats.size(); ++i) js += (i ? "," : "") + jstr(r.mx_formats[i]);
      js += "],\"mx_bad_elements\":" + std::to_string(r.mx_bad_elements) +
            ",\"mx_fp4_tflops\":" + jnum(r.mx_fp4_tflops) +
            ",\"mx_scale_spread\":" + std::to_string(r.mx_scale_spread) +
            ",\"mx_s\":" + jnum(r.mx_s);
    }
    if (r.xcd_ran) {
      namespace xs = ntm::xcs;
      js += ",\"xcd_sweep_xcds\":" + std::to_string(r.xcd_xcds) +
            ",\"xcd_sweep_mib\":" + std::to_string(o.xcd_sweep_mib) +
            ",\"xcd_sweep_ratio\":" + jnum(o.xcd_ratio);
      std::string slow = "[", bad = "[", rule;
      for (auto& c : r.xcd_cells) {
        const std::string k = std::string(",\"xcd_sweep_") + xs::level_name(c.sum.level) + "_" +
                              xs::mode_name(c.sum.mode);
        js += k + "_rate\":" + xs::rates_json(c.sum) + k + "_clock_ghz\":" + xs::clocks_json(c.sum) +
              k + "_min_over_median\":" + jnum(c.sum.min_over_median) +
              k + "_median\":" + jnum(c.sum.median_rate) +
              k + "_passes\":" + std::to_string(c.passes) +
              k + "_span_us\":[" + jnum((double)c.min_span_ticks * 0.01) + "," +
              jnum((double)c.max_span_ticks * 0.01) + "]" +
              k + "_gated\":" + (c.gated ? "true" : "false");
        const std::string at = std::string(",\"level\":") + jstr(xs::level_name(c.sum.level)) +
                               ",\"mode\":" + jstr(xs::mode_name(c.sum.mode)) + "}";
        for (uint32_t x : c.sum.slow) slow += std::string(slow.size() > 1 ? "," : "") + "{\"xcd\":" + std::to_string(x) + at;
        for (uint32_t x : c.sum.bad) bad += std::string(bad.size() > 1 ? "," : "") + "{\"xcd\":" + std::to_string(x) + at;
        if (c.gated && !c.sum.rule_ran) rule = c.sum.rule_skipped;
      }
      js += ",\"xcd_sweep_slow\":" + slow + "],\"xcd_sweep_bad\":" + bad + "]" +
            ",\"xcd_sweep_rule_skipped\":" + jstr(rule) + ",\"xcd_sweep_failures\":[";
      for (size_t i = 0; i < r.xcd_failures.size(); ++i) js += (i ? "," : "") + jstr(r.xcd_failures[i]);
      js += "],\"xcd_sweep_s\":" + jnum(r.xcd_s);
    }
    js += "}";
  }
  js += "],\"rccl_allreduce\":" + coll_json(rccl_rows);
  js += ",\"xgmi_allreduce_bf16\":" + coll_json(xgmi_rows);
  js += ",\"xgmi_simulated_ranks\":" + std::to_string(o.xgmi_sim);
  js += ",\"xgmi_nblk\":" + std::to_string(xtune.nblk ? xtune.nblk : o.xgmi_nblk) +
        ",\"xgmi_one_shot_max_bytes\":" +
        std::to_string(xtune.nblk ? (long)xtune.one_shot_max : o.xgmi_one_shot_max);
  js += ",\"xgmi_tune\":{\"ran\":" + std::string(xtune.ran ? "true" : "false") +
        ",\"seconds\":" + jnum(xtune.seconds) + ",\"table\":" + xtune.table + "}";
  js += ",\"rccl_peak_busbw_bf16_GBps\":" + jnum(rccl_peak_bf16) +
        ",\"xgmi_peak_busbw_bf16_GBps\":" + jnum(xgmi_peak_bf16);
  js += ",\"host_prep\":{\"numa_balancing\":" + std::to_string(hp.numa_balancing) +
        ",\"memlock_unlimited\":" + (hp.memlock_unlimited ? "true" : "false") +
        ",\"iommu_pt\":" + (hp.iommu_pt ? "true" : "false") + "}";
  js += ",\"xgmi_p2p_GBps\":" + p2p_json(p2p) + ",\"xgmi_p2p_min_GBps\":" +
        (p2p.n > 0 ? jnum(p2p.min_gbps) : std::string("null")) +
        ",\"xgmi_p2p_bad_pairs\":" + std::to_string(p2p.bad_pairs);
  double t_gemm = t_hip, t_hbm = t_hip;
  for (auto& r : res) { t_gemm = std::max(t_gemm, r.t_gemm); t_hbm = std::max(t_hbm, r.t_hbm); }
  js += ",\"phases_s\":{\"process_start_to_hip_init\":" + jnum(t_hip - t_start) +
        ",\"gemm_done\":" + jnum(t_gemm - t_start) + ",\"hbm_done\":" + jnum(t_hbm - t_start) +
        ",\"rccl_done\":" + jnum(t_rccl - t_start) + ",\"end\":" + jnum(t_end - t_start) + "}";
  js += ",\"start_epoch_s\":" + jnum(t_start) + ",\"end_epoch_s\":" + jnum(t_end);
  js += ",\"failures\":[";
  for (size_t i = 0; i < g_failures.size(); ++i) js += (i ? "," : "") + jstr(g_failures[i]);
  js += "]";
  if (!o.pushgateway.empty()) js += ",\"pushgateway\":" + jstr(push_status);
  js += "}";
  (void)t_local;
  std::printf("%s\n", js.c_str());
  if (!o.out.empty()) {
    std::ofstream f(o.out);
    f << js << "\n";
  }
  if (!o.termination_log.empty()) {
    // Kubernetes surfaces this file as the pod's termination message
    // (truncated at 4 KiB): the one-line verdict an operator sees first.
    std::string t = "{\"passed\":" + std::string(passed ? "true" : "false") +
                    (node.empty() ? std::string() : ",\"node\":" + jstr(node)) +
                    ",\"n_gpus\":" + std::to_string(n) + ",\"gemm_tflops_aggregate\":" + jnum(agg) +
                    ",\"rccl_peak_busbw_GBps\":" + jnum(peak_rccl) +
                    ",\"seconds\":" + jnum(t_end - t_start);
    if (o.xcd_sweep) {  // the lowest min / median of a gated cell over all GPUs
      double worst = 1e300;
      for (auto& r : res)
        for (auto& c : r.xcd_cells)
          if (c.gated) worst = std::min(worst, c.sum.min_over_median);
      t += ",\"xcd_sweep_min_over_median\":" + (worst < 1e300 ? jnum(worst) : std::string("null"));
    }
    t += ",\"failures\":[";
    for (size_t i = 0; i < g_failures.size() && t.size() < 3500; ++i)
      t += (i ? "," : "") + jstr(g_failures[i].substr(0, 200));
    t += "]}";
    std::ofstream f(o.termination_log);
    f << t << "\n";
  }
  if (!o.prom_out.empty()) {
    std::ofstream f(o.prom_out);
    f << prom_text;
  }
  return passed ? 0 : 1;
}
