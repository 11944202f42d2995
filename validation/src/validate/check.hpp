// amdgpu-validate: what the GPU-side sources share - the per-GPU context, CK, fail,
// the clocks, the one timed-loop helper and the one fault-injection helper.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <mutex>
#include <string>
#include <vector>

#include "ntm/abi.h"

#include "host.hpp"
#include "options.hpp"
#include "report.hpp"

namespace ntm::job {

using Clock = std::chrono::steady_clock;

inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

inline double median3(double a, double b, double c) { return std::max(std::min(a, b), std::min(std::max(a, b), c)); }

// the run's failures: a check that cannot go on (a HIP error, a wrong device) says so
// here and returns false; verdicts on results are collected later (gpu_failures)
inline std::mutex g_fail_mu;
inline std::vector<std::string> g_failures;
inline void fail(const std::string& why) {
  std::lock_guard<std::mutex> l(g_fail_mu);
  g_failures.push_back(why);
}

// A failed HIP call ends the check: nothing is freed, the process is about to exit 1.
#define CK(expr)                                                              \
  do {                                                                        \
    hipError_t _e = (hipError_t)(expr);                                       \
    if (_e != hipSuccess) {                                                   \
      fail(std::string("HIP error ") + hipGetErrorString(_e) + " at " #expr); \
      return false;                                                           \
    }                                                                         \
  } while (0)

// one GPU's thread: its device, whether fault injection acts on it (the LAST GPU),
// the options and the stream every check of this GPU runs on
struct GpuCtx {
  int dev;
  bool last;
  const Opts& o;
  hipStream_t s;
  bool fault(const char* kind) const { return last && o.fault == kind; }
};

// Untimed clock-settle pre-warm: a cold MI355X runs the first launches at boost
// clock, overshoots its power limit a few ms in and throttles, and needs ~25 ms
// of sustained load to settle (profiles/r2_bench/). Timing 5 launches after a
// cold start measures that transient, not the kernel.
template <class Launch>
bool settle(hipStream_t s, double seconds, Launch&& launch) {
  const auto t0 = Clock::now();
  do {
    for (int i = 0; i < 8; ++i) CK(launch());
    CK(hipStreamSynchronize(s));
  } while (since(t0) < seconds);
  return true;
}

// The milliseconds `n` calls of `body` take on `s`: record e0, the calls, record e1,
// `in_flight` on the host while the work runs, synchronize e1, elapsed.
template <class Body, class InFlight>
bool timed_ms(hipStream_t s, hipEvent_t e0, hipEvent_t e1, int n, float& ms, Body&& body, InFlight&& in_flight) {
  CK(hipEventRecord(e0, s));
  for (int i = 0; i < n; ++i) CK(body());
  CK(hipEventRecord(e1, s));
  in_flight();
  CK(hipEventSynchronize(e1));
  CK(hipEventElapsedTime(&ms, e0, e1));
  return true;
}
template <class Body>
bool timed_ms(hipStream_t s, hipEvent_t e0, hipEvent_t e1, int n, float& ms, Body&& body) {
  return timed_ms(s, e0, e1, n, ms, body, [] {});
}

// Fault injection: read the `width`-byte word (2 or 4) at device address `p`, XOR
// `mask` into it, write it back. On `*s` when a stream is given (copy, synchronize,
// copy), with blocking copies otherwise.
inline bool flip_bits(void* p, size_t width, uint32_t mask, const hipStream_t* s) {
  uint32_t w = 0;
  if (s) {
    CK(hipMemcpyAsync(&w, p, width, hipMemcpyDeviceToHost, *s));
    CK(hipStreamSynchronize(*s));
  } else {
    CK(hipMemcpy(&w, p, width, hipMemcpyDeviceToHost));
  }
  w ^= mask;
  if (s) CK(hipMemcpyAsync(p, &w, width, hipMemcpyHostToDevice, *s));
  else CK(hipMemcpy(p, &w, width, hipMemcpyHostToDevice));
  return true;
}

// the opt-in checks, one source file each
bool run_hbm_test(const GpuCtx& g, HbmTestResult& r);    // K4, hbm_test.cpp
bool run_cu_sweep(const GpuCtx& g, CuSweepResult& r);    // K5, cu_sweep.cpp
bool run_host_link(const GpuCtx& g, HostLinkResult& r);  // K6, host_link.cpp
bool run_mx_check(const GpuCtx& g, MxResult& r);         // K7, mx_check.cpp
bool run_xcd_sweep(const GpuCtx& g, XcdSweepResult& r);  // K8, xcd_sweep.cpp
bool run_atomics(const GpuCtx& g, AtomicsResult& r);     // K9, atomics.cpp
bool run_mcore(const GpuCtx& g, McoreResult& r);         // K10, mcore.cpp
bool run_mxq(const GpuCtx& g, MxqResult& r);             // K11, mxq.cpp
bool run_wave(const GpuCtx& g, WaveResult& r);           // K12, wave.cpp
bool run_attn(const GpuCtx& g, AttnResult& r);           // K13, attn.cpp
bool run_pda(const GpuCtx& g, PdaResult& r);             // K14, pda.cpp

// K1 / K2 and the calls of the above on one GPU (gpu.cpp)
bool run_gpu(int dev, bool last, const Opts& o, GpuResult& r);

// C1 / C2 / C3 over all GPUs (collectives.hip)
bool run_rccl(const std::vector<int>& devs, const Opts& o, std::vector<CollRow>& rows);
bool run_xgmi(const std::vector<int>& devs, const Opts& o, std::vector<CollRow>& rows, XgmiTune& tune);
bool run_p2p(const std::vector<int>& devs, const Opts& o, P2pResult& r);

}  // namespace ntm::job
