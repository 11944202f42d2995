// amdgpu-validate: the collectives over all GPUs of the Job - C1 (RCCL all-reduce
// sweep), C2 (the hand-written all-reduce over peer-mapped xGMI) and C3 (the
// per-link pull matrix). The one source of the binary's own with device code: the
// pattern kernels that fill the all-reduce inputs and check the result.
#include <rccl/rccl.h>

#include <cmath>
#include <cstring>

#include "ntm/common.hpp"

#include "check.hpp"
#include "sweeps.hpp"

namespace {  // global, as ever: the kernels keep their symbol names

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

}  // namespace

namespace ntm::job {
namespace {

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

}  // namespace

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
      const double sec = since(t0) / iters;
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

// C3: per-link xGMI check. For every ordered pair (dst <- src), GPU dst pulls
// --p2p-mib MiB out of GPU src's HBM through the peer mapping with the K2 copy
// kernel, so every read crosses the one dst-src link; timed with events on
// dst, pairs one at a time, then a sample window is compared byte for byte.
// A degraded or miswired link is one cell of this matrix, where a ring
// all-reduce's busbw only shows the slowest ring. --p2p-loopback runs the same
// code on a single GPU as pair 0 <- 0 (a local copy) so the path is testable
// on a one-GPU box.
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
      float ms = 0;
      if (!timed_ms(st[d], e0[d], e1[d], iters, ms, [&] { return ntm_stream_copy(src[sidx], dst[d], bytes, st[d]); }))
        return false;
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

// C2 driver. Real mode: rank i on GPU devs[i] (peer access between all pairs,
// one launch per GPU). Simulated mode (--xgmi-sim N): all N ranks on devs[0]
// in one launch (rank = block / nblk), so the whole protocol - entry barrier,
// reduce-scatter, all-gather, exit barrier, epochs - runs on a one-GPU box
// through this same driver. Sizes: xgmi_sizes (512 B .. min(max, 1 GiB));
// <= --xgmi-one-shot-max (256 KiB) takes the one-shot kernel. The kernel
// synchronises the ranks itself (device-side entry barrier), so the timed
// loop launches back to back with no host sync.
bool run_xgmi(const std::vector<int>& devs, const Opts& o, std::vector<CollRow>& rows,
              XgmiTune& tune) {
  const bool sim = o.xgmi_sim > 0;
  const int n = sim ? o.xgmi_sim : (int)devs.size();
  if (n < 1 || n > NTM_XGMI_MAX_RANKS) return true;
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
      return since(t0) / calls;
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
    tune.seconds = since(t_tune);
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
    const double sec = since(t0) / iters;
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

}  // namespace ntm::job
