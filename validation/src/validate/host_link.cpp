// amdgpu-validate K6: host-link (PCIe) check (ntm/host_link.hpp, host side in ntm/host_link_plan.hpp).
// One pinned buffer and one HBM buffer of --host-link-mib: push the HASH pattern
// (device->host), pull and verify on the device (host->device), both at once on
// two streams over the two halves, hipMemcpyAsync both ways on the same buffers
// (the path frameworks use: the reference for the kernels' rate), then the
// pointer chase. Rates are medians of 3, timed with events. The healthy path does
// no CPU work on the data; on a mismatch the host re-checks the pinned buffer to
// say which direction went wrong. corrupt_host_link: the host flips one bit of
// the pinned buffer between push and pull.
#include "check.hpp"
#include "ntm/hbm_test_plan.hpp"
#include "ntm/host_link_plan.hpp"

namespace ntm::job {

bool run_host_link(const GpuCtx& g, HostLinkResult& r) {
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  namespace hl = ntm::hostlink;
  namespace hb = ntm::hbm;
  const auto t_begin = Clock::now();
  const std::string d = "gpu" + std::to_string(dev) + ": ";
  const size_t bytes = (size_t)o.host_link_mib << 20;
  const size_t half = bytes / 2;  // a multiple of 16: bytes is a multiple of 1 MiB
  constexpr int kPat = hb::kPatternHash;
  const unsigned long long seed = 0x4B36ull + (unsigned)dev;
  r.ran = true;
  r.mib = o.host_link_mib;
  char bus[32] = {0};
  if (hipDeviceGetPCIBusId(bus, sizeof bus, dev) != hipSuccess) {
    (void)hipGetLastError();
    bus[0] = 0;
  }
  void *hbuf = nullptr, *dbuf = nullptr;
  if (hipHostMalloc(&hbuf, bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();  // no pinned memory (RLIMIT_MEMLOCK, host RAM): a verdict, no HIP failure
    r.failures.push_back(d + "host link: cannot pin " + std::to_string(o.host_link_mib) + " MiB of host memory");
    r.seconds = since(t_begin);
    return true;
  }
  r.pin_s = since(t_begin);
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
    if (!timed_ms(s, e0, e1, 1, ms, [&] { return ntm_host_link_push(hbuf, bytes, 0, kPat, seed, 0, 0, s); },
                  [&] { if (i == 2 && bus[0]) r.pcie = hl::read_link_state("/sys", bus); }))
      return false;
    t[i] = ms;
  }
  r.d2h_gbps = bytes / (median3(t[0], t[1], t[2]) * 1e-3) / 1e9;
  if (g.fault("corrupt_host_link"))
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
      r.bad_words = hres.bad_words;
      r.bad_bits = hres.bad_bits_or;
      // which direction: is the pinned buffer itself wrong?
      hb::PatternResult host_res;
      const bool host_bad = hl::host_check(hbuf, bytes, 0, kPat, seed, false, host_res) != 0;
      r.failures.push_back(
          hl::data_failure_message(dev, host_bad ? hl::kDirPush : hl::kDirPull, host_bad ? host_res : hres));
    }
  }
  // a stage cut short reports its first pull
  r.h2d_gbps = bytes / ((pulls == 3 ? median3(t[0], t[1], t[2]) : t[0]) * 1e-3) / 1e9;
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
    r.duplex_gbps = 2.0 * half / (median3(t[0], t[1], t[2]) * 1e-3) / 1e9;
    CK(hipMemcpy(&hres, dres, sizeof hres, hipMemcpyDeviceToHost));
    if (hres.bad_words) {
      r.bad_words = hres.bad_words;
      r.bad_bits = hres.bad_bits_or;
      r.failures.push_back(hl::data_failure_message(dev, "duplex host->device read", hres));
    }
    // hipMemcpyAsync on the same buffers, both ways
    for (int dir = 0; dir < 2; ++dir) {
      for (int i = 0; i < 3; ++i) {
        if (!timed_ms(s, e0, e1, 1, ms, [&] {
              return dir == 0 ? hipMemcpyAsync(dbuf, hbuf, bytes, hipMemcpyHostToDevice, s)
                              : hipMemcpyAsync(hbuf, dbuf, bytes, hipMemcpyDeviceToHost, s);
            }))
          return false;
        t[i] = ms;
      }
      (dir == 0 ? r.h2d_copy_gbps : r.d2h_copy_gbps) =
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
        r.failures.push_back(d + "host link chase ended at slot " + std::to_string(out[0]) + " after " +
                             std::to_string(out[2]) + " hops, expected slot " + std::to_string(want) +
                             " after " + std::to_string(hl::kChaseHops));
      else
        r.latency_us = (double)out[1] / khz * 1e3 / hl::kChaseHops;
    }
    // the floor: per direction, on the faster of kernel and hipMemcpyAsync (a degraded link caps both)
    if (o.host_link_floor_gbps > 0) {
      const double h2d = r.h2d_best(), d2h = r.d2h_best();
      if (h2d < o.host_link_floor_gbps)
        r.failures.push_back(hl::rate_failure_message(dev, "host->device", h2d, o.host_link_floor_gbps, r.pcie));
      if (d2h < o.host_link_floor_gbps)
        r.failures.push_back(hl::rate_failure_message(dev, "device->host", d2h, o.host_link_floor_gbps, r.pcie));
    }
  }
  r.xfer_s = since(t_xfer);
  const auto t_free = Clock::now();
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  CK(hipStreamDestroy(s2));
  CK(hipFree(dchase));
  CK(hipFree(dres));
  CK(hipFree(dbuf));
  CK(hipHostFree(hbuf));
  r.free_s = since(t_free);
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
