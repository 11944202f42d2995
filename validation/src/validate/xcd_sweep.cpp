// amdgpu-validate K8: per-XCD sweep (ntm/xcd_sweep.hpp, host side in ntm/xcd_sweep_plan.hpp).
// One buffer of xcds x xcd-sweep-mib, filled once with K4's hash pattern; the l2 and
// mall levels read its first xcds x 1 MiB / 16 MiB (the pattern depends on the position
// alone). Per level: mode alone (one launch per XCD) and together (one launch). Every
// cell runs once untimed with a first guess of the passes, which warms it up and sizes
// the passes for spans of at least 100 us, then once for the record. slow_xcd and
// corrupt_xcd act on the LAST GPU.
#include "check.hpp"
#include "ntm/hbm_test_plan.hpp"
#include "ntm/xcd_sweep_plan.hpp"

namespace ntm::job {

bool run_xcd_sweep(const GpuCtx& g, XcdSweepResult& r) {
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  namespace xs = ntm::xcs;
  const auto t_begin = Clock::now();
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  const uint32_t xcds = std::min<uint32_t>(xs::xcds_expected((uint32_t)prop.multiProcessorCount), xs::kMaxXcds);
  const std::string head = "gpu" + std::to_string(dev) + ": XCD sweep: ";
  r.ran = true;
  r.xcds = xcds;
  r.mib = o.xcd_sweep_mib;
  r.ratio = o.xcd_ratio;
  if (xcds < 1) {
    r.failures.push_back(head + "the device reports " + std::to_string(prop.multiProcessorCount) +
                             " CUs, fewer than one XCD");
    return true;
  }
  const uint32_t hbm_mib = (uint32_t)o.xcd_sweep_mib;
  const size_t bytes = (size_t)xcds * hbm_mib << 20;
  const uint32_t grid = xs::grid_of(xcds, xs::kWgPerCu), mfma_grid = xs::grid_of(xcds, 1);
  const uint32_t all = xs::full_mask(xcds);
  const unsigned long long seed = 0x4B38ull + (unsigned)dev;
  const int slow_xcd = g.fault("slow_xcd") ? (xcds > 5 ? 5 : 0) : xs::kSlowOff;
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
    if (level == xs::kLevelHbm && g.fault("corrupt_xcd")) {
      // one bit of a word in the middle of XCD 3's hbm slice (the last XCD's on a smaller device)
      const size_t off = ((size_t)std::min<uint32_t>(3, xcds - 1) * hbm_mib << 20) + ((size_t)hbm_mib << 19) + 40;
      if (!flip_bits((char*)buf + off, 4, 1u << 9, nullptr)) return false;
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
      for (auto& f : c.sum.failures) r.failures.push_back(f);
      r.cells.push_back(std::move(c));
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
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
