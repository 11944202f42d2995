// amdgpu-validate K4: HBM pattern test (ntm/hbm_pattern.hpp, plan in ntm/hbm_test_plan.hpp).
// Allocates the plan's chunks (a failed hipMalloc ends the list), then per pass:
// write ADDR / verify + invert in place / verify inverted / write HASH (seed =
// pass) / verify. Every chunk of a step is enqueued back to back; the one error
// record is read once per step. The first step that finds a bad word ends the test.
#include "check.hpp"
#include "ntm/hbm_test_plan.hpp"

namespace ntm::job {

bool run_hbm_test(const GpuCtx& g, HbmTestResult& r) {
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  namespace hb = ntm::hbm;
  const auto t_begin = Clock::now();
  size_t fre = 0, tot = 0;
  CK(hipMemGetInfo(&fre, &tot));
  const hb::TestPlan plan = hb::make_test_plan(fre, o.hbm_test_gb);
  r.ran = true;
  r.requested_gb = plan.requested_bytes / 1e9;
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
  r.alloc_s = since(t_begin);
  r.gb = tested / 1e9;
  if (chunks.empty()) {
    if (!plan.chunks.empty()) r.failures.push_back("gpu" + std::to_string(dev) + ": HBM pattern test: no chunk of " + std::to_string(plan.chunks[0]) + " bytes could be allocated");
    else r.failures.push_back("gpu" + std::to_string(dev) + ": HBM pattern test: no free HBM beyond the headroom");
    r.seconds = since(t_begin);
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
      r.bad_words = hres.bad_words;
      r.bad_bits = hres.bad_bits_or;
      r.failures.push_back(hb::failure_message(dev, name, hres));
    }
    return true;
  };
  for (int pass = 0; pass < o.hbm_test_passes && r.failures.empty(); ++pass) {
    if (!step("addr write", 0, hb::kPatternAddr, 0, 0)) return false;
    if (g.fault("corrupt_hbm") && !injected) {  // flip one bit in the last chunk
      injected = true;
      const Chunk& c = chunks.back();
      if (!flip_bits((char*)c.p + ((c.bytes / 2) & ~(size_t)15) + 4, 4, 1u << 13, nullptr)) return false;
    }
    if (!step("addr verify+invert", 2, hb::kPatternAddr, 0, 0)) return false;
    if (!r.failures.empty()) break;
    if (!step("addr inverted verify", 1, hb::kPatternAddr, 0, 1)) return false;
    if (!r.failures.empty()) break;
    if (!step("hash write", 0, hb::kPatternHash, (unsigned long long)pass, 0)) return false;
    if (!step("hash verify", 1, hb::kPatternHash, (unsigned long long)pass, 0)) return false;
  }
  r.steps = steps + "]";
  if (t_write > 0) r.write_gbps = b_write / t_write / 1e9;
  if (t_verify > 0) r.verify_gbps = b_verify / t_verify / 1e9;
  const auto t_free = Clock::now();
  CK(hipFree(dres));
  for (auto& c : chunks) CK(hipFree(c.p));
  r.free_s = since(t_free);
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
