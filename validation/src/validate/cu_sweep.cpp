// amdgpu-validate K5: per-CU compute sweep (ntm/cu_sweep.hpp, host side in ntm/cu_sweep_plan.hpp).
// Launches of 4 workgroups per CU until every CU ran one, at most kMaxLaunches: a CU
// that never ran fails the check. bad_cu: a clean launch learns the CU keys, then the
// sweep runs with the middle key of the sorted list as the CU that flips a bit.
#include "check.hpp"
#include "ntm/cu_sweep_plan.hpp"

namespace ntm::job {

bool run_cu_sweep(const GpuCtx& g, CuSweepResult& r) {
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  namespace cu = ntm::cus;
  const auto t_begin = Clock::now();
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  const uint32_t cus = (uint32_t)prop.multiProcessorCount;
  const unsigned grid = cu::kGridPerCu * cus;
  const int lds = ntm_cu_sweep_max_lds_bytes(dev);
  r.ran = true;
  r.lds_bytes = lds;
  if (lds < 16 || cus == 0) {
    r.failures.push_back("gpu" + std::to_string(dev) + ": CU sweep: cannot read the device's LDS size or CU count");
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
  if (g.fault("bad_cu")) {
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
  r.sum = sweep.summary(cus);
  const std::string verdict = cu::failure_message(dev, r.sum);  // empty = clean
  if (!verdict.empty()) r.failures.push_back(verdict);
  CK(hipFree(dexp));
  CK(hipFree(drec));
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
