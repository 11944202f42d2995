// amdgpu-validate K9: atomics and cross-XCD hand-off check (ntm/atomics.hpp, host side in
// ntm/atomics_plan.hpp). On for NTM_ATOMICS_CHECK=1. Three sub-tests on one GPU:
//   rmw      every op on a table of grid x 128 slots from 2 workgroups per CU, 16 operations
//            per thread (32 per slot), compared bitwise with the reference kernel's table;
//   ticket   8 heads, the same grid, 4 draws per thread, verified on the host;
//   handoff  one episode of 8 workgroups per CU, 4 rounds.
// Rates are reported, never judged. corrupt_atomic and stale_handoff act on the LAST GPU.
#include "check.hpp"
#include "ntm/atomics_plan.hpp"

namespace ntm::job {

bool run_atomics(const GpuCtx& g, AtomicsResult& r) {
  namespace at = ntm::atm;
  const int dev = g.dev;
  hipStream_t s = g.s;
  const auto t_begin = Clock::now();
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  const uint32_t cus = (uint32_t)prop.multiProcessorCount;
  const uint32_t xcds = std::max<uint32_t>(1, std::min<uint32_t>(cus / 32, at::kMaxXcds));
  r.ran = true;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  const unsigned long long seed = 0x4B39ull + (unsigned)dev;

  // ---- rmw
  const uint32_t grid = cus * 2, iters = 16;
  const uint64_t slots = (uint64_t)grid * 128, total = (uint64_t)grid * at::kThreads * iters;
  void *got = nullptr, *ref = nullptr;
  CK(hipMalloc(&got, slots * 8));
  CK(hipMalloc(&ref, slots * 8));
  std::vector<uint64_t> hgot(slots), href(slots);
  for (int op = 0; op < at::kOps; ++op) {
    unsigned long long max_abs = 1;
    while (max_abs < 255 && at::atomics_exact(op, total / slots, 2 * max_abs + 1)) max_abs = 2 * max_abs + 1;
    CK(ntm_atomics_rmw_launch(op, got, slots, grid, iters, seed, max_abs, s));  // untimed: warms the table up
    float ms = 0;
    if (!timed_ms(s, e0, e1, 1, ms, [&] { return ntm_atomics_rmw_launch(op, got, slots, grid, iters, seed, max_abs, s); }))
      return false;
    CK(ntm_atomics_rmw_reference_launch(op, ref, slots, grid, iters, seed, max_abs, s));
    CK(hipStreamSynchronize(s));
    if (op == at::kAddF32 && g.fault("corrupt_atomic") && !flip_bits((char*)got + (slots / 2) * 4, 4, 1u << 9, nullptr))
      return false;
    const size_t bytes = slots * at::slot_bytes(op);
    CK(hipMemcpy(hgot.data(), got, bytes, hipMemcpyDeviceToHost));
    CK(hipMemcpy(href.data(), ref, bytes, hipMemcpyDeviceToHost));
    const at::RmwSummary sum = at::summarize_rmw(op, hgot.data(), href.data(), slots, dev);
    r.ops.push_back({op, sum.bad_slots, ms > 0 ? (double)total / (ms * 1e6) : 0});
    r.failures.insert(r.failures.end(), sum.failures.begin(), sum.failures.end());
  }
  CK(hipFree(got));
  CK(hipFree(ref));

  // ---- ticket
  {
    const uint32_t heads = 8, titers = 4;
    const size_t claim_bytes = ntm_atomics_ticket_claim_bytes(heads, grid, titers);
    const size_t counter_bytes = ntm_atomics_counter_bytes(heads);
    void *counters = nullptr, *claim = nullptr;
    CK(hipMalloc(&counters, counter_bytes));
    CK(hipMalloc(&claim, claim_bytes));
    CK(ntm_atomics_ticket_launch(counters, claim, heads, grid, titers, at::kInjectOff, s));
    std::vector<uint32_t> hc(counter_bytes / 4), hclaim(claim_bytes / 4);
    CK(hipMemcpyAsync(hc.data(), counters, counter_bytes, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(hclaim.data(), claim, claim_bytes, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    const at::TicketSummary sum = at::summarize_tickets(hc.data(), hclaim.data(), heads,
                                                        at::tickets_per_head(heads, grid, titers),
                                                        grid * at::kThreads, titers, dev);
    r.ticket_bad = sum.bad();
    r.failures.insert(r.failures.end(), sum.failures.begin(), sum.failures.end());
    CK(hipFree(counters));
    CK(hipFree(claim));
  }

  // ---- handoff
  {
    const uint32_t e = 8, episodes = std::max<uint32_t>(cus, 1), rounds = 4, n = episodes * e;
    void *slabs = nullptr, *counters = nullptr, *drec = nullptr;
    CK(hipMalloc(&slabs, at::handoff_slab_bytes(episodes, e)));
    CK(hipMalloc(&counters, at::handoff_counter_bytes(episodes)));
    CK(hipMalloc(&drec, (size_t)rounds * n * sizeof(at::Record)));
    CK(ntm_atomics_handoff_init(slabs, episodes, e, seed, 0, s));
    const uint32_t stale_wg = g.fault("stale_handoff") ? (episodes / 2) * e + 1 : at::kInjectOff;
    uint32_t round = 0;
    float ms = 0;
    if (!timed_ms(s, e0, e1, (int)rounds, ms, [&] {
          ++round;
          return ntm_atomics_handoff_launch(slabs, counters, (at::Record*)drec + (size_t)(round - 1) * n, episodes, e,
                                            seed, round, round == rounds ? stale_wg : at::kInjectOff, s);
        }))
      return false;
    std::vector<at::Record> recs((size_t)rounds * n);
    CK(hipMemcpy(recs.data(), drec, recs.size() * sizeof(at::Record), hipMemcpyDeviceToHost));
    const at::HandoffSummary sum = at::summarize_handoff(recs.data(), recs.size(), episodes, e, xcds, rounds, dev);
    r.handoff_bad_words = sum.bad_words;
    r.handoff_stale_words = sum.stale_words;
    r.xcd_pairs_covered = sum.xcd_pairs_covered;
    r.xcds = xcds;
    r.pairs.assign(sum.pairs.begin(), sum.pairs.end());
    r.episodes_per_s = ms > 0 ? (double)episodes * rounds / (ms * 1e-3) : 0;
    r.failures.insert(r.failures.end(), sum.failures.begin(), sum.failures.end());
    CK(hipFree(slabs));
    CK(hipFree(counters));
    CK(hipFree(drec));
  }
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
