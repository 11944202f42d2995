// amdgpu-validate K13: fused attention forward with exact answers (ntm/attn.hpp, host side in
// ntm/attn_plan.hpp). On for NTM_ATTN_CHECK=1. Three sub-tests:
//   1. exact: integer-valued inputs (make_exact, scale_log2 = 1) of kExact*: 384 workgroups, a
//      ragged last query tile and key step, causal and not; O, m and l bitwise against
//      attn_reference_kernel (no matrix, no cross-lane instruction). The launch is repeated,
//      each time compared, until the CU table has shown every CU or kMaxLaunches are spent
//      (a cap, not a retry);
//   2. dense: uniform bf16, causal and not; every element within 2^-7 a + 2^-20 of the
//      reference's fp32 O, a = sum p |v| / l from the reference (profiles/attn/README.md);
//   3. timed: B 4, Hq 32, Hkv 8, Sq = Sk = 4096, causal: the settle of the GEMM stages, then
//      o.iters launches. The rate is reported, never judged.
// A failure names the XCD, SE, SH and CU of the workgroup that computed the tile.
// corrupt_attn: bit 3 of one O element of the LAST GPU's first exact launch is flipped
// before the compare.
#include <set>

#include "check.hpp"
#include "ntm/attn_plan.hpp"
#include "ntm/mx_plan.hpp"  // Mismatch: the record ntm_attn_compare fills

namespace ntm::job {

bool run_attn(const GpuCtx& g, AttnResult& r) {
  namespace at = ntm::attn;
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  const auto t_begin = Clock::now();
  r.ran = true;
  constexpr int kEB = 4, kEHq = 32, kEHkv = 8, kESq = 300, kESk = 333;  // exact
  constexpr int kDB = 2, kDHq = 4, kDHkv = 2, kDS = 320;                // dense
  constexpr int kTB = 4, kTHq = 32, kTHkv = 8, kTS = 4096;              // timed
  constexpr int D = at::kHeadDim;
  const size_t q_elems = (size_t)kTB * kTHq * kTS * D, kv_elems = (size_t)kTB * kTHkv * kTS * D;
  const size_t small_elems = (size_t)kEB * kEHq * kESq * D, small_rows = (size_t)kEB * kEHq * kESq;
  static_assert((size_t)kDB * kDHq * kDS <= (size_t)kEB * kEHq * kESq, "the dense results fit the exact buffers");
  int cus = 0;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  r.cus = (uint32_t)cus;

  uint16_t *dQ = nullptr, *dK = nullptr, *dV = nullptr, *dO = nullptr, *dRefO = nullptr;
  float *dM = nullptr, *dL = nullptr, *dRefM = nullptr, *dRefL = nullptr, *dO32 = nullptr, *dA = nullptr;
  unsigned* dTable = nullptr;
  ntm::mx::Mismatch init, got, *dres = nullptr;
  ntm::mx::mismatch_init(init);
  CK(hipMalloc(&dQ, q_elems * 2));
  CK(hipMalloc(&dO, q_elems * 2));
  CK(hipMalloc(&dK, kv_elems * 2));
  CK(hipMalloc(&dV, kv_elems * 2));
  CK(hipMalloc(&dRefO, small_elems * 2));
  CK(hipMalloc(&dO32, small_elems * 4));
  CK(hipMalloc(&dA, small_elems * 4));
  for (float** p : {&dM, &dL, &dRefM, &dRefL}) CK(hipMalloc(p, small_rows * 4));
  const size_t table_bytes = ntm_attn_table_bytes(kTB, kTHq, kTS);
  CK(hipMalloc(&dTable, table_bytes));
  CK(hipMalloc(&dres, sizeof init));

  // ---- 1. exact
  {
    const at::Inputs in = at::make_exact(kEB, kEHq, kEHkv, kESq, kESk, 0x4B3Du + (unsigned)dev);
    const size_t qh = (size_t)kESq * D, kh = (size_t)kESk * D;
    const size_t q_last = ((size_t)kEB * kEHq - 1) * qh, k_last = ((size_t)kEB * kEHkv - 1) * kh;
    CK(hipMemcpyAsync(dQ, in.qb.data(), in.qb.size() * 2, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dK, in.kb.data(), in.kb.size() * 2, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dV, in.vb.data(), in.vb.size() * 2, hipMemcpyHostToDevice, s));
    const size_t wgs = (size_t)at::grid(kEB, kEHq, kESq);
    std::vector<uint32_t> table(wgs * at::kTableWords);
    for (int causal = 0; causal < 2; ++causal) {
      const char* sub = causal ? "exact causal" : "exact";
      // the predicate on the first and the last (batch, head): the generator is the same for all
      if (!at::attn_exact(in.q.data(), in.k.data(), in.v.data(), 1, 1, 1, kESq, kESk, causal) ||
          !at::attn_exact(in.q.data() + q_last, in.k.data() + k_last, in.v.data() + k_last, 1, 1, 1, kESq, kESk, causal)) {
        r.failures.push_back("gpu" + std::to_string(dev) + ": attn " + sub + ": the generated inputs break attn_exact");
        continue;
      }
      CK(ntm_attn_reference(dQ, dK, dV, dRefO, nullptr, nullptr, dRefM, dRefL, kEB, kEHq, kEHkv, kESq, kESk, causal,
                            1.0f, s));
      std::set<uint32_t> seen;
      for (int launch = 0; launch < at::kMaxLaunches && (launch == 0 || (int)seen.size() < cus); ++launch) {
        CK(hipMemsetAsync(dO, 0xFF, small_elems * 2, s));
        CK(hipMemsetAsync(dTable, 0, wgs * at::kTableWords * 4, s));
        CK(ntm_attn_fwd(dQ, dK, dV, dO, dM, dL, dTable, kEB, kEHq, kEHkv, kESq, kESk, causal, 1.0f, s));
        if (launch == 0 && !causal && g.fault("corrupt_attn") && !flip_bits(dO + small_elems / 2 + 5, 2, 1u << 3, &s))
          return false;
        CK(hipMemcpyAsync(table.data(), dTable, table.size() * 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        for (size_t w = 0; w < wgs; ++w) seen.insert(ntm::cus::cu_key(table[2 * w], table[2 * w + 1]));
        ++r.launches;
        struct Pair { const char* what; const void *e, *g; size_t words; };
        const Pair pairs[3] = {{"O", dRefO, dO, small_elems / 2}, {"m", dRefM, dM, small_rows}, {"l", dRefL, dL, small_rows}};
        for (const Pair& p : pairs) {
          CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s));
          CK(ntm_attn_compare(p.e, p.g, p.words, dres, s));
          CK(hipMemcpyAsync(&got, dres, sizeof got, hipMemcpyDeviceToHost, s));
          CK(hipStreamSynchronize(s));
          if (!got.count) continue;
          r.exact_bad += got.count;
          const std::string head = "gpu" + std::to_string(dev) + ": attn " + sub + " " + p.what + ":";
          bool have = false;  // one line per sub-test and output: the first launch that shows it
          for (auto& f : r.failures) have = have || f.compare(0, head.size(), head) == 0;
          if (!have)
            r.failures.push_back(at::failure_message(dev, sub, p.what, got.count, got.first_index, got.expected, got.got,
                                                     kEHq, kESq, table.data()));
        }
      }
      r.cus_covered = std::max(r.cus_covered, (uint32_t)seen.size());
    }
  }

  // ---- 2. dense
  {
    const size_t nq = (size_t)kDB * kDHq * kDS * D, nk = (size_t)kDB * kDHkv * kDS * D;
    CK(ntm_fill_uniform_bf16(dQ, nq, 0xA770 + 3 * dev, 1.0f, s));
    CK(ntm_fill_uniform_bf16(dK, nk, 0xA771 + 3 * dev, 1.0f, s));
    CK(ntm_fill_uniform_bf16(dV, nk, 0xA772 + 3 * dev, 1.0f, s));
    std::vector<uint16_t> ho(nq);
    std::vector<float> h32(nq), ha(nq);
    std::vector<uint32_t> table((size_t)at::grid(kDB, kDHq, kDS) * at::kTableWords);
    for (int causal = 0; causal < 2; ++causal) {
      const char* sub = causal ? "dense causal" : "dense";
      CK(hipMemsetAsync(dO, 0xFF, nq * 2, s));
      CK(ntm_attn_fwd(dQ, dK, dV, dO, nullptr, nullptr, dTable, kDB, kDHq, kDHkv, kDS, kDS, causal,
                      at::default_scale_log2(), s));
      CK(ntm_attn_reference(dQ, dK, dV, nullptr, dO32, dA, nullptr, nullptr, kDB, kDHq, kDHkv, kDS, kDS, causal,
                            at::default_scale_log2(), s));
      CK(hipMemcpyAsync(ho.data(), dO, nq * 2, hipMemcpyDeviceToHost, s));
      CK(hipMemcpyAsync(h32.data(), dO32, nq * 4, hipMemcpyDeviceToHost, s));
      CK(hipMemcpyAsync(ha.data(), dA, nq * 4, hipMemcpyDeviceToHost, s));
      CK(hipMemcpyAsync(table.data(), dTable, table.size() * 4, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      unsigned long long bad = 0;
      size_t first = 0;
      for (size_t x = 0; x < nq; ++x) {
        uint32_t u = (uint32_t)ho[x] << 16;
        float v;
        std::memcpy(&v, &u, 4);
        const float err = std::fabs(v - h32[x]);
        if (ha[x] > 0 && err / ha[x] > r.dense_worst) r.dense_worst = err / ha[x];
        if (!(err <= at::tolerance(ha[x])) && bad++ == 0) first = x;
      }
      if (bad) {
        r.dense_bad += bad;
        char num[96];
        uint32_t u = (uint32_t)ho[first] << 16;
        float v;
        std::memcpy(&v, &u, 4);
        std::snprintf(num, sizeof num, "error %.3e above 2^-7 a + 2^-20 = %.3e; ", (double)std::fabs(v - h32[first]),
                      (double)at::tolerance(ha[first]));
        at::Where w = at::locate("O", first / 2, kDHq, kDS);
        w.col = (long long)(first % D);
        r.failures.push_back("gpu" + std::to_string(dev) + ": attn " + sub + " O: " + at::where_text(w, table.data()) +
                             ": " + num + std::to_string(bad) + " beyond");
      }
    }
  }

  // ---- 3. timed
  {
    CK(ntm_fill_uniform_bf16(dQ, q_elems, 0xA780 + 3 * dev, 1.0f, s));
    CK(ntm_fill_uniform_bf16(dK, kv_elems, 0xA781 + 3 * dev, 1.0f, s));
    CK(ntm_fill_uniform_bf16(dV, kv_elems, 0xA782 + 3 * dev, 1.0f, s));
    auto fwd = [&] {
      return ntm_attn_fwd(dQ, dK, dV, dO, nullptr, nullptr, nullptr, kTB, kTHq, kTHkv, kTS, kTS, 1, at::default_scale_log2(), s);
    };
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float ms = 0;
    if (!settle(s, o.settle_s, fwd) || !timed_ms(s, e0, e1, o.iters, ms, fwd)) return false;
    r.tflops = ms > 0 ? at::flops(kTB, kTHq, kTS, kTS, 1) / (ms / o.iters * 1e-3) / 1e12 : 0;
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
  }
  for (void* p : {(void*)dQ, (void*)dK, (void*)dV, (void*)dO, (void*)dRefO, (void*)dO32, (void*)dA, (void*)dM, (void*)dL,
                  (void*)dRefM, (void*)dRefL, (void*)dTable, (void*)dres})
    CK(hipFree(p));
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
