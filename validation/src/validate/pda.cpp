// amdgpu-validate K14: paged-KV decode attention with exact answers (ntm/pda.hpp, host side in
// ntm/pda_plan.hpp). On for NTM_PDA_CHECK=1. Three sub-tests:
//   1. exact: B 24, Hq 32, Hkv 8, S 2 (384 workgroups), T 1 and then T 4; lengths of 1 .. 1500
//      that always include 1 (4 at T 4: a sequence holds its new tokens), 16, 17, 64, 65 and
//      1500; a shuffled pool with 2 prefix-shared pairs; the poison page, every unused page and
//      every page tail past len_b hold bf16 NaN. O, m and l bitwise against
//      attn_reference_kernel on the gathered keys of every sequence. The launch is repeated,
//      each time compared, until the CU table has shown every CU or K13's kMaxLaunches are
//      spent (a cap, not a retry). attn_exact is checked on the first and the last sequence;
//   2. dense: uniform bf16, B 8, Hq 8, Hkv 2, T 1, lengths around 320, S 3; every element within
//      attn::tolerance(a) of the reference's fp32 O (profiles/pda/README.md);
//   3. timed: B 32, Hq 32, Hkv 8, T 1, every length 8192, the default S: 1 GiB of K and V
//      together, past the Infinity Cache. kv_bytes / time is reported, never judged.
// A failure names sequence, head, token, column and the CUs of the row's split workgroups.
// corrupt_pda: bit 3 of one O element of the LAST GPU's first exact launch is flipped before
// the compare.
#include <set>

#include "check.hpp"
#include "ntm/mx_plan.hpp"  // Mismatch: the record ntm_attn_compare fills
#include "ntm/pda_plan.hpp"

namespace ntm::job {

bool run_pda(const GpuCtx& g, PdaResult& r) {
  namespace at = ntm::attn;
  namespace pd = ntm::pda;
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  const auto t_begin = Clock::now();
  r.ran = true;
  constexpr int kEB = 24, kEHq = 32, kEHkv = 8, kES = 2, kEMaxLen = 1500;  // exact
  constexpr int kDB = 8, kDHq = 8, kDHkv = 2, kDS = 3;                     // dense
  constexpr int kTB = 32, kTHq = 32, kTHkv = 8, kTLen = 8192;              // timed
  constexpr int D = at::kHeadDim;
  constexpr size_t page_elems = (size_t)pd::kPage * D;
  int cus = 0;
  CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  r.cus = (uint32_t)cus;
  const int timed_splits = pd::pda_splits(kTB, kTHkv, kTLen, cus);
  r.splits = (uint32_t)timed_splits;

  // the lengths of the exact sub-test: the first four long (they are the prefix-shared pairs),
  // the last six the fixed edge lengths
  const uint32_t seed = 0x14DAu + (unsigned)dev;
  std::vector<int32_t> lens1(kEB);
  for (int b = 0; b < kEB; ++b) {
    const uint32_t h = at::attn_hash(seed, 7, (uint32_t)b) >> 8;
    lens1[(size_t)b] = b < 4 ? 256 + (int)(h % (kEMaxLen - 255)) : 1 + (int)(h % kEMaxLen);
  }
  const int fixed[6] = {1, 16, 17, 64, 65, kEMaxLen};
  for (int i = 0; i < 6; ++i) lens1[(size_t)(kEB - 6 + i)] = fixed[i];
  size_t keys = 0;
  for (int32_t n : lens1) keys += (size_t)(n < pd::kMaxT ? pd::kMaxT : n);

  const std::vector<int32_t> timed_lens(kTB, kTLen);
  const pd::PageTable timed_pt = pd::make_page_table(timed_lens, seed, 0);
  const size_t pool_elems = (size_t)timed_pt.pages * kTHkv * page_elems;
  const size_t q_elems = (size_t)kEB * kEHq * pd::kMaxT * D, q_rows = (size_t)kEB * kEHq * pd::kMaxT;
  static_assert((size_t)kTB * kTHq <= (size_t)kEB * kEHq * pd::kMaxT && (size_t)kDB * kDHq <= (size_t)kEB * kEHq,
                "the dense and timed results fit the exact buffers");
  const size_t gathered_elems = keys * kEHkv * D;
  const size_t ws_bytes = std::max(pd::workspace_bytes(kEB, kEHkv, kES), pd::workspace_bytes(kTB, kTHkv, timed_splits));
  const size_t table_bytes = std::max(pd::table_bytes(kEB, kEHkv, kES), pd::table_bytes(kTB, kTHkv, timed_splits));

  uint16_t *dQ = nullptr, *dKp = nullptr, *dVp = nullptr, *dKg = nullptr, *dVg = nullptr, *dO = nullptr, *dRefO = nullptr;
  float *dM = nullptr, *dL = nullptr, *dRefM = nullptr, *dRefL = nullptr, *dO32 = nullptr, *dA = nullptr;
  int32_t *dBt = nullptr, *dLens = nullptr;
  void* dWs = nullptr;
  unsigned* dTable = nullptr;
  ntm::mx::Mismatch init, got, *dres = nullptr;
  ntm::mx::mismatch_init(init);
  CK(hipMalloc(&dQ, q_elems * 2));
  CK(hipMalloc(&dO, q_elems * 2));
  CK(hipMalloc(&dRefO, q_elems * 2));
  CK(hipMalloc(&dO32, q_elems * 4));
  CK(hipMalloc(&dA, q_elems * 4));
  CK(hipMalloc(&dKp, pool_elems * 2));
  CK(hipMalloc(&dVp, pool_elems * 2));
  CK(hipMalloc(&dKg, gathered_elems * 2));
  CK(hipMalloc(&dVg, gathered_elems * 2));
  for (float** p : {&dM, &dL, &dRefM, &dRefL}) CK(hipMalloc(p, q_rows * 4));
  CK(hipMalloc(&dBt, timed_pt.table.size() * 4));
  CK(hipMalloc(&dLens, (size_t)kTB * 4));
  CK(hipMalloc(&dWs, ws_bytes));
  CK(hipMalloc(&dTable, table_bytes));
  CK(hipMalloc(&dres, sizeof init));

  // One reference launch per sequence on its gathered keys (K13's layout, B 1, causal), into
  // the slices of the stacked reference outputs. `off[b]`: element offset of sequence b's keys.
  auto reference = [&](const pd::PageTable& pt, const std::vector<size_t>& off, int Hq, int Hkv, int T, float scale,
                       bool dense) {
    for (int b = 0; b < pt.B; ++b) {
      const size_t rows = (size_t)b * Hq * T;
      CK(ntm_attn_reference(dQ + rows * D, dKg + off[(size_t)b], dVg + off[(size_t)b], dense ? nullptr : dRefO + rows * D,
                            dense ? dO32 + rows * D : nullptr, dense ? dA + rows * D : nullptr, dense ? nullptr : dRefM + rows,
                            dense ? nullptr : dRefL + rows, 1, Hq, Hkv, T, pt.lens[(size_t)b], 1, scale, s));
    }
    return true;
  };
  // the gathered keys of every sequence, contiguous, uploaded
  auto upload_gathered = [&](const pd::PageTable& pt, int Hkv, const std::vector<uint16_t>& kp, const std::vector<uint16_t>& vp,
                             std::vector<size_t>& off) {
    off.assign((size_t)pt.B, 0);
    size_t at_elem = 0;
    for (int b = 0; b < pt.B; ++b) {
      off[(size_t)b] = at_elem;
      const std::vector<uint16_t> kg = pd::gather_from_pages(pt, b, Hkv, kp), vg = pd::gather_from_pages(pt, b, Hkv, vp);
      CK(hipMemcpyAsync(dKg + at_elem, kg.data(), kg.size() * 2, hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(dVg + at_elem, vg.data(), vg.size() * 2, hipMemcpyHostToDevice, s));
      CK(hipStreamSynchronize(s));  // kg and vg leave scope
      at_elem += kg.size();
    }
    return true;
  };

  // ---- 1. exact
  {
    // K and V of a sequence do not depend on T: generated once at T 4, the length-1 sequence again for T 1
    std::vector<at::Inputs> seq4((size_t)kEB);
    for (int b = 0; b < kEB; ++b)
      seq4[(size_t)b] = pd::exact_sequence(seed, b, kEHq, kEHkv, pd::kMaxT, std::max(lens1[(size_t)b], (int32_t)pd::kMaxT));
    for (int T : {1, pd::kMaxT}) {
      const std::string sub = "exact T" + std::to_string(T);
      std::vector<int32_t> lens = lens1;
      for (int32_t& n : lens) n = std::max(n, (int32_t)T);
      const pd::PageTable pt = pd::make_page_table(lens, seed, 2);
      const size_t pool = (size_t)pt.pages * kEHkv * page_elems;
      std::vector<uint16_t> kp(pool, 0x7FC0), vp(pool, 0x7FC0), qb((size_t)kEB * kEHq * T * D);
      std::vector<at::Inputs> own((size_t)kEB);  // the sequences whose length differs from seq4's
      auto inputs = [&](int b) -> const at::Inputs& {
        if (lens[(size_t)b] == seq4[(size_t)b].Sk) return seq4[(size_t)b];
        if (own[(size_t)b].Sk != lens[(size_t)b]) own[(size_t)b] = pd::exact_sequence(seed, b, kEHq, kEHkv, pd::kMaxT, lens[(size_t)b]);
        return own[(size_t)b];
      };
      // the owner of a shared prefix (the even sequence of a pair) is written last: its keys are the ones both read
      for (int b = kEB - 1; b >= 0; --b) {
        const at::Inputs& in = inputs(b);
        pd::scatter_to_pages(pt, b, kEHkv, in.kb.data(), kp);
        pd::scatter_to_pages(pt, b, kEHkv, in.vb.data(), vp);
        for (int h = 0; h < kEHq; ++h)  // token t of head h: the generator's row (h, t)
          std::memcpy(qb.data() + ((size_t)(b * kEHq + h) * T) * D, in.qb.data() + ((size_t)h * pd::kMaxT) * D, (size_t)T * D * 2);
      }
      // the predicate on the first and the last sequence (neither reads another's pages)
      bool exact = true;
      for (int b : {0, kEB - 1}) {
        const at::Inputs& in = inputs(b);
        std::vector<int32_t> q((size_t)kEHq * T * D);
        for (int h = 0; h < kEHq; ++h)
          std::memcpy(q.data() + (size_t)h * T * D, in.q.data() + (size_t)h * pd::kMaxT * D, (size_t)T * D * 4);
        exact = exact && at::attn_exact(q.data(), in.k.data(), in.v.data(), 1, kEHq, kEHkv, T, lens[(size_t)b], 1);
      }
      if (!exact) {
        r.failures.push_back("gpu" + std::to_string(dev) + ": pda " + sub + ": the generated inputs break attn_exact");
        continue;
      }
      std::vector<size_t> off;
      CK(hipMemcpyAsync(dQ, qb.data(), qb.size() * 2, hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(dKp, kp.data(), pool * 2, hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(dVp, vp.data(), pool * 2, hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(dBt, pt.table.data(), pt.table.size() * 4, hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(dLens, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, s));
      if (!upload_gathered(pt, kEHkv, kp, vp, off) || !reference(pt, off, kEHq, kEHkv, T, 1.0f, false)) return false;
      const size_t elems = qb.size(), rows = elems / D, wgs = (size_t)pd::grid(kEB, kEHkv, kES);
      std::vector<uint32_t> table(wgs * pd::kTableWords);
      std::set<uint32_t> seen;
      for (int launch = 0; launch < at::kMaxLaunches && (launch == 0 || (int)seen.size() < cus); ++launch) {
        CK(hipMemsetAsync(dO, 0xFF, elems * 2, s));
        CK(hipMemsetAsync(dWs, 0xFF, pd::workspace_bytes(kEB, kEHkv, kES), s));
        CK(hipMemsetAsync(dTable, 0, wgs * pd::kTableWords * 4, s));
        CK(ntm_pda_fwd(dQ, dKp, dVp, dBt, dLens, dO, dM, dL, dWs, dTable, kEB, kEHq, kEHkv, T, pt.max_pages, pt.pages, kES,
                       1.0f, s));
        if (launch == 0 && T == 1 && g.fault("corrupt_pda") && !flip_bits(dO + elems / 2 + 5, 2, 1u << 3, &s)) return false;
        CK(hipMemcpyAsync(table.data(), dTable, table.size() * 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        for (size_t w = 0; w < wgs; ++w) seen.insert(ntm::cus::cu_key(table[2 * w], table[2 * w + 1]));
        ++r.launches;
        struct Pair { const char* what; const void *e, *g; size_t words; };
        const Pair pairs[3] = {{"O", dRefO, dO, elems / 2}, {"m", dRefM, dM, rows}, {"l", dRefL, dL, rows}};
        for (const Pair& p : pairs) {
          CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s));
          CK(ntm_attn_compare(p.e, p.g, p.words, dres, s));
          CK(hipMemcpyAsync(&got, dres, sizeof got, hipMemcpyDeviceToHost, s));
          CK(hipStreamSynchronize(s));
          if (!got.count) continue;
          r.exact_bad += got.count;
          const std::string head = "gpu" + std::to_string(dev) + ": pda " + sub + " " + p.what + ":";
          bool have = false;  // one line per sub-test and output: the first launch that shows it
          for (auto& f : r.failures) have = have || f.compare(0, head.size(), head) == 0;
          if (!have)
            r.failures.push_back(pd::failure_message(dev, sub.c_str(), p.what, got.count, got.first_index, got.expected,
                                                     got.got, kEHq, kEHkv, T, kES, table.data()));
        }
      }
      r.cus_covered = std::max(r.cus_covered, (uint32_t)seen.size());
    }
  }

  // ---- 2. dense
  {
    std::vector<int32_t> lens(kDB);
    for (int b = 0; b < kDB; ++b) lens[(size_t)b] = 288 + (int)((at::attn_hash(seed, 8, (uint32_t)b) >> 8) % 65u);  // 288 .. 352
    const pd::PageTable pt = pd::make_page_table(lens, seed + 1, 1);
    const size_t pool = (size_t)pt.pages * kDHkv * page_elems, nq = (size_t)kDB * kDHq * D;
    CK(ntm_fill_uniform_bf16(dQ, nq, 0xDA70 + 3 * dev, 1.0f, s));
    CK(ntm_fill_uniform_bf16(dKp, pool, 0xDA71 + 3 * dev, 1.0f, s));
    CK(ntm_fill_uniform_bf16(dVp, pool, 0xDA72 + 3 * dev, 1.0f, s));
    std::vector<uint16_t> kp(pool), vp(pool), ho(nq);
    CK(hipMemcpyAsync(kp.data(), dKp, pool * 2, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(vp.data(), dVp, pool * 2, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(dBt, pt.table.data(), pt.table.size() * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dLens, lens.data(), lens.size() * 4, hipMemcpyHostToDevice, s));
    CK(hipStreamSynchronize(s));
    std::vector<size_t> off;
    if (!upload_gathered(pt, kDHkv, kp, vp, off) || !reference(pt, off, kDHq, kDHkv, 1, at::default_scale_log2(), true))
      return false;
    std::vector<float> h32(nq), ha(nq);
    std::vector<uint32_t> table((size_t)pd::grid(kDB, kDHkv, kDS) * pd::kTableWords);
    CK(hipMemsetAsync(dO, 0xFF, nq * 2, s));
    CK(ntm_pda_fwd(dQ, dKp, dVp, dBt, dLens, dO, nullptr, nullptr, dWs, dTable, kDB, kDHq, kDHkv, 1, pt.max_pages, pt.pages, kDS,
                   at::default_scale_log2(), s));
    CK(hipMemcpyAsync(ho.data(), dO, nq * 2, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(h32.data(), dO32, nq * 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(ha.data(), dA, nq * 4, hipMemcpyDeviceToHost, s));
    CK(hipMemcpyAsync(table.data(), dTable, table.size() * 4, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    unsigned long long bad = 0;
    size_t first = 0;
    auto value = [&](size_t x) {
      const uint32_t u = (uint32_t)ho[x] << 16;
      float v;
      std::memcpy(&v, &u, 4);
      return v;
    };
    for (size_t x = 0; x < nq; ++x) {
      const float err = std::fabs(value(x) - h32[x]);
      if (ha[x] > 0 && err / ha[x] > r.dense_worst) r.dense_worst = err / ha[x];
      if (!(err <= at::tolerance(ha[x])) && bad++ == 0) first = x;
    }
    if (bad) {
      r.dense_bad += bad;
      char num[96];
      std::snprintf(num, sizeof num, "error %.3e above 2^-7 a + 2^-20 = %.3e; ", (double)std::fabs(value(first) - h32[first]),
                    (double)at::tolerance(ha[first]));
      pd::Where w = pd::locate("O", first / 2, kDHq, kDHkv, 1, kDS);
      w.col = (long long)(first % D);
      r.failures.push_back("gpu" + std::to_string(dev) + ": pda dense O: " + pd::where_text(w, kDS, table.data()) + ": " + num +
                           std::to_string(bad) + " beyond");
    }
  }

  // ---- 3. timed
  {
    CK(ntm_fill_uniform_bf16(dQ, (size_t)kTB * kTHq * D, 0xDA80 + 3 * dev, 1.0f, s));
    CK(ntm_fill_uniform_bf16(dKp, pool_elems, 0xDA81 + 3 * dev, 1.0f, s));
    CK(ntm_fill_uniform_bf16(dVp, pool_elems, 0xDA82 + 3 * dev, 1.0f, s));
    CK(hipMemcpyAsync(dBt, timed_pt.table.data(), timed_pt.table.size() * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dLens, timed_lens.data(), timed_lens.size() * 4, hipMemcpyHostToDevice, s));
    auto fwd = [&] {
      return ntm_pda_fwd(dQ, dKp, dVp, dBt, dLens, dO, nullptr, nullptr, dWs, nullptr, kTB, kTHq, kTHkv, 1, timed_pt.max_pages,
                         timed_pt.pages, timed_splits, at::default_scale_log2(), s);
    };
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float ms = 0;
    if (!settle(s, o.settle_s, fwd) || !timed_ms(s, e0, e1, o.iters, ms, fwd)) return false;
    r.kv_gbps = ms > 0 ? pd::kv_bytes(timed_lens.data(), kTB, kTHkv) / (ms / o.iters * 1e-3) / 1e9 : 0;
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
  }
  for (void* p : {(void*)dQ, (void*)dKp, (void*)dVp, (void*)dKg, (void*)dVg, (void*)dO, (void*)dRefO, (void*)dO32, (void*)dA,
                  (void*)dM, (void*)dL, (void*)dRefM, (void*)dRefL, (void*)dBt, (void*)dLens, dWs, (void*)dTable, (void*)dres})
    CK(hipFree(p));
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
