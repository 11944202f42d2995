// amdgpu-validate K12: wave data paths and the special-function unit (ntm/wave_paths.hpp, host
// side in ntm/wave_paths_plan.hpp). On for NTM_WAVE_CHECK=1. Per family the expected table comes
// from the reference kernel (none of the instructions under test), then 2 workgroups per CU run
// the whole family against it and leave one record each, launch after launch until every CU ran
// it or 8 launches are spent (a cap, not a retry):
//   lane   every op of the list on hashed words;
//   ldstr  the four transposed reads on images of 64 rows x 136 bytes (144 for the 6-bit form);
//   valu   v_bitop3_b32 over the 256 tables, v_cvt_pk_bf16_f32 over the boundary list;
//   sfu    the seven transcendentals over their whole input lists: one digest per instruction
//          and workgroup, held to the digest most workgroups agree on; then, once, the distance
//          of every result from the host's bracket (reported; judged where a bound is recorded).
// A workgroup whose digest is off the majority's is named by its HW_ID / XCC_ID; a second, small
// launch then stores the words of one workgroup on that CU and of one on another CU, and the
// first input whose words differ is named with expected, got and bad bits.
// corrupt_wave_sfu: every workgroup on one CU of the LAST GPU flips bit 10 of one v_exp_f32 word.
// corrupt_wave: bit 10 of the row_shr:3 bound_ctrl:0 word of wave 2, lane 19 of workgroup 0 of
// the LAST GPU's first lane launch is flipped before the compare.
#include <set>

#include "check.hpp"
#include "ntm/wave_paths_plan.hpp"

namespace ntm::job {

bool run_wave(const GpuCtx& g, WaveResult& r) {
  namespace wv = ntm::wave;
  const int dev = g.dev;
  hipStream_t s = g.s;
  const auto t_begin = Clock::now();
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  const uint32_t cus = (uint32_t)prop.multiProcessorCount;
  const int grid = (int)(wv::kGridPerCu * cus);
  r.ran = true;
  r.cus = cus;
  const uint32_t seed = 0x4B3Cu + (uint32_t)dev;

  uint32_t *dIn = nullptr, *dExp = nullptr, *dOut = nullptr;
  wv::Record* dRec = nullptr;
  const size_t in_words = 1u << 20, exp_words = 1u << 20;
  CK(hipMalloc(&dIn, in_words * 4));
  CK(hipMalloc(&dExp, exp_words * 4));
  CK(hipMalloc(&dOut, exp_words * 4));
  CK(hipMalloc(&dRec, (size_t)grid * sizeof(wv::Record)));
  std::vector<wv::Record> recs((size_t)grid);
  uint32_t covered_min = ~0u;

  // the coverage loop of one family; on_record sees every written record
  auto sweep = [&](int family, size_t words, const uint32_t* layout, bool inject, auto on_record) -> bool {
    std::set<uint32_t> seen;
    for (int l = 0; l < wv::kMaxLaunches && seen.size() < cus; ++l) {
      CK(hipMemsetAsync(dRec, 0, recs.size() * sizeof(wv::Record), s));
      const uint32_t idx = (uint32_t)(wv::kQuadPerms + 15 + 2) * wv::kThreads + 2 * 64 + 19;  // row_shr:3 bound_ctrl:0
      CK(ntm_wave_sweep(family, dIn, words, layout, dExp, dRec, grid, inject && l == 0 ? 0u : wv::kNoFault, idx, s));
      CK(hipMemcpyAsync(recs.data(), dRec, recs.size() * sizeof(wv::Record), hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      for (const wv::Record& rec : recs) {
        if (rec.magic != wv::kMagic) {
          if (r.failures.empty())
            r.failures.push_back("gpu" + std::to_string(dev) + ": wave " + wv::family_name(family) + ": a workgroup wrote no record");
          continue;
        }
        seen.insert(cus::cu_key(rec.hw_id, rec.xcc_id));
        on_record(rec);
      }
    }
    covered_min = std::min<uint32_t>(covered_min, (uint32_t)seen.size());
    return true;
  };
  auto once = [&](const std::string& line, const std::string& head) {
    for (auto& f : r.failures)
      if (f.compare(0, head.size(), head) == 0) return;
    r.failures.push_back(line);
  };
  const std::string gp = "gpu" + std::to_string(dev) + ": wave ";

  // lane
  {
    std::vector<uint32_t> in(2 * wv::kThreads);
    for (uint32_t t = 0; t < (uint32_t)wv::kThreads; ++t)
      in[t] = wv::hash32(seed, 0, t / 64, 0, t % 64), in[wv::kThreads + t] = wv::hash32(seed, 1, t / 64, 0, t % 64);
    CK(hipMemcpyAsync(dIn, in.data(), in.size() * 4, hipMemcpyHostToDevice, s));
    CK(ntm_wave_lane(1, 0, wv::kLaneOps, dIn, dIn + wv::kThreads, dExp, wv::kThreads, s));
    if (!sweep(wv::kFamLane, in.size(), nullptr, g.fault("corrupt_wave"), [&](const wv::Record& rec) {
          r.lane_bad += rec.bad;
          if (rec.bad) once(wv::lane_failure(dev, rec), gp + "lane");
        }))
      return false;
  }
  // ldstr
  {
    std::vector<uint32_t> in((size_t)wv::kTrForms * wv::kTrMaxBytes / 4, 0u);
    size_t base[wv::kTrForms + 1] = {0};
    for (int f = 0; f < wv::kTrForms; ++f) {
      const auto img = wv::tr_make_image(wv::kTrBits[f], wv::kSweepRows, wv::sweep_stride(wv::kTrBits[f]), seed + (uint32_t)f);
      std::memcpy(in.data() + (size_t)f * wv::kTrMaxBytes / 4, img.data(), img.size());
      wv::TrShape sh;
      wv::tr_shape(wv::kTrBits[f], wv::kSweepRows, wv::sweep_stride(wv::kTrBits[f]), &sh);
      base[f + 1] = base[f] + wv::tr_out_words(sh);
    }
    CK(hipMemcpyAsync(dIn, in.data(), in.size() * 4, hipMemcpyHostToDevice, s));
    for (int f = 0; f < wv::kTrForms; ++f)
      CK(ntm_wave_tr_read(1, wv::kTrBits[f], dIn + (size_t)f * wv::kTrMaxBytes / 4, wv::kSweepRows,
                          wv::sweep_stride(wv::kTrBits[f]), dExp + base[f], s));
    if (!sweep(wv::kFamLdstr, in.size(), nullptr, false, [&](const wv::Record& rec) {
          r.ldstr_bad += rec.bad;
          if (!rec.bad) return;
          int f = 0;
          while (f + 1 < wv::kTrForms && ~rec.first >= base[f + 1]) ++f;
          wv::Record rel = rec;
          rel.first = ~(uint32_t)(~rec.first - base[f]);
          once(wv::indexed_failure(dev, wv::kFamLdstr, "tr_b" + std::to_string(wv::kTrBits[f]) + " stride " + std::to_string(wv::sweep_stride(wv::kTrBits[f])), rel), gp + "ldstr");
        }))
      return false;
  }
  // valu
  {
    const std::vector<uint32_t> cv = wv::cvt_inputs(seed, 1024);
    const uint32_t ncvt = (uint32_t)cv.size();
    std::vector<uint32_t> in(3 * wv::kThreads + 2 * (size_t)ncvt);
    for (uint32_t t = 0; t < 3u * wv::kThreads; ++t) in[t] = wv::hash32(seed, 2 + t / wv::kThreads, (t / 64) & 3, 0, t % 64);
    for (uint32_t i = 0; i < ncvt; ++i) in[3 * wv::kThreads + i] = cv[i], in[3 * wv::kThreads + ncvt + i] = cv[ncvt - 1 - i];
    CK(hipMemcpyAsync(dIn, in.data(), in.size() * 4, hipMemcpyHostToDevice, s));
    CK(ntm_wave_valu(1, wv::kValuBitop, dIn, dIn + wv::kThreads, dIn + 2 * wv::kThreads, dExp, wv::kThreads, s));
    CK(ntm_wave_valu(1, wv::kValuCvt, dIn + 3 * wv::kThreads, dIn + 3 * wv::kThreads + ncvt, nullptr, dExp + 256 * wv::kThreads, ncvt, s));
    if (!sweep(wv::kFamValu, in.size(), &ncvt, false, [&](const wv::Record& rec) {
          r.valu_bad += rec.bad;
          if (!rec.bad) return;
          const uint32_t idx = ~rec.first;
          char what[32];
          if (idx < 256u * wv::kThreads) std::snprintf(what, sizeof what, "bitop3:0x%02x", idx / wv::kThreads);
          else std::snprintf(what, sizeof what, "cvt_pk_bf16_f32");
          wv::Record rel = rec;
          rel.first = ~(idx < 256u * wv::kThreads ? idx % wv::kThreads : idx - 256u * wv::kThreads);
          once(wv::indexed_failure(dev, wv::kFamValu, what, rel), gp + "valu");
        }))
      return false;
  }
  // sfu
  {
    std::vector<uint32_t> in, n(wv::kSfuOps);
    std::vector<wv::SfuList> lists;
    for (int op = 0; op < wv::kSfuOps; ++op) {
      lists.push_back(wv::sfu_inputs(op));
      n[op] = (uint32_t)lists[op].x.size();
      in.insert(in.end(), lists[op].x.begin(), lists[op].x.end());
    }
    if (in.size() > in_words) {
      fail("wave: the sfu input lists outgrew their buffer");
      return false;
    }
    CK(hipMemcpyAsync(dIn, in.data(), in.size() * 4, hipMemcpyHostToDevice, s));
    std::vector<wv::Record> all;
    // corrupt_wave_sfu: every workgroup on the CU that workgroup 0 of a first launch ran on flips
    // bit 10 of result word 1000 of v_exp_f32, in the sweep and in the second launch
    uint32_t fault_key = wv::kNoFault;
    const uint32_t fault_index = 1000;
    if (g.fault("corrupt_wave_sfu")) {
      CK(hipMemsetAsync(dRec, 0, recs.size() * sizeof(wv::Record), s));
      CK(ntm_wave_sweep(wv::kFamSfu, dIn, in.size(), n.data(), nullptr, dRec, grid, wv::kNoFault, 0, s));
      CK(hipMemcpyAsync(recs.data(), dRec, sizeof(wv::Record), hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      fault_key = cus::cu_key(recs[0].hw_id, recs[0].xcc_id);
    }
    {
      std::set<uint32_t> seen;
      for (int l = 0; l < wv::kMaxLaunches && seen.size() < cus; ++l) {
        CK(hipMemsetAsync(dRec, 0, recs.size() * sizeof(wv::Record), s));
        CK(ntm_wave_sweep(wv::kFamSfu, dIn, in.size(), n.data(), nullptr, dRec, grid, fault_key, fault_index, s));
        CK(hipMemcpyAsync(recs.data(), dRec, recs.size() * sizeof(wv::Record), hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        for (const wv::Record& rec : recs) {
          if (rec.magic != wv::kMagic) {
            once(gp + "sfu: a workgroup wrote no record", gp + "sfu");
            continue;
          }
          seen.insert(cus::cu_key(rec.hw_id, rec.xcc_id));
          all.push_back(rec);
        }
      }
      covered_min = std::min<uint32_t>(covered_min, (uint32_t)seen.size());
    }
    // the second launch: one workgroup on the CU `key` (or on another CU) stores its words
    std::vector<uint32_t> words[2];
    wv::Record located[2];
    auto locate = [&](int op, size_t at, uint32_t key, int on_key, bool& found) -> bool {
      uint32_t* dClaim = dExp;
      wv::Record* dOne = (wv::Record*)(dExp + 16);
      found = false;
      for (int l = 0; l < wv::kMaxLaunches && !found; ++l) {
        CK(hipMemsetAsync(dExp, 0, 64 + sizeof(wv::Record), s));
        CK(ntm_wave_sfu_locate(op, dIn + at, n[op], key, on_key, dClaim, dOut, dOne, grid, fault_key, fault_index, s));
        uint32_t claimed = 0;
        CK(hipMemcpyAsync(&claimed, dClaim, 4, hipMemcpyDeviceToHost, s));
        CK(hipStreamSynchronize(s));
        found = claimed != 0;
      }
      if (found) {
        words[on_key].resize(n[op]);
        CK(hipMemcpy(words[on_key].data(), dOut, (size_t)n[op] * 4, hipMemcpyDeviceToHost));
        CK(hipMemcpy(&located[on_key], dOne, sizeof(wv::Record), hipMemcpyDeviceToHost));
      }
      return true;
    };
    size_t list_at = 0;
    for (int op = 0; op < wv::kSfuOps; list_at += n[op], ++op) {
      const uint64_t want = wv::majority_digest(all, op);
      for (const wv::Record& rec : all) {
        if (rec.digest[op] == want) continue;
        ++r.sfu_inconsistent;
        bool seen_line = false;
        for (auto& f : r.failures) seen_line = seen_line || f.compare(0, (gp + "sfu").size(), gp + "sfu") == 0;
        if (seen_line) continue;
        bool on = false, off = false;
        if (!locate(op, list_at, cus::cu_key(rec.hw_id, rec.xcc_id), 1, on) ||
            !locate(op, list_at, cus::cu_key(rec.hw_id, rec.xcc_id), 0, off))
          return false;
        std::string line = wv::sfu_digest_failure(dev, op, rec, want, "not seen again in a second launch");
        if (on && off && wv::sfu_digest_of(words[0].data(), n[op]) == want)
          for (uint32_t i = 0; i < n[op]; ++i)
            if (words[0][i] != words[1][i]) {
              line = wv::sfu_failure(dev, op, located[1], i, lists[op].x[i], words[0][i], words[1][i]);
              break;
            }
        r.failures.push_back(line);
      }
    }
    // accuracy, once: every result against the host's bracket
    size_t at = 0;
    std::vector<uint32_t> lo, hi;
    wv::SfuDistance init, got;
    wv::distance_init(init);
    for (int op = 0; op < wv::kSfuOps; ++op) {
      lo.resize(n[op]), hi.resize(n[op]);
      for (uint32_t i = 0; i < n[op]; ++i) wv::sfu_bracket(op, lists[op].x[i], &lo[i], &hi[i]);
      uint32_t *dLo = dExp, *dHi = dExp + n[op], *dD = dExp + 2 * (size_t)n[op];
      CK(hipMemcpyAsync(dLo, lo.data(), n[op] * 4, hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(dHi, hi.data(), n[op] * 4, hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(dD, &init, sizeof init, hipMemcpyHostToDevice, s));
      CK(ntm_wave_sfu(op, dIn + at, dOut, n[op], s));
      CK(ntm_wave_sfu_distance(dOut, dLo, dHi, n[op], wv::kSfuBound[op], dD, s));
      CK(hipMemcpyAsync(&got, dD, sizeof got, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      r.sfu_max_d[op] = got.max_d;
      r.sfu_max_x[op] = got.max_d ? lists[op].x[got.max_index] : 0;
      if (wv::kSfuBound[op] != wv::kSfuNoBound && got.beyond) {
        r.sfu_beyond += got.beyond;
        once(gp + "sfu " + wv::sfu_name(op) + ": " + std::to_string(got.beyond) + " result(s) beyond " +
                 std::to_string(wv::kSfuBound[op]) + " step(s) of the bracket, first input " +
                 wv::hex32(lists[op].x[got.first_beyond]),
             gp + "sfu " + wv::sfu_name(op) + ": ");
      }
      at += n[op];
    }
  }
  r.cus_covered = covered_min == ~0u ? 0 : covered_min;
  if (r.cus_covered < cus)
    r.failures.push_back(gp + "coverage: " + std::to_string(cus - r.cus_covered) + " of " + std::to_string(cus) +
                         " CUs did not run every family after " + std::to_string(wv::kMaxLaunches) + " launches");
  for (void* p : {(void*)dIn, (void*)dExp, (void*)dOut, (void*)dRec}) CK(hipFree(p));
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
