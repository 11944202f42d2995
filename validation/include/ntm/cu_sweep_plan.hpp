// K5 (per-CU compute sweep) host side: the per-workgroup record the kernel
// writes, the HW_ID / XCC_ID decode, the generators of the sub-tests' operands,
// the expected tables (integer arithmetic only), the aggregation of records
// into a per-CU summary and the failure messages. Pure C++ - no HIP - so the
// Job, the kernel's header (ntm/cu_sweep.hpp) and a CPU-only test program
// share it. Functions the kernel also calls carry NTM_HD.
//
// Sub-tests, per round r of a workgroup of 256 threads (t = thread, w = t / 64
// its wave), all seeded by rs = round_seed(seed, r):
//   lds        every 32-bit word i of the dynamic LDS = h32(i + rs), read back;
//              then its complement, read back
//   valu       4 per-thread chains: hash (u32 multiply / xor / shift), mad
//              (u64 = u32 * u32 + u64), f32 FMA and f64 FMA on small integers
//   mfma_bf16  per wave: D16 = sum of 4 chained 16x16x32 products (K = 128) and
//              D32 = sum of 8 chained 32x32x16 products (K = 128), operands
//              integers in -8 .. 7: |sum| <= 128 * 64 = 8192 < 2^24
//   mfma_fp8   per wave: D = sum of 2 chained 16x16x128 e4m3 products (K = 256),
//              operands integers in -4 .. 3: |sum| <= 256 * 16 = 4096 < 2^24
// The expected table of one round is kRoundWords 32-bit words (layout below);
// element indices in a record count elements within the sub-test's section.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define NTM_HD __host__ __device__
#else
#define NTM_HD
#endif

namespace ntm {
namespace cus {

constexpr int kSubLds = 0, kSubValu = 1, kSubBf16 = 2, kSubFp8 = 3, kSubtests = 4;
inline const char* subtest_name(int s) {
  static const char* const n[kSubtests] = {"lds", "valu", "mfma_bf16", "mfma_fp8"};
  return s >= 0 && s < kSubtests ? n[s] : "?";
}

constexpr int kThreads = 256, kWaves = 4;
constexpr uint32_t kMagic = 0x4B355357u;  // a record the kernel has written
constexpr uint32_t kFaultOff = ~0u;       // fault_key: no injection
constexpr uint32_t kFaultBit = 1u << 7;   // the bit an injected fault flips
constexpr int kFaultThread = 192;         // the thread that flips it (wave 3, lane 0)
constexpr int kMaxIters = 1024;
constexpr int kMaxLaunches = 8;           // cap of the coverage loop
constexpr int kGridPerCu = 4;             // workgroups per CU and launch

// One per workgroup. The kernel writes hw_id .. wg with plain stores; bad[] .. got
// stay as the host zeroed them unless a compare fails (atomics, slow path only).
struct Record {
  uint32_t hw_id;        // raw HW_REG_HW_ID of wave 0
  uint32_t xcc_id;       // raw HW_REG_XCC_ID of wave 0
  uint8_t simd[kWaves];  // SIMD_ID of each wave
  uint32_t magic;        // kMagic
  uint32_t wg;           // blockIdx.x
  uint32_t bad[kSubtests];  // mismatching elements per sub-test
  uint32_t first;        // 0 = none; else (1 + sub-test) | wave << 8 of the first recorded mismatch
  uint32_t first_round;
  uint32_t first_elem;
  uint64_t expected;    // of that mismatch (32-bit values zero-extended)
  uint64_t got;
};
static_assert(sizeof(Record) == 64, "one 64-byte record per workgroup");

// ---- where a wave ran. HW_REG_HW_ID (gfx9): WAVE_ID 3:0, SIMD_ID 5:4, PIPE_ID 7:6,
// CU_ID 11:8, SH_ID 12, SE_ID 15:13; HW_REG_XCC_ID: the XCD in bits 3:0.
struct CuId {
  unsigned xcc, se, sh, cu, simd;
};
NTM_HD inline CuId decode(uint32_t hw_id, uint32_t xcc_id) {
  return CuId{xcc_id & 0xFu, (hw_id >> 13) & 0x7u, (hw_id >> 12) & 0x1u, (hw_id >> 8) & 0xFu,
              (hw_id >> 4) & 0x3u};
}
// (xcc, se, sh, cu) packed into 12 bits: the fault key and the map key.
NTM_HD inline uint32_t cu_key(uint32_t hw_id, uint32_t xcc_id) {
  return ((xcc_id & 0xFu) << 8) | (((hw_id >> 13) & 0x7u) << 5) | (((hw_id >> 12) & 0x1u) << 4) |
         ((hw_id >> 8) & 0xFu);
}
inline CuId key_to_id(uint32_t key) {
  return CuId{(key >> 8) & 0xFu, (key >> 5) & 0x7u, (key >> 4) & 0x1u, key & 0xFu, 0};
}

// ---- generators (shared with the kernel: inputs only, never expected sums)
NTM_HD inline uint32_t h32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
NTM_HD inline uint32_t round_seed(uint32_t seed, uint32_t round) {
  return h32(seed + 0x9E3779B9u * (round + 1u));
}
NTM_HD inline uint32_t lds_word(uint32_t i, uint32_t rs) { return h32(i + rs); }

// MFMA operands. kind: 0 / 1 = A / B of the 16x16x32 chain, 2 / 3 of the 32x32x16
// chain, 4 / 5 of the fp8 chain; i = row of A or column of B (< 32), k < 256.
NTM_HD inline uint32_t operand_hash(uint32_t rs, unsigned kind, unsigned wave, unsigned i,
                                    unsigned k) {
  return h32((((kind * 4u + wave) * 32u + i) << 8 | k) + rs);
}
NTM_HD inline int bf16_operand(uint32_t rs, unsigned kind, unsigned wave, unsigned i, unsigned k) {
  return (int)((operand_hash(rs, kind, wave, i, k) >> 8) & 15u) - 8;  // -8 .. 7
}
NTM_HD inline int fp8_operand(uint32_t rs, unsigned kind, unsigned wave, unsigned i, unsigned k) {
  return (int)((operand_hash(rs, kind, wave, i, k) >> 8) & 7u) - 4;  // -4 .. 3
}
// OCP e4m3 code of an integer in -4 .. 3 (exact): byte v + 4 of the constant
// (-4 = 0xC8, -3 = 0xC4, -2 = 0xC0, -1 = 0xB8, 0 = 0x00, 1 = 0x38, 2 = 0x40, 3 = 0x44).
NTM_HD inline uint32_t e4m3_of_small_int(int v) {
  return (uint32_t)((0x44403800B8C0C4C8ull >> (8 * (unsigned)(v + 4))) & 0xFFu);
}
constexpr int kBf16Steps16 = 4, kBf16Steps32 = 8, kFp8Steps = 2;  // chained MFMAs
constexpr int kBf16K = 128, kFp8K = 256;

// valu chains: the inputs of thread t
constexpr int kHashSteps = 16, kMadSteps = 16, kF32Segments = 4, kF32Steps = 8, kF64Steps = 16;
NTM_HD inline uint32_t valu_hash_chain(uint32_t t, uint32_t rs) {
  uint32_t x = t * 0x9E3779B9u + rs;
  for (uint32_t i = 0; i < (uint32_t)kHashSteps; ++i) x = h32(x + i);
  return x;
}
NTM_HD inline uint64_t valu_mad_chain(uint32_t t, uint32_t rs) {
  uint32_t a = h32(rs + 2u * t + 1u), b = h32(rs ^ (t * 0x85EBCA6Bu));
  uint64_t acc = a;
  for (uint32_t i = 0; i < (uint32_t)kMadSteps; ++i) {
    acc = (uint64_t)a * b + acc;  // v_mad_u64_u32
    a = (uint32_t)acc + i;
    b = (uint32_t)(acc >> 32) | 1u;
  }
  return acc;
}
// FMA chains: step i of chain c (0 = f32, 1 = f64) of thread t multiplies by mul and adds add.
NTM_HD inline uint32_t fma_coeff(uint32_t rs, unsigned c, uint32_t t, unsigned i) {
  return h32(rs + ((c * 64u + i + 1u) << 12) + t);
}
NTM_HD inline int fma_start(uint32_t coeff) { return (int)((coeff >> 16) & 0xFFu) - 128; }
NTM_HD inline int fma_add(uint32_t coeff) { return (int)((coeff >> 8) & 0xFFu) - 128; }
NTM_HD inline int fma_mul(uint32_t coeff, unsigned c) {  // f32: +-2, +-3; f64: +-5, +-7
  const int m = c == 0 ? ((coeff & 1u) ? 3 : 2) : ((coeff & 1u) ? 7 : 5);
  return (coeff & 2u) ? -m : m;
}

// ---- the expected table of one round, in 32-bit words
constexpr uint32_t kOffHash = 0;                       // u32[256]
constexpr uint32_t kOffMad = 256;                      // u64[256]
constexpr uint32_t kOffF32 = 768;                      // f32 bits[256]
constexpr uint32_t kOffF64 = 1024;                     // f64 bits[256]
constexpr uint32_t kOffBf16 = 1536;                    // f32 bits [4][16][16], then [4][32][32]
constexpr uint32_t kBf16Words16 = kWaves * 256, kBf16Words32 = kWaves * 1024;
constexpr uint32_t kOffFp8 = kOffBf16 + kBf16Words16 + kBf16Words32;  // f32 bits [4][16][16]
constexpr uint32_t kRoundWords = kOffFp8 + kWaves * 256;
static_assert(kRoundWords == 7680, "30 KiB per round");

inline size_t expected_bytes(int iters) { return iters > 0 ? (size_t)iters * kRoundWords * 4 : 0; }

inline uint32_t f32_bits_of_int(int64_t v) {  // |v| < 2^24: exact
  const float f = (float)v;
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
inline uint64_t f64_bits_of_int(int64_t v) {  // |v| < 2^53: exact
  const double f = (double)v;
  uint64_t u;
  std::memcpy(&u, &f, 8);
  return u;
}
inline int64_t f32_chain_expected(uint32_t t, uint32_t rs) {
  int64_t total = 0;
  for (int s = 0; s < kF32Segments; ++s) {
    int64_t acc = fma_start(fma_coeff(rs, 0, t, (unsigned)(s * kF32Steps)));
    for (int i = 0; i < kF32Steps; ++i) {
      const uint32_t c = fma_coeff(rs, 0, t, (unsigned)(s * kF32Steps + i));
      acc = acc * fma_mul(c, 0) + fma_add(c);
    }
    total += acc;
  }
  return total;
}
inline int64_t f64_chain_expected(uint32_t t, uint32_t rs) {
  int64_t acc = fma_start(fma_coeff(rs, 1, t, 0));
  for (int i = 0; i < kF64Steps; ++i) {
    const uint32_t c = fma_coeff(rs, 1, t, (unsigned)i);
    acc = acc * fma_mul(c, 1) + fma_add(c);
  }
  return acc;
}

// D[w][i][j] = sum over k of A(i, k) * B(k, j), in integers. Returns the largest |sum|.
template <class Gen>
inline int64_t expected_product(uint32_t* out, int n, int K, unsigned kind_a, uint32_t rs, Gen gen) {
  int64_t peak = 0;
  std::vector<int> a((size_t)n * K), b((size_t)n * K);
  for (unsigned w = 0; w < (unsigned)kWaves; ++w) {
    for (int i = 0; i < n; ++i)
      for (int k = 0; k < K; ++k) {
        a[(size_t)i * K + k] = gen(rs, kind_a, w, (unsigned)i, (unsigned)k);
        b[(size_t)i * K + k] = gen(rs, kind_a + 1, w, (unsigned)i, (unsigned)k);
      }
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) {
        int64_t s = 0;
        for (int k = 0; k < K; ++k) s += (int64_t)a[(size_t)i * K + k] * b[(size_t)j * K + k];
        peak = std::max(peak, s < 0 ? -s : s);
        out[((size_t)w * n + i) * n + j] = f32_bits_of_int(s);
      }
  }
  return peak;
}

// Fills expected_bytes(iters) bytes at `out`.
inline void make_expected(uint32_t* out, int iters, uint32_t seed) {
  for (int r = 0; r < iters; ++r) {
    uint32_t* p = out + (size_t)r * kRoundWords;
    const uint32_t rs = round_seed(seed, (uint32_t)r);
    for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
      p[kOffHash + t] = valu_hash_chain(t, rs);
      const uint64_t m = valu_mad_chain(t, rs);
      p[kOffMad + 2 * t] = (uint32_t)m;
      p[kOffMad + 2 * t + 1] = (uint32_t)(m >> 32);
      p[kOffF32 + t] = f32_bits_of_int(f32_chain_expected(t, rs));
      const uint64_t d = f64_bits_of_int(f64_chain_expected(t, rs));
      p[kOffF64 + 2 * t] = (uint32_t)d;
      p[kOffF64 + 2 * t + 1] = (uint32_t)(d >> 32);
    }
    expected_product(p + kOffBf16, 16, kBf16K, 0, rs, bf16_operand);
    expected_product(p + kOffBf16 + kBf16Words16, 32, kBf16K, 2, rs, bf16_operand);
    expected_product(p + kOffFp8, 16, kFp8K, 4, rs, fp8_operand);
  }
}

// ---- aggregation
struct BadCu {
  uint32_t key = 0;
  CuId id{};               // simd: of the wave that recorded the first mismatch
  uint32_t workgroups = 0, bad_workgroups = 0;
  uint32_t subtests = 0;   // bit s set: sub-test s failed there
  int first_subtest = -1;
  uint32_t first_round = 0, first_elem = 0;
  uint64_t expected = 0, got = 0;
};

struct Summary {
  uint32_t cus = 0;            // CUs the device reports
  uint32_t cus_covered = 0;    // distinct (xcc, se, sh, cu) that ran a workgroup
  uint32_t simds_covered = 0;  // distinct (CU, SIMD) pairs that ran a wave
  uint32_t launches = 0, workgroups = 0, unwritten = 0;
  uint32_t wg_per_cu_min = 0, wg_per_cu_max = 0;
  std::vector<BadCu> bad_cus;  // sorted by key
  bool ok() const { return bad_cus.empty() && unwritten == 0 && cus_covered >= cus && cus > 0; }
};

// Merges launches: add() every launch's records, then summary().
class Sweep {
 public:
  void add(const Record* r, size_t n) {
    ++launches_;
    for (size_t i = 0; i < n; ++i) {
      ++workgroups_;
      if (r[i].magic != kMagic) {
        ++unwritten_;
        continue;
      }
      const uint32_t key = cu_key(r[i].hw_id, r[i].xcc_id);
      Cu& c = cus_[key];
      ++c.workgroups;
      for (int w = 0; w < kWaves; ++w) c.simds |= 1u << (r[i].simd[w] & 3u);
      uint32_t sub = 0;
      for (int s = 0; s < kSubtests; ++s)
        if (r[i].bad[s]) sub |= 1u << s;
      if (!sub && !r[i].first) continue;
      if (!c.bad_workgroups++) c.first = r[i];
      c.subtests |= sub;
    }
  }
  size_t cus_covered() const { return cus_.size(); }
  bool covered(uint32_t cus) const { return cus_.size() >= cus; }
  std::vector<uint32_t> keys() const {
    std::vector<uint32_t> k;
    for (auto& kv : cus_) k.push_back(kv.first);
    return k;
  }
  Summary summary(uint32_t cus) const {
    Summary s;
    s.cus = cus;
    s.cus_covered = (uint32_t)cus_.size();
    s.launches = launches_;
    s.workgroups = workgroups_;
    s.unwritten = unwritten_;
    bool any = false;
    for (auto& kv : cus_) {
      const Cu& c = kv.second;
      for (int b = 0; b < 4; ++b) s.simds_covered += (c.simds >> b) & 1u;
      s.wg_per_cu_min = any ? std::min(s.wg_per_cu_min, c.workgroups) : c.workgroups;
      s.wg_per_cu_max = std::max(s.wg_per_cu_max, c.workgroups);
      any = true;
      if (!c.bad_workgroups) continue;
      BadCu b;
      b.key = kv.first;
      b.id = key_to_id(kv.first);
      b.workgroups = c.workgroups;
      b.bad_workgroups = c.bad_workgroups;
      b.subtests = c.subtests;
      const Record& f = c.first;
      if (f.first) {
        b.first_subtest = (int)(f.first & 0xFFu) - 1;
        b.id.simd = f.simd[(f.first >> 8) & 3u] & 3u;
        b.first_round = f.first_round;
        b.first_elem = f.first_elem;
        b.expected = f.expected;
        b.got = f.got;
      }
      s.bad_cus.push_back(b);
    }
    return s;
  }

 private:
  struct Cu {
    uint32_t workgroups = 0, bad_workgroups = 0, subtests = 0, simds = 0;
    Record first{};
  };
  std::map<uint32_t, Cu> cus_;
  uint32_t launches_ = 0, workgroups_ = 0, unwritten_ = 0;
};

// The coverage loop of the Job and of models.validation_job.cu_sweep_check: launches
// until every one of `cus` CUs ran a workgroup or max_launches are spent (a cap, not a
// retry). launch(l, records) runs launch l, fills records and returns false on an error.
template <class LaunchFn>
inline bool coverage_loop(uint32_t cus, int max_launches, LaunchFn launch, Sweep& sweep) {
  std::vector<Record> recs;
  for (int l = 0; l < max_launches; ++l) {
    recs.clear();
    if (!launch(l, recs)) return false;
    sweep.add(recs.data(), recs.size());
    if (sweep.covered(cus)) break;
  }
  return true;
}

inline std::string hex(uint64_t v) {
  char b[24];
  std::snprintf(b, sizeof b, "0x%llx", (unsigned long long)v);
  return b;
}
inline std::string subtest_list(uint32_t mask) {
  std::string s;
  for (int i = 0; i < kSubtests; ++i)
    if (mask & (1u << i)) s += std::string(s.empty() ? "" : "+") + subtest_name(i);
  return s;
}

// Empty when the sweep passed. Else one line under 200 characters (the termination
// message cuts there): bad CUs first, "gpu3: CU sweep: 1 bad CU of 256: xcd 5 se 2 sh 0
// cu 7 (simd 1) mfma_bf16 round 3 elem 41: expected 0x..., got 0x...; 4 of 4 workgroups
// there failed"; else CUs that never ran, "gpu3: CU sweep: 3 of 256 CUs ran no workgroup
// after 8 launches".
inline std::string failure_message(int gpu, const Summary& s) {
  if (s.ok()) return "";
  std::string m = "gpu" + std::to_string(gpu) + ": CU sweep: ";
  if (!s.bad_cus.empty()) {
    const BadCu& b = s.bad_cus[0];
    m += std::to_string(s.bad_cus.size()) + " bad CU" + (s.bad_cus.size() > 1 ? "s" : "") +
         " of " + std::to_string(s.cus) + ": xcd " + std::to_string(b.id.xcc) + " se " +
         std::to_string(b.id.se) + " sh " + std::to_string(b.id.sh) + " cu " +
         std::to_string(b.id.cu);
    if (b.first_subtest >= 0)
      m += " (simd " + std::to_string(b.id.simd) + ") " + subtest_name(b.first_subtest) +
           " round " + std::to_string(b.first_round) + " elem " + std::to_string(b.first_elem) +
           ": expected " + hex(b.expected) + ", got " + hex(b.got);
    else
      m += " " + subtest_list(b.subtests);
    m += "; " + std::to_string(b.bad_workgroups) + " of " + std::to_string(b.workgroups) +
         " workgroups there failed";
  } else if (s.unwritten) {
    m += std::to_string(s.unwritten) + " of " + std::to_string(s.workgroups) +
         " workgroups wrote no record";
  } else {
    const uint32_t missing = s.cus > s.cus_covered ? s.cus - s.cus_covered : 0;
    m += std::to_string(missing) + " of " + std::to_string(s.cus) + " CUs ran no workgroup after " +
         std::to_string(s.launches) + " launch" + (s.launches == 1 ? "" : "es");
  }
  if (m.size() > 199) m.resize(199);
  return m;
}

// The summary as one JSON object (ops.cu_sweep_summarize parses it; the Job
// takes its cu_sweep_bad_cus list from bad_cus_json).
inline std::string bad_cus_json(const Summary& s) {
  std::string j = "[";
  for (size_t i = 0; i < s.bad_cus.size(); ++i) {
    const BadCu& b = s.bad_cus[i];
    std::string subs;
    for (int t = 0; t < kSubtests; ++t)
      if (b.subtests & (1u << t)) subs += std::string(subs.empty() ? "" : ",") + "\"" + subtest_name(t) + "\"";
    j += std::string(i ? "," : "") + "{\"key\":" + std::to_string(b.key) +
         ",\"xcd\":" + std::to_string(b.id.xcc) + ",\"se\":" + std::to_string(b.id.se) +
         ",\"sh\":" + std::to_string(b.id.sh) + ",\"cu\":" + std::to_string(b.id.cu) +
         ",\"simd\":" + std::to_string(b.id.simd) + ",\"subtests\":[" + subs + "]" +
         ",\"workgroups\":" + std::to_string(b.workgroups) +
         ",\"bad_workgroups\":" + std::to_string(b.bad_workgroups) + ",\"first\":";
    if (b.first_subtest >= 0)
      j += std::string("{\"subtest\":\"") + subtest_name(b.first_subtest) +
           "\",\"round\":" + std::to_string(b.first_round) +
           ",\"elem\":" + std::to_string(b.first_elem) + ",\"expected\":\"" + hex(b.expected) +
           "\",\"got\":\"" + hex(b.got) + "\"}";
    else
      j += "null";
    j += "}";
  }
  return j + "]";
}
inline std::string summary_json(int gpu, const Summary& s) {
  std::string msg = failure_message(gpu, s);
  return "{\"ok\":" + std::string(s.ok() ? "true" : "false") + ",\"cus\":" + std::to_string(s.cus) +
         ",\"cus_covered\":" + std::to_string(s.cus_covered) +
         ",\"simds_covered\":" + std::to_string(s.simds_covered) +
         ",\"launches\":" + std::to_string(s.launches) +
         ",\"workgroups\":" + std::to_string(s.workgroups) +
         ",\"unwritten\":" + std::to_string(s.unwritten) +
         ",\"wg_per_cu_min\":" + std::to_string(s.wg_per_cu_min) +
         ",\"wg_per_cu_max\":" + std::to_string(s.wg_per_cu_max) +
         ",\"bad_cus\":" + bad_cus_json(s) + ",\"message\":\"" + msg + "\"}";
}

}  // namespace cus
}  // namespace ntm
