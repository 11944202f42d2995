// K8 (per-XCD sweep) host side: the per-workgroup record the kernels write, the
// levels and modes, the slice / tile arithmetic, the aggregation of records into
// one row per XCD, the verdict and the failure messages. Pure C++ - no HIP - so
// the Job, the kernels' header (ntm/xcd_sweep.hpp) and a CPU-only test program
// share it.
//
// A GPU's rates in the Job are aggregates over its XCDs; one XCD at 60 % of its
// siblings costs them about 5 %. K8 gives every XCD a work queue of its own and
// a slice of a buffer filled with K4's pattern, times the XCD against its own
// stamps and compares it with the median of its own card:
//   fail XCD x at (level, mode) when rate[x] < ratio * median(rate[0 .. n))
// The rule needs no absolute number and works on one GPU. It runs only when
// ratio > 0 and n >= 3. Wrong data, a tile sum that is not passes *
// tiles_per_slice, an XCD without a workgroup or short of a CU always fail.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <set>
#include <string>
#include <vector>

namespace ntm {
namespace xcs {

constexpr uint32_t kMagic = 0x4B385843u;  // a record the kernel has written
constexpr int kThreads = 256;
constexpr int kLoadsInFlight = 16;                            // 16-byte loads per lane and tile
constexpr uint32_t kTileBytes = kThreads * 16 * kLoadsInFlight;  // 64 KiB
constexpr int kMaxXcds = 16;       // HW_REG_XCC_ID is 4 bits wide
constexpr int kCusPerXcd = 32;
constexpr int kWgPerCu = 2;        // default workgroups per CU of a read launch
constexpr int kHeadStrideWords = 32;  // one 128-byte line per XCD's head word
constexpr size_t kHeadsBytes = (size_t)kMaxXcds * kHeadStrideWords * 4;
constexpr int kSlowOff = -1;       // slow_xcd: no injection
constexpr uint32_t kMaxSlowFactor = 64;
constexpr uint64_t kMinSpanTicks = 10000;  // 100 us of the 100 MHz counter
constexpr uint32_t kMfmaPerBatch = 8 * 64;  // per wave: 64 rounds of clock_probe_kernel's 8 MFMAs
constexpr uint32_t kMaxMfmaBatches = 1u << 16;

constexpr int kLevelL2 = 0, kLevelMall = 1, kLevelHbm = 2, kLevelMfma = 3, kLevels = 4;
constexpr int kModeAlone = 0, kModeTogether = 1, kModes = 2;
inline const char* level_name(int l) {
  static const char* const n[kLevels] = {"l2", "mall", "hbm", "mfma"};
  return l >= 0 && l < kLevels ? n[l] : "?";
}
inline const char* mode_name(int m) { return m == kModeAlone ? "alone" : m == kModeTogether ? "together" : "?"; }
inline const char* unit_of(int level) { return level == kLevelMfma ? "GMFMA/s" : "GB/s"; }

// MiB per XCD of a level; the levels are named by size, not by a residency claim.
inline uint32_t level_mib(int level, uint32_t hbm_mib) {
  const uint32_t m = level == kLevelL2 ? 1u : level == kLevelMall ? 16u : hbm_mib;
  return std::min(m, hbm_mib);
}

// One per workgroup, written by lane 0 with vector stores at the workgroup's end. A
// workgroup whose XCD is not in the launch's mask writes the identity words and tiles = 0.
struct Record {
  uint32_t magic;      // kMagic
  uint32_t hw_id;      // raw HW_REG_HW_ID of wave 0
  uint32_t xcc_id;     // raw HW_REG_XCC_ID
  uint32_t wg;         // blockIdx.x
  uint32_t tiles;      // read: 64 KiB tiles pulled; mfma: MFMAs of the workgroup's 4 waves
  uint32_t bad_words;  // 8-byte words that differed from the pattern
  uint32_t rt_ticks;   // s_memrealtime (100 MHz): first pull -> last load landed
  uint32_t cycles;     // s_memtime (shader clock) over the same span
  uint64_t rt_start;   // s_memrealtime at the first pull
  uint64_t first_off;  // byte offset in the XCD's slice of the lowest bad word
  uint64_t expected;   // of that word
  uint64_t got;
};
static_assert(sizeof(Record) == 64, "one 64-byte record per workgroup");

// (xcc, se, sh, cu) packed as K5's cu_key does (cu_sweep_plan.hpp).
inline uint32_t cu_key(uint32_t hw_id, uint32_t xcc_id) {
  return ((xcc_id & 0xFu) << 8) | (((hw_id >> 13) & 0x7u) << 5) | (((hw_id >> 12) & 0x1u) << 4) |
         ((hw_id >> 8) & 0xFu);
}

// Which cells the rate rule judges; every cell is measured and reported. With all XCDs
// contending for the Infinity Cache and HBM the healthy min / median moved by more than 0.1
// between sessions (mall / together 0.84 - 0.97, hbm / together 0.76 - 0.92:
// profiles/xcd_sweep/README.md), so these two are left out of the verdict.
inline bool gated(int level, int mode) {
  return !(mode == kModeTogether && (level == kLevelMall || level == kLevelHbm));
}

// ---- slice / tile arithmetic. The buffer is `xcds` equal slices, slice x from byte
// x * slice_bytes; a launch reads passes * tiles_per_slice tiles of every slice in its mask.
inline uint32_t xcds_expected(uint32_t cus) { return cus / kCusPerXcd; }
inline bool slice_ok(uint64_t slice_bytes) {
  return slice_bytes >= kTileBytes && slice_bytes % kTileBytes == 0 && slice_bytes / kTileBytes <= (1u << 20);
}
inline uint32_t tiles_per_slice(uint64_t slice_bytes) { return (uint32_t)(slice_bytes / kTileBytes); }
inline bool passes_ok(uint64_t slice_bytes, uint32_t passes) {  // the head word and Record::tiles are 32 bit
  return passes >= 1 && (uint64_t)passes * tiles_per_slice(slice_bytes) < (1ull << 31);
}
inline uint64_t expected_tiles(uint64_t slice_bytes, uint32_t passes) {
  return (uint64_t)passes * tiles_per_slice(slice_bytes);
}
inline uint32_t grid_of(uint32_t xcds, uint32_t wg_per_cu) { return xcds * kCusPerXcd * wg_per_cu; }
inline uint32_t full_mask(uint32_t xcds) { return xcds >= 32 ? ~0u : (1u << xcds) - 1u; }
// The passes that stretch a span of `ticks` at `passes` to kMinSpanTicks, with a factor 2 in
// hand. ticks = 0: nothing was timed, so there is nothing to size from and the passes stay.
inline uint32_t passes_for_min_span(uint32_t passes, uint64_t ticks) {
  if (ticks == 0 || ticks >= kMinSpanTicks) return passes;
  const uint64_t p = ((uint64_t)passes * 2 * kMinSpanTicks + ticks - 1) / ticks;
  return (uint32_t)std::min<uint64_t>(p, 1u << 20);
}

// ---- aggregation: one row per XCD
struct XcdRow {
  uint32_t xcd = 0;
  bool judged = false;       // in the launch's mask
  uint32_t workgroups = 0;   // records of this XCD
  uint32_t pullers = 0;      // of them, with tiles > 0
  uint32_t cus = 0;          // distinct CUs that ran a workgroup
  uint64_t tiles = 0, bytes = 0;
  uint64_t span_ticks = 0;   // max end - min start over this XCD's pullers only
  double rate = 0;           // GB/s, or GMFMA/s at level mfma
  double clock_ghz = 0;      // median over the pullers of cycles / ticks * 0.1
  uint64_t bad_words = 0;
  bool has_first = false;
  uint64_t first_off = 0, expected = 0, got = 0;
  bool slow = false;
  std::string failure;       // this XCD's first failure, empty = clean
};

struct Summary {
  int gpu = 0, level = 0, mode = 0;
  uint32_t xcds = 0, mask = 0;
  uint64_t expected = 0;     // tiles every judged XCD must pull; 0 = not checked (mfma)
  double ratio = 0;
  uint32_t records = 0, unwritten = 0, strays = 0;  // strays: XCC_ID >= xcds
  bool rule_ran = false;
  std::string rule_skipped;  // why not
  double median_rate = 0, min_rate = 0, min_over_median = 0, median_clock = 0;
  std::vector<XcdRow> rows;  // xcds of them
  std::vector<uint32_t> slow, bad;  // XCDs failed by the rule / with wrong data
  std::vector<std::string> failures;
  bool ok() const { return failures.empty(); }
};

inline double median_of(std::vector<double> v) {  // even count: the mean of the middle two
  if (v.empty()) return 0;
  std::sort(v.begin(), v.end());
  const size_t n = v.size();
  return n % 2 ? v[n / 2] : 0.5 * (v[n / 2 - 1] + v[n / 2]);
}

inline std::string hex(uint64_t v) {
  char b[24];
  std::snprintf(b, sizeof b, "0x%llx", (unsigned long long)v);
  return b;
}
inline std::string fixed(double v, int digits) {
  char b[40];
  std::snprintf(b, sizeof b, "%.*f", digits, v);
  return b;
}
inline std::string clip(std::string m) {  // the termination message cuts at 200
  if (m.size() > 199) m.resize(199);
  return m;
}

// Records of one launch, or of several launches with disjoint masks concatenated (mode
// alone: an XCD pulls tiles in one of them only), `mask` the union. Stamps of different
// XCDs are never compared: every span is taken over the XCD's own pullers.
inline Summary summarize(const Record* r, size_t n, int level, int mode, uint32_t xcds, uint32_t mask,
                         uint64_t expected, double ratio, int gpu) {
  Summary s;
  s.gpu = gpu, s.level = level, s.mode = mode, s.ratio = ratio, s.expected = expected;
  s.xcds = std::min<uint32_t>(xcds, kMaxXcds);
  s.mask = mask & full_mask(s.xcds);
  s.records = (uint32_t)n;
  s.rows.resize(s.xcds);
  std::vector<std::set<uint32_t>> cus(s.xcds);
  std::vector<std::vector<double>> clocks(s.xcds);
  std::vector<uint64_t> start(s.xcds, ~0ull), end(s.xcds, 0);
  for (size_t i = 0; i < n; ++i) {
    if (r[i].magic != kMagic) {
      ++s.unwritten;
      continue;
    }
    const uint32_t x = r[i].xcc_id & 0xFu;
    if (x >= s.xcds) {
      ++s.strays;
      continue;
    }
    XcdRow& row = s.rows[x];
    ++row.workgroups;
    cus[x].insert(cu_key(r[i].hw_id, r[i].xcc_id));
    if (r[i].bad_words) {
      if (!row.has_first || r[i].first_off < row.first_off)
        row.first_off = r[i].first_off, row.expected = r[i].expected, row.got = r[i].got;
      row.has_first = true;
      row.bad_words += r[i].bad_words;
    }
    if (!r[i].tiles) continue;
    ++row.pullers;
    row.tiles += r[i].tiles;
    start[x] = std::min(start[x], r[i].rt_start);
    end[x] = std::max(end[x], r[i].rt_start + r[i].rt_ticks);
    if (r[i].rt_ticks) clocks[x].push_back((double)r[i].cycles / (double)r[i].rt_ticks * 0.1);
  }
  const std::string at = std::string(" at ") + level_name(level) + "/" + mode_name(mode);
  const std::string head = "gpu" + std::to_string(gpu) + ": XCD sweep: ";
  std::vector<double> rates, clk;
  for (uint32_t x = 0; x < s.xcds; ++x) {
    XcdRow& row = s.rows[x];
    row.xcd = x;
    row.judged = (s.mask >> x) & 1u;
    row.cus = (uint32_t)cus[x].size();
    row.bytes = level == kLevelMfma ? 0 : row.tiles * kTileBytes;
    row.span_ticks = row.pullers ? end[x] - start[x] : 0;
    if (row.span_ticks) {
      const double sec = (double)row.span_ticks * 1e-8;
      row.rate = (level == kLevelMfma ? (double)row.tiles : (double)row.bytes) / sec * 1e-9;
    }
    row.clock_ghz = median_of(clocks[x]);
    if (!row.judged) continue;
    rates.push_back(row.rate);
    clk.push_back(row.clock_ghz);
  }
  s.median_rate = median_of(rates);
  s.median_clock = median_of(clk);
  s.min_rate = rates.empty() ? 0 : *std::min_element(rates.begin(), rates.end());
  s.min_over_median = s.median_rate > 0 ? s.min_rate / s.median_rate : 0;
  if (!(ratio > 0))
    s.rule_skipped = "ratio 0: report only";
  else if (rates.size() < 3)
    s.rule_skipped = "fewer than 3 XCDs (" + std::to_string(rates.size()) + "): no median to compare with";
  else
    s.rule_ran = true;

  // wrong data first, then coverage and conservation, then the rate rule
  for (XcdRow& row : s.rows) {
    if (!row.bad_words) continue;
    s.bad.push_back(row.xcd);
    row.failure = clip(head + "xcd " + std::to_string(row.xcd) + " read wrong data" + at + ": slice offset " +
                       hex(row.first_off) + ", expected " + hex(row.expected) + ", got " + hex(row.got) +
                       ", bad bits " + hex(row.expected ^ row.got) + "; " + std::to_string(row.bad_words) +
                       " word" + (row.bad_words == 1 ? "" : "s"));
    s.failures.push_back(row.failure);
  }
  if (s.unwritten)
    s.failures.push_back(clip(head + std::to_string(s.unwritten) + " of " + std::to_string(s.records) +
                              " workgroups wrote no record" + at));
  for (XcdRow& row : s.rows) {
    if (!row.judged) continue;
    std::string f;
    if (!row.workgroups)
      f = "xcd " + std::to_string(row.xcd) + " ran no workgroup" + at;
    else if (row.cus < (uint32_t)kCusPerXcd)
      f = "xcd " + std::to_string(row.xcd) + ": " + std::to_string(row.cus) + " of " +
          std::to_string(kCusPerXcd) + " CUs ran a workgroup" + at;
    else if (expected && row.tiles != expected)
      f = "xcd " + std::to_string(row.xcd) + " pulled " + std::to_string(row.tiles) + " tiles" + at +
          ", expected " + std::to_string(expected);
    else if (!row.pullers || !row.span_ticks)
      f = "xcd " + std::to_string(row.xcd) + " timed nothing" + at;
    if (f.empty()) continue;
    f = clip(head + f);
    if (row.failure.empty()) row.failure = f;
    s.failures.push_back(f);
  }
  if (s.rule_ran)
    for (XcdRow& row : s.rows) {
      if (!row.judged || !(row.rate < ratio * s.median_rate)) continue;
      row.slow = true;
      s.slow.push_back(row.xcd);
      const std::string f = clip(
          head + "xcd " + std::to_string(row.xcd) + " slow" + at + ": " + fixed(row.rate, 1) + " " +
          unit_of(level) + " vs median " + fixed(s.median_rate, 1) + " (" +
          fixed(s.median_rate > 0 ? row.rate / s.median_rate : 0, 2) + " < " + fixed(ratio, 2) +
          "); clock " + fixed(row.clock_ghz, 2) + " GHz vs median " + fixed(s.median_clock, 2));
      if (row.failure.empty()) row.failure = f;
      s.failures.push_back(f);
    }
  return s;
}

// The shortest span among the XCDs that timed something, 0 when none did. The passes are sized
// from this: an XCD that ran nothing is a failure of its own and must not stretch the others.
inline uint64_t min_timed_span(const Summary& s) {
  uint64_t m = 0;
  for (const XcdRow& r : s.rows)
    if (r.span_ticks && (!m || r.span_ticks < m)) m = r.span_ticks;
  return m;
}

// Empty when clean, else the first failure: one line under 200 characters.
inline std::string failure_message(const Summary& s) { return s.failures.empty() ? "" : s.failures[0]; }

inline std::string jstr(const std::string& v) {  // the messages hold no quote or backslash
  return "\"" + v + "\"";
}
inline std::string jnum(double v) {
  char b[40];
  std::snprintf(b, sizeof b, "%.6g", v);
  return b;
}
template <class T, class F>
inline std::string jlist(const std::vector<T>& v, F f) {
  std::string j = "[";
  for (size_t i = 0; i < v.size(); ++i) j += (i ? "," : "") + f(v[i]);
  return j + "]";
}
inline std::string rates_json(const Summary& s) {
  return jlist(s.rows, [](const XcdRow& r) { return jnum(r.rate); });
}
inline std::string clocks_json(const Summary& s) {
  return jlist(s.rows, [](const XcdRow& r) { return jnum(r.clock_ghz); });
}
inline std::string xcd_list_json(const std::vector<uint32_t>& v) {
  return jlist(v, [](uint32_t x) { return std::to_string(x); });
}

inline std::string summary_json(const Summary& s) {
  std::string j = "{\"ok\":" + std::string(s.ok() ? "true" : "false") + ",\"gpu\":" + std::to_string(s.gpu) +
                  ",\"level\":" + jstr(level_name(s.level)) + ",\"mode\":" + jstr(mode_name(s.mode)) +
                  ",\"unit\":" + jstr(unit_of(s.level)) + ",\"xcds\":" + std::to_string(s.xcds) +
                  ",\"mask\":" + std::to_string(s.mask) + ",\"expected_tiles\":" + std::to_string(s.expected) +
                  ",\"ratio\":" + jnum(s.ratio) + ",\"rule_ran\":" + (s.rule_ran ? "true" : "false") +
                  ",\"rule_skipped\":" + jstr(s.rule_skipped) + ",\"records\":" + std::to_string(s.records) +
                  ",\"unwritten\":" + std::to_string(s.unwritten) + ",\"strays\":" + std::to_string(s.strays) +
                  ",\"median_rate\":" + jnum(s.median_rate) + ",\"min_rate\":" + jnum(s.min_rate) +
                  ",\"min_over_median\":" + jnum(s.min_over_median) +
                  ",\"median_clock_ghz\":" + jnum(s.median_clock) + ",\"rates\":" + rates_json(s) +
                  ",\"clocks_ghz\":" + clocks_json(s) + ",\"slow\":" + xcd_list_json(s.slow) +
                  ",\"bad\":" + xcd_list_json(s.bad) + ",\"per_xcd\":";
  j += jlist(s.rows, [](const XcdRow& r) {
    std::string o = "{\"xcd\":" + std::to_string(r.xcd) + ",\"judged\":" + (r.judged ? "true" : "false") +
                    ",\"workgroups\":" + std::to_string(r.workgroups) + ",\"pullers\":" + std::to_string(r.pullers) +
                    ",\"cus\":" + std::to_string(r.cus) + ",\"tiles\":" + std::to_string(r.tiles) +
                    ",\"bytes\":" + std::to_string(r.bytes) + ",\"span_ticks\":" + std::to_string(r.span_ticks) +
                    ",\"rate\":" + jnum(r.rate) + ",\"clock_ghz\":" + jnum(r.clock_ghz) +
                    ",\"bad_words\":" + std::to_string(r.bad_words) + ",\"slow\":" + (r.slow ? "true" : "false") +
                    ",\"first\":";
    if (r.has_first)
      o += "{\"offset\":" + jstr(hex(r.first_off)) + ",\"expected\":" + jstr(hex(r.expected)) +
           ",\"got\":" + jstr(hex(r.got)) + ",\"bad_bits\":" + jstr(hex(r.expected ^ r.got)) + "}";
    else
      o += "null";
    return o + ",\"failure\":" + jstr(r.failure) + "}";
  });
  j += ",\"failures\":" + jlist(s.failures, [](const std::string& f) { return jstr(f); });
  return j + ",\"message\":" + jstr(failure_message(s)) + "}";
}

}  // namespace xcs
}  // namespace ntm
