// K6 (host-link check) host side: the pattern word on the host, the chase
// permutation, the PCIe link state from sysfs and the failure messages. Pure
// C++ - no HIP - so the Job, the kernels' header (ntm/host_link.hpp) and a
// CPU-only test program share it.
#pragma once

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "ntm/hbm_test_plan.hpp"

namespace ntm {
namespace hostlink {

using hbm::kPatternAddr;
using hbm::kPatternHash;
using hbm::PatternResult;

// Blocks of the persistent push / pull kernels when the caller names none
// (measured: ntm/host_link.hpp, profiles/host_link/README.md), and the cap on
// what a caller may ask for.
constexpr int kPushBlocks = 16;
constexpr int kPullBlocks = 64;
constexpr int kMaxBlocks = 65536;

constexpr int kChaseSlotBytes = 64;  // one slot per hop: next index (8 B) + padding
constexpr uint32_t kChaseSlots = 1024;
constexpr uint32_t kChaseHops = 4096;

// ---- the pattern on the host (K4's definition, hbm_pattern.hpp, in integers).
// The 32-bit word at logical 32-bit word index w.
inline uint32_t pattern_word32(int pattern, uint64_t w, uint64_t seed, bool invert) {
  uint32_t x;
  if (pattern == kPatternAddr) {
    const uint64_t q = (w >> 1) ^ seed;
    x = (w & 1) ? (uint32_t)(q >> 32) : (uint32_t)q;
  } else {
    x = (uint32_t)w + (uint32_t)seed;
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x ^= (uint32_t)(w >> 32) * 0x9E3779B9u;
  }
  return invert ? ~x : x;
}

// The 8-byte word at logical byte offset `off` (a multiple of 8).
inline uint64_t pattern_word(int pattern, uint64_t off, uint64_t seed, bool invert) {
  const uint64_t w = off / 4;
  return (uint64_t)pattern_word32(pattern, w, seed, invert) |
         ((uint64_t)pattern_word32(pattern, w + 1, seed, invert) << 32);
}

// The slow path of the Job: compares `bytes` (a multiple of 8) of a host
// buffer with the pattern of logical bytes base .. base + bytes, filling a
// record exactly as the device's pattern_report does. Returns the bad words.
inline uint64_t host_check(const void* buf, uint64_t bytes, uint64_t base, int pattern,
                           uint64_t seed, bool invert, PatternResult& r) {
  hbm::pattern_result_init(r);
  const unsigned char* p = (const unsigned char*)buf;
  for (uint64_t o = 0; o + 8 <= bytes; o += 8) {
    uint64_t got;
    std::memcpy(&got, p + o, 8);
    const uint64_t exp = pattern_word(pattern, base + o, seed, invert);
    if (got == exp) continue;
    if (r.bad_words++ == 0) r.first_bad_offset = base + o;
    r.bad_bits_or |= got ^ exp;
    if (r.n_records < (uint32_t)hbm::kMaxRecords) r.records[r.n_records] = {base + o, exp, got};
    ++r.n_records;
  }
  return r.bad_words;
}

// ---- the chase permutation: Sattolo's algorithm, so next[] is one cycle of
// length n whatever the seed. splitmix64 is the generator.
inline uint64_t splitmix64(uint64_t& s) {
  uint64_t z = (s += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

inline std::vector<uint32_t> chase_permutation(uint32_t n, uint64_t seed) {
  std::vector<uint32_t> next(n);
  for (uint32_t i = 0; i < n; ++i) next[i] = i;
  uint64_t s = seed;
  for (uint32_t i = n; i-- > 1;) {  // i = n - 1 .. 1, j in 0 .. i - 1
    const uint32_t j = (uint32_t)(splitmix64(s) % i);
    const uint32_t t = next[i];
    next[i] = next[j];
    next[j] = t;
  }
  return next;
}

// Lays next[] out in `slots` (next.size() * kChaseSlotBytes bytes): slot i
// holds next[i] in its first 8 bytes, zeros behind.
inline void chase_fill(void* slots, const std::vector<uint32_t>& next) {
  std::memset(slots, 0, next.size() * (size_t)kChaseSlotBytes);
  for (size_t i = 0; i < next.size(); ++i) {
    const uint64_t v = next[i];
    std::memcpy((char*)slots + i * kChaseSlotBytes, &v, 8);
  }
}

// The slot `hops` steps behind `start`.
inline uint32_t chase_walk(const std::vector<uint32_t>& next, uint32_t start, uint64_t hops) {
  uint32_t i = start;
  for (uint64_t h = 0; h < hops; ++h) i = next[i];
  return i;
}

// ---- the link state from sysfs. Read only; a missing or unreadable file
// leaves its field unknown (< 0), never an error.
struct LinkState {
  double speed_gts = -1, max_speed_gts = -1;  // GT/s per lane
  int width = -1, max_width = -1;             // lanes
  int numa_node = -1;
  bool numa_known = false;
  bool known() const { return speed_gts > 0 && width > 0; }
};

inline bool read_first_line(const std::string& path, std::string& out) {
  std::ifstream f(path);
  return f && std::getline(f, out) && !out.empty();
}

// sysfs_root is "/sys" on a node; bus_id is hipDeviceGetPCIBusId's
// "0000:c1:00.0" (either letter case).
inline LinkState read_link_state(const std::string& sysfs_root, const std::string& bus_id) {
  std::string id = bus_id;
  for (char& c : id) c = (char)std::tolower((unsigned char)c);
  const std::string d = sysfs_root + "/bus/pci/devices/" + id + "/";
  LinkState s;
  std::string t;
  auto speed = [&](const char* name, double& v) {  // "32.0 GT/s PCIe"
    if (!read_first_line(d + name, t)) return;
    char* end = nullptr;
    const double x = std::strtod(t.c_str(), &end);
    if (end != t.c_str() && x > 0) v = x;
  };
  auto integer = [&](const char* name, int& v) -> bool {
    if (!read_first_line(d + name, t)) return false;
    char* end = nullptr;
    const long x = std::strtol(t.c_str(), &end, 10);
    if (end == t.c_str() || x < -1 || x > 4096) return false;
    v = (int)x;
    return true;
  };
  speed("current_link_speed", s.speed_gts);
  speed("max_link_speed", s.max_speed_gts);
  if (!integer("current_link_width", s.width) || s.width <= 0) s.width = -1;
  if (!integer("max_link_width", s.max_width) || s.max_width <= 0) s.max_width = -1;
  s.numa_known = integer("numa_node", s.numa_node);
  return s;
}

inline std::string fixed1(double v) {
  char b[32];
  std::snprintf(b, sizeof b, "%.1f", v);
  return b;
}

// "PCIe 16.0 GT/s x8, max 32.0 GT/s x16"; empty when the current state is unknown.
inline std::string link_string(const LinkState& s) {
  if (!s.known()) return "";
  std::string m = "PCIe " + fixed1(s.speed_gts) + " GT/s x" + std::to_string(s.width);
  if (s.max_speed_gts > 0 && s.max_width > 0)
    m += ", max " + fixed1(s.max_speed_gts) + " GT/s x" + std::to_string(s.max_width);
  return m;
}

// {"speed_gts":..,"width":..,"max_speed_gts":..,"max_width":..,"numa_node":..}
// with null for an unknown field; "null" when nothing at all could be read.
inline std::string link_json(const LinkState& s) {
  if (!s.known() && s.max_speed_gts <= 0 && s.max_width <= 0 && !s.numa_known) return "null";
  auto num = [](double v) { return v > 0 ? fixed1(v) : std::string("null"); };
  auto in = [](int v) { return v > 0 ? std::to_string(v) : std::string("null"); };
  return "{\"speed_gts\":" + num(s.speed_gts) + ",\"width\":" + in(s.width) +
         ",\"max_speed_gts\":" + num(s.max_speed_gts) + ",\"max_width\":" + in(s.max_width) +
         ",\"numa_node\":" + (s.numa_known ? std::to_string(s.numa_node) : std::string("null")) + "}";
}

// ---- the failure messages: one line each, under 200 characters (the
// termination message cuts there).
constexpr const char* kDirPush = "device->host write or host memory";
constexpr const char* kDirPull = "host->device read";

inline std::string hex(uint64_t v) {
  char b[24];
  std::snprintf(b, sizeof b, "0x%llx", (unsigned long long)v);
  return b;
}

// "gpu3: host link host->device read: 1 bad word(s), at byte 0x...: expected
// 0x..., got 0x..., bad bits 0x..." - words are 8 bytes, the offset is the first
// bad word's in the buffer's logical space. When that word won no record slot
// another word's record follows ("; at 0x...: expected ..."), unless the line
// would then reach 200 characters.
inline std::string data_failure_message(int gpu, const char* direction, const PatternResult& r) {
  const std::string head = "gpu" + std::to_string(gpu) + ": host link " + direction + ": " +
                           std::to_string((unsigned long long)r.bad_words) +
                           " bad word(s), at byte " + hex(r.first_bad_offset);
  const std::string tail = ", bad bits " + hex(r.bad_bits_or);
  const uint32_t n = r.n_records < (uint32_t)hbm::kMaxRecords ? r.n_records
                                                              : (uint32_t)hbm::kMaxRecords;
  const hbm::PatternRecord* rec = nullptr;
  for (uint32_t i = 0; i < n; ++i)
    if (r.records[i].offset == r.first_bad_offset) rec = &r.records[i];
  if (!rec && n > 0) rec = &r.records[0];
  std::string mid;
  if (rec) {
    if (rec->offset != r.first_bad_offset) mid = "; at " + hex(rec->offset);
    mid += ": expected " + hbm::hex64(rec->expected) + ", got " + hbm::hex64(rec->got);
    if (rec->offset != r.first_bad_offset && head.size() + mid.size() + tail.size() >= 200) mid.clear();
  }
  return head + mid + tail;
}

// "gpu3: host link 13.1 GB/s host->device below floor 40 (PCIe 16.0 GT/s x8,
// max 32.0 GT/s x16)"; the parenthesis only when the link state is known.
inline std::string rate_failure_message(int gpu, const char* direction, double gbps, double floor,
                                        const LinkState& s) {
  char f[32];
  std::snprintf(f, sizeof f, "%g", floor);
  std::string m = "gpu" + std::to_string(gpu) + ": host link " + fixed1(gbps) + " GB/s " +
                  direction + " below floor " + f;
  const std::string l = link_string(s);
  return l.empty() ? m : m + " (" + l + ")";
}

}  // namespace hostlink
}  // namespace ntm
