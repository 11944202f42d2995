// K9 (atomics and cross-XCD hand-off check) host side: the op list, the map from an
// operation's number to its slot and operand, the exactness bounds of the float adds,
// the expected tables, the hand-off record, the grid / episode arithmetic, the verdicts
// and the failure messages. Pure C++ - no HIP - so the Job, the kernels' header
// (ntm/atomics.hpp) and a CPU-only test program share it. Functions the kernels also
// call carry NTM_HD.
//
// rmw: operation k = gid * iters + it hits slot k % slots with operand_bits(op, k, ...).
// Integer results do not depend on the order. Float operands are small integers, so
// every partial sum is an integer the format holds exactly and the result does not
// depend on the order either (atomics_exact). A packed slot is two 16-bit cells: op k
// adds its value to cell (k / slots) & 1 and +0 to the other, so a cell takes every
// second add of its slot and the bound holds per cell. cas: every contender tries
// 0 -> k + 1 once; the launch then maps the winner to slot + 1 when it is one of the
// slot's own contenders, which makes the table comparable.
//
// tickets: `heads` counters; thread gid draws ticket number it from head
// (gid + it) % heads and stores gid into claim[head][ticket].
//
// handoff: episodes of E consecutive workgroups; the last arriver of an episode reads
// what the other E - 1 wrote (Record below).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#if defined(__HIPCC__)
#define NTM_HD __host__ __device__
#else
#define NTM_HD
#endif

namespace ntm {
namespace atm {

constexpr uint32_t kMagic = 0x4B394154u;      // a hand-off record the kernel has written
constexpr uint32_t kSlabMagic = 0x51AB0000u;  // + round: first word of a slab's header
constexpr int kThreads = 256;
constexpr int kMaxXcds = 16;                  // HW_REG_XCC_ID is 4 bits wide
constexpr uint32_t kSlabBytes = 4096;         // one 16-byte word per thread
constexpr uint32_t kSlabWords = kSlabBytes / 16;
constexpr int kLineWords = 32;                // counters sit on 128-byte lines of their own
constexpr uint32_t kSentinel = 0xFFFFFFFFu;   // a claim entry nobody wrote
constexpr uint32_t kMaxEpisodeSize = 64;
constexpr uint32_t kInjectOff = 0xFFFFFFFFu;  // inject_wg / inject_gid: none
constexpr uint32_t kStaleLineWord = 16;       // stale_handoff: 16-byte words 16 .. 19 of the slab
constexpr int kClassNone = 0, kClassStale = 1, kClassCorrupt = 2;

enum Op : int {
  kAddU32, kAddU64, kAndU32, kOrU32, kXorU32, kMinI32, kMaxI32, kMaxU64, kCasU32,
  kAddF32, kAddF64, kAddBf16x2, kAddF16x2, kOps
};
inline const char* op_name(int op) {
  static const char* const n[kOps] = {"add_u32", "add_u64", "and_u32", "or_u32", "xor_u32", "min_i32", "max_i32",
                                      "max_u64", "cas_u32", "add_f32", "add_f64", "add_bf16x2", "add_f16x2"};
  return op >= 0 && op < kOps ? n[op] : "?";
}
NTM_HD inline bool is_float(int op) { return op >= kAddF32 && op < kOps; }
NTM_HD inline bool is_packed(int op) { return op == kAddBf16x2 || op == kAddF16x2; }
// cas: {claim word, success count}
NTM_HD inline uint32_t slot_bytes(int op) {
  return op == kAddU64 || op == kMaxU64 || op == kCasU32 || op == kAddF64 ? 8u : 4u;
}
NTM_HD inline uint64_t init_value(int op) {
  return op == kAndU32 ? 0xFFFFFFFFull : op == kMinI32 ? 0x7FFFFFFFull : op == kMaxI32 ? 0x80000000ull : 0ull;
}

// The float adds are exact in any order when no partial sum can leave the integers the
// format holds: adds x max |operand| < 2^24 (fp32), < 2^53 (fp64), <= 255 (bf16), <= 2047
// (fp16); a packed cell takes every second add of its slot. Integer ops: any shape.
inline bool atomics_exact(int op, uint64_t adds_per_slot, uint64_t max_abs) {
  if (op < 0 || op >= kOps) return false;
  if (!is_float(op)) return true;
  if (max_abs < 1) return false;
  const unsigned __int128 sum = (unsigned __int128)(is_packed(op) ? (adds_per_slot + 1) / 2 : adds_per_slot) * max_abs;
  return op == kAddF32 ? sum < ((unsigned __int128)1 << 24)
       : op == kAddF64 ? sum < ((unsigned __int128)1 << 53)
       : op == kAddBf16x2 ? sum <= 255 : sum <= 2047;
}

NTM_HD inline uint64_t hash64(uint64_t x) {  // splitmix64's finaliser
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}
NTM_HD inline uint64_t op_hash(uint64_t k, uint64_t seed) { return hash64(seed * 0x100000001B3ull ^ hash64(k)); }
NTM_HD inline uint64_t slot_of(uint64_t k, uint64_t slots) { return k % slots; }
// the small integer a float op adds: uniform in -max_abs .. max_abs
NTM_HD inline int64_t float_operand(uint64_t k, uint64_t seed, uint64_t max_abs) {
  return (int64_t)(op_hash(k, seed) % (2 * max_abs + 1)) - (int64_t)max_abs;
}
NTM_HD inline uint32_t f32_bits(float f) {
  uint32_t u;
  __builtin_memcpy(&u, &f, 4);
  return u;
}
NTM_HD inline uint64_t f64_bits(double f) {
  uint64_t u;
  __builtin_memcpy(&u, &f, 8);
  return u;
}
NTM_HD inline uint32_t bf16_bits_of_int(int v) { return f32_bits((float)v) >> 16; }  // |v| <= 256: exact
NTM_HD inline uint32_t f16_bits_of_int(int v) {                                       // |v| <= 2048: exact
  if (v == 0) return 0;
  const uint32_t a = (uint32_t)(v < 0 ? -v : v);
  int e = 0;
  while ((a >> (e + 1)) != 0) ++e;
  return (v < 0 ? 0x8000u : 0u) | ((uint32_t)(e + 15) << 10) | ((e <= 10 ? a << (10 - e) : a >> (e - 10)) & 0x3FFu);
}
// The operand of operation k as the bits the atomic takes (low 4 bytes for a 4-byte op).
NTM_HD inline uint64_t operand_bits(int op, uint64_t k, uint64_t seed, uint64_t max_abs, uint64_t slots) {
  const uint64_t h = op_hash(k, seed);
  switch (op) {
    case kAddU32: case kXorU32: case kMinI32: case kMaxI32: return (uint32_t)h;
    case kAddU64: case kMaxU64: return h;
    // one operation in eight clears (sets) one bit, the others none: bits survive hundreds of operations
    case kAndU32: return ((h >> 13) & 7u) ? 0xFFFFFFFFu : ~(1u << ((h >> 8) & 31u));
    case kOrU32: return ((h >> 13) & 7u) ? 0u : 1u << ((h >> 8) & 31u);
    case kCasU32: return (uint32_t)(k + 1);
    case kAddF32: return f32_bits((float)float_operand(k, seed, max_abs));
    case kAddF64: return f64_bits((double)float_operand(k, seed, max_abs));
    default: {
      const int v = (int)float_operand(k, seed, max_abs);
      const uint32_t b = op == kAddBf16x2 ? bf16_bits_of_int(v) : f16_bits_of_int(v);
      return ((k / slots) & 1u) ? b << 16 : b;
    }
  }
}

// What slot s holds after operations 0 .. total: folds k = s, s + slots, ... in order, with
// no atomic (the reference kernel runs this with one thread per slot, the host as it is).
NTM_HD inline uint64_t expected_slot(int op, uint64_t s, uint64_t slots, uint64_t total, uint64_t seed,
                                     uint64_t max_abs) {
  uint64_t acc = init_value(op);
  int64_t sum[2] = {0, 0};
  for (uint64_t k = s; k < total; k += slots) {
    const uint64_t v = is_float(op) ? 0 : operand_bits(op, k, seed, max_abs, slots);
    switch (op) {
      case kAddU32: acc = (uint32_t)(acc + v); break;
      case kAddU64: acc += v; break;
      case kAndU32: acc &= v; break;
      case kOrU32: acc |= v; break;
      case kXorU32: acc ^= v; break;
      case kMinI32: if ((int32_t)v < (int32_t)acc) acc = v; break;
      case kMaxI32: if ((int32_t)v > (int32_t)acc) acc = v; break;
      case kMaxU64: if (v > acc) acc = v; break;
      case kCasU32: if (acc == 0) acc = (1ull << 32) | (s + 1); break;  // the first contender wins, one success
      default: sum[is_packed(op) ? (k / slots) & 1u : 0] += float_operand(k, seed, max_abs);
    }
  }
  switch (op) {
    case kAddF32: return f32_bits((float)sum[0]);
    case kAddF64: return f64_bits((double)sum[0]);
    case kAddBf16x2: return bf16_bits_of_int((int)sum[0]) | (bf16_bits_of_int((int)sum[1]) << 16);
    case kAddF16x2: return f16_bits_of_int((int)sum[0]) | (f16_bits_of_int((int)sum[1]) << 16);
    default: return acc;
  }
}
// cas: the claim word of slot s as the launch leaves it. A winner that is one of the
// slot's own contenders becomes s + 1; anything else stays and compares unequal.
NTM_HD inline uint32_t cas_canonical(uint32_t claim, uint64_t s, uint64_t slots, uint64_t total) {
  return claim != 0 && (uint64_t)(claim - 1) < total && (uint64_t)(claim - 1) % slots == s ? (uint32_t)(s + 1) : claim;
}

inline bool rmw_shape_ok(int op, uint64_t slots, uint32_t grid, uint32_t iters, uint64_t max_abs) {
  if (op < 0 || op >= kOps || slots < 1 || slots > (1u << 24) || grid < 1 || iters < 1 || iters > (1u << 16)) return false;
  const uint64_t total = (uint64_t)grid * kThreads * iters;
  if (total >= (1ull << 32) || total % slots) return false;  // cas stores k + 1 in 32 bits
  return !is_float(op) || (max_abs < (1ull << 52) && atomics_exact(op, total / slots, max_abs));
}

// ---- tickets
inline bool ticket_shape_ok(uint32_t heads, uint32_t grid, uint32_t iters) {
  return heads >= 1 && heads <= 1024 && grid >= 1 && iters >= 1 && iters <= 4096 &&
         ((uint64_t)grid * kThreads) % heads == 0 && (uint64_t)grid * kThreads * iters < (1ull << 31);
}
NTM_HD inline uint32_t ticket_head(uint32_t gid, uint32_t it, uint32_t heads) { return (gid + it) % heads; }
inline uint64_t tickets_per_head(uint32_t heads, uint32_t grid, uint32_t iters) {
  return (uint64_t)grid * kThreads / heads * iters;
}

// ---- hand-off
inline bool handoff_shape_ok(uint32_t episodes, uint32_t e) {
  return episodes >= 1 && e >= 2 && e <= kMaxEpisodeSize && (uint64_t)episodes * e <= (1u << 20);
}
inline size_t handoff_slab_bytes(uint32_t episodes, uint32_t e) { return (size_t)episodes * e * kSlabBytes; }
inline size_t handoff_counter_bytes(uint32_t episodes) { return (size_t)episodes * kLineWords * 4; }
// the 32-bit seed of a round's pattern: consecutive rounds differ, so every word differs
NTM_HD inline uint32_t round_seed(uint64_t seed, uint32_t round) { return (uint32_t)seed + round * 0x9E3779B1u; }
NTM_HD inline uint32_t sleep_count(uint32_t wg, uint64_t seed, uint32_t round) {  // x s_sleep 8 (512 cycles)
  return (uint32_t)(hash64(seed ^ ((uint64_t)round << 32 | wg)) & 7u);
}

// One per workgroup, written by lane 0 with vector stores at the workgroup's end.
struct Record {
  uint32_t magic;          // kMagic
  uint32_t hw_id, xcc_id;  // raw HW_REG_HW_ID / HW_REG_XCC_ID of wave 0
  uint32_t wg;             // blockIdx.x
  uint32_t episode;
  uint32_t episodes_read;  // 1: this workgroup arrived last and read the episode
  uint32_t words_checked;  // 16-byte words the reader compared
  uint32_t bad_words;      // of them, different from this round's pattern
  uint32_t stale_words;    // of the bad ones, equal to last round's pattern
  uint32_t writer_mask;    // XCDs of the writers whose slabs the reader checked
  uint32_t warm_bad;       // words of the warm-up read that matched neither round
  uint32_t first_class;    // kClassNone / kClassStale / kClassCorrupt
  uint32_t writer_hw, writer_xcc, writer_wg;  // of the first bad word's slab
  uint32_t first_off;      // byte offset of the first bad 8 bytes in the episode's slabs
  uint64_t expected, got;  // those 8 bytes
  uint32_t ticket, sleeps, pad0, pad1;
};
static_assert(sizeof(Record) == 96, "six 16-byte words per workgroup");

struct CuPlace { uint32_t xcd, se, sh, cu; };
inline CuPlace place(uint32_t hw_id, uint32_t xcc_id) {  // as K5's decode (cu_sweep_plan.hpp)
  return {xcc_id & 0xFu, (hw_id >> 13) & 0x7u, (hw_id >> 12) & 0x1u, (hw_id >> 8) & 0xFu};
}

inline std::string hex(uint64_t v) {
  char b[24];
  std::snprintf(b, sizeof b, "0x%llx", (unsigned long long)v);
  return b;
}
inline std::string clip(std::string m) {  // the termination message cuts at 200
  if (m.size() > 199) m.resize(199);
  return m;
}
inline std::string jstr(const std::string& v) { return "\"" + v + "\""; }  // the messages hold no quote
inline std::string jlist(const std::vector<std::string>& v) {
  std::string j = "[";
  for (size_t i = 0; i < v.size(); ++i) j += (i ? "," : "") + jstr(v[i]);
  return j + "]";
}
constexpr size_t kMaxMessages = 8;  // per sub-test; the counts are complete

struct RmwSummary {
  int gpu = 0, op = 0;
  uint64_t slots = 0, bad_slots = 0;
  bool has_first = false;
  uint64_t first_slot = 0, expected = 0, got = 0;
  std::vector<std::string> failures;
  bool ok() const { return failures.empty(); }
};
// got / expected: `slots` words of slot_bytes(op), as the launches leave them
inline RmwSummary summarize_rmw(int op, const void* got, const void* expected, uint64_t slots, int gpu) {
  RmwSummary s;
  s.gpu = gpu, s.op = op, s.slots = slots;
  const bool wide = slot_bytes(op) == 8;
  for (uint64_t i = 0; i < slots; ++i) {
    const uint64_t g = wide ? ((const uint64_t*)got)[i] : ((const uint32_t*)got)[i];
    const uint64_t e = wide ? ((const uint64_t*)expected)[i] : ((const uint32_t*)expected)[i];
    if (g == e) continue;
    if (!s.has_first) s.has_first = true, s.first_slot = i, s.expected = e, s.got = g;
    if (++s.bad_slots <= kMaxMessages)
      s.failures.push_back(clip("gpu" + std::to_string(gpu) + ": atomics: " + op_name(op) + " slot " + std::to_string(i) +
                                ": expected " + hex(e) + ", got " + hex(g) + ", bad bits " + hex(e ^ g)));
  }
  return s;
}
inline std::string rmw_json(const RmwSummary& s) {
  return "{\"ok\":" + std::string(s.ok() ? "true" : "false") + ",\"gpu\":" + std::to_string(s.gpu) + ",\"op\":" +
         jstr(op_name(s.op)) + ",\"slots\":" + std::to_string(s.slots) + ",\"bad_slots\":" + std::to_string(s.bad_slots) +
         ",\"first\":" + (s.has_first ? "{\"slot\":" + std::to_string(s.first_slot) + ",\"expected\":" + jstr(hex(s.expected)) +
                                        ",\"got\":" + jstr(hex(s.got)) + ",\"bad_bits\":" + jstr(hex(s.expected ^ s.got)) + "}"
                                      : std::string("null")) +
         ",\"failures\":" + jlist(s.failures) + ",\"message\":" + jstr(s.failures.empty() ? "" : s.failures[0]) + "}";
}

struct TicketSummary {
  int gpu = 0;
  uint64_t missing = 0, duplicate = 0, invalid = 0, short_counters = 0;
  uint64_t bad() const { return missing + duplicate + invalid + short_counters; }
  std::vector<std::string> failures;
  bool ok() const { return failures.empty(); }
};
// counters: `heads` words kLineWords apart; claim: heads x per_head entries (a thread's gid,
// kSentinel where nobody wrote); every gid in 0 .. threads must hold exactly `iters` entries.
inline TicketSummary summarize_tickets(const uint32_t* counters, const uint32_t* claim, uint32_t heads,
                                       uint64_t per_head, uint32_t threads, uint32_t iters, int gpu) {
  TicketSummary s;
  s.gpu = gpu;
  const std::string head = "gpu" + std::to_string(gpu) + ": atomics: ticket: ";
  auto say = [&](const std::string& m) {
    if (s.failures.size() < kMaxMessages) s.failures.push_back(clip(head + m));
  };
  for (uint32_t h = 0; h < heads; ++h) {
    const uint64_t c = counters[(size_t)h * kLineWords];
    if (c == per_head) continue;
    ++s.short_counters;
    say("head " + std::to_string(h) + " counter " + (c < per_head ? "short" : "over") + ": " + std::to_string(c) +
        ", expected " + std::to_string(per_head));
  }
  std::vector<uint32_t> held(threads, 0);
  for (uint32_t h = 0; h < heads; ++h)
    for (uint64_t t = 0; t < per_head; ++t) {
      const uint32_t g = claim[(size_t)h * per_head + t];
      const std::string at = "head " + std::to_string(h) + " ticket " + std::to_string(t);
      if (g == kSentinel) {
        ++s.missing;
        say(at + " missing: nobody wrote the entry");
      } else if (g >= threads) {
        ++s.invalid;
        say(at + " invalid: holds " + hex(g) + ", no thread of the launch");
      } else if (++held[g] > iters) {
        ++s.duplicate;
        say(at + " duplicate: thread " + std::to_string(g) + " holds " + std::to_string(held[g]) + " entries, expected " +
            std::to_string(iters));
      }
    }
  return s;
}
inline std::string ticket_json(const TicketSummary& s) {
  return "{\"ok\":" + std::string(s.ok() ? "true" : "false") + ",\"gpu\":" + std::to_string(s.gpu) +
         ",\"missing\":" + std::to_string(s.missing) + ",\"duplicate\":" + std::to_string(s.duplicate) +
         ",\"invalid\":" + std::to_string(s.invalid) + ",\"short_counters\":" + std::to_string(s.short_counters) +
         ",\"bad\":" + std::to_string(s.bad()) + ",\"failures\":" + jlist(s.failures) + ",\"message\":" +
         jstr(s.failures.empty() ? "" : s.failures[0]) + "}";
}

struct HandoffSummary {
  int gpu = 0;
  uint32_t episodes = 0, e = 0, xcds = 0;
  uint32_t records = 0, unwritten = 0, readers = 0;
  uint64_t words_checked = 0, expected_words = 0, bad_words = 0, stale_words = 0, warm_bad = 0;
  uint32_t xcd_pairs_covered = 0, cross_pairs = 0;
  std::vector<uint8_t> pairs;  // kMaxXcds x kMaxXcds, [writer][reader]
  std::vector<std::string> failures;
  bool ok() const { return failures.empty(); }
};
// Records of one launch (or of several rounds of the same shape, concatenated: `launches`).
inline HandoffSummary summarize_handoff(const Record* r, size_t n, uint32_t episodes, uint32_t e, uint32_t xcds,
                                        uint32_t launches, int gpu) {
  HandoffSummary s;
  s.gpu = gpu, s.episodes = episodes, s.e = e, s.xcds = std::min<uint32_t>(xcds, kMaxXcds);
  s.records = (uint32_t)n;
  s.expected_words = (uint64_t)launches * episodes * e * kSlabWords;
  s.pairs.assign((size_t)kMaxXcds * kMaxXcds, 0);
  const std::string head = "gpu" + std::to_string(gpu) + ": atomics: handoff: ";
  auto say = [&](const std::string& m) {
    if (s.failures.size() < kMaxMessages) s.failures.push_back(clip(head + m));
  };
  std::vector<uint32_t> readers_of((size_t)episodes, 0);
  for (size_t i = 0; i < n; ++i) {
    if (r[i].magic != kMagic) {
      ++s.unwritten;
      continue;
    }
    s.warm_bad += r[i].warm_bad;
    if (!r[i].episodes_read) continue;
    ++s.readers;
    if (r[i].episode < episodes) ++readers_of[r[i].episode];
    s.words_checked += r[i].words_checked;
    s.bad_words += r[i].bad_words;
    s.stale_words += r[i].stale_words;
    const uint32_t rx = r[i].xcc_id & 0xFu;
    for (uint32_t w = 0; w < (uint32_t)kMaxXcds; ++w)
      if ((r[i].writer_mask >> w) & 1u) s.pairs[(size_t)w * kMaxXcds + rx] = 1;
    if (r[i].bad_words) {
      const CuPlace rd = place(r[i].hw_id, r[i].xcc_id), wr = place(r[i].writer_hw, r[i].writer_xcc);
      say(std::string(r[i].first_class == kClassStale ? "stale" : "corrupt") + " word: reader xcd " + std::to_string(rd.xcd) +
          " se " + std::to_string(rd.se) + " cu " + std::to_string(rd.cu) + ", writer xcd " + std::to_string(wr.xcd) +
          " cu " + std::to_string(wr.cu) + " (workgroup " + std::to_string(r[i].writer_wg) + "), episode " +
          std::to_string(r[i].episode) + ", offset " + hex(r[i].first_off) + ", expected " + hex(r[i].expected) +
          ", got " + hex(r[i].got) + "; " + std::to_string(r[i].bad_words) + " bad, " +
          std::to_string(r[i].stale_words) + " stale");
    }
  }
  for (uint32_t w = 0; w < (uint32_t)kMaxXcds; ++w)
    for (uint32_t x = 0; x < (uint32_t)kMaxXcds; ++x)
      if (s.pairs[(size_t)w * kMaxXcds + x]) ++s.xcd_pairs_covered, s.cross_pairs += w != x;
  if (s.unwritten) say(std::to_string(s.unwritten) + " of " + std::to_string(s.records) + " workgroups wrote no record");
  if (s.warm_bad) say(std::to_string(s.warm_bad) + " words of the warm-up read matched neither round's pattern");
  for (uint32_t ep = 0; ep < episodes; ++ep)
    if (readers_of[ep] != launches)
      say("episode " + std::to_string(ep) + " had " + std::to_string(readers_of[ep]) + " readers, expected " +
          std::to_string(launches));
  if (s.words_checked != s.expected_words)
    say(std::to_string(s.words_checked) + " words checked, expected " + std::to_string(s.expected_words));
  if (s.xcds > 1 && s.cross_pairs == 0)
    say("no cross-XCD pair was checked on " + std::to_string(s.xcds) + " XCDs: the run proved nothing");
  return s;
}
inline std::string handoff_json(const HandoffSummary& s) {
  std::string m = "[";
  for (uint32_t w = 0; w < s.xcds; ++w) {
    m += w ? ",[" : "[";
    for (uint32_t x = 0; x < s.xcds; ++x) m += (x ? "," : "") + std::to_string((int)s.pairs[(size_t)w * kMaxXcds + x]);
    m += "]";
  }
  return "{\"ok\":" + std::string(s.ok() ? "true" : "false") + ",\"gpu\":" + std::to_string(s.gpu) +
         ",\"episodes\":" + std::to_string(s.episodes) + ",\"episode_size\":" + std::to_string(s.e) +
         ",\"xcds\":" + std::to_string(s.xcds) + ",\"records\":" + std::to_string(s.records) +
         ",\"unwritten\":" + std::to_string(s.unwritten) + ",\"readers\":" + std::to_string(s.readers) +
         ",\"words_checked\":" + std::to_string(s.words_checked) + ",\"expected_words\":" + std::to_string(s.expected_words) +
         ",\"bad_words\":" + std::to_string(s.bad_words) + ",\"stale_words\":" + std::to_string(s.stale_words) +
         ",\"warm_bad\":" + std::to_string(s.warm_bad) + ",\"xcd_pairs_covered\":" + std::to_string(s.xcd_pairs_covered) +
         ",\"cross_xcd_pairs\":" + std::to_string(s.cross_pairs) + ",\"pairs\":" + m + "]" +
         ",\"failures\":" + jlist(s.failures) + ",\"message\":" + jstr(s.failures.empty() ? "" : s.failures[0]) + "}";
}

}  // namespace atm
}  // namespace ntm
