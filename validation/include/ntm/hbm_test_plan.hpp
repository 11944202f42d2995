// K4 (HBM pattern test) host side: the error record the device kernels fill,
// the chunk plan and the failure message. Pure C++ - no HIP - so the Job, the
// kernels' header (ntm/hbm_pattern.hpp) and a CPU-only test program share it.
//
// The plan: the tested space is `tested_bytes` of logical addresses 0 ..
// tested_bytes, cut into chunks of at most 16 GiB (so a chunk's float4 count
// stays below 2^32) and, but for a last remainder, at least 1 GiB: each chunk is
// written completely before it is read back, and 1 GiB is far beyond the
// 256 MiB Infinity Cache + 32 MiB L2 that could otherwise serve the read.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace ntm {
namespace hbm {

constexpr int kPatternAddr = 0;  // each 8-byte word = its own global 8-byte index ^ seed
constexpr int kPatternHash = 1;  // each 32-bit word = a multiplicative hash of its global index

constexpr int kMaxRecords = 4;

struct PatternRecord {
  uint64_t offset;    // logical byte offset (base_bytes + offset in the buffer) of the 8-byte word
  uint64_t expected;
  uint64_t got;
};

// One per verify launch (or per step: the kernels only ever add to it).
// Touched only on a mismatch. Initialise with pattern_result_init().
struct alignas(64) PatternResult {
  uint64_t bad_words;         // 8-byte words that differ
  uint64_t bad_bits_or;       // OR of expected ^ got over them
  uint64_t first_bad_offset;  // smallest logical byte offset of one; all ones = none
  uint32_t n_records;         // mismatches that asked for a record slot (may exceed kMaxRecords)
  uint32_t pad;
  PatternRecord records[kMaxRecords];
};
static_assert(sizeof(PatternResult) == 128, "PatternResult is one 128-byte record");

inline void pattern_result_init(PatternResult& r) {
  r = PatternResult{};
  r.first_bad_offset = ~0ull;
}

constexpr uint64_t kGiB = 1ull << 30;
constexpr uint64_t kMaxChunkBytes = 16 * kGiB;
constexpr uint64_t kMinChunkBytes = 1 * kGiB;
constexpr size_t kMaxChunks = 1024;  // 1 - 16 TiB: bounds the list whatever "free" claims

// What stays untouched: 2 GiB or 2 % of the free memory, whichever is larger
// (the runtime's own allocations, RCCL's later buffers, fragmentation).
inline uint64_t default_headroom(uint64_t free_bytes) {
  const uint64_t pct = free_bytes / 50;
  return pct > 2 * kGiB ? pct : 2 * kGiB;
}

struct TestPlan {
  uint64_t requested_bytes = 0;  // what was asked for (for < 0: all that may be tested)
  uint64_t tested_bytes = 0;     // sum of chunks, <= free - headroom
  uint64_t headroom_bytes = 0;
  std::vector<uint64_t> chunks;  // bytes, each a multiple of 16
};

// requested_gb in units of 1e9 bytes (as every other *_gb of the Job); < 0 =
// all free memory minus the headroom, 0 = nothing. A request above what is
// free is clamped, not refused. max_chunk is held to 1 .. 16 GiB, the list
// to kMaxChunks chunks (tested_bytes then stays below the request).
inline TestPlan make_test_plan(uint64_t free_bytes, double requested_gb, uint64_t headroom_bytes,
                               uint64_t max_chunk = kMaxChunkBytes) {
  TestPlan p;
  p.headroom_bytes = headroom_bytes;
  const uint64_t avail = free_bytes > headroom_bytes ? free_bytes - headroom_bytes : 0;
  if (requested_gb < 0)
    p.requested_bytes = avail;
  else if (requested_gb * 1e9 >= 1.8e19)
    p.requested_bytes = ~0ull;
  else
    p.requested_bytes = (uint64_t)(requested_gb * 1e9);
  uint64_t want = (p.requested_bytes < avail ? p.requested_bytes : avail) & ~15ull;
  if (max_chunk > kMaxChunkBytes) max_chunk = kMaxChunkBytes;
  if (max_chunk < kMinChunkBytes) max_chunk = kMinChunkBytes;
  max_chunk &= ~15ull;
  while (want > 0 && p.chunks.size() < kMaxChunks) {
    const uint64_t c = want < max_chunk ? want : max_chunk;
    p.chunks.push_back(c);
    p.tested_bytes += c;
    want -= c;
  }
  return p;
}

inline TestPlan make_test_plan(uint64_t free_bytes, double requested_gb) {
  return make_test_plan(free_bytes, requested_gb, default_headroom(free_bytes));
}

inline std::string hex64(uint64_t v) {
  char b[24];
  std::snprintf(b, sizeof b, "0x%016llx", (unsigned long long)v);
  return b;
}

// "gpu3: HBM pattern test (hash verify): 1 bad word(s), first at byte offset 0x...:
// expected 0x..., got 0x..., bad bits 0x..." - words are 8 bytes, the offset is in the
// tested space. Kept under 200 characters: the termination message cuts there.
inline std::string failure_message(int gpu, const char* what, const PatternResult& r) {
  std::string m = "gpu" + std::to_string(gpu) + ": HBM pattern test (" + what + "): " +
                  std::to_string((unsigned long long)r.bad_words) +
                  " bad word(s), first at byte offset " + hex64(r.first_bad_offset);
  // the record of the first bad word, when it won a slot; else the first record
  const uint32_t n = r.n_records < (uint32_t)kMaxRecords ? r.n_records : (uint32_t)kMaxRecords;
  const PatternRecord* rec = nullptr;
  for (uint32_t i = 0; i < n; ++i)
    if (r.records[i].offset == r.first_bad_offset) rec = &r.records[i];
  if (!rec && n > 0) rec = &r.records[0];
  if (rec) {
    if (rec->offset != r.first_bad_offset) m += "; at " + hex64(rec->offset);
    m += ": expected " + hex64(rec->expected) + ", got " + hex64(rec->got);
  }
  return m + ", bad bits " + hex64(r.bad_bits_or);
}

}  // namespace hbm
}  // namespace ntm
