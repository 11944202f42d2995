// K4: HBM pattern test kernels for the validation Job - write a pattern that
// is a function of the address over (nearly) all of HBM, read it back and
// compare on the device. K2 (aux_kernels.hpp) measures the streams' rate on
// 2 GiB; these check that every tested byte holds what was put there.
//
// Same access shape as the tuned K2 copy: 256 threads, 16 B per lane per
// access, nontemporal loads and stores, size_t indexing, a block owns one
// 256*U-vector tile (the host launches one block per tile; the loop only runs
// again beyond 2^31 - 1 tiles), the sub-tile tail is spread over the grid.
// U = kWriteUnroll / kVerifyUnroll below.
//
// The pattern, with w = (base_bytes + byte offset) / 4 the 64-bit global index
// of a 32-bit word, lo / hi its halves (base_bytes is the caller's logical
// offset, so a test in chunks covers one address space):
//   ADDR (0)  each 8-byte word = its global 8-byte index (w / 2) ^ seed (64 bit):
//             unique over all of HBM, so an aliasing address range shows
//   HASH (1)  each 32-bit word: x = lo + (uint32)seed; x ^= x >> 16;
//             x *= 0x7feb352d; x ^= x >> 15; x ^= hi * 0x9E3779B9
//   invert    XORs every bit.
// ALU budget: ~90 full-rate VALU lane-slots per 16 B at 7 TB/s; HASH spends 4
// 32-bit multiplies (quarter rate) per 16 B plus one per lane for hi, ADDR
// none; no 64-bit multiply anywhere in the loops.
//
// A mismatch is rare and slow on purpose: the healthy path executes no atomic
// and (verify) no store.
#pragma once

#include "ntm/common.hpp"
#include "ntm/hbm_test_plan.hpp"

namespace ntm {
namespace hbm {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

// float4 per lane per tile, measured on MI355X at 4 GiB (profiles/hbm_memtest/): the
// write is fastest with one 4 KiB tile per block (6.8 TB/s; 6.0 / 5.9 / 5.5 at 2 / 4 / 8),
// the verify kernels run at the rate of the K2 read and copy at 2, the K2 copy's shape.
constexpr int kWriteUnroll = 1;
constexpr int kVerifyUnroll = 2;

// The 4 words at 32-bit word index w0 (a multiple of 4, so neither w0 + 3 nor
// the 8-byte index w0 / 2 + 1 carries into the upper half).
template <int PAT>
__device__ __forceinline__ u32x4 pattern_vec(uint64_t w0, uint64_t seed, uint32_t inv) {
  u32x4 v;
  if constexpr (PAT == kPatternAddr) {
    const uint64_t q = w0 >> 1;
    const uint32_t ql = (uint32_t)q ^ (uint32_t)seed;
    const uint32_t qh = (uint32_t)(q >> 32) ^ (uint32_t)(seed >> 32);
    v = u32x4{ql, qh, ql ^ 1u, qh};  // q is even: (q + 1) ^ s == (q ^ s) ^ 1
  } else {
    const uint32_t lo = (uint32_t)w0 + (uint32_t)seed;
    const uint32_t hm = (uint32_t)(w0 >> 32) * 0x9E3779B9u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      uint32_t x = lo + (uint32_t)j;
      x ^= x >> 16;
      x *= 0x7feb352du;
      x ^= x >> 15;
      v[j] = x ^ hm;
    }
  }
  return v ^ inv;
}

template <int PAT, int U>
__global__ void __launch_bounds__(256)
    hbm_pattern_write_kernel(u32x4* __restrict__ ptr, size_t n4, uint64_t base_w, uint64_t seed,
                             uint32_t inv) {
  constexpr size_t kTile = 256 * U;
  const size_t ntiles = n4 / kTile;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t i0 = t * kTile + threadIdx.x;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const size_t i = i0 + (size_t)j * 256;
      __builtin_nontemporal_store(pattern_vec<PAT>(base_w + 4 * i, seed, inv), ptr + i);
    }
  }
  for (size_t i = ntiles * kTile + (size_t)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * 256)
    __builtin_nontemporal_store(pattern_vec<PAT>(base_w + 4 * i, seed, inv), ptr + i);
}

// The slow path: d = expected ^ got of one 16-byte vector with a bit set.
__device__ __noinline__ void pattern_report(PatternResult* out, uint64_t logical_off, u32x4 e,
                                            u32x4 d) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint64_t diff = (uint64_t)d[2 * h] | ((uint64_t)d[2 * h + 1] << 32);
    if (!diff) continue;
    const uint64_t exp = (uint64_t)e[2 * h] | ((uint64_t)e[2 * h + 1] << 32);
    const uint64_t off = logical_off + 8 * h;
    atomicAdd((unsigned long long*)&out->bad_words, 1ull);
    atomicOr((unsigned long long*)&out->bad_bits_or, (unsigned long long)diff);
    atomicMin((unsigned long long*)&out->first_bad_offset, (unsigned long long)off);
    if (*(volatile uint32_t*)&out->n_records < (uint32_t)kMaxRecords) {
      const uint32_t slot = atomicAdd(&out->n_records, 1u);
      if (slot < (uint32_t)kMaxRecords) {
        out->records[slot].offset = off;
        out->records[slot].expected = exp;
        out->records[slot].got = exp ^ diff;
      }
    }
  }
}

// Reads and compares; INV also stores the complement of the expected pattern
// in place (moving inversions: one pass where write + verify would be two).
template <int PAT, int U, bool INV>
__global__ void __launch_bounds__(256)
    hbm_pattern_verify_kernel(u32x4* __restrict__ ptr, size_t n4, uint64_t base_w, uint64_t seed,
                              uint32_t inv, PatternResult* __restrict__ out) {
  constexpr size_t kTile = 256 * U;
  const size_t ntiles = n4 / kTile;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t i0 = t * kTile + threadIdx.x;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = __builtin_nontemporal_load(ptr + i0 + (size_t)j * 256);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const size_t i = i0 + (size_t)j * 256;
      const u32x4 e = pattern_vec<PAT>(base_w + 4 * i, seed, inv);
      const u32x4 d = v[j] ^ e;
      if (d.x | d.y | d.z | d.w) pattern_report(out, (base_w + 4 * i) * 4, e, d);
      if constexpr (INV) __builtin_nontemporal_store(~e, ptr + i);
    }
  }
  for (size_t i = ntiles * kTile + (size_t)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * 256) {
    const u32x4 g = __builtin_nontemporal_load(ptr + i);
    const u32x4 e = pattern_vec<PAT>(base_w + 4 * i, seed, inv);
    const u32x4 d = g ^ e;
    if (d.x | d.y | d.z | d.w) pattern_report(out, (base_w + 4 * i) * 4, e, d);
    if constexpr (INV) __builtin_nontemporal_store(~e, ptr + i);
  }
}

}  // namespace hbm
}  // namespace ntm
