// K6: host-link (PCIe) check kernels for the validation Job - the GPU writes K4's
// pattern into pinned, device-mapped host memory (device->host), reads host
// memory back and compares on the device (host->device), and follows a pointer
// chain through host memory for the link's read round-trip latency.
//
// The pattern is K4's (hbm_pattern.hpp: pattern_vec<PAT>, ADDR / HASH, seed,
// invert, the logical base; a mismatch goes through pattern_report into the
// 128-byte PatternResult), so a host buffer and an HBM buffer speak the same
// words and reference.hbm_pattern_words describes both.
//
// Not K4's launch shape. One 4 KiB tile per block over 64 Ki blocks is tuned
// for a 7 TB/s stream; a ~60 GB/s link with a microsecond-class round trip is
// bound by the bytes in flight. These are persistent grid-stride kernels: the
// host picks a fixed number of blocks, a block walks tiles of 256 * U vectors
// (16 B per lane per access), the sub-tile tail is spread over the grid, every
// index is a size_t. Knobs: blocks, U, nontemporal (NT) against default
// accesses. Measured defaults: see the constants below.
//
// The healthy pull path executes no atomic and no store (STORE writes what it
// read to an HBM destination so a test can look at the bytes that arrived).
#pragma once

#include "ntm/hbm_pattern.hpp"
#include "ntm/host_link_plan.hpp"

namespace ntm {
namespace hostlink {

using hbm::PatternResult;
using hbm::pattern_report;
using hbm::pattern_vec;
using hbm::u32x4;

// Defaults from the sweep of tools/host_link_rates.py on an MI355X (PCIe 32 GT/s
// x16) at 256 MiB, 7 interleaved rounds, medians (profiles/host_link/README.md;
// blocks 16 .. 2048 x U 1 / 2 / 4 / 8 x NT, hipMemcpyAsync on the same buffers
// as two more candidates of every round):
//   push  hipMemcpyAsync 56.7 GB/s (55.5 - 56.8 over the rounds). Plain stores
//         beat nontemporal ones by 2 GB/s at every blocks x U (55.4 - 56.8
//         against 53.3 - 54.9); fewer blocks are faster (16: 56.7, 32: 56.1,
//         >= 64: 55.4 - 55.7) and U does not matter. 16 blocks, U = 4, plain:
//         56.75 = 1.00 of hipMemcpyAsync.
//   pull  hipMemcpyAsync 57.14 GB/s (57.13 - 57.17). NT and plain loads read
//         the same. The rate is flat at 57.0 - 57.5 from 256 KiB to 1 MiB in
//         flight (blocks x 4 KiB x U), drops to 48.9 at 64 KiB (16 blocks, U =
//         1: latency bound, 1.4 us per round trip) and to 55.3 - 55.9 from
//         2 MiB up. 64 blocks, U = 4 (1 MiB in flight, a factor 4 above the
//         knee for a link with a longer round trip): 57.44 = 1.005.
// kPushBlocks / kPullBlocks: host_link_plan.hpp.
constexpr int kPushUnroll = 4;
constexpr int kPullUnroll = 4;
constexpr bool kPushNontemporal = false;
constexpr bool kPullNontemporal = true;

template <bool NT>
__device__ __forceinline__ u32x4 link_load(const u32x4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT>
__device__ __forceinline__ void link_store(u32x4 v, u32x4* p) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

// device->host: the pattern of logical words base_w .. into host memory.
template <int PAT, int U, bool NT = kPushNontemporal>
__global__ void __launch_bounds__(256)
    host_link_push_kernel(u32x4* __restrict__ host, size_t n4, uint64_t base_w, uint64_t seed,
                          uint32_t inv) {
  constexpr size_t kTile = 256 * (size_t)U;
  const size_t ntiles = n4 / kTile;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t i0 = t * kTile + threadIdx.x;
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const size_t i = i0 + (size_t)j * 256;
      link_store<NT>(pattern_vec<PAT>(base_w + 4 * i, seed, inv), host + i);
    }
  }
  for (size_t i = ntiles * kTile + (size_t)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * 256)
    link_store<NT>(pattern_vec<PAT>(base_w + 4 * i, seed, inv), host + i);
}

// host->device: reads host memory, compares with the pattern; STORE also
// writes the bytes read to dst (HBM, n4 vectors).
template <int PAT, int U, bool STORE, bool NT = kPullNontemporal>
__global__ void __launch_bounds__(256)
    host_link_pull_kernel(const u32x4* __restrict__ host, size_t n4, uint64_t base_w,
                          uint64_t seed, uint32_t inv, u32x4* __restrict__ dst,
                          PatternResult* __restrict__ out) {
  constexpr size_t kTile = 256 * (size_t)U;
  const size_t ntiles = n4 / kTile;
  for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const size_t i0 = t * kTile + threadIdx.x;
    u32x4 v[U];
#pragma unroll
    for (int j = 0; j < U; ++j) v[j] = link_load<NT>(host + i0 + (size_t)j * 256);
#pragma unroll
    for (int j = 0; j < U; ++j) {
      const size_t i = i0 + (size_t)j * 256;
      const u32x4 e = pattern_vec<PAT>(base_w + 4 * i, seed, inv);
      const u32x4 d = v[j] ^ e;
      if (d.x | d.y | d.z | d.w) pattern_report(out, (base_w + 4 * i) * 4, e, d);
      if constexpr (STORE) dst[i] = v[j];
    }
  }
  for (size_t i = ntiles * kTile + (size_t)blockIdx.x * 256 + threadIdx.x; i < n4;
       i += (size_t)gridDim.x * 256) {
    const u32x4 g = link_load<NT>(host + i);
    const u32x4 e = pattern_vec<PAT>(base_w + 4 * i, seed, inv);
    const u32x4 d = g ^ e;
    if (d.x | d.y | d.z | d.w) pattern_report(out, (base_w + 4 * i) * 4, e, d);
    if constexpr (STORE) dst[i] = g;
  }
}

// Read round-trip latency: one lane follows the chain laid out in host memory
// (host_link_plan.hpp chase_fill: one 64-byte slot per hop, its first 8 bytes
// the index of the next slot) for exactly `hops` dependent 8-byte loads. Each
// load is a system-scope atomic load, so no cache level between the lane and
// the link can serve it. No spinning, no flag: a fixed trip count, and an
// index that is not a slot (corrupt host memory) ends the walk at once.
// out[0] = the final slot index (or the bad value read), out[1] = elapsed
// wall_clock64() ticks, out[2] = hops done.
__global__ void __launch_bounds__(64)
    host_link_chase_kernel(const unsigned long long* __restrict__ slots, unsigned long long nslots,
                           unsigned long long start, unsigned hops,
                           unsigned long long* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  unsigned long long idx = start;
  unsigned done = 0;
  const long long t0 = wall_clock64();
  for (; done < hops && idx < nslots; ++done)
    idx = __hip_atomic_load(slots + idx * (kChaseSlotBytes / 8), __ATOMIC_RELAXED,
                            __HIP_MEMORY_SCOPE_SYSTEM);
  const long long t1 = wall_clock64();
  out[0] = idx;
  out[1] = (unsigned long long)(t1 - t0);
  out[2] = done;
}

}  // namespace hostlink
}  // namespace ntm
