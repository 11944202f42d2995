// K8: per-XCD sweep kernels for the validation Job (host side, record and verdict:
// ntm/xcd_sweep_plan.hpp). Every rate the Job reports elsewhere is an aggregate
// over the 8 XCDs; these kernels time each XCD by itself.
//
// HIP promises nothing about placement, so nothing here assumes which XCD a block
// index gets: every workgroup reads HW_REG_XCC_ID and HW_REG_HW_ID and acts on
// what it finds.
//
// xcd_read_kernel - verified streaming read, one work queue per XCD. The buffer is
// `xcds` equal slices filled with K4's pattern (hbm_pattern.hpp, logical base 0 at
// the buffer's start), slice x belongs to XCD x. A workgroup whose XCD is not in
// xcd_mask writes its identity and returns. Every other one pulls 64 KiB tiles
// (256 lanes x 16 B x 16 loads in flight) of its own XCD's slice from that XCD's
// head word, one returning device-scope atomicAdd per tile, until the head passes
// passes * tiles_per_slice; tile = head % tiles_per_slice. Pulling makes the sum
// independent of how many workgroups landed on the XCD. Every 16-byte load is
// compared with the pattern as K6's pull kernel does: the data is never stored
// and no atomic touches it. Mismatches are counted in registers, merged in LDS
// at the end and written with the record by lane 0 (plain vector stores).
//
// xcd_mfma_kernel - clock_probe_kernel's back-to-back bf16 MFMA loop per wave
// between the same two stamp pairs, in batches of kMfmaPerBatch; the record's
// tiles = MFMAs of the workgroup, clock = cycles / ticks * 0.1 GHz.
//
// slow_xcd / slow_factor (fault injection only): a workgroup on that XCD measures
// each tile's (batch's) duration in s_memrealtime ticks and s_sleep-waits until
// slow_factor x that has passed since the tile's start. Sleeping lowers the XCD's
// own contention and with it the duration of the tiles that follow, so the wait
// takes the longest tile the workgroup has seen (the ones taken while its
// siblings were loading too). The data path is the healthy one.
#pragma once

#include "ntm/common.hpp"
#include "ntm/hbm_pattern.hpp"
#include "ntm/xcd_sweep_plan.hpp"

namespace ntm {
namespace xcs {

using hbm::pattern_vec;
using hbm::u32x4;

struct ReadArgs {
  const u32x4* buf;        // xcds * slice_bytes, the pattern from logical word 0
  uint64_t slice_vecs;     // slice_bytes / 16
  uint32_t tiles_per_slice;
  uint32_t limit;          // passes * tiles_per_slice
  uint32_t xcds, xcd_mask;
  uint64_t seed;
  uint32_t* heads;         // kMaxXcds heads, kHeadStrideWords apart, zeroed by the launch
  Record* records;         // one per workgroup
  int slow_xcd;            // kSlowOff = none
  uint32_t slow_factor;
};

__device__ __forceinline__ unsigned hw_id_raw() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}

// All of a wave's vector loads have landed before the stamp that follows.
__device__ __forceinline__ void loads_landed() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// Sleeps until `factor` x `dt` ticks have passed since t0 (bounded: 10 ms).
__device__ __forceinline__ void slow_wait(uint64_t t0, uint64_t dt, uint32_t factor) {
  uint64_t until = dt * factor;
  if (until > (1u << 20)) until = 1u << 20;
  while (__builtin_amdgcn_s_memrealtime() - t0 < until) __builtin_amdgcn_s_sleep(8);
}

__device__ __forceinline__ void write_record(Record* rec, unsigned hw, unsigned xcc, uint32_t tiles,
                                             uint32_t bad, uint64_t r0, uint64_t r1, uint64_t c0,
                                             uint64_t c1, uint64_t off, uint64_t exp, uint64_t got) {
  u32x4* p = reinterpret_cast<u32x4*>(rec);
  p[0] = u32x4{kMagic, hw, xcc, blockIdx.x};
  p[1] = u32x4{tiles, bad, (uint32_t)(r1 - r0), (uint32_t)(c1 - c0)};
  p[2] = u32x4{(uint32_t)r0, (uint32_t)(r0 >> 32), (uint32_t)off, (uint32_t)(off >> 32)};
  p[3] = u32x4{(uint32_t)exp, (uint32_t)(exp >> 32), (uint32_t)got, (uint32_t)(got >> 32)};
}

template <int PAT>
__global__ void __launch_bounds__(kThreads) xcd_read_kernel(ReadArgs a) {
  __shared__ uint32_t s_head;
  __shared__ uint32_t s_bad;
  __shared__ unsigned long long s_first, s_exp, s_got;
  const unsigned t = threadIdx.x;
  const unsigned hw = hw_id_raw(), xcc = xcc_id_raw(), x = xcc & 0xFu;
  Record* rec = a.records + blockIdx.x;
  if (x >= a.xcds || !((a.xcd_mask >> x) & 1u)) {
    if (t == 0) write_record(rec, hw, xcc, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    return;
  }
  if (t == 0) s_bad = 0, s_first = ~0ull;
  const bool slow = (int)x == a.slow_xcd && a.slow_factor > 1;
  const u32x4* slice = a.buf + (size_t)x * a.slice_vecs;
  const uint64_t slice_w = (uint64_t)x * a.slice_vecs * 4;  // the slice's first logical 32-bit word
  uint32_t* head = a.heads + x * kHeadStrideWords;
  uint32_t tiles = 0, bad = 0;
  uint64_t first = ~0ull, fexp = 0, fgot = 0, dt_max = 0;
  const uint64_t c0 = __builtin_amdgcn_s_memtime();
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  for (;;) {
    if (t == 0) s_head = atomicAdd(head, 1u);
    __syncthreads();
    const uint32_t h = s_head;
    __syncthreads();  // everyone has read s_head before lane 0 overwrites it
    if (h >= a.limit) break;
    // the tile starts here for all 4 waves at once: a stamp in front of the barrier would
    // count the siblings' sleep as this wave's tile and the waits would feed each other
    const uint64_t ts = slow ? __builtin_amdgcn_s_memrealtime() : 0;
    const size_t i0 = (size_t)(h % a.tiles_per_slice) * (kThreads * kLoadsInFlight) + t;
    u32x4 v[kLoadsInFlight];
#pragma unroll
    for (int j = 0; j < kLoadsInFlight; ++j) v[j] = __builtin_nontemporal_load(slice + i0 + (size_t)j * kThreads);
#pragma unroll
    for (int j = 0; j < kLoadsInFlight; ++j) {
      const size_t i = i0 + (size_t)j * kThreads;
      const u32x4 e = pattern_vec<PAT>(slice_w + 4 * i, a.seed, 0u);
      const u32x4 d = v[j] ^ e;
      if (d.x | d.y | d.z | d.w) {  // the slow path: registers only
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {
          const uint64_t diff = (uint64_t)d[2 * hh] | ((uint64_t)d[2 * hh + 1] << 32);
          if (!diff) continue;
          const uint64_t off = (uint64_t)i * 16 + 8 * hh;
          ++bad;
          if (off < first) {
            first = off;
            fexp = (uint64_t)e[2 * hh] | ((uint64_t)e[2 * hh + 1] << 32);
            fgot = fexp ^ diff;
          }
        }
      }
    }
    ++tiles;
    if (slow) {
      loads_landed();
      const uint64_t dt = __builtin_amdgcn_s_memrealtime() - ts;
      dt_max = dt > dt_max ? dt : dt_max;
      slow_wait(ts, dt_max, a.slow_factor);
    }
  }
  loads_landed();
  const uint64_t c1 = __builtin_amdgcn_s_memtime();
  const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
  if (bad) {  // merge the workgroup's mismatches in LDS
    atomicAdd(&s_bad, bad);
    atomicMin(&s_first, (unsigned long long)first);
  }
  __syncthreads();
  if (bad && s_first == first) s_exp = fexp, s_got = fgot;  // offsets are unique per lane
  __syncthreads();
  if (t == 0) {
    const bool any = s_bad != 0;
    write_record(rec, hw, xcc, tiles, s_bad, r0, r1, c0, c1, any ? s_first : 0, any ? s_exp : 0,
                 any ? s_got : 0);
  }
}

struct MfmaArgs {
  Record* records;
  float* sink;             // one float nobody reads (keeps the MFMAs)
  uint32_t batches, seed;
  uint32_t xcds, xcd_mask;
  int slow_xcd;
  uint32_t slow_factor;
};

__global__ void __launch_bounds__(kThreads) xcd_mfma_kernel(MfmaArgs a) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const unsigned t = threadIdx.x, lane = t & 63u;
  const unsigned hw = hw_id_raw(), xcc = xcc_id_raw(), x = xcc & 0xFu;
  Record* rec = a.records + blockIdx.x;
  if (x >= a.xcds || !((a.xcd_mask >> x) & 1u)) {
    if (t == 0) write_record(rec, hw, xcc, 0, 0, 0, 0, 0, 0, 0, 0, 0);
    return;
  }
  const bool slow = (int)x == a.slow_xcd && a.slow_factor > 1;
  i32x4 va, vb;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    // bf16 pairs with small exponents: random mantissas, no inf / nan (clock_probe_kernel)
    const unsigned h = (unsigned)mix64(((unsigned long long)a.seed << 32) ^ (lane * 8 + i));
    va[i] = (int)(h & 0x3F7F3F7Fu);
    vb[i] = (int)((h >> 5) & 0x3F7F3F7Fu);
  }
  f32x4 acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint64_t dt_max = 0;
  const uint64_t c0 = __builtin_amdgcn_s_memtime();
  const uint64_t r0 = __builtin_amdgcn_s_memrealtime();
  for (uint32_t b = 0; b < a.batches; ++b) {
    const uint64_t ts = slow ? __builtin_amdgcn_s_memrealtime() : 0;
    for (uint32_t it = 0; it < kMfmaPerBatch / 8; ++it) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        asm volatile("v_mfma_f32_16x16x32_bf16 %0, %1, %2, %0" : "+a"(acc[j]) : "v"(va), "v"(vb));
    }
    if (slow) {
      asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");
      const uint64_t dt = __builtin_amdgcn_s_memrealtime() - ts;
      dt_max = dt > dt_max ? dt : dt_max;
      slow_wait(ts, dt_max, a.slow_factor);
    }
  }
  asm volatile("s_nop 15\n\ts_nop 15" ::: "memory");  // MFMA results land before VALU reads
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) s += acc[j][0] + acc[j][1] + acc[j][2] + acc[j][3];
  const uint64_t c1 = __builtin_amdgcn_s_memtime();
  const uint64_t r1 = __builtin_amdgcn_s_memrealtime();
  if (s == 12345.678f) a.sink[0] = s;
  if (t == 0)
    write_record(rec, hw, xcc, a.batches * kMfmaPerBatch * (kThreads / 64), 0, r0, r1, c0, c1, 0, 0, 0);
}

inline bool slow_ok(int slow_xcd, uint32_t slow_factor) {
  return slow_xcd >= kSlowOff && slow_xcd < kMaxXcds && slow_factor >= 1 && slow_factor <= kMaxSlowFactor;
}

// Zeroes the heads and launches one read over `grid` workgroups on `stream`. buf holds
// xcds * slice_bytes of pattern `pattern` (K4's ids) with `seed` from logical byte 0.
inline hipError_t launch_xcd_read(const void* buf, uint64_t slice_bytes, uint32_t xcds, uint32_t xcd_mask,
                                  uint32_t passes, int pattern, uint64_t seed, uint32_t grid, int slow_xcd,
                                  uint32_t slow_factor, uint32_t* heads, Record* records, hipStream_t stream) {
  if (!buf || (uintptr_t)buf % 16 || !heads || !records || (uintptr_t)records % 16 || grid == 0 ||
      xcds < 1 || xcds > (uint32_t)kMaxXcds || !slice_ok(slice_bytes) || !passes_ok(slice_bytes, passes) ||
      !slow_ok(slow_xcd, slow_factor) ||
      (pattern != hbm::kPatternAddr && pattern != hbm::kPatternHash))
    return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(heads, 0, kHeadsBytes, stream);
  if (e != hipSuccess) return e;
  ReadArgs a{(const u32x4*)buf, slice_bytes / 16, tiles_per_slice(slice_bytes),
             (uint32_t)expected_tiles(slice_bytes, passes), xcds, xcd_mask, seed, heads, records,
             slow_xcd, slow_factor};
  if (pattern == hbm::kPatternAddr)
    hipLaunchKernelGGL(xcd_read_kernel<hbm::kPatternAddr>, dim3(grid), dim3(kThreads), 0, stream, a);
  else
    hipLaunchKernelGGL(xcd_read_kernel<hbm::kPatternHash>, dim3(grid), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

inline hipError_t launch_xcd_mfma(uint32_t grid, uint32_t batches, uint32_t seed, uint32_t xcds,
                                  uint32_t xcd_mask, int slow_xcd, uint32_t slow_factor, Record* records,
                                  float* sink, hipStream_t stream) {
  if (!records || (uintptr_t)records % 16 || !sink || grid == 0 || batches < 1 || batches > kMaxMfmaBatches ||
      xcds < 1 || xcds > (uint32_t)kMaxXcds || !slow_ok(slow_xcd, slow_factor))
    return hipErrorInvalidValue;
  MfmaArgs a{records, sink, batches, seed, xcds, xcd_mask, slow_xcd, slow_factor};
  hipLaunchKernelGGL(xcd_mfma_kernel, dim3(grid), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace xcs
}  // namespace ntm
