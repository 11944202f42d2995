// K9: atomics and cross-XCD hand-off kernels for the validation Job (host side, records
// and verdicts: ntm/atomics_plan.hpp). The only atomics the other checks issue are
// integer adds of 1 whose result nobody looks at; these kernels check the value every
// kind of atomic produced, and move plain-stored bytes from one XCD's L2 to another
// inside a launch.
//
// Rule for all of them: no workgroup waits on memory another one writes. There is no
// spin, no poll and no inter-workgroup barrier; the hand-off is the "last arriver"
// form, so no placement can hang it. HIP promises nothing about placement: the
// workgroups read HW_REG_XCC_ID / HW_REG_HW_ID and report what they found.
//
// atomics_rmw_kernel<OP>   non-returning agent-scope read-modify-write, operation
//                          k = gid * iters + it on slot k % slots; the table is compared
//                          with atomics_reference_kernel's, which uses no atomic.
// atomics_ticket_kernel    returning fetch-adds hand out tickets; the drawer stores its
//                          gid into claim[head][ticket] with a plain store.
// atomics_handoff_kernel   per episode of E workgroups: warm (plain loads of all E slabs,
//                          which still hold last round's pattern), delay, write the own
//                          slab with this round's pattern, publish (every wave's
//                          s_waitcnt vmcnt(0), barrier, lane 0: agent release fence,
//                          s_waitcnt vmcnt(0), relaxed agent fetch_add), and the workgroup
//                          that drew E - 1 acquires and compares all E slabs.
#pragma once

#include "ntm/atomics_plan.hpp"
#include "ntm/common.hpp"
#include "ntm/hbm_pattern.hpp"

namespace ntm {
namespace atm {

using hbm::pattern_vec;
using hbm::u32x4;

#define NTM_ATM_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ unsigned hw_id_raw() {
  unsigned v;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(v));
  return v;
}
__device__ __forceinline__ void vm_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

struct RmwArgs {
  void* table;  // slots x slot_bytes(op), holding init_value(op)
  uint64_t slots, seed, max_abs;
  uint32_t iters;
};

typedef short bf16x2_t __attribute__((ext_vector_type(2)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));

template <int OP>
__global__ void __launch_bounds__(kThreads) atomics_rmw_kernel(RmwArgs a) {
  const uint64_t gid = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  for (uint32_t it = 0; it < a.iters; ++it) {
    const uint64_t k = gid * a.iters + it;
    const uint64_t s = slot_of(k, a.slots);
    const uint64_t v = operand_bits(OP, k, a.seed, a.max_abs, a.slots);
    uint32_t* p32 = (uint32_t*)a.table + s;
    unsigned long long* p64 = (unsigned long long*)a.table + s;
    if constexpr (OP == kAddU32) __hip_atomic_fetch_add(p32, (uint32_t)v, NTM_ATM_RLX_AGENT);
    if constexpr (OP == kAddU64) __hip_atomic_fetch_add(p64, (unsigned long long)v, NTM_ATM_RLX_AGENT);
    if constexpr (OP == kAndU32) __hip_atomic_fetch_and(p32, (uint32_t)v, NTM_ATM_RLX_AGENT);
    if constexpr (OP == kOrU32) __hip_atomic_fetch_or(p32, (uint32_t)v, NTM_ATM_RLX_AGENT);
    if constexpr (OP == kXorU32) __hip_atomic_fetch_xor(p32, (uint32_t)v, NTM_ATM_RLX_AGENT);
    if constexpr (OP == kMinI32) __hip_atomic_fetch_min((int*)p32, (int)(uint32_t)v, NTM_ATM_RLX_AGENT);
    if constexpr (OP == kMaxI32) __hip_atomic_fetch_max((int*)p32, (int)(uint32_t)v, NTM_ATM_RLX_AGENT);
    if constexpr (OP == kMaxU64) __hip_atomic_fetch_max(p64, (unsigned long long)v, NTM_ATM_RLX_AGENT);
    if constexpr (OP == kCasU32) {  // one try, no retry: {claim, successes} per slot
      uint32_t* claim = (uint32_t*)a.table + 2 * s;
      uint32_t zero = 0;
      if (__hip_atomic_compare_exchange_strong(claim, &zero, (uint32_t)v, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_add(claim + 1, 1u, NTM_ATM_RLX_AGENT);
    }
    if constexpr (OP == kAddF32) {
      float f;
      const uint32_t b = (uint32_t)v;
      __builtin_memcpy(&f, &b, 4);
      unsafeAtomicAdd((float*)p32, f);
    }
    if constexpr (OP == kAddF64) {
      double f;
      __builtin_memcpy(&f, &v, 8);
      unsafeAtomicAdd((double*)p64, f);
    }
    if constexpr (OP == kAddBf16x2) {
      bf16x2_t x;
      const uint32_t b = (uint32_t)v;
      __builtin_memcpy(&x, &b, 4);
      __builtin_amdgcn_global_atomic_fadd_v2bf16((NTM_AS1 bf16x2_t*)p32, x);
    }
    if constexpr (OP == kAddF16x2) {
      f16x2_t x;
      const uint32_t b = (uint32_t)v;
      __builtin_memcpy(&x, &b, 4);
      __builtin_amdgcn_global_atomic_fadd_v2f16((NTM_AS1 f16x2_t*)p32, x);
    }
  }
}

// fills the table with init_value(op); one thread per slot
__global__ void __launch_bounds__(kThreads) atomics_init_kernel(void* table, uint64_t slots, int op) {
  const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= slots) return;
  if (slot_bytes(op) == 8) ((uint64_t*)table)[s] = init_value(op);
  else ((uint32_t*)table)[s] = (uint32_t)init_value(op);
}

// cas only, after the rmw launch: the winner becomes slot + 1 when it was a contender of the slot
__global__ void __launch_bounds__(kThreads) atomics_cas_canonical_kernel(uint32_t* table, uint64_t slots, uint64_t total) {
  const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s < slots) table[2 * s] = cas_canonical(table[2 * s], s, slots, total);
}

// the expected table with no atomic: one thread per slot folds its operations in order
__global__ void __launch_bounds__(kThreads) atomics_reference_kernel(void* table, int op, uint64_t slots, uint64_t total,
                                                                     uint64_t seed, uint64_t max_abs) {
  const uint64_t s = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (s >= slots) return;
  const uint64_t v = expected_slot(op, s, slots, total, seed, max_abs);
  if (slot_bytes(op) == 8) ((uint64_t*)table)[s] = v;
  else ((uint32_t*)table)[s] = (uint32_t)v;
}

inline uint32_t slot_grid(uint64_t slots) { return (uint32_t)((slots + kThreads - 1) / kThreads); }

template <int OP>
inline void launch_rmw_op(const RmwArgs& a, uint32_t grid, hipStream_t stream) {
  hipLaunchKernelGGL(atomics_rmw_kernel<OP>, dim3(grid), dim3(kThreads), 0, stream, a);
}

// Initialises `table` (slots x slot_bytes(op)) and runs grid x 256 x iters operations on it.
inline hipError_t launch_rmw(int op, void* table, uint64_t slots, uint32_t grid, uint32_t iters, uint64_t seed,
                             uint64_t max_abs, hipStream_t stream) {
  if (!table || (uintptr_t)table % 8 || !rmw_shape_ok(op, slots, grid, iters, max_abs)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(atomics_init_kernel, dim3(slot_grid(slots)), dim3(kThreads), 0, stream, table, slots, op);
  const RmwArgs a{table, slots, seed, is_float(op) ? max_abs : 1, iters};
  switch (op) {
    case kAddU32: launch_rmw_op<kAddU32>(a, grid, stream); break;
    case kAddU64: launch_rmw_op<kAddU64>(a, grid, stream); break;
    case kAndU32: launch_rmw_op<kAndU32>(a, grid, stream); break;
    case kOrU32: launch_rmw_op<kOrU32>(a, grid, stream); break;
    case kXorU32: launch_rmw_op<kXorU32>(a, grid, stream); break;
    case kMinI32: launch_rmw_op<kMinI32>(a, grid, stream); break;
    case kMaxI32: launch_rmw_op<kMaxI32>(a, grid, stream); break;
    case kMaxU64: launch_rmw_op<kMaxU64>(a, grid, stream); break;
    case kCasU32: launch_rmw_op<kCasU32>(a, grid, stream); break;
    case kAddF32: launch_rmw_op<kAddF32>(a, grid, stream); break;
    case kAddF64: launch_rmw_op<kAddF64>(a, grid, stream); break;
    case kAddBf16x2: launch_rmw_op<kAddBf16x2>(a, grid, stream); break;
    default: launch_rmw_op<kAddF16x2>(a, grid, stream); break;
  }
  if (op == kCasU32)
    hipLaunchKernelGGL(atomics_cas_canonical_kernel, dim3(slot_grid(slots)), dim3(kThreads), 0, stream,
                       (uint32_t*)table, slots, (uint64_t)grid * kThreads * iters);
  return hipGetLastError();
}

inline hipError_t launch_rmw_reference(int op, void* table, uint64_t slots, uint32_t grid, uint32_t iters,
                                       uint64_t seed, uint64_t max_abs, hipStream_t stream) {
  if (!table || (uintptr_t)table % 8 || !rmw_shape_ok(op, slots, grid, iters, max_abs)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(atomics_reference_kernel, dim3(slot_grid(slots)), dim3(kThreads), 0, stream, table, op, slots,
                     (uint64_t)grid * kThreads * iters, seed, is_float(op) ? max_abs : 1);
  return hipGetLastError();
}

// ---- tickets
__global__ void __launch_bounds__(kThreads) atomics_ticket_kernel(uint32_t* counters, uint32_t* claim, uint32_t heads,
                                                                  uint32_t per_head, uint32_t iters,
                                                                  uint32_t inject_gid) {
  const uint32_t gid = blockIdx.x * kThreads + threadIdx.x;
  for (uint32_t it = 0; it < iters; ++it) {
    const uint32_t h = ticket_head(gid, it, heads);
    uint32_t t = __hip_atomic_fetch_add(counters + (size_t)h * kLineWords, 1u, NTM_ATM_RLX_AGENT);
    if (gid == inject_gid && it == 0) ++t;  // fault injection: one entry too high
    if (t < per_head) claim[(size_t)h * per_head + t] = gid;  // a ticket past the table shows as a counter over
  }
}

// Zeroes the counters, fills the claim table with kSentinel and draws grid x 256 x iters tickets.
inline hipError_t launch_tickets(uint32_t* counters, uint32_t* claim, uint32_t heads, uint32_t grid, uint32_t iters,
                                 uint32_t inject_gid, hipStream_t stream) {
  if (!counters || !claim || !ticket_shape_ok(heads, grid, iters)) return hipErrorInvalidValue;
  const uint64_t per_head = tickets_per_head(heads, grid, iters);
  hipError_t e = hipMemsetAsync(counters, 0, (size_t)heads * kLineWords * 4, stream);
  if (e == hipSuccess) e = hipMemsetAsync(claim, 0xFF, (size_t)heads * per_head * 4, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(atomics_ticket_kernel, dim3(grid), dim3(kThreads), 0, stream, counters, claim, heads,
                     (uint32_t)per_head, iters, inject_gid);
  return hipGetLastError();
}

// ---- hand-off
struct HandoffArgs {
  u32x4* slabs;        // episodes x E slabs of kSlabBytes holding round - 1
  uint32_t* counters;  // one per episode, kLineWords apart, zeroed by the launch
  Record* records;     // one per workgroup
  uint32_t e, round;
  uint64_t seed;
  uint32_t inject_wg;  // kInjectOff = none
};

// 16-byte word `w` of workgroup wg's slab in `round` (word 0 is the header's place)
__device__ __forceinline__ u32x4 slab_word(uint32_t wg, uint32_t w, uint64_t seed, uint32_t round) {
  return pattern_vec<hbm::kPatternHash>(((uint64_t)wg * kSlabWords + w) * 4, round_seed(seed, round), 0u);
}

// every slab gets `round`'s pattern and a header naming the workgroup that owns it
__global__ void __launch_bounds__(kThreads) atomics_handoff_init_kernel(u32x4* slabs, uint64_t seed, uint32_t round) {
  const uint32_t t = threadIdx.x, wg = blockIdx.x;
  slabs[(size_t)wg * kSlabWords + t] =
      t == 0 ? u32x4{kSlabMagic + round, hw_id_raw(), xcc_id_raw(), wg} : slab_word(wg, t, seed, round);
}

__global__ void __launch_bounds__(kThreads) atomics_handoff_kernel(HandoffArgs a) {
  __shared__ uint32_t s_ticket, s_bad, s_stale, s_warm, s_first, s_mask, s_w[8];
  const uint32_t t = threadIdx.x, wg = blockIdx.x;
  const uint32_t ep = wg / a.e, wg0 = ep * a.e;
  const unsigned hw = hw_id_raw(), xcc = xcc_id_raw();
  if (t == 0) s_bad = 0, s_stale = 0, s_warm = 0, s_first = ~0u, s_mask = 0;
  __syncthreads();
  // 1. warm: last round's lines into this CU's L1 and this XCD's L2 (a sibling may have written already)
  uint32_t warm_bad = 0;
  for (uint32_t j = 0; j < a.e; ++j) {
    const u32x4 g = a.slabs[(size_t)(wg0 + j) * kSlabWords + t];
    if (t == 0) {
      warm_bad += !((g.x == kSlabMagic + a.round || g.x == kSlabMagic + a.round - 1) && g.w == wg0 + j);
    } else {
      const u32x4 d0 = g ^ slab_word(wg0 + j, t, a.seed, a.round - 1), d1 = g ^ slab_word(wg0 + j, t, a.seed, a.round);
      warm_bad += (d0.x | d0.y | d0.z | d0.w) && (d1.x | d1.y | d1.z | d1.w);
    }
  }
  if (warm_bad) atomicAdd(&s_warm, warm_bad);
  // 2. delay: uneven arrival, waiting on nothing
  const uint32_t sleeps = sleep_count(wg, a.seed, a.round);
  for (uint32_t i = 0; i < sleeps; ++i) __builtin_amdgcn_s_sleep(8);
  // 3. write the own slab; the injected writer leaves one 64-byte line at last round's pattern
  {
    const bool old = wg == a.inject_wg && t >= kStaleLineWord && t < kStaleLineWord + 4;
    a.slabs[(size_t)wg * kSlabWords + t] =
        t == 0 ? u32x4{kSlabMagic + a.round, hw, xcc, wg} : slab_word(wg, t, a.seed, old ? a.round - 1 : a.round);
  }
  // 4. publish
  vm_drain();
  __syncthreads();
  if (t == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    vm_drain();
    s_ticket = __hip_atomic_fetch_add(a.counters + (size_t)ep * kLineWords, 1u, NTM_ATM_RLX_AGENT);
  }
  __syncthreads();
  const uint32_t ticket = s_ticket;
  Record* rec = a.records + wg;
  u32x4* p = reinterpret_cast<u32x4*>(rec);
  if (ticket != a.e - 1) {
    if (t == 0) {
      p[0] = u32x4{kMagic, hw, xcc, wg};
      p[1] = u32x4{ep, 0, 0, 0};
      p[2] = u32x4{0, 0, s_warm, kClassNone};
      p[3] = u32x4{0, 0, 0, 0};
      p[4] = u32x4{0, 0, 0, 0};
      p[5] = u32x4{ticket, sleeps, 0, 0};
    }
    return;
  }
  // 5. reduce: this workgroup arrived last
  if (t == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    vm_drain();
  }
  __syncthreads();
  uint32_t bad = 0, stale = 0, mask = 0, first = ~0u, fcls = kClassNone, fj = 0;
  uint64_t fexp = 0, fgot = 0;
  for (uint32_t j = 0; j < a.e; ++j) {
    const u32x4 g = a.slabs[(size_t)(wg0 + j) * kSlabWords + t];
    u32x4 e, o;  // this round's and last round's word; the header's hw / xcc are the writer's to say
    if (t == 0) {
      e = u32x4{kSlabMagic + a.round, g.y, g.z, wg0 + j};
      o = u32x4{kSlabMagic + a.round - 1, g.y, g.z, wg0 + j};
      mask |= 1u << (g.z & 0xFu);
    } else {
      e = slab_word(wg0 + j, t, a.seed, a.round);
      o = slab_word(wg0 + j, t, a.seed, a.round - 1);
    }
    const u32x4 d = g ^ e;
    if (d.x | d.y | d.z | d.w) {  // the slow path
      const u32x4 d0 = g ^ o;
      const bool is_stale = !(d0.x | d0.y | d0.z | d0.w);
      ++bad;
      stale += is_stale;
      const int hh = (d.x | d.y) ? 0 : 1;
      const uint32_t off = (j * kSlabWords + t) * 16 + 8 * hh;
      if (off < first) {
        first = off, fj = j, fcls = is_stale ? kClassStale : kClassCorrupt;
        fexp = (uint64_t)e[2 * hh] | ((uint64_t)e[2 * hh + 1] << 32);
        fgot = (uint64_t)g[2 * hh] | ((uint64_t)g[2 * hh + 1] << 32);
      }
    }
  }
  if (bad) {
    atomicAdd(&s_bad, bad);
    atomicAdd(&s_stale, stale);
    atomicMin(&s_first, first);
  }
  __syncthreads();
  if (bad && s_first == first) {  // offsets are unique per lane: one lane names the first bad word
    const u32x4 h = a.slabs[(size_t)(wg0 + fj) * kSlabWords];
    s_w[0] = h.y, s_w[1] = h.z, s_w[2] = wg0 + fj, s_w[3] = fcls;
    s_w[4] = (uint32_t)fexp, s_w[5] = (uint32_t)(fexp >> 32), s_w[6] = (uint32_t)fgot, s_w[7] = (uint32_t)(fgot >> 32);
  }
  if (mask) s_mask = mask;  // lane 0 read every header
  __syncthreads();
  if (t == 0) {
    const bool any = s_bad != 0;
    p[0] = u32x4{kMagic, hw, xcc, wg};
    p[1] = u32x4{ep, 1, a.e * kSlabWords, s_bad};
    p[2] = u32x4{s_stale, s_mask, s_warm, any ? s_w[3] : (uint32_t)kClassNone};
    p[3] = any ? u32x4{s_w[0], s_w[1], s_w[2], s_first} : u32x4{0, 0, 0, 0};
    p[4] = any ? u32x4{s_w[4], s_w[5], s_w[6], s_w[7]} : u32x4{0, 0, 0, 0};
    p[5] = u32x4{ticket, sleeps, 0, 0};
  }
}

inline hipError_t launch_handoff_init(void* slabs, uint32_t episodes, uint32_t e, uint64_t seed, uint32_t round,
                                      hipStream_t stream) {
  if (!slabs || (uintptr_t)slabs % 16 || !handoff_shape_ok(episodes, e)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(atomics_handoff_init_kernel, dim3(episodes * e), dim3(kThreads), 0, stream, (u32x4*)slabs, seed, round);
  return hipGetLastError();
}

// One round: the slabs hold round - 1 (launch_handoff_init, or the round before), round >= 1.
inline hipError_t launch_handoff(void* slabs, uint32_t* counters, Record* records, uint32_t episodes, uint32_t e,
                                 uint64_t seed, uint32_t round, uint32_t inject_wg, hipStream_t stream) {
  if (!slabs || (uintptr_t)slabs % 16 || !counters || !records || (uintptr_t)records % 16 ||
      !handoff_shape_ok(episodes, e) || round < 1 || round > 0xFFFFu ||
      (inject_wg != kInjectOff && inject_wg >= episodes * e))
    return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(counters, 0, handoff_counter_bytes(episodes), stream);
  if (err != hipSuccess) return err;
  const HandoffArgs a{(u32x4*)slabs, counters, records, e, round, seed, inject_wg};
  hipLaunchKernelGGL(atomics_handoff_kernel, dim3(episodes * e), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

}  // namespace atm
}  // namespace ntm
