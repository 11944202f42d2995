// K5: per-CU compute sweep for the validation Job. K1 proves that the GPU
// computes a correct GEMM; this kernel ties a compute fault to the CU it sits
// on. One workgroup of 256 threads (4 waves, normally one per SIMD) takes all
// of a CU's LDS, so a grid of a few workgroups per CU spreads over the chip,
// and runs `iters` rounds of four known-answer sub-tests whose results are
// exact (ntm/cu_sweep_plan.hpp: generators, table layout, record):
//   lds        every word of the dynamic LDS written (ds_write_b128), read back
//              by another wave and compared, then the same with the complement
//   valu       u32 hash, v_mad_u64_u32, f32 FMA and f64 FMA chains per thread
//   mfma_bf16  chained v_mfma_f32_16x16x32_bf16 and v_mfma_f32_32x32x16_bf16
//   mfma_fp8   chained v_mfma_f32_16x16x128_f8f6f4 on e4m3, unit scales
// valu and MFMA results are compared bitwise with a table the host computed in
// integers; the LDS pattern is recomputed by the VALU (as K4 does for HBM).
//
// Every wave reads HW_REG_HW_ID (SIMD_ID is per wave) and HW_REG_XCC_ID. Each
// workgroup writes its record's identity fields with plain stores; the bad
// counts and the first mismatch are touched only when a compare fails, with
// atomics on that slow path alone, so the host zeroes the records first.
//
// Operand layouts (cdna_hip_programming.md "Fragment layout", as the K1 kernels):
//   16x16x32 bf16: lane l holds A[l & 15][8 (l >> 4) + j], B[8 (l >> 4) + j][l & 15], j < 8;
//                  D register r = D[4 (l >> 4) + r][l & 15]
//   32x32x16 bf16: lane l holds A[l & 31][8 (l >> 5) + j], B[8 (l >> 5) + j][l & 31], j < 8;
//                  D register r = D[(r & 3) + 8 (r >> 2) + 4 (l >> 5)][l & 31]
//   16x16x128 f8:  lane l holds 32 k of A[l & 15] and of B[.][l & 15], the same k in the
//                  same byte of both (the sum over k is exact in any order); D as 16x16x32
#pragma once

#include "ntm/common.hpp"
#include "ntm/cu_sweep_plan.hpp"
#include "ntm/gemm_bf16.hpp"

namespace ntm {
namespace cus {

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

struct SweepArgs {
  Record* records;          // one per workgroup, zeroed by the host
  const uint32_t* expected;  // make_expected(iters, seed)
  int iters;
  uint32_t lds_bytes;       // multiple of 16, the launch's dynamic LDS
  uint32_t seed;
  uint32_t fault_key;       // cu_key whose workgroups flip one bit; kFaultOff = none
  int fault_subtest;
};

// The slow path: one element differs.
__device__ __noinline__ void sweep_report(Record* rec, int sub, unsigned wave, uint32_t round,
                                          uint32_t elem, uint64_t expected, uint64_t got) {
  atomicAdd(&rec->bad[sub], 1u);
  if (atomicCAS(&rec->first, 0u, (uint32_t)(1 + sub) | (wave << 8)) == 0u) {
    rec->first_round = round;
    rec->first_elem = elem;
    rec->expected = expected;
    rec->got = got;
  }
}

// By value on purpose: __builtin_bit_cast applied directly to a vector element
// (acc[q]) reads element 0 whatever q is.
__device__ __forceinline__ uint32_t f32_bits(float v) { return __builtin_bit_cast(uint32_t, v); }

// The project's rule for MFMA results (tools/mfma_hazard_scan.py): no VALU touches an
// accumulator within 19 wait states of the MFMA, the 16-pass requirement, whatever the
// shape. The compiler pads only to each shape's own minimum, so every chain ends here.
// (There is no s_nop builtin: this is K1's mfma_drain, two s_nop 15.)
__device__ __forceinline__ void sweep_mfma_drain() {
  __builtin_amdgcn_sched_barrier(0);
  ::ntm::gemm::mfma_drain();
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ uint32_t bf16_bits_of_small_int(int v) {  // |v| <= 8: exact
  return f32_bits((float)v) >> 16;
}

// 8 bf16 of row / column i, k0 .. k0 + 7
__device__ __forceinline__ bf16x8 bf16_fragment(uint32_t rs, unsigned kind, unsigned wave,
                                                unsigned i, unsigned k0) {
  u32x4 p;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    p[j] = bf16_bits_of_small_int(bf16_operand(rs, kind, wave, i, k0 + 2 * j)) |
           (bf16_bits_of_small_int(bf16_operand(rs, kind, wave, i, k0 + 2 * j + 1)) << 16);
  return __builtin_bit_cast(bf16x8, p);
}

// 32 e4m3 of row / column i, k0 .. k0 + 31
__device__ __forceinline__ i32x8 fp8_fragment(uint32_t rs, unsigned kind, unsigned wave, unsigned i,
                                              unsigned k0) {
  i32x8 p;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uint32_t w = 0;
#pragma unroll
    for (int b = 0; b < 4; ++b)
      w |= e4m3_of_small_int(fp8_operand(rs, kind, wave, i, k0 + 4 * j + b)) << (8 * b);
    p[j] = (int)w;
  }
  return p;
}

__global__ void __launch_bounds__(kThreads) cu_sweep_kernel(SweepArgs a) {
  extern __shared__ __attribute__((aligned(16))) u32x4 sweep_lds[];
  const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
  unsigned hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  const unsigned xcc = xcc_id_raw();
  Record* rec = a.records + blockIdx.x;
  if (lane == 0) {
    rec->simd[wave] = (uint8_t)((hw >> 4) & 3u);
    if (wave == 0) {
      rec->hw_id = hw;
      rec->xcc_id = xcc;
      rec->magic = kMagic;
      rec->wg = blockIdx.x;
    }
  }
  // fault injection: one thread of a workgroup on the chosen CU flips one bit of one
  // computed value of one sub-test, in round 0
  const bool inject = a.fault_key != kFaultOff && t == (unsigned)kFaultThread &&
                      cu_key(hw, xcc) == a.fault_key;
  const uint32_t n16 = a.lds_bytes / 16;
  const unsigned tr = (t + 64u) & 255u;  // reads what the next wave wrote

  for (int r = 0; r < a.iters; ++r) {
    const uint32_t rs = round_seed(a.seed, (uint32_t)r);
    const uint32_t* exp = a.expected + (size_t)r * kRoundWords;
    const uint32_t flip = inject && r == 0 ? kFaultBit : 0u;

    // ---- lds
    {
      const uint32_t f = a.fault_subtest == kSubLds ? flip : 0u;
      for (uint32_t v = t; v < n16; v += kThreads) {
        u32x4 p;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = lds_word(4 * v + j, rs);
        sweep_lds[v] = p;
      }
      __syncthreads();
      for (uint32_t v = tr; v < n16; v += kThreads) {
        u32x4 g = sweep_lds[v];
        if (v == 0) g[0] ^= f;
        u32x4 p;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = lds_word(4 * v + j, rs);
        const u32x4 d = g ^ p;
        if (d[0] | d[1] | d[2] | d[3]) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (d[j]) sweep_report(rec, kSubLds, wave, (uint32_t)r, 4 * v + j, p[j], g[j]);
        }
        sweep_lds[v] = ~p;
      }
      __syncthreads();
      for (uint32_t v = t; v < n16; v += kThreads) {
        const u32x4 g = sweep_lds[v];
        u32x4 p;
#pragma unroll
        for (int j = 0; j < 4; ++j) p[j] = ~lds_word(4 * v + j, rs);
        const u32x4 d = g ^ p;
        if (d[0] | d[1] | d[2] | d[3]) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (d[j]) sweep_report(rec, kSubLds, wave, (uint32_t)r, 4 * v + j, p[j], g[j]);
        }
      }
    }

    // ---- valu
    {
      const uint32_t f = a.fault_subtest == kSubValu ? flip : 0u;
      const uint32_t h = valu_hash_chain(t, rs) ^ f;
      if (h != exp[kOffHash + t])
        sweep_report(rec, kSubValu, wave, (uint32_t)r, t, exp[kOffHash + t], h);
      const uint64_t m = valu_mad_chain(t, rs);
      const uint64_t me = *(const uint64_t*)(exp + kOffMad + 2 * t);
      if (m != me) sweep_report(rec, kSubValu, wave, (uint32_t)r, 256 + t, me, m);
      float total = 0.f;
#pragma unroll
      for (int s = 0; s < kF32Segments; ++s) {
        float acc = (float)fma_start(fma_coeff(rs, 0, t, (unsigned)(s * kF32Steps)));
#pragma unroll
        for (int i = 0; i < kF32Steps; ++i) {
          const uint32_t c = fma_coeff(rs, 0, t, (unsigned)(s * kF32Steps + i));
          acc = __builtin_fmaf(acc, (float)fma_mul(c, 0), (float)fma_add(c));
        }
        total = __builtin_fmaf(acc, 1.0f, total);
      }
      const uint32_t fb = f32_bits(total);
      if (fb != exp[kOffF32 + t])
        sweep_report(rec, kSubValu, wave, (uint32_t)r, 512 + t, exp[kOffF32 + t], fb);
      double dacc = (double)fma_start(fma_coeff(rs, 1, t, 0));
#pragma unroll
      for (int i = 0; i < kF64Steps; ++i) {
        const uint32_t c = fma_coeff(rs, 1, t, (unsigned)i);
        dacc = __builtin_fma(dacc, (double)fma_mul(c, 1), (double)fma_add(c));
      }
      const uint64_t db = __builtin_bit_cast(uint64_t, dacc);
      const uint64_t de = *(const uint64_t*)(exp + kOffF64 + 2 * t);
      if (db != de) sweep_report(rec, kSubValu, wave, (uint32_t)r, 768 + t, de, db);
    }

    // ---- mfma_bf16
    {
      const uint32_t f = a.fault_subtest == kSubBf16 ? flip : 0u;
      f32x4 d16 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < kBf16Steps16; ++s) {
        const unsigned k0 = 32u * s + 8u * (lane >> 4);
        d16 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf16_fragment(rs, 0, wave, lane & 15u, k0),
                                                      bf16_fragment(rs, 1, wave, lane & 15u, k0),
                                                      d16, 0, 0, 0);
      }
      sweep_mfma_drain();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t el = wave * 256u + (4u * (lane >> 4) + q) * 16u + (lane & 15u);
        const uint32_t g = f32_bits(d16[q]) ^ (q == 0 ? f : 0u);
        if (g != exp[kOffBf16 + el])
          sweep_report(rec, kSubBf16, wave, (uint32_t)r, el, exp[kOffBf16 + el], g);
      }
      f32x16 d32;
#pragma unroll
      for (int q = 0; q < 16; ++q) d32[q] = 0.f;
#pragma unroll
      for (int s = 0; s < kBf16Steps32; ++s) {
        const unsigned k0 = 16u * s + 8u * (lane >> 5);
        d32 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(bf16_fragment(rs, 2, wave, lane & 31u, k0),
                                                      bf16_fragment(rs, 3, wave, lane & 31u, k0),
                                                      d32, 0, 0, 0);
      }
      sweep_mfma_drain();
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const unsigned row = (q & 3u) + 8u * (q >> 2) + 4u * (lane >> 5);
        const uint32_t el = kBf16Words16 + wave * 1024u + row * 32u + (lane & 31u);
        const uint32_t g = f32_bits(d32[q]);
        if (g != exp[kOffBf16 + el])
          sweep_report(rec, kSubBf16, wave, (uint32_t)r, el, exp[kOffBf16 + el], g);
      }
    }

    // ---- mfma_fp8 (format 0 = e4m3, E8M0 scale 127 = 2^0)
    {
      const uint32_t f = a.fault_subtest == kSubFp8 ? flip : 0u;
      f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < kFp8Steps; ++s) {
        const unsigned k0 = 128u * s + 32u * (lane >> 4);
        d = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(
            fp8_fragment(rs, 4, wave, lane & 15u, k0), fp8_fragment(rs, 5, wave, lane & 15u, k0), d,
            0, 0, 0, 127, 0, 127);
      }
      sweep_mfma_drain();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t el = wave * 256u + (4u * (lane >> 4) + q) * 16u + (lane & 15u);
        const uint32_t g = f32_bits(d[q]) ^ (q == 0 ? f : 0u);
        if (g != exp[kOffFp8 + el])
          sweep_report(rec, kSubFp8, wave, (uint32_t)r, el, exp[kOffFp8 + el], g);
      }
    }
  }
}

inline bool sweep_lds_bytes_ok(size_t lds_bytes) { return lds_bytes >= 16 && lds_bytes % 16 == 0; }

// Zeroes `grid` records and launches one sweep on `stream`. lds_bytes above the
// device's per-block maximum is refused by the runtime (the error is returned).
inline hipError_t launch_cu_sweep(Record* records, const uint32_t* expected, unsigned grid, int iters,
                                  size_t lds_bytes, uint32_t seed, uint32_t fault_key,
                                  int fault_subtest, hipStream_t stream) {
  if (!records || !expected || grid == 0 || iters < 1 || iters > kMaxIters ||
      !sweep_lds_bytes_ok(lds_bytes) || lds_bytes > (1u << 20) ||
      (fault_key != kFaultOff && (fault_subtest < 0 || fault_subtest >= kSubtests)))
    return hipErrorInvalidValue;
  hipError_t e = hipFuncSetAttribute((const void*)cu_sweep_kernel,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) {  // e.g. lds_bytes above the device's maximum
    (void)hipGetLastError();
    return e;
  }
  e = hipMemsetAsync(records, 0, (size_t)grid * sizeof(Record), stream);
  if (e != hipSuccess) return e;
  SweepArgs a{records, expected, iters, (uint32_t)lds_bytes, seed, fault_key, fault_subtest};
  hipLaunchKernelGGL(cu_sweep_kernel, dim3(grid), dim3(kThreads), lds_bytes, stream, a);
  return hipGetLastError();
}

}  // namespace cus
}  // namespace ntm
