// K12 wave data-path and special-function check: the gfx950 kernels. Four families, each an
// instruction kernel and a reference kernel that uses none of the instructions under test
// (maps, generators, records and messages: ntm/wave_paths_plan.hpp):
//   lane   DPP modifiers, ds_bpermute_b32 / ds_permute_b32, ds_swizzle_b32, v_permlane16_swap /
//          v_permlane32_swap, v_readlane / v_readfirstlane; the reference moves the words
//          through LDS by the plan's src_lane
//   ldstr  ds_read_b64_tr_b16 / _tr_b8 / _tr_b4 and ds_read_b96_tr_b6 on an LDS image; the
//          reference fetches the same elements byte by byte and shifts
//   sfu    v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32, v_sqrt_f32, v_sin_f32, v_cos_f32: raw
//          result words, a 64-bit digest per workgroup, and the ordered-integer distance of a
//          result from a host-built bracket
//   valu   v_bitop3_b32 over all 256 truth tables and v_cvt_pk_bf16_f32; the reference is
//          bit-by-bit / integer round-to-nearest-even
// Workgroups are 256 threads; every transposed read is issued under full EXEC (addresses are
// clamped, stores are masked: pad, don't mask); every loop has a fixed trip count; no workgroup
// waits on another; every result leaves through an ordinary vector store.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "ntm/common.hpp"  // xcc_id_raw
#include "ntm/wave_paths_plan.hpp"

namespace ntm {
namespace wave {

#define NTM_WAVE_LDS(T) __attribute__((address_space(3))) T*
typedef short wv_s16x4 __attribute__((ext_vector_type(4)));
typedef int wv_i32x2 __attribute__((ext_vector_type(2)));
typedef int wv_i32x3 __attribute__((ext_vector_type(3)));
typedef float wv_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 wv_bf16x2 __attribute__((ext_vector_type(2)));

// One transposed read at LDS byte address `p` (8-byte aligned; 16-byte for the 6-bit form) ->
// the lane's 2 (3) result dwords in r[0 .. 2]. EXEC must be all ones.
template <int BITS>
__device__ __forceinline__ void tr_read(const unsigned char* p, uint32_t r[3]) {
  r[2] = 0;
  if constexpr (BITS == 16) {
    const wv_s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((NTM_WAVE_LDS(wv_s16x4))p);
    const wv_i32x2 w = __builtin_bit_cast(wv_i32x2, v);
    r[0] = (uint32_t)w[0], r[1] = (uint32_t)w[1];
  } else if constexpr (BITS == 8) {
    const wv_i32x2 w = __builtin_amdgcn_ds_read_tr8_b64_v2i32((NTM_WAVE_LDS(wv_i32x2))p);
    r[0] = (uint32_t)w[0], r[1] = (uint32_t)w[1];
  } else if constexpr (BITS == 4) {
    const wv_i32x2 w = __builtin_amdgcn_ds_read_tr4_b64_v2i32((NTM_WAVE_LDS(wv_i32x2))p);
    r[0] = (uint32_t)w[0], r[1] = (uint32_t)w[1];
  } else {
    const wv_i32x3 w = __builtin_amdgcn_ds_read_tr6_b96_v3i32((NTM_WAVE_LDS(wv_i32x3))p);
    r[0] = (uint32_t)w[0], r[1] = (uint32_t)w[1], r[2] = (uint32_t)w[2];
  }
}


// ------------------------------------------------------------------ record
__device__ __forceinline__ void record_begin(Record* rec) {
  const unsigned t = threadIdx.x;
  unsigned hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  const unsigned xcc = xcc_id_raw();
  if ((t & 63u) == 0) {
    rec->simd[t >> 6] = (uint8_t)((hw >> 4) & 3u);
    if (t == 0) rec->hw_id = hw, rec->xcc_id = xcc, rec->magic = kMagic, rec->wg = blockIdx.x;
  }
}
// Each thread keeps its own smallest mismatch; the workgroup's smallest index wins and its
// owner alone stores expected / got. Called by all 256 threads.
struct Mine {
  uint32_t index = ~0u, expected = 0, got = 0, count = 0;
  __device__ __forceinline__ void judge(uint32_t idx, uint32_t e, uint32_t g) {
    if (e == g) return;
    ++count;
    if (idx < index) index = idx, expected = e, got = g;
  }
};
__device__ __forceinline__ void record_end(Record* rec, const Mine& m) {
  if (m.count) {
    atomicAdd(&rec->bad, m.count);
    atomicMax(&rec->first, ~m.index);
  }
  __syncthreads();
  if (m.count && *(volatile uint32_t*)&rec->first == ~m.index) rec->expected = m.expected, rec->got = m.got;
}

// ------------------------------------------------------------------ lane
template <int I>
__device__ __forceinline__ uint32_t dpp_one(uint32_t x, uint32_t y) {
  constexpr LaneOp op = lane_op(I);
  return (uint32_t)__builtin_amdgcn_update_dpp((int)y, (int)x, op.ctrl, op.row_mask, op.bank_mask, op.bound != 0);
}
template <int... I>
__device__ __forceinline__ uint32_t dpp_any(int i, uint32_t x, uint32_t y, std::integer_sequence<int, I...>) {
  uint32_t r = 0;
  ((i == I ? (void)(r = dpp_one<I>(x, y)) : (void)0), ...);
  return r;
}
template <int... I>
__device__ __forceinline__ uint32_t swizzle_any(int i, uint32_t x, std::integer_sequence<int, I...>) {
  uint32_t r = 0;
  ((i == I ? (void)(r = (uint32_t)__builtin_amdgcn_ds_swizzle((int)x, swizzle_at(I))) : (void)0), ...);
  return r;
}
// op `opi` (uniform over the workgroup) on this lane's words x and y, with the instruction
__device__ __forceinline__ uint32_t lane_apply(int opi, uint32_t x, uint32_t y, int l) {
  const LaneOp op = lane_op(opi);
  uint32_t r = y;
  switch (op.kind) {
    case kDpp:
      r = dpp_any(opi, x, y, std::make_integer_sequence<int, kDppOps>{});
      if (src_lane(op, l) == kSkip) r = 0;
      break;
    case kBpermute: r = (uint32_t)__builtin_amdgcn_ds_bpermute((int)bpermute_index(op.ctrl, l), (int)x); break;
    case kPermute: r = (uint32_t)__builtin_amdgcn_ds_permute((int)permute_index(op.ctrl, l), (int)x); break;
    case kSwizzle: r = swizzle_any(opi - kFirstSwizzleOp, x, std::make_integer_sequence<int, kSwizzles>{}); break;
    case kSwap16: {
      const auto p = __builtin_amdgcn_permlane16_swap(x, y, false, false);
      r = op.ctrl ? p[1] : p[0];
      break;
    }
    case kSwap32: {
      const auto p = __builtin_amdgcn_permlane32_swap(x, y, false, false);
      r = op.ctrl ? p[1] : p[0];
      break;
    }
    case kReadlane: r = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)op.ctrl); break;
    case kReadfirst: r = (uint32_t)__builtin_amdgcn_readfirstlane((int)x); break;
    case kReadfirstBranch:
      if (l >= (int)op.ctrl) r = (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
      break;
    case kBpermuteBranch:
      if (l >= 32) r = (uint32_t)__builtin_amdgcn_ds_bpermute((int)branch_bpermute_index(l), (int)x);
      break;
  }
  return r;
}
// the same through LDS: every lane's words are in lx / ly of its wave
__device__ __forceinline__ uint32_t lane_reference(int opi, const uint32_t* lx, const uint32_t* ly, int l) {
  return lane_expected(lane_op(opi), l, lx, ly);
}

// words x[n], y[n] (n a multiple of 256) -> out[k * n + i] for ops op_first + k, k < op_count
template <bool REF>
__global__ void __launch_bounds__(256) wave_lane_kernel(const uint32_t* x, const uint32_t* y, uint32_t* out, int op_first,
                                                        int op_count, size_t n) {
  __shared__ uint32_t lx[kThreads], ly[kThreads];
  const unsigned t = threadIdx.x, l = t & 63u, wb = t & ~63u;
  const size_t i = (size_t)blockIdx.x * kThreads + t;
  const uint32_t xv = x[i], yv = y[i];
  if (REF) {
    lx[t] = xv, ly[t] = yv;
    __syncthreads();
  }
  for (int k = 0; k < op_count; ++k)
    out[(size_t)k * n + i] = REF ? lane_reference(op_first + k, lx + wb, ly + wb, (int)l) : lane_apply(op_first + k, xv, yv, (int)l);
}
// sweep: every workgroup runs all ops on x[256], y[256] against expected[kLaneOps * 256]
__global__ void __launch_bounds__(256) wave_lane_sweep_kernel(const uint32_t* x, const uint32_t* y, const uint32_t* expected,
                                                              Record* records, uint32_t fault_wg, uint32_t fault_index) {
  Record* rec = records + blockIdx.x;
  record_begin(rec);
  const unsigned t = threadIdx.x;
  const uint32_t xv = x[t], yv = y[t];
  Mine m;
  for (int k = 0; k < kLaneOps; ++k) {
    const uint32_t idx = (uint32_t)k * kThreads + t;
    uint32_t g = lane_apply(k, xv, yv, (int)(t & 63u));
    if (blockIdx.x == fault_wg && idx == fault_index) g ^= kFaultBit;
    m.judge(idx, expected[idx], g);
  }
  record_end(rec, m);
}

// ------------------------------------------------------------------ ldstr
// image -> LDS, then per iteration one transposed read per lane (REF: bit gathers with byte reads)
__device__ __forceinline__ uint32_t tr_reference_word(const TrShape& s, const unsigned char* lds, int it, int d, int t) {
  if (d >= tr_words(s.bits)) return 0;
  const int b = it * 16 + t / 16, i = t % 16;
  uint32_t w = 0;
  for (int q = (d * 32) / s.bits; q * s.bits < d * 32 + 32 && q < tr_elems(s.bits); ++q) {
    int j, e;
    tr_src(s.bits, i, q, &j, &e);
    const unsigned char* p = lds + tr_addr(s, b, j);
    // the element's bits, gathered from the (at most 3) bytes that hold them
    const int first = e * s.bits;
    uint32_t v = 0;
    for (int k = 0; k < 3; ++k) {
      const int byte = first / 8 + k;
      if (byte * 8 < first + s.bits) v |= (uint32_t)p[byte] << (8 * k);
    }
    v = (v >> (first % 8)) & ((1u << s.bits) - 1u);
    const int pos = q * s.bits - d * 32;  // where the element starts in this dword; may be negative
    w |= pos >= 0 ? v << pos : v >> -pos;
  }
  return w;
}
template <int BITS, bool REF>
__device__ __forceinline__ void tr_block(const TrShape& s, const unsigned char* lds, int it, int t, uint32_t r[3]) {
  if (REF) {
    for (int d = 0; d < 3; ++d) r[d] = tr_reference_word(s, lds, it, d, t);
  } else {
    tr_read<BITS>(lds + tr_addr(s, it * 16 + t / 16, t % 16), r);
  }
}
__device__ __forceinline__ void tr_load_image(unsigned char* lds, const uint32_t* image, const TrShape& s) {
  const int words = s.rows * s.stride / 4;
  for (int i = threadIdx.x; i < kTrMaxBytes / 4; i += kThreads) ((uint32_t*)lds)[i] = i < words ? image[i] : 0u;
  __syncthreads();
}
template <int BITS, bool REF>
__global__ void __launch_bounds__(256) wave_tr_kernel(const uint32_t* image, TrShape s, uint32_t* out) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kTrMaxBytes];
  tr_load_image(lds, image, s);
  const int t = threadIdx.x;
  for (int it = 0; it < s.iters; ++it) {
    uint32_t r[3];
    tr_block<BITS, REF>(s, lds, it, t, r);
    for (int d = 0; d < 3; ++d) out[(size_t)(it * 3 + d) * kThreads + t] = r[d];
  }
}
template <int BITS>
__device__ __forceinline__ void tr_sweep_form(const TrShape& s, unsigned char* lds, const uint32_t* image,
                                              const uint32_t* expected, uint32_t base, Mine& m) {
  __syncthreads();
  tr_load_image(lds, image, s);
  const int t = threadIdx.x;
  for (int it = 0; it < s.iters; ++it) {
    uint32_t r[3];
    tr_read<BITS>(lds + tr_addr(s, it * 16 + t / 16, t % 16), r);
    for (int d = 0; d < 3; ++d) {
      const uint32_t idx = base + (uint32_t)(it * 3 + d) * kThreads + (uint32_t)t;
      m.judge(idx, expected[idx], r[d]);
    }
  }
}
struct TrSweepArgs {
  const uint32_t* image[kTrForms];
  TrShape shape[kTrForms];
  uint32_t base[kTrForms];
};
__global__ void __launch_bounds__(256) wave_tr_sweep_kernel(TrSweepArgs a, const uint32_t* expected, Record* records) {
  __shared__ __attribute__((aligned(16))) unsigned char lds[kTrMaxBytes];
  Record* rec = records + blockIdx.x;
  record_begin(rec);
  Mine m;
  tr_sweep_form<16>(a.shape[0], lds, a.image[0], expected, a.base[0], m);
  tr_sweep_form<8>(a.shape[1], lds, a.image[1], expected, a.base[1], m);
  tr_sweep_form<4>(a.shape[2], lds, a.image[2], expected, a.base[2], m);
  tr_sweep_form<6>(a.shape[3], lds, a.image[3], expected, a.base[3], m);
  record_end(rec, m);
}

// ------------------------------------------------------------------ sfu
template <int OP>
__device__ __forceinline__ uint32_t sfu_apply(uint32_t xb) {
  const float x = __builtin_bit_cast(float, xb);
  float y;
  if constexpr (OP == kSfuExp) y = __builtin_amdgcn_exp2f(x);
  else if constexpr (OP == kSfuLog) y = __builtin_amdgcn_logf(x);
  else if constexpr (OP == kSfuRcp) y = __builtin_amdgcn_rcpf(x);
  else if constexpr (OP == kSfuRsq) y = __builtin_amdgcn_rsqf(x);
  else if constexpr (OP == kSfuSqrt) y = __builtin_amdgcn_sqrtf(x);
  else if constexpr (OP == kSfuSin) y = __builtin_amdgcn_sinf(x);
  else y = __builtin_amdgcn_cosf(x);
  return __builtin_bit_cast(uint32_t, y);
}
__device__ __forceinline__ uint32_t sfu_any(int op, uint32_t x) {
  switch (op) {
    case kSfuExp: return sfu_apply<kSfuExp>(x);
    case kSfuLog: return sfu_apply<kSfuLog>(x);
    case kSfuRcp: return sfu_apply<kSfuRcp>(x);
    case kSfuRsq: return sfu_apply<kSfuRsq>(x);
    case kSfuSqrt: return sfu_apply<kSfuSqrt>(x);
    case kSfuSin: return sfu_apply<kSfuSin>(x);
    default: return sfu_apply<kSfuCos>(x);
  }
}
__global__ void __launch_bounds__(256) wave_sfu_kernel(int op, const uint32_t* x, uint32_t* y, size_t n) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i < n) y[i] = sfu_any(op, x[i]);
}
struct SfuSweepArgs {
  const uint32_t* x[kSfuOps];
  uint32_t n[kSfuOps];
};
// every workgroup runs the whole input list of every instruction and leaves one digest each
// (xcc, se, sh, cu) of the CU this wave runs on, as cus::cu_key packs it
__device__ __forceinline__ uint32_t my_cu_key() {
  unsigned hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  return cus::cu_key(hw, xcc_id_raw());
}
// fault_key (kNoFault: none): every workgroup that runs on the CU with that key flips kFaultBit
// of result word fault_index of instruction 0 - in the sweep and in the locate launch alike, so
// that the injected CU behaves like one whose pipe is wrong.
__global__ void __launch_bounds__(256) wave_sfu_sweep_kernel(SfuSweepArgs a, Record* records, uint32_t fault_key,
                                                             uint32_t fault_index) {
  __shared__ uint64_t part[kThreads];
  Record* rec = records + blockIdx.x;
  record_begin(rec);
  const unsigned t = threadIdx.x;
  const bool faulty = my_cu_key() == fault_key;
  for (int op = 0; op < kSfuOps; ++op) {
    uint64_t acc = kDigestInit;
    for (uint32_t i = t; i < a.n[op]; i += kThreads) {
      uint32_t w = sfu_any(op, a.x[op][i]);
      if (faulty && op == 0 && i == fault_index) w ^= kFaultBit;
      acc = digest_step(acc, w);
    }
    __syncthreads();
    part[t] = digest_mix(acc, t);
    __syncthreads();
    for (unsigned h = kThreads / 2; h > 0; h >>= 1) {
      if (t < h) part[t] += part[t + h];
      __syncthreads();
    }
    if (t == 0) rec->digest[op] = part[0];
  }
}
// The second, small launch behind an inconsistent digest: of `grid` workgroups the first that
// runs on the CU `key` (on_key) - or on any other CU (!on_key) - claims the launch, stores the
// result words of instruction `op` on x[n] to y and fills its record; the others return at once.
__global__ void __launch_bounds__(256) wave_sfu_locate_kernel(int op, const uint32_t* x, uint32_t n, uint32_t key, int on_key,
                                                              uint32_t* claim, uint32_t* y, Record* rec, uint32_t fault_key,
                                                              uint32_t fault_index) {
  __shared__ int mine;
  const uint32_t here = my_cu_key();
  if (threadIdx.x == 0) mine = ((here == key) == (on_key != 0)) && atomicCAS(claim, 0u, 1u) == 0u;
  __syncthreads();
  if (!mine) return;
  record_begin(rec);
  for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
    uint32_t w = sfu_any(op, x[i]);
    if (here == fault_key && op == 0 && i == fault_index) w ^= kFaultBit;
    y[i] = w;
  }
}
__global__ void __launch_bounds__(256) wave_sfu_distance_kernel(const uint32_t* y, const uint32_t* lo, const uint32_t* hi,
                                                                size_t n, uint32_t bound, SfuDistance* out) {
  uint32_t best = 0, best_i = ~0u, beyond = 0, first = ~0u;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads) {
    const uint32_t d = sfu_distance(y[i], lo[i], hi[i]);
    if (d > best) best = d, best_i = (uint32_t)i;
    if (d > bound) {
      ++beyond;
      if ((uint32_t)i < first) first = (uint32_t)i;
    }
  }
  if (best) atomicMax(&out->max_d, best);
  if (beyond) atomicAdd(&out->beyond, beyond), atomicMin(&out->first_beyond, first);
}
// second pass: the smallest index that has the largest distance
__global__ void __launch_bounds__(256) wave_sfu_distance_index_kernel(const uint32_t* y, const uint32_t* lo,
                                                                      const uint32_t* hi, size_t n, SfuDistance* out) {
  const uint32_t best = out->max_d;
  if (!best) return;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (size_t)gridDim.x * kThreads)
    if (sfu_distance(y[i], lo[i], hi[i]) == best) atomicMin(&out->max_index, (uint32_t)i);
}

// ------------------------------------------------------------------ valu
template <int... T>
__device__ __forceinline__ void bitop3_all(uint32_t a, uint32_t b, uint32_t c, uint32_t* out, size_t stride,
                                           std::integer_sequence<int, T...>) {
  ((out[(size_t)T * stride] = (uint32_t)__builtin_amdgcn_bitop3_b32((int)a, (int)b, (int)c, T)), ...);
}
__device__ __forceinline__ uint32_t cvt_pk(uint32_t lo, uint32_t hi) {
  const wv_f32x2 f = {__builtin_bit_cast(float, lo), __builtin_bit_cast(float, hi)};
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, wv_bf16x2));
}
// bitop3: a, b, c [n] -> out[table * n + i] for the 256 tables; cvt: a (low half), b (high half) -> out[i]
template <bool REF>
__global__ void __launch_bounds__(256) wave_valu_kernel(int op, const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                        uint32_t* out, size_t n) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  if (op == kValuCvt) {
    out[i] = REF ? cvt_pk_expected(a[i], b[i]) : cvt_pk(a[i], b[i]);
  } else if (REF) {
    for (int tt = 0; tt < 256; ++tt) out[(size_t)tt * n + i] = bitop3_expected(a[i], b[i], c[i], (uint32_t)tt);
  } else {
    bitop3_all(a[i], b[i], c[i], out + i, n, std::make_integer_sequence<int, 256>{});
  }
}
template <int... T>
__device__ __forceinline__ void bitop3_judge(uint32_t a, uint32_t b, uint32_t c, const uint32_t* expected, uint32_t t,
                                             Mine& m, std::integer_sequence<int, T...>) {
  ((m.judge((uint32_t)T * kThreads + t, expected[(uint32_t)T * kThreads + t],
            (uint32_t)__builtin_amdgcn_bitop3_b32((int)a, (int)b, (int)c, T))), ...);
}
// sweep: a, b, c [256] through the 256 tables, then cvt over lo[ncvt], hi[ncvt];
// expected = [256 * 256] then [ncvt]
__global__ void __launch_bounds__(256) wave_valu_sweep_kernel(const uint32_t* a, const uint32_t* b, const uint32_t* c,
                                                              const uint32_t* lo, const uint32_t* hi, uint32_t ncvt,
                                                              const uint32_t* expected, Record* records) {
  Record* rec = records + blockIdx.x;
  record_begin(rec);
  const unsigned t = threadIdx.x;
  Mine m;
  bitop3_judge(a[t], b[t], c[t], expected, t, m, std::make_integer_sequence<int, 256>{});
  for (uint32_t i = t; i < ncvt; i += kThreads) m.judge(256u * kThreads + i, expected[256u * kThreads + i], cvt_pk(lo[i], hi[i]));
  record_end(rec, m);
}

// ------------------------------------------------------------------ launchers
// Every launcher returns hipErrorInvalidValue and launches nothing on a null pointer, a bad
// op / form id, a misaligned buffer or a bad shape.
inline bool aligned4(const void* p) { return p && ((uintptr_t)p % 4) == 0; }
inline hipError_t launch_lane(bool reference, int op_first, int op_count, const void* x, const void* y, void* out, size_t n,
                              hipStream_t s) {
  if (!aligned4(x) || !aligned4(y) || !aligned4(out) || n == 0 || n % kThreads || op_first < 0 || op_count <= 0 ||
      op_first + op_count > kLaneOps)
    return hipErrorInvalidValue;
  const dim3 g((unsigned)(n / kThreads)), b(kThreads);
  if (reference) hipLaunchKernelGGL(wave_lane_kernel<true>, g, b, 0, s, (const uint32_t*)x, (const uint32_t*)y, (uint32_t*)out, op_first, op_count, n);
  else hipLaunchKernelGGL(wave_lane_kernel<false>, g, b, 0, s, (const uint32_t*)x, (const uint32_t*)y, (uint32_t*)out, op_first, op_count, n);
  return hipGetLastError();
}
inline hipError_t launch_tr_read(bool reference, int bits, const void* image, int rows, int stride, void* out, hipStream_t s) {
  TrShape sh;
  if (!image || !aligned4(out) || ((uintptr_t)image % 16) || !tr_shape(bits, rows, stride, &sh)) return hipErrorInvalidValue;
  const dim3 g(1), b(kThreads);
  auto* im = (const uint32_t*)image;
  auto* o = (uint32_t*)out;
#define NTM_WAVE_TR(B)                                                                        \
  if (bits == B) {                                                                            \
    if (reference) hipLaunchKernelGGL((wave_tr_kernel<B, true>), g, b, 0, s, im, sh, o);      \
    else hipLaunchKernelGGL((wave_tr_kernel<B, false>), g, b, 0, s, im, sh, o);               \
  }
  NTM_WAVE_TR(16) NTM_WAVE_TR(8) NTM_WAVE_TR(4) NTM_WAVE_TR(6)
#undef NTM_WAVE_TR
  return hipGetLastError();
}
inline hipError_t launch_sfu(int op, const void* x, void* y, size_t n, hipStream_t s) {
  if (op < 0 || op >= kSfuOps || !aligned4(x) || !aligned4(y) || n == 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(wave_sfu_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, op,
                     (const uint32_t*)x, (uint32_t*)y, n);
  return hipGetLastError();
}
inline hipError_t launch_sfu_distance(const void* y, const void* lo, const void* hi, size_t n, uint32_t bound, void* out,
                                      hipStream_t s) {
  if (!aligned4(y) || !aligned4(lo) || !aligned4(hi) || !aligned4(out) || n == 0 || n > 0x7FFFFFFFu) return hipErrorInvalidValue;
  const size_t blocks = (n + kThreads - 1) / kThreads;
  const dim3 g((unsigned)(blocks < 1024 ? blocks : 1024)), b(kThreads);
  hipLaunchKernelGGL(wave_sfu_distance_kernel, g, b, 0, s, (const uint32_t*)y, (const uint32_t*)lo, (const uint32_t*)hi, n,
                     bound, (SfuDistance*)out);
  hipLaunchKernelGGL(wave_sfu_distance_index_kernel, g, b, 0, s, (const uint32_t*)y, (const uint32_t*)lo,
                     (const uint32_t*)hi, n, (SfuDistance*)out);
  return hipGetLastError();
}
inline hipError_t launch_valu(bool reference, int op, const void* a, const void* b, const void* c, void* out, size_t n,
                              hipStream_t s) {
  if ((op != kValuBitop && op != kValuCvt) || !aligned4(a) || !aligned4(b) || (op == kValuBitop && !aligned4(c)) ||
      !aligned4(out) || n == 0)
    return hipErrorInvalidValue;
  const dim3 g((unsigned)((n + kThreads - 1) / kThreads)), bl(kThreads);
  if (reference) hipLaunchKernelGGL(wave_valu_kernel<true>, g, bl, 0, s, op, (const uint32_t*)a, (const uint32_t*)b, (const uint32_t*)c, (uint32_t*)out, n);
  else hipLaunchKernelGGL(wave_valu_kernel<false>, g, bl, 0, s, op, (const uint32_t*)a, (const uint32_t*)b, (const uint32_t*)c, (uint32_t*)out, n);
  return hipGetLastError();
}
inline hipError_t launch_sfu_locate(int op, const void* x, uint32_t n, uint32_t key, int on_key, void* claim, void* y,
                                    void* record, int grid, uint32_t fault_key, uint32_t fault_index, hipStream_t s) {
  if (op < 0 || op >= kSfuOps || !aligned4(x) || !aligned4(y) || !aligned4(claim) || !record || ((uintptr_t)record % 8) ||
      n == 0 || grid <= 0)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(wave_sfu_locate_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, op, (const uint32_t*)x, n, key, on_key,
                     (uint32_t*)claim, (uint32_t*)y, (Record*)record, fault_key, fault_index);
  return hipGetLastError();
}
inline hipError_t launch_sfu_sweep(const void* const x[kSfuOps], const uint32_t n[kSfuOps], void* records, int grid,
                                   uint32_t fault_key, uint32_t fault_index,
                                   hipStream_t s) {
  if (!records || ((uintptr_t)records % 8) || grid <= 0) return hipErrorInvalidValue;
  SfuSweepArgs a;
  for (int op = 0; op < kSfuOps; ++op) {
    if (!aligned4(x[op]) || n[op] == 0) return hipErrorInvalidValue;
    a.x[op] = (const uint32_t*)x[op], a.n[op] = n[op];
  }
  hipLaunchKernelGGL(wave_sfu_sweep_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, a, (Record*)records, fault_key,
                     fault_index);
  return hipGetLastError();
}
inline hipError_t launch_valu_sweep(const void* abc, const void* lo, const void* hi, uint32_t ncvt, const void* expected,
                                    void* records, int grid, hipStream_t s) {
  if (!aligned4(abc) || !aligned4(lo) || !aligned4(hi) || !aligned4(expected) || !records || ((uintptr_t)records % 8) ||
      grid <= 0 || ncvt == 0)
    return hipErrorInvalidValue;
  const uint32_t* w = (const uint32_t*)abc;
  hipLaunchKernelGGL(wave_valu_sweep_kernel, dim3((unsigned)grid), dim3(kThreads), 0, s, w, w + kThreads, w + 2 * kThreads,
                     (const uint32_t*)lo, (const uint32_t*)hi, ncvt, (const uint32_t*)expected, (Record*)records);
  return hipGetLastError();
}

// The per-CU sweeps behind one entry. `in`: the family's inputs as consecutive 32-bit words in
// one device buffer (16-byte aligned, in_words long), `layout` a host array, `expected` the table
// a reference kernel made of the inputs, `records` grid zeroed Records.
//   lane   in = x[256] y[256]; expected [kLaneOps * 256]; fault_wg / fault_index flip kFaultBit
//          of one result word of one workgroup before its compare (kNoFault: none)
//   ldstr  in = the four images of 64 rows x sweep_stride() bytes (16, 8, 4, 6 bit), each padded to 16 KiB;
//          expected = the four tr_out_words() tables in that order
//   sfu    layout = n[7]; in = the seven input lists; no table: the records carry digests; fault_wg is
//          here the key of a CU (cus::cu_key) whose workgroups flip kFaultBit of word fault_index of
//          instruction 0
//   valu   layout = {ncvt}; in = a[256] b[256] c[256] lo[ncvt] hi[ncvt]; expected [256 * 256 + ncvt]
inline hipError_t launch_sweep(int family, const void* in, size_t in_words, const uint32_t* layout, const void* expected,
                               void* records, int grid, uint32_t fault_wg, uint32_t fault_index, hipStream_t s) {
  if (!in || ((uintptr_t)in % 16) || !records || ((uintptr_t)records % 8) || grid <= 0 || family < 0 || family >= kFamilies ||
      (family != kFamSfu && !aligned4(expected)) || ((family == kFamSfu || family == kFamValu) && !layout))
    return hipErrorInvalidValue;
  const uint32_t* w = (const uint32_t*)in;
  const dim3 g((unsigned)grid), b(kThreads);
  auto* rec = (Record*)records;
  if (family == kFamLane) {
    if (in_words < 2 * kThreads) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wave_lane_sweep_kernel, g, b, 0, s, w, w + kThreads, (const uint32_t*)expected, rec, fault_wg, fault_index);
    return hipGetLastError();
  }
  if (family == kFamLdstr) {
    if (in_words < (size_t)kTrForms * kTrMaxBytes / 4) return hipErrorInvalidValue;
    TrSweepArgs a;
    uint32_t base = 0;
    for (int f = 0; f < kTrForms; ++f) {
      a.image[f] = w + (size_t)f * kTrMaxBytes / 4;
      if (!tr_shape(kTrBits[f], kSweepRows, sweep_stride(kTrBits[f]), &a.shape[f])) return hipErrorInvalidValue;
      a.base[f] = base;
      base += (uint32_t)a.shape[f].iters * 3 * kThreads;
    }
    hipLaunchKernelGGL(wave_tr_sweep_kernel, g, b, 0, s, a, (const uint32_t*)expected, rec);
    return hipGetLastError();
  }
  if (family == kFamSfu) {
    const void* x[kSfuOps];
    size_t at = 0;
    for (int op = 0; op < kSfuOps; ++op) x[op] = w + at, at += layout[op];
    if (at > in_words) return hipErrorInvalidValue;
    return launch_sfu_sweep(x, layout, records, grid, fault_wg, fault_index, s);
  }
  const uint32_t ncvt = layout[0];
  if ((size_t)3 * kThreads + 2 * (size_t)ncvt > in_words) return hipErrorInvalidValue;
  return launch_valu_sweep(w, w + 3 * kThreads, w + 3 * kThreads + ncvt, ncvt, expected, records, grid, s);
}

}  // namespace wave
}  // namespace ntm
