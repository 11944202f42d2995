// K11: MX quantise / dequantise on the device with the gfx950 scaled-conversion
// instructions (v_cvt_scalef32_*), and reference kernels that do the same jobs
// with integer bit arithmetic only (ntm/mxq_plan.hpp). Semantics, layouts and
// what happens outside the judged domain: mxq_plan.hpp.
//
// What the one-instruction probe (tools/mxq_cvt_probe.py, profiles/mxq/) showed
// and these kernels rely on:
//  - the scale operand is an fp32 of which only the exponent field counts; the
//    down conversions divide by 2^(exp - 127), the up conversions multiply;
//  - pk_fp4: src0 -> low nibble, src1 -> high nibble of the byte the selector
//    names; pk_fp8 / pk_bf8: src0 -> low byte of the selected 16-bit half;
//  - 2xpk16 interleaves its two vectors: six-bit slot 2i holds src0[i] and
//    slot 2i + 1 holds src1[i] (kFp6Interleaved), the slots as one
//    little-endian bit string; pk32_f32_fp6 / bf6 return slot s as element s;
//  - ties go to the even code, element subnormals are produced;
//  - a finite overflow saturates in the 4- and 6-bit formats but gives NaN
//    (e4m3) / infinity (e5m2) in the 8-bit ones, so every kernel clamps the
//    magnitude in plain code before the conversion;
//  - sr_pk_fp4 adds random bits 10 .. 31 (second value: 9 .. 30) and sr_fp8
//    bits 12 .. 31 to the dropped fraction bits.
#pragma once

#include <hip/hip_runtime.h>

#include "ntm/mxq_plan.hpp"

namespace ntm {
namespace mxq {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x32 __attribute__((ext_vector_type(32)));
typedef unsigned u32x6 __attribute__((ext_vector_type(6)));
typedef short i16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));

constexpr bool kFp6Interleaved = true;   // measured: profiles/mxq/README.md
constexpr int kThreads = 256;

template <int FMT>
struct F {
  static constexpr int bits = mx::kFormatTable[FMT].bits;
  static constexpr int mb = mx::kFormatTable[FMT].man_bits;
  static constexpr int bias = mx::kFormatTable[FMT].bias;
  static constexpr int emax = kEmaxElem[FMT];
  static constexpr int max_code = kMaxCode[FMT];
};

__device__ __forceinline__ float as_f(uint32_t b) { return __builtin_bit_cast(float, b); }
__device__ __forceinline__ uint32_t as_u(float f) { return __builtin_bit_cast(uint32_t, f); }

// ---- thin wrappers of the instructions: two values down into `old`, SEL a compile-time selector
template <int FMT, int SEL>  // fp4: SEL = byte 0 .. 3; fp8: SEL = half 0 .. 1
__device__ __forceinline__ uint32_t cvt_pk_down(uint32_t old, float a, float b, float scale) {
  if constexpr (FMT == mx::kFmtE2M1) {
    return __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(old, a, b, scale, SEL);
  } else if constexpr (FMT == mx::kFmtE4M3) {
    i16x2 r = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(__builtin_bit_cast(i16x2, old), a, b, scale, SEL != 0);
    return __builtin_bit_cast(uint32_t, r);
  } else {
    static_assert(FMT == mx::kFmtE5M2, "pk down: e2m1, e4m3, e5m2");
    i16x2 r = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(__builtin_bit_cast(i16x2, old), a, b, scale, SEL != 0);
    return __builtin_bit_cast(uint32_t, r);
  }
}
template <int FMT>
__device__ __forceinline__ u32x6 cvt_pk32_down(f32x16 a, f32x16 b, float scale) {
  if constexpr (FMT == mx::kFmtE2M3) return __builtin_amdgcn_cvt_scalef32_2xpk16_fp6_f32(a, b, scale);
  else return __builtin_amdgcn_cvt_scalef32_2xpk16_bf6_f32(a, b, scale);
}
template <int FMT, int SEL>
__device__ __forceinline__ f32x2 cvt_pk_up(uint32_t src, float scale) {
  if constexpr (FMT == mx::kFmtE2M1) return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(src, scale, SEL);
  else if constexpr (FMT == mx::kFmtE4M3) return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(src, scale, SEL != 0);
  else return __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(src, scale, SEL != 0);
}
template <int FMT>
__device__ __forceinline__ f32x32 cvt_pk32_up(u32x6 src, float scale) {
  if constexpr (FMT == mx::kFmtE2M3) return __builtin_amdgcn_cvt_scalef32_pk32_f32_fp6(src, scale);
  else return __builtin_amdgcn_cvt_scalef32_pk32_f32_bf6(src, scale);
}

// the largest finite value of the format times 2^(byte - 127), as fp32 bits (saturating at
// the largest fp32): the clamp bound of a block
template <int FMT>
__device__ __forceinline__ uint32_t clamp_bound(int byte) {
  const int E = byte + F<FMT>::emax;
  constexpr uint32_t frac = (uint32_t)(F<FMT>::max_code & ((1 << F<FMT>::mb) - 1)) << (23 - F<FMT>::mb);
  return E >= 255 ? 0x7F7FFFFFu : ((uint32_t)E << 23) | frac;
}
__device__ __forceinline__ float clamp_mag(float v, uint32_t bound) {
  const uint32_t b = as_u(v), m = b & 0x7FFFFFFFu;
  return as_f((b & 0x80000000u) | (m > bound ? bound : m));
}

// ---- loads of 8 consecutive source elements as fp32 (a bf16 widens exactly)
template <bool BF16, bool ALIGNED>
__device__ __forceinline__ void load8(const void* x, size_t idx, float (&v)[8]) {
  if constexpr (BF16) {
    const uint16_t* p = (const uint16_t*)x + idx;
    if constexpr (ALIGNED) {
      const uint4 w = *(const uint4*)p;
      const uint32_t u[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) v[2 * i] = as_f(u[i] << 16), v[2 * i + 1] = as_f(u[i] & 0xFFFF0000u);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = as_f((uint32_t)p[i] << 16);
    }
  } else {
    const float* p = (const float*)x + idx;
    if constexpr (ALIGNED) {
      const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
      v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = p[i];
    }
  }
}
template <bool BF16, bool ALIGNED>
__device__ __forceinline__ void store8(void* y, size_t idx, const float (&v)[8]) {
  if constexpr (BF16) {
    uint16_t* p = (uint16_t*)y + idx;
    uint32_t u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      u[i] = (uint32_t)f32_to_bf16_rne(as_u(v[2 * i])) | ((uint32_t)f32_to_bf16_rne(as_u(v[2 * i + 1])) << 16);
    if constexpr (ALIGNED) {
      *(uint4*)p = make_uint4(u[0], u[1], u[2], u[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) p[2 * i] = (uint16_t)u[i], p[2 * i + 1] = (uint16_t)(u[i] >> 16);
    }
  } else {
    float* p = (float*)y + idx;
    if constexpr (ALIGNED) {
      *(float4*)p = make_float4(v[0], v[1], v[2], v[3]);
      *(float4*)(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) p[i] = v[i];
    }
  }
}

// Scale bytes of `group` (1 or 4) consecutive lanes' blocks -> memory. Lane l holds the
// byte of block `blk` when (l % group == 0) and `valid`. Four consecutive blocks whose first
// index is a multiple of 4 go out as one dword from the first of their lanes; the last,
// partial four of the array as single bytes. Every lane of the wave must call this.
template <int GROUP>
__device__ __forceinline__ void store_scales(uint8_t* scales, size_t blk, size_t blocks, uint32_t byte, bool valid) {
  const uint32_t b1 = byte | ((uint32_t)__shfl_xor((int)byte, GROUP) << 8);
  const uint32_t b2 = b1 | ((uint32_t)__shfl_xor((int)b1, 2 * GROUP) << 16);
  const int lane = threadIdx.x & 63;
  if (!valid || lane % GROUP) return;
  const bool whole = (blk | 3) < blocks;  // blocks blk & ~3 .. blk | 3 all exist
  if (whole) {
    if (lane % (4 * GROUP) == 0) *(uint32_t*)(scales + blk) = b2;
  } else {
    scales[blk] = (uint8_t)byte;
  }
}

// ---- quantise. GIVEN: the scale bytes come from `scales` (the element-level form,
// mxq_cvt) instead of the rule. SR (e2m1, e4m3): stochastic rounding, the random word of
// element i of the matrix (row * K + k) is hash32(seed, kStreamSr, i).
//
// fp4 / fp8: a thread owns 8 elements, four consecutive lanes one block. The block count
// need not fill a wave: lanes past the end load nothing and store nothing, and since a
// row holds a whole number of blocks the four lanes of a block are in or out together.
template <int FMT, bool BF16, bool ALIGNED, bool GIVEN, bool SR>
__global__ void __launch_bounds__(kThreads)
mxq_quantize_kernel(const void* __restrict__ x, uint8_t* __restrict__ packed, uint8_t* __restrict__ scales, int R,
                    int K, int ldx, unsigned long long seed) {
  const size_t o = (size_t)blockIdx.x * kThreads + threadIdx.x;  // octet of elements
  const size_t per_row = (size_t)K / 8, total = (size_t)R * per_row;
  const bool valid = o < total;
  const size_t row = valid ? o / per_row : 0, c8 = valid ? o % per_row : 0;
  float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (valid) load8<BF16, ALIGNED>(x, row * (size_t)ldx + c8 * 8, v);
  uint32_t byte;
  if constexpr (GIVEN) {
    byte = valid ? scales[o >> 2] : (uint32_t)mx::kScaleBias;
  } else {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) m = max(m, as_u(v[i]) & 0x7FFFFFFFu);
    m = max(m, (uint32_t)__shfl_xor((int)m, 1));
    m = max(m, (uint32_t)__shfl_xor((int)m, 2));
    byte = (uint32_t)scale_byte(m, F<FMT>::emax);
  }
  const float scale = as_f(byte << 23);
  const uint32_t bound = clamp_bound<FMT>((int)byte);
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = clamp_mag(v[i], bound);
  uint32_t w0 = 0, w1 = 0;
  if constexpr (SR) {
    const size_t e0 = row * (size_t)K + c8 * 8;
    uint32_t rnd[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) rnd[i] = mx::hash32(seed, kStreamSr, e0 + i);
    if constexpr (FMT == mx::kFmtE2M1) {
      // the instruction takes one random word for its two values: issue it once per
      // element with that element's word and keep that element's nibble
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const f32x2 pair = {v[2 * i], v[2 * i + 1]};
        const uint32_t lo = __builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, pair, rnd[2 * i], scale, 0);
        const uint32_t hi = __builtin_amdgcn_cvt_scalef32_sr_pk_fp4_f32(0u, pair, rnd[2 * i + 1], scale, 0);
        w0 |= ((lo & 0x0Fu) | (hi & 0xF0u)) << (8 * i);
      }
    } else {
      static_assert(!SR || FMT == mx::kFmtE2M1 || FMT == mx::kFmtE4M3, "stochastic rounding: e2m1 and e4m3");
      int a = 0, b = 0;
      a = __builtin_amdgcn_cvt_scalef32_sr_fp8_f32(a, v[0], rnd[0], scale, 0);
      a = __builtin_amdgcn_cvt_scalef32_sr_fp8_f32(a, v[1], rnd[1], scale, 1);
      a = __builtin_amdgcn_cvt_scalef32_sr_fp8_f32(a, v[2], rnd[2], scale, 2);
      a = __builtin_amdgcn_cvt_scalef32_sr_fp8_f32(a, v[3], rnd[3], scale, 3);
      b = __builtin_amdgcn_cvt_scalef32_sr_fp8_f32(b, v[4], rnd[4], scale, 0);
      b = __builtin_amdgcn_cvt_scalef32_sr_fp8_f32(b, v[5], rnd[5], scale, 1);
      b = __builtin_amdgcn_cvt_scalef32_sr_fp8_f32(b, v[6], rnd[6], scale, 2);
      b = __builtin_amdgcn_cvt_scalef32_sr_fp8_f32(b, v[7], rnd[7], scale, 3);
      w0 = (uint32_t)a, w1 = (uint32_t)b;
    }
  } else if constexpr (FMT == mx::kFmtE2M1) {
    w0 = cvt_pk_down<FMT, 0>(w0, v[0], v[1], scale);
    w0 = cvt_pk_down<FMT, 1>(w0, v[2], v[3], scale);
    w0 = cvt_pk_down<FMT, 2>(w0, v[4], v[5], scale);
    w0 = cvt_pk_down<FMT, 3>(w0, v[6], v[7], scale);
  } else {
    w0 = cvt_pk_down<FMT, 0>(w0, v[0], v[1], scale);
    w0 = cvt_pk_down<FMT, 1>(w0, v[2], v[3], scale);
    w1 = cvt_pk_down<FMT, 0>(w1, v[4], v[5], scale);
    w1 = cvt_pk_down<FMT, 1>(w1, v[6], v[7], scale);
  }
  if (valid) {
    if constexpr (FMT == mx::kFmtE2M1) *(uint32_t*)(packed + o * 4) = w0;
    else *(uint2*)(packed + o * 8) = make_uint2(w0, w1);
  }
  if constexpr (!GIVEN) store_scales<4>(scales, o >> 2, total >> 2, byte, valid);
}

// 6-bit formats: a thread owns a block, 32 floats in, one 2xpk16, 6 dwords out.
template <int FMT, bool BF16, bool ALIGNED, bool GIVEN>
__global__ void __launch_bounds__(kThreads)
mxq_quantize6_kernel(const void* __restrict__ x, uint8_t* __restrict__ packed, uint8_t* __restrict__ scales, int R,
                     int K, int ldx) {
  const size_t blk = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t KB = (size_t)K / mx::kBlock, blocks = (size_t)R * KB;
  const bool valid = blk < blocks;
  const size_t row = valid ? blk / KB : 0, kb = valid ? blk % KB : 0;
  float v[32];
#pragma unroll
  for (int i = 0; i < 32; ++i) v[i] = 0;
  if (valid) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t[8];
      load8<BF16, ALIGNED>(x, row * (size_t)ldx + kb * mx::kBlock + j * 8, t);
#pragma unroll
      for (int i = 0; i < 8; ++i) v[8 * j + i] = t[i];
    }
  }
  uint32_t byte;
  if constexpr (GIVEN) {
    byte = valid ? scales[blk] : (uint32_t)mx::kScaleBias;
  } else {
    uint32_t m = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) m = max(m, as_u(v[i]) & 0x7FFFFFFFu);
    byte = (uint32_t)scale_byte(m, F<FMT>::emax);
  }
  const float scale = as_f(byte << 23);
  const uint32_t bound = clamp_bound<FMT>((int)byte);
  f32x16 a, b;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    a[i] = clamp_mag(v[kFp6Interleaved ? 2 * i : i], bound);
    b[i] = clamp_mag(v[kFp6Interleaved ? 2 * i + 1 : 16 + i], bound);
  }
  const u32x6 w = cvt_pk32_down<FMT>(a, b, scale);
  if (valid) {
    uint2* p = (uint2*)(packed + blk * 24);
    p[0] = make_uint2(w[0], w[1]);
    p[1] = make_uint2(w[2], w[3]);
    p[2] = make_uint2(w[4], w[5]);
  }
  if constexpr (!GIVEN) store_scales<1>(scales, blk, blocks, byte, valid);
}

// ---- dequantise, the inverse: 8 elements (fp4 / fp8) or a block (6-bit) per thread
template <int FMT, bool BF16, bool ALIGNED>
__global__ void __launch_bounds__(kThreads)
mxq_dequantize_kernel(const uint8_t* __restrict__ packed, const uint8_t* __restrict__ scales, void* __restrict__ y,
                      int R, int K, int ldx) {
  if constexpr (F<FMT>::bits == 6) {
    const size_t blk = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t KB = (size_t)K / mx::kBlock;
    if (blk >= (size_t)R * KB) return;
    const uint2* p = (const uint2*)(packed + blk * 24);
    const uint2 p0 = p[0], p1 = p[1], p2 = p[2];
    const u32x6 w = {p0.x, p0.y, p1.x, p1.y, p2.x, p2.y};
    const f32x32 r = cvt_pk32_up<FMT>(w, as_f((uint32_t)scales[blk] << 23));
    const size_t at = (blk / KB) * (size_t)ldx + (blk % KB) * mx::kBlock;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) t[i] = r[8 * j + i];
      store8<BF16, ALIGNED>(y, at + j * 8, t);
    }
  } else {
    const size_t o = (size_t)blockIdx.x * kThreads + threadIdx.x;
    const size_t per_row = (size_t)K / 8;
    if (o >= (size_t)R * per_row) return;
    const float scale = as_f((uint32_t)scales[o >> 2] << 23);
    f32x2 r0, r1, r2, r3;
    if constexpr (FMT == mx::kFmtE2M1) {
      const uint32_t w = *(const uint32_t*)(packed + o * 4);
      r0 = cvt_pk_up<FMT, 0>(w, scale), r1 = cvt_pk_up<FMT, 1>(w, scale);
      r2 = cvt_pk_up<FMT, 2>(w, scale), r3 = cvt_pk_up<FMT, 3>(w, scale);
    } else {
      const uint2 w = *(const uint2*)(packed + o * 8);
      r0 = cvt_pk_up<FMT, 0>(w.x, scale), r1 = cvt_pk_up<FMT, 1>(w.x, scale);
      r2 = cvt_pk_up<FMT, 0>(w.y, scale), r3 = cvt_pk_up<FMT, 1>(w.y, scale);
    }
    const float t[8] = {r0[0], r0[1], r1[0], r1[1], r2[0], r2[1], r3[0], r3[1]};
    store8<BF16, ALIGNED>(y, (o / per_row) * (size_t)ldx + (o % per_row) * 8, t);
  }
}

// ---- the reference kernels: the integer arithmetic of mxq_plan.hpp, no conversion
// instruction and no float operation. One thread per block; whole bytes per block (16, 24
// or 32), so plain byte stores never share a byte between threads.
template <int FMT, bool BF16, bool GIVEN>
__global__ void __launch_bounds__(kThreads)
mxq_reference_quantize_kernel(const void* __restrict__ x, uint8_t* __restrict__ packed, uint8_t* __restrict__ scales,
                              int R, int K, int ldx) {
  const size_t blk = (size_t)blockIdx.x * kThreads + threadIdx.x;
  const size_t KB = (size_t)K / mx::kBlock;
  if (blk >= (size_t)R * KB) return;
  const size_t at = (blk / KB) * (size_t)ldx + (blk % KB) * mx::kBlock;
  auto bits_at = [&](int k) -> uint32_t {
    if constexpr (BF16) return (uint32_t)((const uint16_t*)x)[at + k] << 16;
    else return ((const uint32_t*)x)[at + k];
  };
  int byte;
  if constexpr (GIVEN) {
    byte = scales[blk];
  } else {
    uint32_t m = 0;
    for (int k = 0; k < mx::kBlock; ++k) m = max(m, bits_at(k) & 0x7FFFFFFFu);
    byte = scale_byte(m, F<FMT>::emax);
    scales[blk] = (uint8_t)byte;
  }
  constexpr int bits = F<FMT>::bits;
  uint8_t* out = packed + blk * (mx::kBlock * bits / 8);
  // four codes make 2 (fp4), 3 (fp6) or 4 (fp8) whole bytes
  for (int k = 0; k < mx::kBlock; k += 4) {
    uint32_t word = 0;
    for (int i = 0; i < 4; ++i)
      word |= (uint32_t)quantize_code(bits, F<FMT>::mb, F<FMT>::bias, F<FMT>::max_code, bits_at(k + i), byte)
              << (i * bits);
    for (int i = 0; i < bits / 2; ++i) out[k / 4 * (bits / 2) + i] = (uint8_t)(word >> (8 * i));
  }
}

template <int FMT, bool BF16>
__global__ void __launch_bounds__(kThreads)
mxq_reference_dequantize_kernel(const uint8_t* __restrict__ packed, const uint8_t* __restrict__ scales,
                                void* __restrict__ y, int R, int K, int ldx) {
  const size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (size_t)R * K) return;
  constexpr int bits = F<FMT>::bits;
  const size_t row = i / K, k = i % K;
  const uint8_t* prow = packed + row * ((size_t)K * bits / 8);
  const size_t bit = k * bits;
  uint32_t c = prow[bit >> 3] >> (bit & 7);
  if ((bit & 7) + bits > 8) c |= (uint32_t)prow[(bit >> 3) + 1] << (8 - (bit & 7));
  c &= (1u << bits) - 1;
  const uint32_t v = dequantize_bits(bits, F<FMT>::mb, F<FMT>::bias, (int)c, scales[row * (K / mx::kBlock) + k / mx::kBlock]);
  if constexpr (BF16) ((uint16_t*)y)[row * (size_t)ldx + k] = f32_to_bf16_rne(v);
  else ((uint32_t*)y)[row * (size_t)ldx + k] = v;
}

// ---- launchers. Argument errors return hipErrorInvalidValue and launch nothing: a bad
// format, dtype or rounding mode, K % 32, ldx < K, a null pointer, a packed pointer that is
// not 16-byte aligned or a scales pointer that is not 4-byte aligned, stochastic rounding
// for a format other than e2m1 / e4m3 or for a reference kernel.
inline bool args_ok(int fmt, int dtype, const void* x, const void* packed, const void* scales, int R, int K, int ldx) {
  return mx::format_ok(fmt) && (dtype == kF32 || dtype == kBf16) && x && packed && scales && shape_ok(R, K, ldx) &&
         (uintptr_t)packed % 16 == 0 && (uintptr_t)scales % 4 == 0;
}
inline bool wide_ok(const void* x, int ldx, int dtype) {  // 16-byte loads / stores of the fp32 / bf16 side
  const size_t es = dtype == kBf16 ? 2 : 4;
  return (uintptr_t)x % 16 == 0 && (size_t)ldx * es % 16 == 0;
}
inline unsigned grid_for(size_t threads) { return (unsigned)((threads + kThreads - 1) / kThreads); }

template <int FMT, bool GIVEN>
inline hipError_t launch_quantize_fmt(bool reference, int dtype, const void* x, uint8_t* packed, uint8_t* scales,
                                      int R, int K, int ldx, int rounding, unsigned long long seed, hipStream_t s) {
  const size_t blocks = (size_t)R * (K / mx::kBlock);
  const bool wide = wide_ok(x, ldx, dtype), bf = dtype == kBf16;
  if (reference) {
    if (bf) hipLaunchKernelGGL((mxq_reference_quantize_kernel<FMT, true, GIVEN>), dim3(grid_for(blocks)), dim3(kThreads), 0, s, x, packed, scales, R, K, ldx);
    else hipLaunchKernelGGL((mxq_reference_quantize_kernel<FMT, false, GIVEN>), dim3(grid_for(blocks)), dim3(kThreads), 0, s, x, packed, scales, R, K, ldx);
    return hipGetLastError();
  }
#define NTM_MXQ_PICK(KERNEL, GRID, ...)                                                                              \
  if (bf && wide) hipLaunchKernelGGL((KERNEL<FMT, true, true, __VA_ARGS__>), dim3(GRID), dim3(kThreads), 0, s, ARGS);  \
  else if (bf) hipLaunchKernelGGL((KERNEL<FMT, true, false, __VA_ARGS__>), dim3(GRID), dim3(kThreads), 0, s, ARGS);    \
  else if (wide) hipLaunchKernelGGL((KERNEL<FMT, false, true, __VA_ARGS__>), dim3(GRID), dim3(kThreads), 0, s, ARGS);  \
  else hipLaunchKernelGGL((KERNEL<FMT, false, false, __VA_ARGS__>), dim3(GRID), dim3(kThreads), 0, s, ARGS);
  if constexpr (F<FMT>::bits == 6) {
#define ARGS x, packed, scales, R, K, ldx
    NTM_MXQ_PICK(mxq_quantize6_kernel, grid_for(blocks), GIVEN)
#undef ARGS
  } else {
#define ARGS x, packed, scales, R, K, ldx, seed
    if (rounding == kStochastic) {
      if constexpr (FMT == mx::kFmtE2M1 || FMT == mx::kFmtE4M3) {
        NTM_MXQ_PICK(mxq_quantize_kernel, grid_for(blocks * 4), GIVEN, true)
      }
    } else {
      NTM_MXQ_PICK(mxq_quantize_kernel, grid_for(blocks * 4), GIVEN, false)
    }
#undef ARGS
  }
#undef NTM_MXQ_PICK
  return hipGetLastError();
}

// given = false: quantise with the scale rule (scales is written); true: mxq_cvt (scales is read)
inline hipError_t launch_quantize(bool reference, bool given, int fmt, int dtype, const void* x, void* packed,
                                  void* scales, int R, int K, int ldx, int rounding, unsigned long long seed,
                                  hipStream_t s) {
  if (!args_ok(fmt, dtype, x, packed, scales, R, K, ldx)) return hipErrorInvalidValue;
  if (rounding != kRne && rounding != kStochastic) return hipErrorInvalidValue;
  if (rounding == kStochastic && (reference || (fmt != mx::kFmtE2M1 && fmt != mx::kFmtE4M3))) return hipErrorInvalidValue;
  auto* p = (uint8_t*)packed;
  auto* sc = (uint8_t*)scales;
#define NTM_MXQ_FMT(FMT)                                                                                         \
  case FMT:                                                                                                      \
    return given ? launch_quantize_fmt<FMT, true>(reference, dtype, x, p, sc, R, K, ldx, rounding, seed, s)      \
                 : launch_quantize_fmt<FMT, false>(reference, dtype, x, p, sc, R, K, ldx, rounding, seed, s);
  switch (fmt) {
    NTM_MXQ_FMT(mx::kFmtE4M3) NTM_MXQ_FMT(mx::kFmtE5M2) NTM_MXQ_FMT(mx::kFmtE2M3) NTM_MXQ_FMT(mx::kFmtE3M2)
    NTM_MXQ_FMT(mx::kFmtE2M1)
  }
#undef NTM_MXQ_FMT
  return hipErrorInvalidValue;
}

template <int FMT>
inline hipError_t launch_dequantize_fmt(bool reference, int dtype, const uint8_t* packed, const uint8_t* scales,
                                        void* y, int R, int K, int ldx, hipStream_t s) {
  const bool wide = wide_ok(y, ldx, dtype), bf = dtype == kBf16;
  if (reference) {
    const unsigned g = grid_for((size_t)R * K);
    if (bf) hipLaunchKernelGGL((mxq_reference_dequantize_kernel<FMT, true>), dim3(g), dim3(kThreads), 0, s, packed, scales, y, R, K, ldx);
    else hipLaunchKernelGGL((mxq_reference_dequantize_kernel<FMT, false>), dim3(g), dim3(kThreads), 0, s, packed, scales, y, R, K, ldx);
    return hipGetLastError();
  }
  const unsigned g = grid_for((size_t)R * K / (F<FMT>::bits == 6 ? 32 : 8));
  if (bf && wide) hipLaunchKernelGGL((mxq_dequantize_kernel<FMT, true, true>), dim3(g), dim3(kThreads), 0, s, packed, scales, y, R, K, ldx);
  else if (bf) hipLaunchKernelGGL((mxq_dequantize_kernel<FMT, true, false>), dim3(g), dim3(kThreads), 0, s, packed, scales, y, R, K, ldx);
  else if (wide) hipLaunchKernelGGL((mxq_dequantize_kernel<FMT, false, true>), dim3(g), dim3(kThreads), 0, s, packed, scales, y, R, K, ldx);
  else hipLaunchKernelGGL((mxq_dequantize_kernel<FMT, false, false>), dim3(g), dim3(kThreads), 0, s, packed, scales, y, R, K, ldx);
  return hipGetLastError();
}
inline hipError_t launch_dequantize(bool reference, int fmt, int dtype, const void* packed, const void* scales,
                                    void* y, int R, int K, int ldx, hipStream_t s) {
  if (!args_ok(fmt, dtype, y, packed, scales, R, K, ldx)) return hipErrorInvalidValue;
  auto* p = (const uint8_t*)packed;
  auto* sc = (const uint8_t*)scales;
  switch (fmt) {
    case mx::kFmtE4M3: return launch_dequantize_fmt<mx::kFmtE4M3>(reference, dtype, p, sc, y, R, K, ldx, s);
    case mx::kFmtE5M2: return launch_dequantize_fmt<mx::kFmtE5M2>(reference, dtype, p, sc, y, R, K, ldx, s);
    case mx::kFmtE2M3: return launch_dequantize_fmt<mx::kFmtE2M3>(reference, dtype, p, sc, y, R, K, ldx, s);
    case mx::kFmtE3M2: return launch_dequantize_fmt<mx::kFmtE3M2>(reference, dtype, p, sc, y, R, K, ldx, s);
    case mx::kFmtE2M1: return launch_dequantize_fmt<mx::kFmtE2M1>(reference, dtype, p, sc, y, R, K, ldx, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace mxq
}  // namespace ntm
