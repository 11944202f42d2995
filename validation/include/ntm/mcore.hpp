// K10: matrix-core check kernels for the data paths K1 and K7 never issue - the fp64, fp32,
// fp16 and int8 MFMAs and the two 2:4 structured-sparse SMFMACs of gfx950 - with an
// independent reference that uses no matrix instruction and a bitwise compare. Host side
// (format table, packers, generators, the exactness bound, messages): ntm/mcore_plan.hpp.
//
// C[M x N] = A[M x K] * B[N x K]^T, row-major. A sparse A comes as Ac[M][K/2] and Ai[M][K/4].
//
// mcore_gemm_kernel<FMT>: 256 threads (2 x 2 waves of 64 x 64 outputs) per 128 x 128 tile.
// One K-step is 128 bytes of every row of B (16 / 32 / 64 / 128 / 64 / 128 k for f64 / f32 /
// f16 / i8 / sp_bf16 / sp_i8), 128 bytes of a dense A's rows, 64 bytes of Ac plus K-step / 4
// bytes of Ai. A K-step goes global -> registers (16-byte loads, issued before the MFMAs of
// the step before) -> LDS (one buffer, two barriers per step).
//
// LDS reads without bank conflicts: every staged row is padded by 16 bytes, so the pitch is
// 144 B = 36 banks (80 B = 20 banks for Ac). The 16 lanes of a lane group read the same
// column of 16 consecutive rows; 36 r mod 64 (20 r mod 64) runs through sixteen different
// multiples of 4, so the sixteen 16-byte reads fall on sixteen different 4-bank slots, and
// the narrower 8- and 4-byte reads of f64 / f32, whose four lane groups sit side by side in
// one slot, stay apart as well.
//
// Operand maps (lane l, g = l >> 4, measured with the one-instruction probe
// ntm_mcore_mfma_probe of libntm_experimental.so; validation/README.md has the table):
//   f64, f32   A[row l & 15][k = g], B[k = g][col l & 15], one element per lane;
//   f16        element j of 8: k = 8 g + j;
//   i8         byte j of 16: k = 16 g + j;
//   sp_bf16    A element j of 8: kept value j & 1 of group 4 g + (j >> 1), so a lane group owns
//              k 16 g .. 16 g + 15; index VGPR bits 2 j + 1 .. 2 j: that value's position, which
//              is p0 | p1 << 2 of group 4 g + q in bits 4 q + 3 .. 4 q. B is split like the
//              8-bit operands of K7: elements 0-7 hold k 8 g + j, elements 8-15 k 32 + 8 g + j - 8;
//   sp_i8      A byte j of 16: kept value j & 1 of group 8 g + (j >> 1) (k 32 g .. 32 g + 31),
//              index bits as above with q = 0 .. 7, all 32 in use; B bytes 0-15 hold k 16 g + j,
//              bytes 16-31 k 64 + 16 g + j - 16.
//   Both sparse forms are called with cbsz = abid = 0, which takes the index from the low bits
//   (16 for bf16, where abid bit 0 would select the high half; all 32 for int8).
// C/D: column l & 15, row 4 g + r (f64: row g + 4 r). Only the builtins are used, so the
// compiler places the hazard no-ops; no workgroup waits on another.
#pragma once

#include <type_traits>

#include "ntm/common.hpp"
#include "ntm/mcore_plan.hpp"

namespace ntm {
namespace mc {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x16 __attribute__((ext_vector_type(16)));

constexpr int kThreads = 256;
constexpr int kStepBytes = 128;  // of a row of B per K-step
constexpr int kPad = 16;

template <int FMT>
struct Tile {
  static constexpr bool kSparse = FMT >= kSpBf16;
  static constexpr int kElem = kFormatTable[FMT].elem_bytes;
  static constexpr int kStepK = kStepBytes / kElem;                       // k per K-step
  static constexpr int kInstrK = FMT == kF64 || FMT == kF32 ? 4 : FMT == kF16 ? 32 : FMT == kI8 || FMT == kSpBf16 ? 64 : 128;
  static constexpr int kSub = kStepK / kInstrK;                           // instructions deep per K-step
  static constexpr int kARow = kSparse ? kStepBytes / 2 : kStepBytes;     // bytes of A / Ac per row and step
  static constexpr int kIRow = kSparse ? kStepK / 4 : 0;                  // bytes of Ai per row and step
  static constexpr int kAPitch = kARow + kPad, kBPitch = kStepBytes + kPad, kIPitch = kIRow + kPad;
  static constexpr int kAChunks = kTile * (kARow / 16) / kThreads;        // 16-byte loads per thread: 4 or 2
  static constexpr int kBChunks = kTile * (kStepBytes / 16) / kThreads;   // 4
  using Acc = typename std::conditional<FMT == kF64, f64x4, typename std::conditional<kFormatTable[FMT].integer, i32x4, f32x4>::type>::type;
};

template <int N>
struct Words {
  unsigned w[N];
};
template <int N>
__device__ __forceinline__ Words<N> lds_words(const unsigned char* p) {
  Words<N> r;
#pragma unroll
  for (int i = 0; i < N; ++i) r.w[i] = ((const unsigned*)p)[i];
  return r;
}

// the index VGPR of a lane: the low four bits of n consecutive Ai bytes, lowest group first
template <int N>
__device__ __forceinline__ int index_reg(const unsigned char* p) {
  unsigned v = 0;
#pragma unroll
  for (int q = 0; q < N; ++q) v |= (unsigned)(p[q] & 15) << (4 * q);
  return (int)v;
}

// The dense B fragment of a sparse instruction: registers 0-3 from bytes 16 g .. 16 g + 15 of
// the row's K-step, registers 4-7 from bytes 64 + 16 g .. (the map in the header comment)
__device__ __forceinline__ Words<8> sparse_b(const unsigned char* b, int g) {
  const Words<4> lo = lds_words<4>(b + 16 * g), hi = lds_words<4>(b + 64 + 16 * g);
  Words<8> r;
#pragma unroll
  for (int i = 0; i < 4; ++i) r.w[i] = lo.w[i], r.w[4 + i] = hi.w[i];
  return r;
}

// One matrix instruction of sub-step u on lane group g's fragments: a / b point at the lane's
// row of the staged K-step, ai at its row of Ai.
template <int FMT>
__device__ __forceinline__ typename Tile<FMT>::Acc mma(const unsigned char* a, const unsigned char* ai,
                                                       const unsigned char* b, int g, int u,
                                                       typename Tile<FMT>::Acc c) {
  if constexpr (FMT == kF64) {
    return __builtin_amdgcn_mfma_f64_16x16x4f64(*(const double*)(a + (4 * u + g) * 8), *(const double*)(b + (4 * u + g) * 8), c, 0, 0, 0);
  } else if constexpr (FMT == kF32) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(*(const float*)(a + (4 * u + g) * 4), *(const float*)(b + (4 * u + g) * 4), c, 0, 0, 0);
  } else if constexpr (FMT == kF16) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(*(const f16x8*)(a + 64 * u + 16 * g), *(const f16x8*)(b + 64 * u + 16 * g), c, 0, 0, 0);
  } else if constexpr (FMT == kI8) {
    return __builtin_amdgcn_mfma_i32_16x16x64_i8(*(const i32x4*)(a + 64 * u + 16 * g), *(const i32x4*)(b + 64 * u + 16 * g), c, 0, 0, 0);
  } else if constexpr (FMT == kSpBf16) {
    const auto fa = lds_words<4>(a + 16 * g);
    const Words<8> fb = sparse_b(b, g);
    return __builtin_amdgcn_smfmac_f32_16x16x64_bf16(__builtin_bit_cast(bf16x8, fa), __builtin_bit_cast(bf16x16, fb), c,
                                                     index_reg<4>(ai + 4 * g), 0, 0);
  } else {
    const auto fa = lds_words<4>(a + 16 * g);
    const Words<8> fb = sparse_b(b, g);
    return __builtin_amdgcn_smfmac_i32_16x16x128_i8(__builtin_bit_cast(i32x4, fa), __builtin_bit_cast(i32x8, fb), c,
                                                    index_reg<8>(ai + 8 * g), 0, 0);
  }
}

template <int FMT>
struct AccElem {
  using type = typename std::conditional<FMT == kF64, double, typename std::conditional<kFormatTable[FMT].integer, int, float>::type>::type;
};

template <int FMT>
__global__ void __launch_bounds__(kThreads)
mcore_gemm_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ AI,
                  const unsigned char* __restrict__ B, typename AccElem<FMT>::type* __restrict__ C, int M, int N,
                  int K) {
  using T = Tile<FMT>;
  using Acc = typename T::Acc;
  __shared__ __attribute__((aligned(16))) unsigned char la[kTile * T::kAPitch];
  __shared__ __attribute__((aligned(16))) unsigned char lb[kTile * T::kBPitch];
  __shared__ __attribute__((aligned(16))) unsigned char li[T::kSparse ? kTile * T::kIPitch : 16];
  const int t = threadIdx.x, l = t & 63, w = t >> 6, g = l >> 4;
  const int wm = w >> 1, wn = w & 1;
  const size_t m0 = (size_t)blockIdx.y * kTile, n0 = (size_t)blockIdx.x * kTile;
  const size_t a_pitch = (size_t)(T::kSparse ? K / 2 : K) * T::kElem, b_pitch = (size_t)K * T::kElem, i_pitch = (size_t)K / 4;
  const int steps = K / T::kStepK;
  constexpr int kACols = T::kARow / 16, kBCols = kStepBytes / 16, kICols = T::kSparse ? T::kIRow / 16 : 1;

  u32x4 ga[T::kAChunks], gb[T::kBChunks], gi = {0, 0, 0, 0};
  auto load_global = [&](int s) {
#pragma unroll
    for (int i = 0; i < T::kAChunks; ++i) {
      const int c = t + i * kThreads, row = c / kACols, col = c % kACols;
      ga[i] = *(const u32x4*)(A + (m0 + row) * a_pitch + (size_t)s * T::kARow + col * 16);
    }
#pragma unroll
    for (int i = 0; i < T::kBChunks; ++i) {
      const int c = t + i * kThreads, row = c / kBCols, col = c % kBCols;
      gb[i] = *(const u32x4*)(B + (n0 + row) * b_pitch + (size_t)s * kStepBytes + col * 16);
    }
    if constexpr (T::kSparse) {
      if (t < kTile * kICols) gi = *(const u32x4*)(AI + (m0 + t / kICols) * i_pitch + (size_t)s * T::kIRow + (t % kICols) * 16);
    }
  };
  auto store_lds = [&]() {
#pragma unroll
    for (int i = 0; i < T::kAChunks; ++i) {
      const int c = t + i * kThreads, row = c / kACols, col = c % kACols;
      *(u32x4*)(&la[row * T::kAPitch + col * 16]) = ga[i];
    }
#pragma unroll
    for (int i = 0; i < T::kBChunks; ++i) {
      const int c = t + i * kThreads, row = c / kBCols, col = c % kBCols;
      *(u32x4*)(&lb[row * T::kBPitch + col * 16]) = gb[i];
    }
    if constexpr (T::kSparse) {
      if (t < kTile * kICols) *(u32x4*)(&li[(t / kICols) * T::kIPitch + (t % kICols) * 16]) = gi;
    }
  };

  Acc acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = Acc{0, 0, 0, 0};

  load_global(0);
  for (int s = 0; s < steps; ++s) {
    store_lds();
    __syncthreads();
    if (s + 1 < steps) load_global(s + 1);
#pragma unroll
    for (int u = 0; u < T::kSub; ++u)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) {
        const int ar = wm * 64 + mt * 16 + (l & 15);
#pragma unroll
        for (int nt = 0; nt < 4; ++nt)
          acc[mt][nt] = mma<FMT>(&la[ar * T::kAPitch], &li[T::kSparse ? ar * T::kIPitch : 0],
                                 &lb[(wn * 64 + nt * 16 + (l & 15)) * T::kBPitch], g, u, acc[mt][nt]);
      }
    __syncthreads();  // every read of this step is done before the next step's stores
  }

  // C/D of the 16 x 16 shapes: column l & 15; row 4 g + r, for f64 g + 4 r
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t row = m0 + wm * 64 + mt * 16 + (FMT == kF64 ? g + 4 * r : 4 * g + r);
        const size_t col = n0 + wn * 64 + nt * 16 + (l & 15);
        C[row * (size_t)N + col] = acc[mt][nt][r];
      }
}

// ---- the reference: no matrix instruction. A 16 x 16 block of threads computes a 16 x 16
// patch of C, one element per thread: 32 k of the 16 + 16 rows are converted to the
// accumulator's type and staged in LDS (a sparse A expanded from Ac / Ai on the way), then
// every thread runs a plain fma (integer multiply-add) loop in k order.
template <int FMT>
__device__ __forceinline__ typename AccElem<FMT>::type ref_elem(const unsigned char* base, size_t idx) {
  if constexpr (FMT == kF64) return ((const double*)base)[idx];
  else if constexpr (FMT == kF32) return ((const float*)base)[idx];
  else if constexpr (FMT == kF16) return (float)((const _Float16*)base)[idx];
  else if constexpr (FMT == kSpBf16) return __uint_as_float((unsigned)((const unsigned short*)base)[idx] << 16);
  else return (int)((const signed char*)base)[idx];
}

template <int FMT>
__global__ void __launch_bounds__(256)
mcore_ref_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ AI,
                 const unsigned char* __restrict__ B, typename AccElem<FMT>::type* __restrict__ C, int M, int N,
                 int K) {
  using E = typename AccElem<FMT>::type;
  constexpr bool sparse = kFormatTable[FMT].sparse;
  __shared__ E sa[16][33], sb[16][33];
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
  const size_t i0 = (size_t)blockIdx.y * 16, j0 = (size_t)blockIdx.x * 16;
  E acc = 0;
  for (int k0 = 0; k0 < K; k0 += 32) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int r = (t >> 5) + 8 * h, k = k0 + (t & 31);
      E a = 0;
      if constexpr (sparse) {
        const unsigned ib = AI[(i0 + r) * (size_t)(K / 4) + k / 4];
        const int p = k & 3, slot = p == (int)(ib & 3) ? 0 : p == (int)((ib >> 2) & 3) ? 1 : -1;
        if (slot >= 0) a = ref_elem<FMT>(A, (i0 + r) * (size_t)(K / 2) + 2 * (k / 4) + slot);
      } else {
        a = ref_elem<FMT>(A, (i0 + r) * (size_t)K + k);
      }
      sa[r][t & 31] = a;
      sb[r][t & 31] = ref_elem<FMT>(B, (j0 + r) * (size_t)K + k);
    }
    __syncthreads();
    for (int k = 0; k < 32; ++k) {
      if constexpr (FMT == kF64) acc = fma(sa[ti][k], sb[tj][k], acc);
      else if constexpr (kFormatTable[FMT].integer) acc += sa[ti][k] * sb[tj][k];
      else acc = fmaf(sa[ti][k], sb[tj][k], acc);
    }
    __syncthreads();
  }
  C[(i0 + ti) * (size_t)N + j0 + tj] = acc;
}

// ---- the compare: bitwise, 4- or 8-byte words (W = uint32_t / uint64_t). The healthy path
// executes no atomic and no store. mcore_compare_finish_kernel (one thread, after it on the
// stream) fills expected / got of the first differing word.
template <typename W>
__global__ void __launch_bounds__(256)
mcore_compare_kernel(const W* __restrict__ expected, const W* __restrict__ got, size_t n, Mismatch* out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (expected[i] == got[i]) continue;
    atomicAdd((unsigned long long*)&out->count, 1ull);
    atomicMin((unsigned long long*)&out->first_index, (unsigned long long)i);
  }
}
template <typename W>
__global__ void mcore_compare_finish_kernel(const W* __restrict__ expected, const W* __restrict__ got, size_t n,
                                            Mismatch* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || out->count == 0 || out->first_index >= n) return;
  out->expected = expected[out->first_index];
  out->got = got[out->first_index];
}

// ---- launchers. AI is ignored by the dense formats.
inline bool args_ok(int fmt, const void* A, const void* AI, const void* B, const void* C, int M, int N, int K) {
  if (!format_ok(fmt) || !shape_ok(M, N, K) || !A || !B || !C) return false;
  if (kFormatTable[fmt].sparse && (!AI || ((uintptr_t)AI % 16))) return false;
  return !((uintptr_t)A % 16) && !((uintptr_t)B % 16) && !((uintptr_t)C % 8);
}

template <int FMT>
inline void launch_one(bool ref, const void* A, const void* AI, const void* B, void* C, int M, int N, int K,
                       hipStream_t s) {
  using E = typename AccElem<FMT>::type;
  auto* a = (const unsigned char*)A;
  auto* ai = (const unsigned char*)AI;
  auto* b = (const unsigned char*)B;
  if (ref)
    hipLaunchKernelGGL(mcore_ref_kernel<FMT>, dim3((unsigned)(N / 16), (unsigned)(M / 16)), dim3(256), 0, s, a, ai, b,
                       (E*)C, M, N, K);
  else
    hipLaunchKernelGGL(mcore_gemm_kernel<FMT>, dim3((unsigned)(N / kTile), (unsigned)(M / kTile)), dim3(kThreads), 0,
                       s, a, ai, b, (E*)C, M, N, K);
}

inline hipError_t launch_mcore(bool ref, int fmt, const void* A, const void* AI, const void* B, void* C, int M, int N,
                               int K, hipStream_t s) {
  if (!args_ok(fmt, A, AI, B, C, M, N, K)) return hipErrorInvalidValue;
  switch (fmt) {
    case kF64: launch_one<kF64>(ref, A, AI, B, C, M, N, K, s); break;
    case kF32: launch_one<kF32>(ref, A, AI, B, C, M, N, K, s); break;
    case kF16: launch_one<kF16>(ref, A, AI, B, C, M, N, K, s); break;
    case kI8: launch_one<kI8>(ref, A, AI, B, C, M, N, K, s); break;
    case kSpBf16: launch_one<kSpBf16>(ref, A, AI, B, C, M, N, K, s); break;
    default: launch_one<kSpI8>(ref, A, AI, B, C, M, N, K, s); break;
  }
  return hipGetLastError();
}

// `out`: one initialised Mismatch (mismatch_init) in device memory, 8-byte aligned; n words
// of word_bytes (4 or 8) each.
inline hipError_t launch_mcore_compare(const void* expected, const void* got, size_t n, int word_bytes, void* out,
                                       hipStream_t s) {
  if (!expected || !got || !out || (word_bytes != 4 && word_bytes != 8) || ((uintptr_t)expected % word_bytes) ||
      ((uintptr_t)got % word_bytes) || ((uintptr_t)out % 8))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const size_t blocks = (n + 255) / 256;
  const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096));
  if (word_bytes == 8) {
    hipLaunchKernelGGL(mcore_compare_kernel<uint64_t>, grid, dim3(256), 0, s, (const uint64_t*)expected,
                       (const uint64_t*)got, n, (Mismatch*)out);
    hipLaunchKernelGGL(mcore_compare_finish_kernel<uint64_t>, dim3(1), dim3(1), 0, s, (const uint64_t*)expected,
                       (const uint64_t*)got, n, (Mismatch*)out);
  } else {
    hipLaunchKernelGGL(mcore_compare_kernel<uint32_t>, grid, dim3(256), 0, s, (const uint32_t*)expected,
                       (const uint32_t*)got, n, (Mismatch*)out);
    hipLaunchKernelGGL(mcore_compare_finish_kernel<uint32_t>, dim3(1), dim3(1), 0, s, (const uint32_t*)expected,
                       (const uint32_t*)got, n, (Mismatch*)out);
  }
  return hipGetLastError();
}

}  // namespace mc
}  // namespace ntm
