// K7: MX block-scaled matrix check kernels for the validation Job - a GEMM on
// the scaled f8f6f4 matrix instruction in every element format it takes, with a
// real E8M0 scale per 32-element block, an independent reference that uses no
// matrix core, and a bitwise compare. Host side (formats, packing, generators,
// the exactness bound, messages): ntm/mx_plan.hpp.
//
// C[M x N] (fp32) = A[M x K] * B[N x K]^T; A and B share one format FMT (the
// instruction's cbsz / blgp code), row-major packed (mx_plan.hpp), with scale
// bytes SA[M][K/32] and SB[N][K/32].
//
// mx_gemm_kernel<FMT>: 256 threads (2 x 2 waves of 64 x 64 outputs) per 128 x
// 128 tile, K-step 128 = one v_mfma_scale_f32_16x16x128_f8f6f4 deep. A
// K-step's operand rows go global -> registers (16 B loads) -> LDS, two LDS
// buffers, one barrier per K-step: the loads of step s + 1 are issued before
// the MFMAs of step s and stored after them.
//
// Operand and scale lane maps, measured with the one-instruction probe of
// libntm_experimental.so (profiles/mx/README.md) and pinned by the decode sweep
// (one non-zero per row): the low byte (op_sel 0) of lane l's scale VGPR is the
// scale of row (or column) l & 15, k-block l >> 4, for every format. The 6-
// and 4-bit formats keep that block's 32 consecutive values in lane l. The
// 8-bit formats do not: lane l's registers 0-3 hold k 16 g .. 16 g + 15 and its
// registers 4-7 hold k 64 + 16 g .. 64 + 16 g + 15 (g = l >> 4), so its values
// belong to the blocks g >> 1 and 2 + (g >> 1), whose scales the hardware takes
// from the lanes that own those blocks. Each lane reads its own scale byte from
// SA / SB one K-step ahead. Only the builtin is used, so the compiler
// places the hazard no-ops. LDS rows are padded by 16 B for the 4- and 6-bit
// formats (fewer bank conflicts on the fragment reads); the 8-bit rows are not,
// to stay within 64 KiB of static LDS.
#pragma once

#include "ntm/common.hpp"
#include "ntm/mx_plan.hpp"

namespace ntm {
namespace mx {

typedef int i32x8 __attribute__((ext_vector_type(8)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

constexpr int kThreads = 256;

template <int FMT>
struct Tile {
  static constexpr int kBits = FMT <= kFmtE5M2 ? 8 : FMT == kFmtE2M1 ? 4 : 6;
  static constexpr int kRowBytes = kTile * kBits / 8;          // one K-step of one row: 128 / 96 / 64
  static constexpr int kStride = kRowBytes + (kBits == 8 ? 0 : 16);  // LDS row pitch
  static constexpr int kChunksPerRow = kRowBytes / 16;         // 8 / 6 / 4
  static constexpr int kChunks = kTile * kChunksPerRow / kThreads;  // per thread and operand: 4 / 3 / 2
  static constexpr int kFragBytes = kBlock * kBits / 8;        // a lane's 32 values: 32 / 24 / 16
  static constexpr int kOperandBytes = kTile * kStride;        // one operand, one buffer
};

// Lane group g's 32 values of one row (`row`: its 128 k in LDS) into the
// instruction's 8-VGPR operand (the 6- and 4-bit formats use the low 6 / 4
// registers).
template <int FMT>
__device__ __forceinline__ i32x8 load_frag(const unsigned char* row, int g) {
  i32x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
  const unsigned char* p = row + g * Tile<FMT>::kFragBytes;
  if constexpr (Tile<FMT>::kBits == 8) {  // k 16 g .. + 15 and 64 + 16 g .. + 15
    const u32x4 lo = *(const u32x4*)(row + 16 * g), hi = *(const u32x4*)(row + 64 + 16 * g);
    v[0] = lo[0], v[1] = lo[1], v[2] = lo[2], v[3] = lo[3];
    v[4] = hi[0], v[5] = hi[1], v[6] = hi[2], v[7] = hi[3];
  } else if constexpr (Tile<FMT>::kBits == 6) {  // 24 B at an 8-byte boundary
    const u32x2 x = *(const u32x2*)p, y = *(const u32x2*)(p + 8), z = *(const u32x2*)(p + 16);
    v[0] = x[0], v[1] = x[1], v[2] = y[0], v[3] = y[1], v[4] = z[0], v[5] = z[1];
  } else {
    const u32x4 lo = *(const u32x4*)p;
    v[0] = lo[0], v[1] = lo[1], v[2] = lo[2], v[3] = lo[3];
  }
  return v;
}

template <int FMT>
__global__ void __launch_bounds__(kThreads)
mx_gemm_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ B,
               const unsigned char* __restrict__ SA, const unsigned char* __restrict__ SB,
               float* __restrict__ C, int M, int N, int K) {
  using T = Tile<FMT>;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][2][T::kOperandBytes];
  const int t = threadIdx.x, l = t & 63, w = t >> 6;
  const int wm = w >> 1, wn = w & 1;
  const size_t m0 = (size_t)blockIdx.y * kTile, n0 = (size_t)blockIdx.x * kTile;
  const size_t pitch = (size_t)K * T::kBits / 8;  // bytes per row of A and B
  const int KB = K / kBlock, steps = K / kTile;

  // global -> register staging: chunk c of the tile is 16 B of row c / kChunksPerRow
  u32x4 ga[T::kChunks], gb[T::kChunks];
  auto load_global = [&](int s) {
#pragma unroll
    for (int i = 0; i < T::kChunks; ++i) {
      const int c = t + i * kThreads, row = c / T::kChunksPerRow, col = c % T::kChunksPerRow;
      const size_t off = (size_t)s * T::kRowBytes + (size_t)col * 16;
      ga[i] = *(const u32x4*)(A + (m0 + row) * pitch + off);
      gb[i] = *(const u32x4*)(B + (n0 + row) * pitch + off);
    }
  };
  auto store_lds = [&](int buf) {
#pragma unroll
    for (int i = 0; i < T::kChunks; ++i) {
      const int c = t + i * kThreads, row = c / T::kChunksPerRow, col = c % T::kChunksPerRow;
      *(u32x4*)(&lds[buf][0][row * T::kStride + col * 16]) = ga[i];
      *(u32x4*)(&lds[buf][1][row * T::kStride + col * 16]) = gb[i];
    }
  };
  // this lane's scale bytes of one K-step: rows wm * 64 + 16 mt + (l & 15) of A,
  // columns wn * 64 + 16 nt + (l & 15) of B, k-block 4 s + (l >> 4)
  int sa[4], sb[4], sa_next[4], sb_next[4];
  auto load_scales = [&](int s, int (&a)[4], int (&b)[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = SA[(m0 + wm * 64 + i * 16 + (l & 15)) * KB + s * 4 + (l >> 4)];
      b[i] = SB[(n0 + wn * 64 + i * 16 + (l & 15)) * KB + s * 4 + (l >> 4)];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  load_global(0);
  load_scales(0, sa, sb);
  store_lds(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    const int buf = s & 1;
    if (s + 1 < steps) {
      load_global(s + 1);
      load_scales(s + 1, sa_next, sb_next);
    }
    i32x8 fb[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      fb[nt] = load_frag<FMT>(&lds[buf][1][(wn * 64 + nt * 16 + (l & 15)) * T::kStride], l >> 4);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
      const i32x8 fa =
          load_frag<FMT>(&lds[buf][0][(wm * 64 + mt * 16 + (l & 15)) * T::kStride], l >> 4);
#pragma unroll
      for (int nt = 0; nt < 4; ++nt)
        acc[mt][nt] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fa, fb[nt], acc[mt][nt], FMT, FMT,
                                                                       0, sa[mt], 0, sb[nt]);
    }
    if (s + 1 < steps) {
      // buffer buf ^ 1 was last read in step s - 1, before the barrier that ended it
      store_lds(buf ^ 1);
#pragma unroll
      for (int i = 0; i < 4; ++i) sa[i] = sa_next[i], sb[i] = sb_next[i];
    }
    __syncthreads();
  }

  // C/D layout of the 16x16 shapes: column l & 15, rows 4 (l >> 4) + r
#pragma unroll
  for (int mt = 0; mt < 4; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const size_t row = m0 + wm * 64 + mt * 16 + 4 * (l >> 4) + r;
        const size_t col = n0 + wn * 64 + nt * 16 + (l & 15);
        C[row * (size_t)N + col] = acc[mt][nt][r];
      }
}

// ---- the reference: no matrix core. A 16 x 16 block of threads computes a
// 16 x 16 patch of C, one element per thread. Per k-block the block stages the
// 16 + 16 packed row pieces in LDS (4-byte loads); each thread then extracts
// both codes per k with integer operations, turns each into mantissa x
// 2^exponent, applies both block scales to A's value with ldexpf (exact: the
// scaled value stays far inside fp32's range for the Job's inputs) and adds
// the product in an fp32 FMA chain in k order. Under mx_plan.hpp's bound every
// step is exact.
__device__ __forceinline__ int dev_code(const uint32_t* piece, int k, int bits) {
  const int bit = k * bits, w = bit >> 5, sh = bit & 31;
  uint32_t v = piece[w] >> sh;
  if (sh + bits > 32) v |= piece[w + 1] << (32 - sh);  // only inside the piece: 32 * bits is a word multiple
  return (int)(v & ((1u << bits) - 1));
}
__device__ __forceinline__ float dev_value(int code, int bits, int exp_bits, int man_bits, int bias,
                                           int extra_exp) {
  const int m = code & ((1 << man_bits) - 1);
  const int e = (code >> man_bits) & ((1 << exp_bits) - 1);
  const int mant = e ? (m | (1 << man_bits)) : m;
  const int exp2 = (e ? e : 1) - bias - man_bits;
  const float v = ldexpf((float)mant, exp2 + extra_exp);
  return (code >> (bits - 1)) & 1 ? -v : v;
}

__global__ void __launch_bounds__(256)
mx_ref_kernel(const unsigned char* __restrict__ A, const unsigned char* __restrict__ B,
              const unsigned char* __restrict__ SA, const unsigned char* __restrict__ SB,
              float* __restrict__ C, int M, int N, int K, int bits, int exp_bits, int man_bits,
              int bias) {
  __shared__ uint32_t piece[32][8];  // rows 0-15: A, 16-31: B; bits words of 32 values each
  const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
  const size_t i0 = (size_t)blockIdx.y * 16, j0 = (size_t)blockIdx.x * 16;
  const size_t pitch = (size_t)K * bits / 8;
  const int KB = K / kBlock, words = bits;  // 32 values * bits / 32
  const int lr = t / words, lw = t % words;  // the word this thread stages (t < 32 * words)
  const unsigned char* src = nullptr;
  if (lr < 32) src = (lr < 16 ? A + (i0 + lr) * pitch : B + (j0 + lr - 16) * pitch) + (size_t)lw * 4;
  float acc = 0.f;
  for (int kb = 0; kb < KB; ++kb) {
    if (src) piece[lr][lw] = *(const uint32_t*)(src + (size_t)kb * words * 4);
    __syncthreads();
    const int scale = (int)SA[(i0 + ti) * KB + kb] + (int)SB[(j0 + tj) * KB + kb] - 2 * kScaleBias;
    for (int k = 0; k < kBlock; ++k) {
      const float a = dev_value(dev_code(piece[ti], k, bits), bits, exp_bits, man_bits, bias, scale);
      const float b = dev_value(dev_code(piece[16 + tj], k, bits), bits, exp_bits, man_bits, bias, 0);
      acc = fmaf(a, b, acc);
    }
    __syncthreads();
  }
  C[(i0 + ti) * (size_t)N + j0 + tj] = acc;
}

// ---- the compare: bitwise, 32-bit words. The healthy path executes no atomic
// and no store. mx_compare_finish_kernel (one thread, after it on the stream)
// fills expected / got of the first differing word.
__global__ void __launch_bounds__(256)
mx_compare_kernel(const uint32_t* __restrict__ expected, const uint32_t* __restrict__ got, size_t n,
                  Mismatch* out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (expected[i] == got[i]) continue;
    atomicAdd((unsigned long long*)&out->count, 1ull);
    atomicMin((unsigned long long*)&out->first_index, (unsigned long long)i);
  }
}
__global__ void mx_compare_finish_kernel(const uint32_t* __restrict__ expected,
                                         const uint32_t* __restrict__ got, size_t n, Mismatch* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || out->count == 0 || out->first_index >= n) return;
  out->expected = expected[out->first_index];
  out->got = got[out->first_index];
}

// ---- launchers
inline hipError_t launch_mx_gemm(int fmt, const void* A, const void* B, const void* SA,
                                 const void* SB, float* C, int M, int N, int K, hipStream_t s) {
  if (!format_ok(fmt) || !shape_ok(M, N, K) || !A || !B || !SA || !SB || !C ||
      ((uintptr_t)A % 16) || ((uintptr_t)B % 16) || ((uintptr_t)C % 4))
    return hipErrorInvalidValue;
  const dim3 g((unsigned)(N / kTile), (unsigned)(M / kTile)), b(kThreads);
  auto* a = (const unsigned char*)A;
  auto* bb = (const unsigned char*)B;
  auto* sa = (const unsigned char*)SA;
  auto* sb = (const unsigned char*)SB;
  switch (fmt) {
    case kFmtE4M3: hipLaunchKernelGGL(mx_gemm_kernel<kFmtE4M3>, g, b, 0, s, a, bb, sa, sb, C, M, N, K); break;
    case kFmtE5M2: hipLaunchKernelGGL(mx_gemm_kernel<kFmtE5M2>, g, b, 0, s, a, bb, sa, sb, C, M, N, K); break;
    case kFmtE2M3: hipLaunchKernelGGL(mx_gemm_kernel<kFmtE2M3>, g, b, 0, s, a, bb, sa, sb, C, M, N, K); break;
    case kFmtE3M2: hipLaunchKernelGGL(mx_gemm_kernel<kFmtE3M2>, g, b, 0, s, a, bb, sa, sb, C, M, N, K); break;
    default: hipLaunchKernelGGL(mx_gemm_kernel<kFmtE2M1>, g, b, 0, s, a, bb, sa, sb, C, M, N, K); break;
  }
  return hipGetLastError();
}

inline hipError_t launch_mx_reference(int fmt, const void* A, const void* B, const void* SA,
                                      const void* SB, float* C, int M, int N, int K, hipStream_t s) {
  if (!format_ok(fmt) || !shape_ok(M, N, K) || !A || !B || !SA || !SB || !C ||
      ((uintptr_t)A % 4) || ((uintptr_t)B % 4) || ((uintptr_t)C % 4))
    return hipErrorInvalidValue;
  const Format& f = kFormatTable[fmt];
  hipLaunchKernelGGL(mx_ref_kernel, dim3((unsigned)(N / 16), (unsigned)(M / 16)), dim3(256), 0, s,
                     (const unsigned char*)A, (const unsigned char*)B, (const unsigned char*)SA,
                     (const unsigned char*)SB, C, M, N, K, f.bits, f.exp_bits, f.man_bits, f.bias);
  return hipGetLastError();
}

// `out`: one initialised Mismatch (mismatch_init) in device memory, 8-byte aligned.
inline hipError_t launch_mx_compare(const void* expected, const void* got, size_t n, void* out,
                                    hipStream_t s) {
  if (!expected || !got || !out || ((uintptr_t)expected % 4) || ((uintptr_t)got % 4) ||
      ((uintptr_t)out % 8))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(mx_compare_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s,
                     (const uint32_t*)expected, (const uint32_t*)got, n, (Mismatch*)out);
  hipLaunchKernelGGL(mx_compare_finish_kernel, dim3(1), dim3(1), 0, s, (const uint32_t*)expected,
                     (const uint32_t*)got, n, (Mismatch*)out);
  return hipGetLastError();
}

}  // namespace mx
}  // namespace ntm
