// K13: fused attention forward for gfx950 (bf16, head dimension 128, grouped-query, causal
// or not) and its reference kernel. Shapes, the arithmetic contract, the LDS budget and the
// exact-input machinery are in ntm/attn_plan.hpp; read the contract there first.
//
// attn_fwd_kernel: one workgroup of 4 waves per 128 query rows of one (batch, head); wave w
// owns rows 32 w .. 32 w + 31 and walks the keys in steps of 64. K and V of a step are staged
// through registers into LDS, double-buffered: the loads of step t + 1 are issued before the
// MFMAs of step t and written to the other buffer after them, one barrier per step.
//   S^T = K Q^T  on v_mfma_f32_32x32x16_bf16 (A = K rows from LDS, B = Q^T, held in registers
//         for the whole kernel): a lane holds 2 x 16 scores of ONE query (lane & 31), so the
//         row maximum and sum are register loops and one exchange with lane ^ 32;
//   O^T += V^T P^T: the S^T accumulator, exponentiated and packed to bf16, is the B operand
//         as it stands (the accumulator-as-operand idiom: registers 8 s .. 8 s + 7 are k-step
//         s, element j being key 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3)), and V^T in that
//         same key order comes from two ds_read_b64_tr_b16 of the row-major V stage.
// alpha, m and l live once per lane; O^T keeps the query on the lane, so the rescale is a
// per-lane multiply. Ragged query and key tiles are masked here: rows past Sk are staged as
// zeros and scored -inf, rows past Sq are computed and not stored.
//
// attn_reference_kernel: one thread per output row and column, plain fp32 loops in index
// order, two passes (row maximum, then p, l and sum bf16(p) v), no matrix and no cross-lane
// instruction; integer-valued exponents get their power of two from exponent bits.
#pragma once

#include <atomic>
#include <cstdint>

#include "ntm/attn_plan.hpp"
#include "ntm/common.hpp"
#include "ntm/mx_plan.hpp"  // Mismatch: the record of the bitwise compare (host-only header)

namespace ntm {
namespace attn {

typedef float at_f32x16 __attribute__((ext_vector_type(16)));
typedef short at_s16x4 __attribute__((ext_vector_type(4)));
typedef short at_s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned at_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned at_u32x2 __attribute__((ext_vector_type(2)));
#define NTM_ATTN_LDS(T) __attribute__((address_space(3))) T*

struct FwdArgs {
  const uint16_t *q, *k, *v;
  uint16_t* o;
  float *m, *l;     // optional
  uint32_t* table;  // optional: kTableWords per workgroup
  int Hq, Hkv, Sq, Sk, causal, qtiles;
  float scale_log2;
};

// 16 bytes (8 bf16) of row `row` of a [rows][128] bf16 matrix at element offset `col`, or zeros
__device__ __forceinline__ at_u32x4 load_chunk(const uint16_t* base, long long row, long long rows, int col) {
  at_u32x4 z = {0u, 0u, 0u, 0u};
  if (row < rows) z = *(const at_u32x4*)(base + row * kHeadDim + col);
  return z;
}

__global__ void __launch_bounds__(kThreads) attn_fwd_kernel(FwdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char attn_lds[];
  const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, c = lane & 31u, hh = lane >> 5;
  unsigned hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  const unsigned xcc = xcc_id_raw();
  const long long wg = blockIdx.x, qt = wg % a.qtiles, bh = wg / a.qtiles;
  const long long head = bh % a.Hq, batch = bh / a.Hq;
  if (a.table && t == 0) {
    a.table[wg * kTableWords] = hw;
    a.table[wg * kTableWords + 1] = xcc;
  }
  const long long i = qt * kQTile + wave * 32 + c;  // this lane's query row
  const uint16_t* qh = a.q + bh * a.Sq * kHeadDim;
  const long long kvh = batch * a.Hkv + head / (a.Hq / a.Hkv);
  const uint16_t* kh = a.k + kvh * a.Sk * kHeadDim;
  const uint16_t* vh = a.v + kvh * a.Sk * kHeadDim;

  // Q^T as the B operand of the 32x32x16 MFMA: element j of k-step ks is Q[i][16 ks + 8 hh + j]
  bf16x8 bq[8];
#pragma unroll
  for (int ks = 0; ks < 8; ++ks)
    bq[ks] = __builtin_bit_cast(bf16x8, load_chunk(qh, i, a.Sq, 16 * ks + 8 * (int)hh));

  // the last key this row sees
  long long lim = (long long)a.Sk - 1;
  if (a.causal && i + a.Sk - a.Sq < lim) lim = i + a.Sk - a.Sq;

  // staging: chunk x = t + 256 n of a 64 x 16-chunk tile is row x >> 4, chunk x & 15
  at_u32x4 kreg[4], vreg[4];
  auto load_step = [&](int step) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int x = (int)t + kThreads * n;
      const long long row = (long long)step * kKeyStep + (x >> 4);
      kreg[n] = load_chunk(kh, row, a.Sk, (x & 15) * 8);
      vreg[n] = load_chunk(vh, row, a.Sk, (x & 15) * 8);
    }
  };
  auto store_step = [&](int buf) {
    unsigned char* kl = attn_lds + buf * kLdsStageBytes;
    unsigned char* vl = kl + kKeyStep * kLdsRowBytes;
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      const int x = (int)t + kThreads * n, off = (x >> 4) * kLdsRowBytes + (x & 15) * 16;
      *(at_u32x4*)(kl + off) = kreg[n];
      *(at_u32x4*)(vl + off) = vreg[n];
    }
  };

  at_f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
  float m_run = -__builtin_inff(), l_run = 0.f;  // l_run: this lane half's share of the row sum

  const int steps = key_steps(qt, a.Sq, a.Sk, a.causal);
  load_step(0);
  store_step(0);
  __syncthreads();
  for (int step = 0; step < steps; ++step) {
    const bool more = step + 1 < steps;  // workgroup-uniform
    if (more) load_step(step + 1);
    const unsigned char* kl = attn_lds + (step & 1) * kLdsStageBytes;
    const unsigned char* vl = kl + kKeyStep * kLdsRowBytes;

    // S^T: two 32-key tiles; register r of tile kt is key 32 kt + (r & 3) + 8 (r >> 2) + 4 hh
    at_f32x16 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const bf16x8 ka = *(const bf16x8*)(kl + (kt * 32 + (int)c) * kLdsRowBytes + (16 * ks + 8 * (int)hh) * 2);
        s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ka, bq[ks], s[kt], 0, 0, 0);
      }
    }
    const int lim_local = (int)(lim - (long long)step * kKeyStep);  // may be negative: nothing visible
    float mt = -__builtin_inff();
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * (int)hh;
        s[kt][r] = key <= lim_local ? s[kt][r] : -__builtin_inff();
        mt = __builtin_fmaxf(mt, s[kt][r]);
      }
    mt = __builtin_fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = __builtin_fmaxf(m_run, mt);  // finite from step 0 on: key 0 is visible to every row
    const float alpha = __builtin_amdgcn_exp2f(a.scale_log2 * (m_run - m_new));
    m_run = m_new;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[kt][r] = __builtin_amdgcn_exp2f(a.scale_log2 * (s[kt][r] - m_new));
        sum += s[kt][r];
      }
    l_run = l_run * alpha + sum;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;

    // O^T += V^T P^T. All 64 lanes are active here: the transposed reads need that.
    const unsigned q4 = (lane & 15u) >> 2, p4 = lane & 3u, g1 = (lane >> 4) & 1u;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int ss = 0; ss < 2; ++ss) {
        bf16x8 pb;
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[j] = (__bf16)s[kt][8 * ss + j];  // v_cvt_pk_bf16_f32: nearest even
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const unsigned char* p0 = vl + (kt * 32 + 16 * ss + 4 * (int)hh + (int)q4) * kLdsRowBytes +
                                    (dt * 32 + 16 * (int)g1 + 4 * (int)p4) * 2;
          const at_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((NTM_ATTN_LDS(at_s16x4))p0);
          const at_s16x4 hi =
              __builtin_amdgcn_ds_read_tr16_b64_v4i16((NTM_ATTN_LDS(at_s16x4))(p0 + 8 * kLdsRowBytes));
          const at_s16x8 va = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, va), pb, oacc[dt], 0, 0, 0);
        }
      }
    if (more) store_step((step + 1) & 1);
    __syncthreads();
  }

  const float l_row = l_run + __shfl_xor(l_run, 32);
  if (i < a.Sq) {
    uint16_t* orow = a.o + (bh * a.Sq + i) * kHeadDim;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {  // registers 4 g .. 4 g + 3: columns dt 32 + 8 g + 4 hh + 0 .. 3
        uint32_t w[2];
#pragma unroll
        for (int e = 0; e < 2; ++e) {
          const uint32_t b0 = f32_to_bf16_bits(__fdiv_rn(oacc[dt][4 * g + 2 * e], l_row));
          const uint32_t b1 = f32_to_bf16_bits(__fdiv_rn(oacc[dt][4 * g + 2 * e + 1], l_row));
          w[e] = b0 | b1 << 16;
        }
        at_u32x2 pk = {w[0], w[1]};
        *(at_u32x2*)(orow + dt * 32 + 8 * g + 4 * (int)hh) = pk;
      }
    if (hh == 0) {
      if (a.m) a.m[bh * a.Sq + i] = m_run;
      if (a.l) a.l[bh * a.Sq + i] = l_row;
    }
  }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p % 16) == 0; }

inline hipError_t launch_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* m, float* l,
                                  unsigned* table, int B, int Hq, int Hkv, int Sq, int Sk, int causal,
                                  float scale_log2, hipStream_t s) {
  if (!Q || !K || !V || !O || !aligned16(Q) || !aligned16(K) || !aligned16(V) || !aligned16(O) ||
      !shape_ok(B, Hq, Hkv, Sq, Sk, causal) || !(scale_log2 > 0.f) || ((uintptr_t)m % 4) || ((uintptr_t)l % 4) ||
      ((uintptr_t)table % 4))
    return hipErrorInvalidValue;
  // more than 64 KiB of dynamic LDS needs the attribute: set once per device (bit = device index)
  static std::atomic<unsigned long long> lds_set{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(lds_set.load(std::memory_order_acquire) & bit)) {
    e = hipFuncSetAttribute((const void*)attn_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e != hipSuccess) return e;
    lds_set.fetch_or(bit, std::memory_order_release);
  }
  FwdArgs a{(const uint16_t*)Q, (const uint16_t*)K, (const uint16_t*)V, (uint16_t*)O, m, l, table,
            Hq, Hkv, Sq, Sk, causal ? 1 : 0, (int)query_tiles(Sq), scale_log2};
  hipLaunchKernelGGL(attn_fwd_kernel, dim3((unsigned)grid(B, Hq, Sq)), dim3(kThreads), kLdsBytes, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ reference
struct RefArgs {
  const uint16_t *q, *k, *v;
  uint16_t* o;                 // optional bf16 result
  float *o32, *absum, *m, *l;  // optional: fp32 result before the pack, sum p |v| / l, row maximum, row sum
  long long rows;              // B * Hq * Sq
  int Hq, Hkv, Sq, Sk, causal;
  float scale_log2;
};

// 2^x: from exponent bits where x is an integer (0 below -149, a denormal down to it), else exp2f
__device__ inline float ref_exp2(float x) {
  if (x < -149.f) return 0.f;
  if (x <= 0.f && x == __builtin_truncf(x)) {
    const int n = (int)x;
    const uint32_t bits = n >= -126 ? (uint32_t)(n + 127) << 23 : 1u << (n + 149);
    float f;
    __builtin_memcpy(&f, &bits, 4);
    return f;
  }
  return exp2f(x);
}

__device__ inline float ref_score(const uint16_t* q, const uint16_t* k) {
  float s = 0.f;
  for (int d = 0; d < kHeadDim; ++d) s = __builtin_fmaf(bf16_bits_to_f32(q[d]), bf16_bits_to_f32(k[d]), s);
  return s;
}

__global__ void __launch_bounds__(kHeadDim) attn_reference_kernel(RefArgs a) {
  const int d = (int)threadIdx.x;
  for (long long row = blockIdx.x; row < a.rows; row += gridDim.x) {
    const long long i = row % a.Sq, bh = row / a.Sq, head = bh % a.Hq, batch = bh / a.Hq;
    const long long kvh = batch * a.Hkv + head / (a.Hq / a.Hkv);
    const uint16_t* q = a.q + row * kHeadDim;
    const uint16_t* kh = a.k + kvh * a.Sk * kHeadDim;
    const uint16_t* vh = a.v + kvh * a.Sk * kHeadDim;
    const long long n = visible_keys(i, a.Sq, a.Sk, a.causal);
    float top = -__builtin_inff();
    for (long long j = 0; j < n; ++j) top = __builtin_fmaxf(top, ref_score(q, kh + j * kHeadDim));
    float l = 0.f, acc = 0.f, ab = 0.f;
    for (long long j = 0; j < n; ++j) {
      const float p = ref_exp2(a.scale_log2 * (ref_score(q, kh + j * kHeadDim) - top));
      const float v = bf16_bits_to_f32(vh[j * kHeadDim + d]);
      l += p;
      acc = __builtin_fmaf(bf16_bits_to_f32(f32_to_bf16_bits(p)), v, acc);
      ab = __builtin_fmaf(p, __builtin_fabsf(v), ab);
    }
    const float o = __fdiv_rn(acc, l);
    if (a.o) a.o[row * kHeadDim + d] = f32_to_bf16_bits(o);
    if (a.o32) a.o32[row * kHeadDim + d] = o;
    if (a.absum) a.absum[row * kHeadDim + d] = __fdiv_rn(ab, l);
    if (d == 0) {
      if (a.m) a.m[row] = top;
      if (a.l) a.l[row] = l;
    }
  }
}

inline hipError_t launch_attn_reference(const void* Q, const void* K, const void* V, void* O, float* O32,
                                        float* absum, float* m, float* l, int B, int Hq, int Hkv, int Sq, int Sk,
                                        int causal, float scale_log2, hipStream_t s) {
  if (!Q || !K || !V || !shape_ok(B, Hq, Hkv, Sq, Sk, causal) || !(scale_log2 > 0.f) || ((uintptr_t)Q % 2) ||
      ((uintptr_t)K % 2) || ((uintptr_t)V % 2) || ((uintptr_t)O % 2) || ((uintptr_t)O32 % 4) ||
      ((uintptr_t)absum % 4) || ((uintptr_t)m % 4) || ((uintptr_t)l % 4))
    return hipErrorInvalidValue;
  const long long rows = (long long)B * Hq * Sq;
  RefArgs a{(const uint16_t*)Q, (const uint16_t*)K, (const uint16_t*)V, (uint16_t*)O, O32, absum, m, l,
            rows, Hq, Hkv, Sq, Sk, causal ? 1 : 0, scale_log2};
  const long long blocks = rows < (1ll << 20) ? rows : (1ll << 20);
  hipLaunchKernelGGL(attn_reference_kernel, dim3((unsigned)blocks), dim3(kHeadDim), 0, s, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------ compare
// Counts the 4-byte words that differ into a K7 mismatch record (mx_plan.hpp Mismatch: count,
// smallest index, then the words there). `out`: one initialised record, 8-byte aligned.
__global__ void __launch_bounds__(256)
attn_compare_kernel(const uint32_t* __restrict__ expected, const uint32_t* __restrict__ got, size_t n,
                    ntm::mx::Mismatch* out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    if (expected[i] == got[i]) continue;
    atomicAdd((unsigned long long*)&out->count, 1ull);
    atomicMin((unsigned long long*)&out->first_index, (unsigned long long)i);
  }
}
__global__ void attn_compare_finish_kernel(const uint32_t* __restrict__ expected, const uint32_t* __restrict__ got,
                                           size_t n, ntm::mx::Mismatch* out) {
  if (threadIdx.x != 0 || blockIdx.x != 0 || out->count == 0 || out->first_index >= n) return;
  out->expected = expected[out->first_index];
  out->got = got[out->first_index];
}
inline hipError_t launch_attn_compare(const void* expected, const void* got, size_t n, void* out, hipStream_t s) {
  if (!expected || !got || !out || ((uintptr_t)expected % 4) || ((uintptr_t)got % 4) || ((uintptr_t)out % 8))
    return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(attn_compare_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s,
                     (const uint32_t*)expected, (const uint32_t*)got, n, (ntm::mx::Mismatch*)out);
  hipLaunchKernelGGL(attn_compare_finish_kernel, dim3(1), dim3(1), 0, s, (const uint32_t*)expected,
                     (const uint32_t*)got, n, (ntm::mx::Mismatch*)out);
  return hipGetLastError();
}

}  // namespace attn
}  // namespace ntm
