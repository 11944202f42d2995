// K14: paged-KV decode attention ("pda") for gfx950: bf16, head dimension 128, 1 .. 4 new tokens
// per sequence over a KV cache of 16-token pages reached through a block table, the keys cut
// over S workgroups per (sequence, key/value head) (split-KV) and the partials merged afterwards.
// Shapes, the split plan, the arithmetic contract, the LDS budget and the stage depth are in
// ntm/pda_plan.hpp; read the contract there first. The reference and the compare are K13's
// (attn_reference_kernel on the gathered keys, attn_compare_kernel).
//
// pda_split_kernel: grid B * Hkv * S, 4 waves. The G * T rows of one key/value head (padded to
// 32) are the 32-wide side of both MFMAs; Q^T is held in LDS, shared by the waves. Wave w walks the
// key steps w, w + 4, ... of its workgroup's range, alone: nothing is shared until the end, so
// the key loop has no workgroup barrier.
//   K rows go 16 bytes per lane straight from their pages into the registers that are the A
//     operand of S^T = K Q^T (v_mfma_f32_32x32x16_bf16); the block table is read once per step
//     (4 page ids, one load, handed round with v_readlane);
//   the row maximum, v_exp_f32 and the bf16 pack run in K13's register layout;
//   V goes through registers into the wave's own LDS stage and comes back through
//     ds_read_b64_tr_b16 for O^T += V^T P^T.
// Rows at or past len_b, and rows of a page id outside the pool, never reach a register that is
// used: K lanes read Q's first row in their place, V lanes their page's tail (or page 0), and the
// result is replaced by zeros.
// After the loop each wave writes its partial into its own stage, one barrier, and the
// workgroup merges the four in wave order and writes (acc fp32 [32][128], m, l) to the
// workspace, and its HW_ID / XCC_ID to the optional table.
//
// pda_combine_kernel: a second launch on the same stream, grid B * Hkv: merges the S partials
// of each row in split order, divides, packs and writes O, m and l. The kernel boundary is the
// only cross-workgroup ordering: no flags, no atomics, no in-kernel hand-off.
#pragma once

#include <atomic>
#include <cstdint>

#include "ntm/attn.hpp"
#include "ntm/pda_plan.hpp"

namespace ntm {
namespace pda {

using ntm::attn::at_f32x16;
using ntm::attn::at_s16x4;
using ntm::attn::at_s16x8;
using ntm::attn::at_u32x2;
using ntm::attn::at_u32x4;
typedef float pda_f32x4 __attribute__((ext_vector_type(4)));

struct SplitArgs {
  const uint16_t *q, *kpool, *vpool;
  const int32_t *block_table, *seq_lens;
  float* ws;
  uint32_t* table;  // optional: kTableWords per workgroup
  int Hq, Hkv, T, max_pages, pages, S;
  float scale_log2;
};

// alpha of a partial with maximum mp under the merged maximum m: 0 for an empty partial, so
// that -inf - -inf never reaches the exponent
__device__ __forceinline__ float merge_alpha(float scale_log2, float mp, float m) {
  return mp == -__builtin_inff() ? 0.f : __builtin_amdgcn_exp2f(scale_log2 * (mp - m));
}

// Two waves per SIMD asked for: the register budget is then 256, no accumulator lives in an AGPR
// (the MFMAs take their VGPR form) and two workgroups share a CU. The build fits it without
// scratch (profiles/pda/README.md records the compiler's report); Q^T in LDS, K and V never in
// registers together and the mask kept out of full steps are what make it fit.
__global__ void __launch_bounds__(kThreads, 2) pda_split_kernel(SplitArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char pda_lds[];
  const unsigned t = threadIdx.x, lane = t & 63u, c = lane & 31u, hh = lane >> 5;
  const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(t >> 6));  // scalar: the key loop is wave-uniform
  unsigned hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  const unsigned xcc = xcc_id_raw();
  const long long wg = blockIdx.x, bk = wg / a.S, b = bk / a.Hkv;
  const int split = (int)(wg % a.S), hkv = (int)(bk % a.Hkv);
  if (a.table && t == 0) {
    a.table[wg * kTableWords] = hw;
    a.table[wg * kTableWords + 1] = xcc;
  }
  const int G = a.Hq / a.Hkv, rows = G * a.T;
  int len = a.seq_lens[b];
  len = len < 0 ? 0 : len;
  len = len > a.max_pages * kPage ? a.max_pages * kPage : len;  // every key below len has a table entry
  const int32_t* bt = a.block_table + b * a.max_pages;
  const uint16_t* qh = a.q + (b * a.Hq + (long long)hkv * G) * a.T * kHeadDim;  // rows g * T + t are contiguous

  // Q^T as the B operand of the 32x32x16 MFMA: element j of k-step ks is Q[row c][16 ks + 8 hh + j].
  // It is the same for the four waves and is kept in LDS behind the stages, [ks][lane] x 16 bytes,
  // not in 32 registers per lane: each S^T step reads its 8 chunks back (conflict-free b128 reads).
  unsigned char* ql = pda_lds + kWaves * kLdsWaveBytes;
  if (wave == 0) {
#pragma unroll
    for (int ks = 0; ks < 8; ++ks)
      *(at_u32x4*)(ql + (ks * 64 + (int)lane) * 16) = ntm::attn::load_chunk(qh, (long long)c, rows, 16 * ks + 8 * (int)hh);
  }
  __syncthreads();
  // the last key this row sees. A padded row (Q zeros, never stored) sees every key, so that it
  // does not force the mask on full steps.
  const int lim = (int)c < rows ? len - a.T + (int)c % a.T : len - 1;

  unsigned char* vl = pda_lds + wave * kLdsWaveBytes;  // this wave's stage
  int pg[4];                                           // the 4 physical pages of a step, wave-uniform
  at_u32x4 kreg[2][8], vreg[16];
  const at_u32x4 zero4 = {0u, 0u, 0u, 0u};
  auto read_pages = [&](int step) {
    int idx = step * (kKeyStep / kPage) + (int)(lane & 3u);
    idx = idx < a.max_pages ? idx : a.max_pages - 1;  // a page past the table holds no key below len
    const int mine = bt[idx];
#pragma unroll
    for (int j = 0; j < 4; ++j) pg[j] = __builtin_amdgcn_readlane(mine, j);
  };
  // K: row 32 kt + c of the step, 16 bytes at element 16 ks + 8 hh: the A operand as it stands
  auto load_k = [&](int step) {
#pragma unroll
    for (int kt = 0; kt < 2; ++kt) {
      const int key = step * kKeyStep + kt * 32 + (int)c;
      const int page = (c >> 4) ? pg[2 * kt + 1] : pg[2 * kt];
      const bool ok = key < len && (unsigned)page < (unsigned)a.pages;
      // a lane without a row loads Q's first row instead (always there) and drops it: no branch round the loads
      const uint16_t* row =
          ok ? a.kpool + (((long long)page * a.Hkv + hkv) * kPage + (key & (kPage - 1))) * kHeadDim : qh;
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        const at_u32x4 x = *(const at_u32x4*)(row + 16 * ks + 8 * (int)hh);
        kreg[kt][ks] = ok ? x : zero4;
      }
    }
  };
  // V: chunk x = lane + 64 n of a 64 x 16-chunk tile is row x >> 4 = 4 n + (lane >> 4), chunk x & 15:
  // the 4 loads of a page differ by a constant, so a step needs 4 per-lane addresses. A page id
  // outside the pool reads page 0 instead; what a lane reads at or past len_b (a page tail, the
  // poison page) is dropped, never used.
  auto load_v = [&](int step) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool page_ok = (unsigned)pg[j] < (unsigned)a.pages;
      const uint16_t* base = a.vpool + (((long long)(page_ok ? pg[j] : 0) * a.Hkv + hkv) * kPage + (int)(lane >> 4)) * kHeadDim +
                             8 * (int)(lane & 15u);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int n = 4 * j + i, key = step * kKeyStep + 4 * n + (int)(lane >> 4);
        const at_u32x4 x = *(const at_u32x4*)(base + 4 * i * kHeadDim);
        vreg[n] = page_ok && key < len ? x : zero4;
      }
    }
  };

  at_f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.f;
  float m_run = -__builtin_inff(), l_run = 0.f;  // l_run: this lane half's share of the row sum

  const Range range = split_range(len, split, a.S);
  int step = range.begin + (int)wave;
  if (step < range.end) {
    read_pages(step);
    load_k(step);
  }
  for (; step < range.end; step += kWaves) {  // wave-uniform
    // S^T: two 32-key tiles; register r of tile kt is key 32 kt + (r & 3) + 8 (r >> 2) + 4 hh
    at_f32x16 s[2];
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      const bf16x8 bq = *(const bf16x8*)(ql + (ks * 64 + (int)lane) * 16);
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
        s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, kreg[kt][ks]), bq, s[kt], 0, 0, 0);
    }
    const int lim_local = lim - step * kKeyStep;  // may be negative: nothing visible
    __builtin_amdgcn_sched_barrier(0);  // V's loads stay behind the MFMAs that free K's registers
    load_v(step);                       // V of this step is in flight under the softmax
    // the mask, only in a step whose end some row of the wave does not see (the last ones)
    float mt = -__builtin_inff();
    if (__builtin_amdgcn_ballot_w64(lim_local < kKeyStep - 1) != 0) {
#pragma unroll
      for (int kt = 0; kt < 2; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + (r & 3) + 8 * (r >> 2);
          s[kt][r] = key <= lim_local - 4 * (int)hh ? s[kt][r] : -__builtin_inff();
        }
    }
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) mt = __builtin_fmaxf(mt, s[kt][r]);
    mt = __builtin_fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = __builtin_fmaxf(m_run, mt);
    // a row that has seen no key yet subtracts 0, not -inf: alpha and every p come out 0
    const float m_sub = m_new == -__builtin_inff() ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(a.scale_log2 * (m_run - m_sub));
    m_run = m_new;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 2; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        s[kt][r] = __builtin_amdgcn_exp2f(a.scale_log2 * (s[kt][r] - m_sub));
        sum += s[kt][r];
      }
    l_run = l_run * alpha + sum;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;

    // V of this step into the wave's stage; the stage's last reader was this wave, one step ago
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int n = 0; n < 16; ++n)
      *(at_u32x4*)(vl + (4 * n + (int)(lane >> 4)) * kLdsRowBytes + (int)(lane & 15u) * 16) = vreg[n];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_sched_barrier(0);  // K's loads stay behind the stores that free V's registers
    if (step + kWaves < range.end) {    // V is staged: K of the wave's next step is in flight under P V
      read_pages(step + kWaves);
      load_k(step + kWaves);
    }

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
  }

  // the wave's partial into its own stage: row c, registers 4 g .. 4 g + 3 of tile dt are
  // columns dt 32 + 8 g + 4 hh + 0 .. 3
  const float l_row = l_run + __shfl_xor(l_run, 32);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const pda_f32x4 v4 = {oacc[dt][4 * g], oacc[dt][4 * g + 1], oacc[dt][4 * g + 2], oacc[dt][4 * g + 3]};
      *(pda_f32x4*)(vl + (int)c * kMergeRowBytes + (dt * 32 + 8 * g + 4 * (int)hh) * 4) = v4;
    }
  if (hh == 0) {
    float* st = (float*)(vl + kMergeStatsOffset);
    st[c] = m_run;
    st[kRows + c] = l_row;
  }
  __syncthreads();

  // the merge of the four waves, in wave order
  float* out = a.ws + wg * kPartialFloats;
#pragma unroll 4
  for (int n = 0; n < kRows * kHeadDim / kThreads; ++n) {
    const int e = (int)t + kThreads * n, row = e >> 7, col = e & (kHeadDim - 1);
    float mw[kWaves], m = -__builtin_inff();
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      mw[w] = ((const float*)(pda_lds + w * kLdsWaveBytes + kMergeStatsOffset))[row];
      m = __builtin_fmaxf(m, mw[w]);
    }
    float acc = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const float part = *(const float*)(pda_lds + w * kLdsWaveBytes + row * kMergeRowBytes + col * 4);
      acc = __fadd_rn(acc, __fmul_rn(merge_alpha(a.scale_log2, mw[w], m), part));
    }
    out[e] = acc;
  }
  if (t < (unsigned)kRows) {
    float mw[kWaves], m = -__builtin_inff(), l = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      mw[w] = ((const float*)(pda_lds + w * kLdsWaveBytes + kMergeStatsOffset))[t];
      m = __builtin_fmaxf(m, mw[w]);
    }
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
      const float part = ((const float*)(pda_lds + w * kLdsWaveBytes + kMergeStatsOffset))[kRows + t];
      l = __fadd_rn(l, __fmul_rn(merge_alpha(a.scale_log2, mw[w], m), part));
    }
    out[kRows * kHeadDim + t] = m;
    out[kRows * kHeadDim + kRows + t] = l;
  }
}

struct CombineArgs {
  const float* ws;
  uint16_t* o;
  float *m, *l;  // optional
  int Hq, Hkv, T, S;
  float scale_log2;
};

// One workgroup per (sequence, key/value head); a thread owns two neighbouring columns of a row.
__global__ void __launch_bounds__(kThreads) pda_combine_kernel(CombineArgs a) {
  const long long bk = blockIdx.x, b = bk / a.Hkv;
  const int hkv = (int)(bk % a.Hkv), G = a.Hq / a.Hkv, rows = G * a.T;
  const float* base = a.ws + bk * a.S * kPartialFloats;
  const long long row0 = (b * a.Hq + (long long)hkv * G) * a.T;
  for (int n = 0; n < kRows * kHeadDim / 2 / kThreads; ++n) {
    const int p = (int)threadIdx.x + kThreads * n, row = p >> 6, col = 2 * (p & 63);
    if (row >= rows) continue;
    float m = -__builtin_inff();
    for (int s = 0; s < a.S; ++s) m = __builtin_fmaxf(m, base[(long long)s * kPartialFloats + kRows * kHeadDim + row]);
    float l = 0.f, acc0 = 0.f, acc1 = 0.f;
    for (int s = 0; s < a.S; ++s) {
      const float* part = base + (long long)s * kPartialFloats;
      const float alpha = merge_alpha(a.scale_log2, part[kRows * kHeadDim + row], m);
      l = __fadd_rn(l, __fmul_rn(alpha, part[kRows * kHeadDim + kRows + row]));
      acc0 = __fadd_rn(acc0, __fmul_rn(alpha, part[row * kHeadDim + col]));
      acc1 = __fadd_rn(acc1, __fmul_rn(alpha, part[row * kHeadDim + col + 1]));
    }
    const uint32_t b0 = f32_to_bf16_bits(__fdiv_rn(acc0, l)), b1 = f32_to_bf16_bits(__fdiv_rn(acc1, l));
    *(uint32_t*)(a.o + (row0 + row) * kHeadDim + col) = b0 | b1 << 16;
    if (col == 0) {
      if (a.m) a.m[row0 + row] = m;
      if (a.l) a.l[row0 + row] = l;
    }
  }
}

inline hipError_t launch_pda_fwd(const void* Q, const void* Kpool, const void* Vpool, const int* block_table,
                                 const int* seq_lens, void* O, float* m, float* l, void* workspace, unsigned* table,
                                 int B, int Hq, int Hkv, int T, int max_pages, int pages, int splits, float scale_log2,
                                 hipStream_t s) {
  using ntm::attn::aligned16;
  if (!Q || !Kpool || !Vpool || !block_table || !seq_lens || !O || !workspace || !aligned16(Q) || !aligned16(Kpool) ||
      !aligned16(Vpool) || !aligned16(O) || !aligned16(workspace) || !shape_ok(B, Hq, Hkv, T, max_pages, pages, splits) ||
      !(scale_log2 > 0.f) || ((uintptr_t)block_table % 4) || ((uintptr_t)seq_lens % 4) || ((uintptr_t)m % 4) ||
      ((uintptr_t)l % 4) || ((uintptr_t)table % 4))
    return hipErrorInvalidValue;
  // more than 64 KiB of dynamic LDS needs the attribute: set once per device (bit = device index)
  static std::atomic<unsigned long long> lds_set{0};
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = 1ull << (dev & 63);
  if (!(lds_set.load(std::memory_order_acquire) & bit)) {
    e = hipFuncSetAttribute((const void*)pda_split_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes);
    if (e != hipSuccess) return e;
    lds_set.fetch_or(bit, std::memory_order_release);
  }
  SplitArgs sa{(const uint16_t*)Q, (const uint16_t*)Kpool, (const uint16_t*)Vpool, block_table, seq_lens,
               (float*)workspace, table, Hq, Hkv, T, max_pages, pages, splits, scale_log2};
  hipLaunchKernelGGL(pda_split_kernel, dim3((unsigned)grid(B, Hkv, splits)), dim3(kThreads), kLdsBytes, s, sa);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  CombineArgs ca{(const float*)workspace, (uint16_t*)O, m, l, Hq, Hkv, T, splits, scale_log2};
  hipLaunchKernelGGL(pda_combine_kernel, dim3((unsigned)(B * Hkv)), dim3(kThreads), 0, s, ca);
  return hipGetLastError();
}

}  // namespace pda
}  // namespace ntm
