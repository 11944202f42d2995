// K13 (fused attention forward) host side: shapes, the grid and LDS budget of
// ntm_attn_fwd, the flop count, the exact-input predicate and generator, the tolerance of
// the dense sub-test and the failure message. Pure C++ - no HIP - so the Job, the kernels'
// header (ntm/attn.hpp) and a CPU-only test program share it. ops/attn.py mirrors it in numpy.
//
// Q [B][Hq][Sq][128], K and V [B][Hkv][Sk][128], O [B][Hq][Sq][128], all contiguous bf16;
// m and l [B][Hq][Sq] fp32. Query head h reads key/value head h / (Hq / Hkv). causal is
// bottom-right aligned: key j is visible to query i iff j <= i + Sk - Sq, and needs Sk >= Sq.
//
// The arithmetic contract of ntm_attn_fwd (what makes an exact test possible):
//   s     = q . k, accumulated in fp32 on v_mfma_f32_32x32x16_bf16;
//   p     = exp2(scale_log2 * (s - m_run)) on v_exp_f32, m_run the running maximum of the raw s;
//   l     = the sum of the fp32 p;
//   p is rounded to bf16 (nearest even) before the second MFMA, which accumulates in fp32;
//   alpha = exp2(scale_log2 * (m_old - m_new)) rescales l and the accumulator at each key step;
//   O     = one correctly rounded fp32 division acc / l, then a nearest-even pack to bf16.
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "ntm/cu_sweep_plan.hpp"  // NTM_HD, h32, the HW_ID decode

namespace ntm {
namespace attn {

constexpr int kHeadDim = 128;
constexpr int kQTile = 128;    // query rows per workgroup: 4 waves of 32
constexpr int kKeyStep = 64;   // keys per LDS stage
constexpr int kThreads = 256, kWaves = 4;
constexpr int kMaxSk = 65536;
constexpr int kMaxLaunches = 8;  // cap of the Job's CU-coverage loop
// One LDS row of K or V: 128 bf16 and 16 bytes of padding, so that neither the 16-byte row
// reads of K nor the transposed 8-byte reads of V start on one bank in every lane.
constexpr int kLdsRowBytes = kHeadDim * 2 + 16;
constexpr int kLdsStageBytes = 2 * kKeyStep * kLdsRowBytes;  // K and V of one key step
constexpr int kLdsBytes = 2 * kLdsStageBytes;                // double-buffered
static_assert(kLdsBytes <= 160 * 1024, "ntm_attn_fwd must fit the 160 KiB of LDS of a gfx950 CU");
static_assert(kLdsRowBytes % 16 == 0, "rows are written with 16-byte stores");
constexpr int kTableWords = 2;  // per workgroup: raw HW_REG_HW_ID, raw HW_REG_XCC_ID of wave 0

inline bool shape_ok(long long B, long long Hq, long long Hkv, long long Sq, long long Sk, int causal) {
  if (B < 1 || Hq < 1 || Hkv < 1 || Sq < 1 || Sk < 1 || Sk > kMaxSk || Hq % Hkv) return false;
  if (causal && Sk < Sq) return false;
  const long long tiles = (Sq + kQTile - 1) / kQTile;
  // the grid is one-dimensional, and every element index fits 63 bits with room to spare
  return B <= (1ll << 20) && Hq <= (1ll << 16) && Sq <= (1ll << 32) && B * Hq <= (1ll << 31) / tiles;
}
inline long long query_tiles(long long Sq) { return (Sq + kQTile - 1) / kQTile; }
inline long long grid(long long B, long long Hq, long long Sq) { return B * Hq * query_tiles(Sq); }
// Key steps the workgroup of query tile `qt` walks: all of them, or with causal those that
// hold a key visible to the tile's last row.
NTM_HD inline int key_steps(long long qt, long long Sq, int Sk, int causal) {
  const int all = (Sk + kKeyStep - 1) / kKeyStep;
  if (!causal) return all;
  long long last = (qt + 1) * kQTile;
  if (last > Sq) last = Sq;
  const long long jmax = last - 1 + Sk - Sq;  // >= 0: Sk >= Sq
  const long long n = jmax / kKeyStep + 1;
  return n < all ? (int)n : all;
}
// keys visible to query row i
NTM_HD inline long long visible_keys(long long i, long long Sq, long long Sk, int causal) {
  if (!causal) return Sk;
  const long long n = i + Sk - Sq + 1;
  return n < Sk ? n : Sk;
}
// 4 * B * Hq * Sq * Sk * 128, restricted to the visible (query, key) pairs when causal
inline double flops(long long B, long long Hq, long long Sq, long long Sk, int causal) {
  double pairs = (double)Sq * (double)Sk;
  // rows see Sk - Sq + 1 .. Sk keys: an arithmetic series
  if (causal) pairs = (double)Sq * ((double)(Sk - Sq + 1) + (double)Sk) / 2.0;
  return 4.0 * (double)B * (double)Hq * pairs * kHeadDim;
}
inline float default_scale_log2() { return 1.4426950408889634f / 11.313708498984761f; }  // log2(e) / sqrt(128)

// ---- exact inputs. Q and K hold integers, so every s is an integer; with scale_log2 = 1
// every visible score of a row is either within kExactR of the row maximum ("near") or at
// least kExactGap below it ("far"), and the far ones lie within kExactR of each other. V holds
// integers of magnitude at most 4 and Sk <= 4096. Then p and alpha are powers of two
// 2^0 .. 2^-R or exactly 0 (2^-200 and below is 0 in fp32), l and every partial sum of P V
// stay below 2^14 with granularity 2^-R: 24 bits, exact in fp32 in every summation order.
constexpr int kExactR = 10, kExactGap = 200, kExactMaxV = 4, kExactMaxSk = 4096;
constexpr int kExactMaxOperand = 256;  // integers up to 2^8 are bf16 values

// q [B][Hq][Sq][128], k and v [B][Hkv][Sk][128] as integers. Integer arithmetic only.
inline bool attn_exact(const int32_t* q, const int32_t* k, const int32_t* v, long long B, long long Hq,
                       long long Hkv, long long Sq, long long Sk, int causal) {
  if (!q || !k || !v || !shape_ok(B, Hq, Hkv, Sq, Sk, causal) || Sk > kExactMaxSk) return false;
  const size_t nq = (size_t)(B * Hq * Sq) * kHeadDim, nk = (size_t)(B * Hkv * Sk) * kHeadDim;
  for (size_t x = 0; x < nq; ++x)
    if (std::abs(q[x]) > kExactMaxOperand) return false;
  for (size_t x = 0; x < nk; ++x)
    if (std::abs(k[x]) > kExactMaxOperand || std::abs(v[x]) > kExactMaxV) return false;
  const long long group = Hq / Hkv;
  std::vector<int64_t> s((size_t)Sk);
  for (long long b = 0; b < B; ++b)
    for (long long h = 0; h < Hq; ++h) {
      const int32_t* kh = k + (size_t)((b * Hkv + h / group) * Sk) * kHeadDim;
      for (long long i = 0; i < Sq; ++i) {
        const int32_t* qi = q + (size_t)((b * Hq + h) * Sq + i) * kHeadDim;
        const long long n = visible_keys(i, Sq, Sk, causal);
        int64_t top = INT64_MIN;
        for (long long j = 0; j < n; ++j) {
          int64_t acc = 0;
          for (int d = 0; d < kHeadDim; ++d) acc += (int64_t)qi[d] * kh[(size_t)j * kHeadDim + d];
          if (acc >= (1 << 24) || acc <= -(1 << 24)) return false;
          s[(size_t)j] = acc;
          if (acc > top) top = acc;
        }
        int64_t far_lo = INT64_MAX, far_hi = INT64_MIN;
        for (long long j = 0; j < n; ++j) {
          const int64_t below = top - s[(size_t)j];
          if (below <= kExactR) continue;
          if (below < kExactGap) return false;
          if (s[(size_t)j] < far_lo) far_lo = s[(size_t)j];
          if (s[(size_t)j] > far_hi) far_hi = s[(size_t)j];
        }
        if (far_hi > far_lo && far_hi - far_lo > kExactR) return false;
      }
    }
  return true;
}

// The generator. Dimension kGapDim carries the near / far split (q = 10; k = 21 for a near
// key, 0 for a far one: 210 apart), the ten dimensions 3 + 12 u carry one bit each in q and
// in k (a sum of 0 .. 10), and every other dimension holds a value of -3 .. 3 in q and one
// per (batch, kv head, dimension) in k that all keys share: it moves the row's scores
// together. A quarter of the keys are near.
constexpr int kGapDim = 5, kGapQ = 10, kGapK = 21, kBitDims = 10;
constexpr uint32_t kStreamQ = 1, kStreamK = 2, kStreamV = 3, kStreamNear = 4, kStreamW = 5;
NTM_HD inline uint32_t attn_hash(uint32_t seed, uint32_t stream, uint32_t idx) {
  return ntm::cus::h32(ntm::cus::h32(seed ^ (stream * 0x9E3779B9u)) + idx);
}
NTM_HD inline bool bit_dim(int d) { return d >= 3 && (d - 3) % 12 == 0 && (d - 3) / 12 < kBitDims; }
NTM_HD inline int small7(uint32_t h) { return (int)((h >> 8) % 7u) - 3; }  // -3 .. 3
inline int exact_q(uint32_t seed, uint32_t row, int d) {  // row: flat (b, h, i)
  if (d == kGapDim) return kGapQ;
  const uint32_t h = attn_hash(seed, kStreamQ, row * (uint32_t)kHeadDim + (uint32_t)d);
  return bit_dim(d) ? (int)((h >> 8) & 1u) : small7(h);
}
inline int exact_k(uint32_t seed, uint32_t head, uint32_t row, int d) {  // head: flat (b, hkv); row: flat (b, hkv, j)
  if (d == kGapDim) return (attn_hash(seed, kStreamNear, row) >> 8) % 4u == 0 ? kGapK : 0;
  if (bit_dim(d)) return (int)((attn_hash(seed, kStreamK, row * (uint32_t)kHeadDim + (uint32_t)d) >> 8) & 1u);
  return small7(attn_hash(seed, kStreamW, head * (uint32_t)kHeadDim + (uint32_t)d));
}
inline int exact_v(uint32_t seed, uint32_t row, int d) {
  return (int)((attn_hash(seed, kStreamV, row * (uint32_t)kHeadDim + (uint32_t)d) >> 8) % 9u) - 4;  // -4 .. 4
}
struct Inputs {
  long long B = 0, Hq = 0, Hkv = 0, Sq = 0, Sk = 0;
  std::vector<int32_t> q, k, v;      // the integers
  std::vector<uint16_t> qb, kb, vb;  // their bf16 bits
};
// the bf16 bits of an integer of magnitude <= 256 (exact)
inline uint16_t bf16_of_int(int v) {
  if (v == 0) return 0;
  const uint16_t sign = v < 0 ? 0x8000u : 0;
  unsigned a = (unsigned)(v < 0 ? -v : v);
  int e = 0;
  while ((a >> (e + 1)) != 0) ++e;  // a in [2^e, 2^(e+1)), e <= 8
  const unsigned man7 = e <= 7 ? (a << (7 - e)) & 0x7Fu : (a >> (e - 7)) & 0x7Fu;
  return (uint16_t)(sign | (uint16_t)((e + 127) << 7) | (uint16_t)man7);
}
inline Inputs make_exact(long long B, long long Hq, long long Hkv, long long Sq, long long Sk, uint32_t seed) {
  Inputs in;
  in.B = B, in.Hq = Hq, in.Hkv = Hkv, in.Sq = Sq, in.Sk = Sk;
  const size_t qrows = (size_t)(B * Hq * Sq), krows = (size_t)(B * Hkv * Sk);
  in.q.resize(qrows * kHeadDim), in.k.resize(krows * kHeadDim), in.v.resize(krows * kHeadDim);
  for (size_t r = 0; r < qrows; ++r)
    for (int d = 0; d < kHeadDim; ++d) in.q[r * kHeadDim + d] = exact_q(seed, (uint32_t)r, d);
  for (size_t r = 0; r < krows; ++r)
    for (int d = 0; d < kHeadDim; ++d) {
      in.k[r * kHeadDim + d] = exact_k(seed, (uint32_t)(r / (size_t)Sk), (uint32_t)r, d);
      in.v[r * kHeadDim + d] = exact_v(seed, (uint32_t)r, d);
    }
  auto bits = [](const std::vector<int32_t>& x) {
    std::vector<uint16_t> o(x.size());
    for (size_t i = 0; i < x.size(); ++i) o[i] = bf16_of_int(x[i]);
    return o;
  };
  in.qb = bits(in.q), in.kb = bits(in.k), in.vb = bits(in.v);
  return in;
}

// ---- the dense sub-test: |O - reference fp32 O| <= 2^-7 a + 2^-20 per element, with
// a = sum p |v| / l from the reference kernel (derivation: profiles/attn/README.md).
NTM_HD inline float tolerance(float a) { return 0.0078125f * a + 9.5367431640625e-07f; }

// ---- failure lines: one line under 200 characters.
// "gpu3: attn exact causal O: batch 0 head 1 row 5 col 6: xcd 2 se 1 sh 0 cu 3: expected
//  0x3f803f80, got 0x3f803f81, bad bits 0x00000001; 1 differ". `what` is "O" (a word is two
// bf16 elements, col the first), "m" or "l" (no col); `word` the flat index of the 4-byte word.
inline std::string hex32(uint32_t v) {
  char b[16];
  std::snprintf(b, sizeof b, "0x%08x", v);
  return b;
}
struct Where {
  long long b, h, row, col, wg;
};
inline Where locate(const char* what, uint64_t word, long long Hq, long long Sq) {
  const bool o = what[0] == 'O';
  const uint64_t flat = o ? word * 2 / kHeadDim : word;  // (b, h, row)
  Where w;
  w.col = o ? (long long)(word * 2 % kHeadDim) : -1;
  w.row = (long long)(flat % (uint64_t)Sq);
  w.h = (long long)(flat / (uint64_t)Sq % (uint64_t)Hq);
  w.b = (long long)(flat / (uint64_t)Sq / (uint64_t)Hq);
  w.wg = (w.b * Hq + w.h) * query_tiles(Sq) + w.row / kQTile;
  return w;
}
inline std::string where_text(const Where& w, const uint32_t* table) {
  std::string s = "batch " + std::to_string(w.b) + " head " + std::to_string(w.h) + " row " + std::to_string(w.row);
  if (w.col >= 0) s += " col " + std::to_string(w.col);
  if (table) {
    const ntm::cus::CuId id = ntm::cus::decode(table[w.wg * kTableWords], table[w.wg * kTableWords + 1]);
    s += ": xcd " + std::to_string(id.xcc) + " se " + std::to_string(id.se) + " sh " + std::to_string(id.sh) +
         " cu " + std::to_string(id.cu);
  }
  return s;
}
inline std::string failure_message(int gpu, const char* sub, const char* what, uint64_t count, uint64_t word,
                                   uint32_t expected, uint32_t got, long long Hq, long long Sq,
                                   const uint32_t* table) {
  return "gpu" + std::to_string(gpu) + ": attn " + sub + " " + what + ": " +
         where_text(locate(what, word, Hq, Sq), table) + ": expected " + hex32(expected) + ", got " + hex32(got) +
         ", bad bits " + hex32(expected ^ got) + "; " + std::to_string((unsigned long long)count) + " differ";
}

}  // namespace attn
}  // namespace ntm
