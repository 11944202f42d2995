// K14 (paged-KV decode attention, "pda") host side: shapes, the split plan, the workspace and
// LDS budget of ntm_pda_fwd, the bytes a pass reads, the page-table generator, scatter / gather
// of host vectors, exact inputs per sequence and the failure message. Pure C++ - no HIP - so the
// Job, the kernels' header (ntm/pda.hpp) and a CPU-only test program share it. ops/pda.py
// mirrors it in numpy. The exact-input machinery is attn_plan.hpp's, unchanged.
//
// Q and O [B][Hq][T][128] bf16, T = 1 .. 4 new tokens; m and l [B][Hq][T] fp32. The K pool and
// the V pool [pages][Hkv][16][128] bf16 (kPage = 16 tokens per page); block_table
// [B][max_pages] int32 names the physical page of every logical page of a sequence; seq_lens
// [B] int32, T <= len_b <= 65536. G = Hq / Hkv and G * T <= 32: the rows of one key/value head
// fill one 32-wide MFMA side, row g * T + t being token t of query head hkv * G + g. Row (g, t)
// of sequence b sees key j iff j <= len_b - T + t: K13's bottom-right causal with Sq = T and
// Sk = len_b.
//
// The split plan. Sequence b has steps_b = ceil(len_b / 64) key steps. Split s of S takes the
// steps [s * per_b, min((s + 1) * per_b, steps_b)), per_b = ceil(steps_b / S): the ranges tile
// [0, steps_b), and the last ones are empty when S * per_b overshoots steps_b. Inside a
// workgroup wave w takes that range's steps w, w + 4, ...
//
// The arithmetic contract of ntm_pda_fwd: K13's (attn_plan.hpp) for every partial, plus the
// merge.
//   A partial is (m_p, l_p, acc_p) over the keys of one wave of one split, computed exactly as
//   K13 computes a row: s on v_mfma_f32_32x32x16_bf16, p = exp2(scale_log2 * (s - m_run)) on
//   v_exp_f32, l the sum of the fp32 p, p rounded to bf16 (nearest even) before the second
//   MFMA, alpha = exp2(scale_log2 * (m_old - m_new)) at each key step: l and the accumulator are
//   multiplied by it, then the second MFMA accumulates onto the rescaled accumulator, as in
//   K13. A partial without a visible key is (-inf, 0, 0).
//   Partials are merged in a fixed order: the waves 0 .. 3 of a workgroup first (in
//   pda_split_kernel), then the splits 0 .. S - 1 (in pda_combine_kernel):
//     m       = max(m_p)
//     alpha_p = exp2(scale_log2 * (m_p - m)) on v_exp_f32, DEFINED as 0 when m_p = -inf:
//               no inf - inf ever reaches the exponent (inside a partial likewise: a key step in
//               which a row sees nothing leaves its state as it was)
//     l       = sum alpha_p * l_p,  acc = sum alpha_p * acc_p, each a multiply and an add in
//               fp32, in that order
//   O = one correctly rounded fp32 division acc / l, then a nearest-even pack to bf16.
//   Keys at or past len_b are never used: they are staged as zeros, in K and in V, and scored
//   -inf, so a poisoned page tail or poison page cannot reach a product. A page id outside
//   [0, pages) is treated the same way (zeros), never dereferenced.
// On attn_exact inputs every weight is a power of two within kExactR of the row's top score, or
// exactly 0, so the merge is exact in fp32 in every grouping and attn_reference_kernel on the
// gathered keys is a bitwise oracle for O, m and l.
//
// Stage depth (cdna_hip_programming.md Appendix B 'Attention decode'; MI355X_MICROARCH.md
// 'Indexed rows: gather into LDS': about 72 KiB in flight per CU hide an HBM miss). Depth one,
// half a step at a time: a wave always has one 16 KiB load in flight - V of step n (through
// registers into its own LDS stage) issued right after S^T of step n, under the softmax, and K
// of step n + 1 (straight into the registers the first MFMA reads) issued once V is staged, under
// P V. K and V never hold registers together and Q^T lives in LDS, so the kernel fits the 256
// registers of two waves per SIMD without scratch (the compiler's report is recorded in
// profiles/pda/README.md): two workgroups share a CU (2 x 77824 bytes of LDS), 8 waves x 16 KiB =
// 128 KiB in flight per CU, above the 72 KiB. A whole step ahead would cost 128 more VGPRs per lane and halve the waves per CU: the
// same bytes in flight. The rate is recorded in profiles/pda/README.md and not tuned.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

#include "ntm/attn_plan.hpp"

namespace ntm {
namespace pda {

using ntm::attn::kHeadDim;
constexpr int kPage = 16;      // tokens per page
constexpr int kKeyStep = 64;   // keys per step of one wave: 4 pages
constexpr int kRows = 32;      // G * T rows of one key/value head, padded
constexpr int kMaxT = 4;
constexpr int kThreads = 256, kWaves = 4;
constexpr int kMaxLen = 65536;
constexpr int kMaxSplits = 64;
constexpr int kMinStepsPerSplit = 4;
constexpr int kTableWords = 2;  // per workgroup: raw HW_REG_HW_ID, raw HW_REG_XCC_ID of wave 0
// One wave's LDS stage: 64 V rows of 128 bf16 and 16 bytes of padding (K13's row). After the key
// loop the same bytes hold the wave's partial for the merge: 32 rows of 128 fp32 and 16 bytes
// of padding, then m[32] and l[32].
constexpr int kLdsRowBytes = kHeadDim * 2 + 16;
constexpr int kLdsWaveBytes = kKeyStep * kLdsRowBytes;
constexpr int kLdsQBytes = 8 * 64 * 16;  // Q^T of the 32 rows as the MFMA's B operand: [k-step][lane] x 16 bytes
constexpr int kLdsBytes = kWaves * kLdsWaveBytes + kLdsQBytes;
constexpr int kMergeRowBytes = kHeadDim * 4 + 16;
constexpr int kMergeStatsOffset = kRows * kMergeRowBytes;
static_assert(2 * kLdsBytes <= 160 * 1024, "two workgroups of ntm_pda_fwd share the 160 KiB of LDS of a gfx950 CU");
static_assert(kMergeStatsOffset + 2 * kRows * 4 <= kLdsWaveBytes, "a wave's partial fits its own stage");
static_assert(kLdsRowBytes % 16 == 0 && kMergeRowBytes % 16 == 0, "rows are written with 16-byte stores");
// One workgroup's partial in the workspace: acc [32][128] fp32, then m[32], then l[32].
constexpr int kPartialFloats = kRows * kHeadDim + 2 * kRows;

inline bool shape_ok(long long B, long long Hq, long long Hkv, long long T, long long max_pages, long long pages,
                     long long S) {
  if (B < 1 || Hq < 1 || Hkv < 1 || T < 1 || T > kMaxT || max_pages < 1 || pages < 1 || S < 1 || S > kMaxSplits)
    return false;
  if (Hq % Hkv || Hq / Hkv * T > kRows || max_pages > kMaxLen / kPage) return false;
  // the grid is one-dimensional, and every element index fits 63 bits with room to spare
  return B <= (1ll << 20) && Hq <= (1ll << 10) && pages <= (1ll << 24) && B * Hkv * S < (1ll << 31);
}
inline long long grid(long long B, long long Hkv, long long S) { return B * Hkv * S; }
inline size_t workspace_bytes(long long B, long long Hkv, long long S) {
  return B < 1 || Hkv < 1 || S < 1 ? 0 : (size_t)grid(B, Hkv, S) * kPartialFloats * 4;
}
inline size_t table_bytes(long long B, long long Hkv, long long S) {
  return B < 1 || Hkv < 1 || S < 1 ? 0 : (size_t)grid(B, Hkv, S) * kTableWords * 4;
}
NTM_HD inline int key_steps(int len) { return (len + kKeyStep - 1) / kKeyStep; }
struct Range {
  int begin, end;  // key steps [begin, end); empty when begin >= end
};
NTM_HD inline Range split_range(int len, int s, int S) {
  const int steps = key_steps(len), per = (steps + S - 1) / S;
  Range r;
  r.begin = s * per < steps ? s * per : steps;
  r.end = (s + 1) * per < steps ? (s + 1) * per : steps;
  return r;
}
// The default S: the smallest with B * Hkv * S >= 2 * cus (two workgroups per CU), capped so
// that every split of the longest sequence keeps at least 4 steps (S <= steps / 4), within
// 1 .. kMaxSplits.
inline int pda_splits(long long B, long long Hkv, long long max_len, long long cus) {
  if (B < 1 || Hkv < 1 || max_len < 1 || cus < 1) return 1;
  long long want = (2 * cus + B * Hkv - 1) / (B * Hkv);
  const long long cap = ((max_len + kKeyStep - 1) / kKeyStep) / kMinStepsPerSplit;
  if (want > cap) want = cap;
  if (want > kMaxSplits) want = kMaxSplits;
  return want < 1 ? 1 : (int)want;
}
// the K and V bytes a pass must read: every key below len_b of every key/value head, once
inline double kv_bytes(const int32_t* lens, long long B, long long Hkv) {
  double keys = 0;
  for (long long b = 0; b < B; ++b) keys += (double)lens[b];
  return keys * (double)Hkv * kHeadDim * 2.0 * 2.0;
}

// ---- the page-table generator. The pool has one page per logical page of every sequence and
// one poison page; a seeded Fisher-Yates permutation hands the physical pages out, so
// consecutive logical pages are not adjacent. Sequence 2 i + 1 of the first `shared_pairs`
// pairs points its first min(n_2i, n_2i+1) / 2 logical pages at those of sequence 2 i (prefix
// sharing; its own pages of that range stay unused). Every entry past a sequence's last page
// names the poison page: a valid id, so that a read past the end shows as poison, not a fault.
constexpr uint32_t kStreamPerm = 6;
struct PageTable {
  int B = 0, max_pages = 0, pages = 0, poison = 0;
  std::vector<int32_t> lens, table;  // table [B][max_pages]
};
inline int pages_of(int len) { return (len + kPage - 1) / kPage; }
inline PageTable make_page_table(const std::vector<int32_t>& lens, uint32_t seed, int shared_pairs) {
  PageTable pt;
  pt.B = (int)lens.size(), pt.lens = lens;
  int total = 0;
  for (int32_t n : lens) {
    total += pages_of(n);
    if (pages_of(n) > pt.max_pages) pt.max_pages = pages_of(n);
  }
  pt.pages = total + 1;
  std::vector<int32_t> perm((size_t)pt.pages);
  for (int i = 0; i < pt.pages; ++i) perm[(size_t)i] = i;
  for (int i = pt.pages - 1; i >= 1; --i) {
    const uint32_t j = ntm::attn::attn_hash(seed, kStreamPerm, (uint32_t)i) % (uint32_t)(i + 1);
    const int32_t x = perm[(size_t)i];
    perm[(size_t)i] = perm[j], perm[j] = x;
  }
  pt.poison = perm[(size_t)total];
  pt.table.assign((size_t)pt.B * pt.max_pages, pt.poison);
  int next = 0;
  for (int b = 0; b < pt.B; ++b)
    for (int p = 0; p < pages_of(lens[(size_t)b]); ++p) pt.table[(size_t)b * pt.max_pages + p] = perm[(size_t)next++];
  for (int i = 0; i < shared_pairs && 2 * i + 1 < pt.B; ++i) {
    const int a = 2 * i, b = 2 * i + 1;
    // whole pages only, all of them below both lengths
    int share = lens[(size_t)a] / kPage < lens[(size_t)b] / kPage ? lens[(size_t)a] / kPage : lens[(size_t)b] / kPage;
    share /= 2;
    for (int p = 0; p < share; ++p) pt.table[(size_t)b * pt.max_pages + p] = pt.table[(size_t)a * pt.max_pages + p];
  }
  return pt;
}
// src [Hkv][len][128] of sequence b -> pool [pages][Hkv][16][128], and back
template <typename E>
inline void scatter_to_pages(const PageTable& pt, int b, int Hkv, const E* src, std::vector<E>& pool) {
  const int len = pt.lens[(size_t)b];
  for (int h = 0; h < Hkv; ++h)
    for (int j = 0; j < len; ++j) {
      const size_t pg = (size_t)pt.table[(size_t)b * pt.max_pages + j / kPage];
      const E* s = src + ((size_t)h * len + j) * kHeadDim;
      E* d = pool.data() + ((pg * Hkv + h) * kPage + j % kPage) * kHeadDim;
      for (int x = 0; x < kHeadDim; ++x) d[x] = s[x];
    }
}
template <typename E>
inline std::vector<E> gather_from_pages(const PageTable& pt, int b, int Hkv, const std::vector<E>& pool) {
  const int len = pt.lens[(size_t)b];
  std::vector<E> out((size_t)Hkv * len * kHeadDim);
  for (int h = 0; h < Hkv; ++h)
    for (int j = 0; j < len; ++j) {
      const size_t pg = (size_t)pt.table[(size_t)b * pt.max_pages + j / kPage];
      const E* s = pool.data() + ((pg * Hkv + h) * kPage + j % kPage) * kHeadDim;
      E* d = out.data() + ((size_t)h * len + j) * kHeadDim;
      for (int x = 0; x < kHeadDim; ++x) d[x] = s[x];
    }
  return out;
}

// ---- exact inputs of one sequence, from attn_plan.hpp's generator: q [Hq][T][128], k and v
// [Hkv][len][128]. The dimensions that all keys of a head share (exact_k's `head`) depend on the
// key/value head alone, not on the sequence, so keys of two sequences may share a row's softmax
// (prefix sharing) and attn_exact still holds; every other stream is hashed per sequence.
inline ntm::attn::Inputs exact_sequence(uint32_t seed, int b, int Hq, int Hkv, int T, int len) {
  namespace at = ntm::attn;
  at::Inputs in;
  in.B = 1, in.Hq = Hq, in.Hkv = Hkv, in.Sq = T, in.Sk = len;
  const size_t qrows = (size_t)Hq * T, krows = (size_t)Hkv * len;
  in.q.resize(qrows * kHeadDim), in.k.resize(krows * kHeadDim), in.v.resize(krows * kHeadDim);
  for (size_t r = 0; r < qrows; ++r)
    for (int d = 0; d < kHeadDim; ++d) in.q[r * kHeadDim + d] = at::exact_q(seed, (uint32_t)((size_t)b * 4096 + r), d);  // Hq * T <= 4096
  for (int h = 0; h < Hkv; ++h)
    for (int j = 0; j < len; ++j) {
      const uint32_t row = ((uint32_t)b * (uint32_t)Hkv + (uint32_t)h) * (uint32_t)kMaxLen + (uint32_t)j;
      const size_t at_row = ((size_t)h * len + j) * kHeadDim;
      for (int d = 0; d < kHeadDim; ++d) {
        in.k[at_row + d] = at::exact_k(seed, (uint32_t)h, row, d);
        in.v[at_row + d] = at::exact_v(seed, row, d);
      }
    }
  auto bits = [](const std::vector<int32_t>& x) {
    std::vector<uint16_t> o(x.size());
    for (size_t i = 0; i < x.size(); ++i) o[i] = at::bf16_of_int(x[i]);
    return o;
  };
  in.qb = bits(in.q), in.kb = bits(in.k), in.vb = bits(in.v);
  return in;
}

// ---- failure lines: one line under 200 characters.
// "gpu3: pda exact T4 O: seq 23 head 31 tok 3 col 126: cu 7.3.1.15 0.0.0.2 (xcd.se.sh.cu):
//  expected 0x3f803f80, got 0x3f803f81, bad bits 0x00000001; 1 differ". `what` is "O" (a word
// is two bf16 elements, col the first), "m" or "l" (no col); `word` the flat index of the 4-byte
// word; the CUs are those of the first 4 split workgroups that fed the row, in split order.
struct Where {
  long long b, h, t, col, wg;  // wg: the row's split 0
};
inline Where locate(const char* what, uint64_t word, long long Hq, long long Hkv, long long T, long long S) {
  const bool o = what[0] == 'O';
  const uint64_t flat = o ? word * 2 / kHeadDim : word;  // (b, h, t)
  Where w;
  w.col = o ? (long long)(word * 2 % kHeadDim) : -1;
  w.t = (long long)(flat % (uint64_t)T);
  w.h = (long long)(flat / (uint64_t)T % (uint64_t)Hq);
  w.b = (long long)(flat / (uint64_t)T / (uint64_t)Hq);
  w.wg = (w.b * Hkv + w.h / (Hq / Hkv)) * S;
  return w;
}
inline std::string where_text(const Where& w, long long S, const uint32_t* table) {
  std::string s = "seq " + std::to_string(w.b) + " head " + std::to_string(w.h) + " tok " + std::to_string(w.t);
  if (w.col >= 0) s += " col " + std::to_string(w.col);
  if (table) {
    s += ": cu";
    for (long long i = 0; i < S && i < 4; ++i) {
      const ntm::cus::CuId id = ntm::cus::decode(table[(w.wg + i) * kTableWords], table[(w.wg + i) * kTableWords + 1]);
      s += " " + std::to_string(id.xcc) + "." + std::to_string(id.se) + "." + std::to_string(id.sh) + "." +
           std::to_string(id.cu);
    }
    s += " (xcd.se.sh.cu)";
  }
  return s;
}
inline std::string failure_message(int gpu, const char* sub, const char* what, uint64_t count, uint64_t word,
                                   uint32_t expected, uint32_t got, long long Hq, long long Hkv, long long T,
                                   long long S, const uint32_t* table) {
  using ntm::attn::hex32;
  return "gpu" + std::to_string(gpu) + ": pda " + sub + " " + what + ": " +
         where_text(locate(what, word, Hq, Hkv, T, S), S, table) + ": expected " + hex32(expected) + ", got " +
         hex32(got) + ", bad bits " + hex32(expected ^ got) + "; " + std::to_string((unsigned long long)count) +
         " differ";
}

}  // namespace pda
}  // namespace ntm
