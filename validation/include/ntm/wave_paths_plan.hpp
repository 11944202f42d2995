// K12 (wave data-path and special-function check) host side: the op list of the `lane`
// family and its lane map src_lane, the transposed-read maps and image generator of `ldstr`,
// the input lists and brackets of `sfu`, the truth-table evaluator and bf16 rounding of `valu`,
// the per-workgroup record, the verdict and the failure messages. Pure C++ - no HIP - so the
// Job, the kernels (ntm/wave_paths.hpp) and a CPU-only test program share it; functions the
// kernels also call carry NTM_HD. ops/wave.py mirrors it in numpy.
//
// lane: thread t of a workgroup (wave w = t / 64, lane l = t % 64) holds two words, x and y
// (hash32 streams 0 and 1). Op i of lane_ops() maps them to one exact output word:
// out[l] = x[s] for s = src_lane(op, l) in 0 .. 63, y[s - 64] for s in 64 .. 127, y[l] for
// kOld, 0 for kZero and for kSkip (a lane whose result this file does not claim to know).
//   DPP (v_mov_b32_dpp, old = y): ctrl is the 9-bit dpp_ctrl. A lane that row_mask / bank_mask
//   disable keeps old. An enabled lane whose source does not exist (shifted in from outside its
//   row or the wave) keeps old with bound_ctrl off and reads 0 with bound_ctrl on.
//     quad_perm [a,b,c,d]  lane 4k+j reads lane 4k + (a,b,c,d)[j]
//     row_shl:n            lane reads lane + n of its row of 16;  row_shr:n  lane - n
//     row_ror:n            lane reads (lane - n) mod 16 of its row
//     wave_shl:1           lane reads lane + 1 (63: none);  wave_rol:1  (lane + 1) mod 64
//     wave_shr:1           lane reads lane - 1 (0: none);   wave_ror:1  (lane - 1) mod 64
//     row_mirror           15 - lane within the row;  row_half_mirror  7 - lane within 8
//     row_bcast:15         lanes 16 .. 63 read lane 15 of the row before theirs
//     row_bcast:31         lanes 32 .. 63 read lane 31
//     row_newbcast:n       lane reads lane n of its row
//   Not judged (kSkip): row 0 under row_bcast:15 and rows 0 - 1 under row_bcast:31.
//   ds_bpermute_b32: out[l] = x[(index[l] >> 2) & 63]; ds_permute_b32: out[(index[l] >> 2) & 63] = x[l]
//   ds_swizzle_b32: offset bit 15 set = quad_perm in bits 7:0; clear = within each 32 lanes
//     lane' = ((lane & and) | or) ^ xor, and = bits 4:0, or = 9:5, xor = 14:10
//   v_permlane32_swap vdst=x, src=y: lanes 32 .. 63 of x exchange with lanes 0 .. 31 of y;
//   v_permlane16_swap: rows 1 and 3 of x exchange with rows 0 and 2 of y (ctrl 0 / 1 = which
//     of the two results is stored)
//   v_readlane n: every lane gets x[n]; v_readfirstlane: x[0]
//   Partial EXEC, the two cases whose result is defined: v_readfirstlane inside `if (l >= k)`
//   (lanes >= k get x[k], the rest keep y) and ds_bpermute_b32 inside `if (l >= 32)` reading
//   active lanes only. DPP, ds_permute and ds_swizzle under partial EXEC, and a ds_bpermute
//   that reads an inactive lane, are not issued.
//
// ldstr: see tr_src() below. sfu, valu: see their sections.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "ntm/cu_sweep_plan.hpp"  // NTM_HD, h32, the HW_ID decode

namespace ntm {
namespace wave {

using cus::h32;

constexpr int kThreads = 256, kWaves = 4, kLanes = 64;
constexpr int kFamLane = 0, kFamLdstr = 1, kFamSfu = 2, kFamValu = 3, kFamilies = 4;
inline const char* family_name(int f) {
  static const char* const n[kFamilies] = {"lane", "ldstr", "sfu", "valu"};
  return f >= 0 && f < kFamilies ? n[f] : "?";
}
constexpr uint32_t kMagic = 0x4B31324Bu;
constexpr int kMaxLaunches = cus::kMaxLaunches, kGridPerCu = 2;
constexpr uint32_t kNoFault = ~0u;
constexpr uint32_t kFaultBit = 1u << 10;

NTM_HD inline uint32_t hash32(uint32_t seed, uint32_t stream, uint32_t w, uint32_t r, uint32_t l) {
  return h32(seed + 0x9E3779B9u * (((((stream * 4u + w) << 8) | (r & 255u)) << 6 | l) + 1u));
}

// ------------------------------------------------------------------ lane
enum : uint8_t { kDpp = 0, kBpermute, kPermute, kSwizzle, kSwap16, kSwap32, kReadlane, kReadfirst,
                 kReadfirstBranch, kBpermuteBranch, kLaneKinds };
constexpr int kOld = -1, kZero = -2, kSkip = -3;

struct LaneOp {
  uint8_t kind;
  uint16_t ctrl;
  uint8_t bound, row_mask, bank_mask;
};

constexpr int kQuadPerms = 8, kSwizzles = 8, kMaskSets = 3;
constexpr int kDppCtrls = kQuadPerms + 45 + 4 + 4 + 16;
constexpr int kDppOps = kDppCtrls * 2 * kMaskSets;
constexpr int kLaneOps = kDppOps + 3 + 2 + kSwizzles + 2 + 2 + 64 + 1 + 2 + 1;
NTM_HD constexpr uint16_t quad_perm_at(int i) {
  // identity 0123, reverse 3210, the four broadcasts, 1032 and 2301
  constexpr uint16_t q[kQuadPerms] = {0xE4, 0x1B, 0x00, 0x55, 0xAA, 0xFF, 0xB1, 0x4E};
  return q[i];
}
NTM_HD constexpr uint16_t swizzle_at(int i) {
  // xor 1, xor 16, reverse 32, and 0x1E or 1, and 0x10 or 3 xor 4; quad reverse, quad broadcast 0, quad 1032
  constexpr uint16_t sw[kSwizzles] = {0x041F, 0x401F, 0x7C1F, 0x003E, 0x1070, 0x801B, 0x8000, 0x80B1};
  return sw[i];
}
NTM_HD constexpr uint8_t row_mask_at(int m) { return m == 1 ? 0x5 : 0xF; }
NTM_HD constexpr uint8_t bank_mask_at(int m) { return m == 2 ? 0x6 : 0xF; }
NTM_HD constexpr uint16_t dpp_ctrl_at(int i) {
  if (i < kQuadPerms) return quad_perm_at(i);
  i -= kQuadPerms;
  if (i < 15) return (uint16_t)(0x101 + i);       // row_shl
  if (i < 30) return (uint16_t)(0x111 + i - 15);  // row_shr
  if (i < 45) return (uint16_t)(0x121 + i - 30);  // row_ror
  i -= 45;
  if (i < 4) return (uint16_t)(0x130 + 4 * i);  // wave_shl, wave_rol, wave_shr, wave_ror
  i -= 4;
  if (i < 4) return (uint16_t)(0x140 + i);  // row_mirror, row_half_mirror, row_bcast:15, row_bcast:31
  return (uint16_t)(0x150 + i - 4);         // row_newbcast
}
// op i of the list: the DPP controls with both bound_ctrl settings under full masks, then under
// row_mask 0x5, then under bank_mask 0x6; then the other kinds
NTM_HD constexpr LaneOp lane_op(int i) {
  if (i < kDppOps)
    return LaneOp{kDpp, dpp_ctrl_at(i % kDppCtrls), (uint8_t)((i / kDppCtrls) & 1), row_mask_at(i / (2 * kDppCtrls)),
                  bank_mask_at(i / (2 * kDppCtrls))};
  i -= kDppOps;
  if (i < 3) return LaneOp{kBpermute, (uint16_t)i, 0, 0xF, 0xF};
  i -= 3;
  if (i < 2) return LaneOp{kPermute, (uint16_t)i, 0, 0xF, 0xF};
  i -= 2;
  if (i < kSwizzles) return LaneOp{kSwizzle, swizzle_at(i), 0, 0xF, 0xF};
  i -= kSwizzles;
  if (i < 2) return LaneOp{kSwap16, (uint16_t)i, 0, 0xF, 0xF};
  i -= 2;
  if (i < 2) return LaneOp{kSwap32, (uint16_t)i, 0, 0xF, 0xF};
  i -= 2;
  if (i < 64) return LaneOp{kReadlane, (uint16_t)i, 0, 0xF, 0xF};
  i -= 64;
  if (i == 0) return LaneOp{kReadfirst, 0, 0, 0xF, 0xF};
  if (i == 1) return LaneOp{kReadfirstBranch, 5, 0, 0xF, 0xF};
  if (i == 2) return LaneOp{kReadfirstBranch, 37, 0, 0xF, 0xF};
  return LaneOp{kBpermuteBranch, 0, 0, 0xF, 0xF};
}
constexpr int kFirstSwizzleOp = kDppOps + 5;

// the index word lane l gives ds_bpermute (variant 0 a bijection, 1 many to one, 2 a bijection
// with bits outside 2 .. 7 set) and ds_permute (variants 0 and 1: the bijections 0 and 2)
NTM_HD inline uint32_t bpermute_index(int variant, int l) {
  if (variant == 0) return (uint32_t)((((l * 37 + 11) & 63) ^ 0x15) << 2);
  if (variant == 1) return (h32(0xB5u + (uint32_t)l) & 60u) << 2;
  return (uint32_t)(((l * 29 + 5) & 63) << 2) | (h32(0x99u + (uint32_t)l) & 0xFFFFFF03u);
}
NTM_HD inline uint32_t permute_index(int variant, int l) { return bpermute_index(variant ? 2 : 0, l); }
NTM_HD inline uint32_t branch_bpermute_index(int l) { return (uint32_t)((32 + ((l * 13 + 7) & 31)) << 2); }

// the lane a DPP control reads: 0 .. 63, kOld for "no such lane", kSkip for not judged
NTM_HD inline int dpp_src(unsigned ctrl, int l) {
  const int row = l & ~15, i = l & 15, n = (int)(ctrl & 15u);
  if (ctrl < 0x100) return (l & ~3) | (int)((ctrl >> (2 * (l & 3))) & 3u);
  if (ctrl >= 0x101 && ctrl <= 0x10F) return i + n < 16 ? l + n : kOld;
  if (ctrl >= 0x111 && ctrl <= 0x11F) return i >= n ? l - n : kOld;
  if (ctrl >= 0x121 && ctrl <= 0x12F) return row | ((i - n) & 15);
  if (ctrl == 0x130) return l < 63 ? l + 1 : kOld;
  if (ctrl == 0x134) return (l + 1) & 63;
  if (ctrl == 0x138) return l > 0 ? l - 1 : kOld;
  if (ctrl == 0x13C) return (l - 1) & 63;
  if (ctrl == 0x140) return row | (15 - i);
  if (ctrl == 0x141) return (l & ~7) | (7 - (l & 7));
  if (ctrl == 0x142) return l >= 16 ? row - 1 : kSkip;
  if (ctrl == 0x143) return l >= 32 ? 31 : kSkip;
  if (ctrl >= 0x150 && ctrl <= 0x15F) return row | n;
  return kSkip;
}

NTM_HD inline int src_lane(const LaneOp& op, int l) {
  switch (op.kind) {
    case kDpp: {
      if (!((op.row_mask >> (l >> 4)) & 1) || !((op.bank_mask >> ((l & 15) >> 2)) & 1)) return kOld;
      const int s = dpp_src(op.ctrl, l);
      return s == kOld ? (op.bound ? kZero : kOld) : s;
    }
    case kBpermute: return (int)((bpermute_index(op.ctrl, l) >> 2) & 63u);
    case kPermute:
      for (int s = 0; s < kLanes; ++s)
        if ((int)((permute_index(op.ctrl, s) >> 2) & 63u) == l) return s;
      return kSkip;
    case kSwizzle:
      if (op.ctrl & 0x8000) return (l & ~3) | ((op.ctrl >> (2 * (l & 3))) & 3);
      return (l & 32) | ((((l & 31) & (op.ctrl & 31)) | ((op.ctrl >> 5) & 31)) ^ ((op.ctrl >> 10) & 31));
    case kSwap16:
      if (op.ctrl == 0) return ((l >> 4) & 1) ? 64 + l - 16 : l;  // new vdst: odd rows from y's row before
      return ((l >> 4) & 1) ? 64 + l : l + 16;                    // new src: even rows from x's row after
    case kSwap32:
      if (op.ctrl == 0) return l < 32 ? l : 64 + l - 32;
      return l < 32 ? l + 32 : 64 + l;
    case kReadlane: return op.ctrl & 63;
    case kReadfirst: return 0;
    case kReadfirstBranch: return l >= (int)op.ctrl ? (int)op.ctrl : kOld;
    case kBpermuteBranch: return l >= 32 ? (int)((branch_bpermute_index(l) >> 2) & 63u) : kOld;
  }
  return kSkip;
}
NTM_HD inline uint32_t lane_expected(const LaneOp& op, int l, const uint32_t* x, const uint32_t* y) {
  const int s = src_lane(op, l);
  return s >= 64 ? y[s - 64] : s >= 0 ? x[s] : s == kOld ? y[l] : 0u;
}

inline std::string dpp_name(unsigned c) {
  char b[48];
  if (c < 0x100) std::snprintf(b, sizeof b, "quad_perm:[%u,%u,%u,%u]", c & 3, (c >> 2) & 3, (c >> 4) & 3, (c >> 6) & 3);
  else if (c <= 0x10F) std::snprintf(b, sizeof b, "row_shl:%u", c & 15);
  else if (c <= 0x11F) std::snprintf(b, sizeof b, "row_shr:%u", c & 15);
  else if (c <= 0x12F) std::snprintf(b, sizeof b, "row_ror:%u", c & 15);
  else if (c == 0x130) return "wave_shl:1";
  else if (c == 0x134) return "wave_rol:1";
  else if (c == 0x138) return "wave_shr:1";
  else if (c == 0x13C) return "wave_ror:1";
  else if (c == 0x140) return "row_mirror";
  else if (c == 0x141) return "row_half_mirror";
  else if (c == 0x142) return "row_bcast:15";
  else if (c == 0x143) return "row_bcast:31";
  else std::snprintf(b, sizeof b, "row_newbcast:%u", c & 15);
  return b;
}
// "row_shr:3 bound_ctrl:0", "row_shl:1 bound_ctrl:1 row_mask:0x5", "ds_swizzle 0x041f", "readlane 7"
inline std::string lane_op_name(const LaneOp& op) {
  char b[64];
  switch (op.kind) {
    case kDpp: {
      std::string s = dpp_name(op.ctrl) + " bound_ctrl:" + std::to_string((int)op.bound);
      if (op.row_mask != 0xF) std::snprintf(b, sizeof b, " row_mask:0x%x", op.row_mask), s += b;
      if (op.bank_mask != 0xF) std::snprintf(b, sizeof b, " bank_mask:0x%x", op.bank_mask), s += b;
      return s;
    }
    case kBpermute: return "ds_bpermute " + std::to_string(op.ctrl);
    case kPermute: return "ds_permute " + std::to_string(op.ctrl);
    case kSwizzle: std::snprintf(b, sizeof b, "ds_swizzle 0x%04x", op.ctrl); return b;
    case kSwap16: return "permlane16_swap " + std::to_string(op.ctrl);
    case kSwap32: return "permlane32_swap " + std::to_string(op.ctrl);
    case kReadlane: return "readlane " + std::to_string(op.ctrl);
    case kReadfirst: return "readfirstlane";
    case kReadfirstBranch: return "readfirstlane branch " + std::to_string(op.ctrl);
    case kBpermuteBranch: return "ds_bpermute branch";
  }
  return "?";
}

// ------------------------------------------------------------------ ldstr
// A transposed read works per group of 16 consecutive lanes on a block of rows x 16 columns of
// BITS-bit elements. Each lane's address names one slot: 8 bytes (16 bytes, 12 used, for the
// 6-bit form) of E = 64 / BITS (16) consecutive elements of one row; P = 16 / E lanes cover a
// row, so lane j of the group supplies row j / P, columns E (j % P) .. The result of lane i
// holds `rows` elements, element q in bits [q BITS, (q + 1) BITS) of its 64 (96) bits:
//   16-bit (cdna_hip_programming.md T10): lane i receives column i, row q in its element q -
//   element q of lane i is element i % 4 of the slot of lane 4 q + i / 4.
//   8-, 4- and 6-bit: measured with tools/wave_lane_map_probe.py (profiles/wave/lane_map_probe.log):
//   "=> ds_read_b64_tr_b8 stride 32: element q of group lane i is element i % 8 of the slot of
//   group lane 2 q + i // 8: True", "=> ds_read_b64_tr_b4 stride 32: element q of group lane i is
//   element i % 16 of the slot of group lane 1 q + i // 16: True", "=> ds_read_b96_tr_b6 stride
//   32: element q of group lane i is element i % 16 of the slot of group lane 1 q + i // 16: True",
//   each with "every element's bits are consecutive image bits in order: True". The 6-bit form
//   needs 16-byte aligned addresses: "=> ds_read_b96_tr_b6 at 8 mod 16: every source lies in a
//   slot of the reader's own 16-lane group: False"; its row strides are multiples of 16.
constexpr int kTrForms = 4;
constexpr int kTrBits[kTrForms] = {16, 8, 4, 6};
NTM_HD inline int tr_form(int bits) { return bits == 16 ? 0 : bits == 8 ? 1 : bits == 4 ? 2 : bits == 6 ? 3 : -1; }
NTM_HD inline int tr_elems(int bits) { return bits == 6 ? 16 : 64 / bits; }      // E: per slot and per result
NTM_HD inline int tr_slot_bytes(int bits) { return bits == 6 ? 16 : 8; }
NTM_HD inline int tr_lanes_per_row(int bits) { return 16 / tr_elems(bits); }      // P
NTM_HD inline int tr_rows(int bits) { return tr_elems(bits); }                    // rows of a block
NTM_HD inline int tr_words(int bits) { return bits == 6 ? 3 : 2; }
NTM_HD inline int tr_align(int bits) { return bits == 6 ? 16 : 8; }
constexpr int kTrMaxBytes = 16384, kTrMaxWidth = 128;
// the per-CU sweep's image: 64 rows of 136 bytes (padded rows); 144 for the 6-bit form
constexpr int kSweepRows = 64;
NTM_HD inline int sweep_stride(int bits) { return bits == 6 ? 144 : 136; }

// element q of the result of group lane i = element *e of the slot whose address lane *j gave
NTM_HD inline void tr_src(int bits, int i, int q, int* j, int* e) {
  const int E = tr_elems(bits), P = tr_lanes_per_row(bits);
  *j = q * P + i / E;
  *e = i % E;
}

struct TrShape {
  int bits, rows, stride, width, row_blocks, col_blocks, blocks, iters;
};
// rows a multiple of the block's, stride a multiple of the form's alignment and >= 32, image
// within 16 KiB
NTM_HD inline bool tr_shape(int bits, int rows, int stride, TrShape* s) {
  if (tr_form(bits) < 0 || rows <= 0 || stride < 32 || stride % tr_align(bits) || rows % tr_rows(bits) ||
      (long long)rows * stride > kTrMaxBytes)
    return false;
  s->bits = bits, s->rows = rows, s->stride = stride;
  s->width = (stride < kTrMaxWidth ? stride : kTrMaxWidth) & ~31;
  s->row_blocks = rows / tr_rows(bits);
  s->col_blocks = s->width / (tr_lanes_per_row(bits) * tr_slot_bytes(bits));
  s->blocks = s->row_blocks * s->col_blocks;
  s->iters = (s->blocks + 15) / 16;
  return true;
}
// byte address of the slot lane j of the group supplies for block b (clamped to the last block)
NTM_HD inline int tr_addr(const TrShape& s, int b, int j) {
  if (b >= s.blocks) b = s.blocks - 1;
  const int P = tr_lanes_per_row(s.bits), sb = tr_slot_bytes(s.bits);
  const int rb = b / s.col_blocks, cb = b % s.col_blocks;
  return (rb * tr_rows(s.bits) + j / P) * s.stride + (cb * P + j % P) * sb;
}
// result layout of one workgroup: word d of thread t in iteration it at [(it * 3 + d) * 256 + t];
// thread t works on block it * 16 + t / 16 as group lane t % 16
inline size_t tr_out_words(const TrShape& s) { return (size_t)s.iters * 3 * kThreads; }
// the reference, one bit at a time from the image's bytes
inline uint32_t tr_expected_word(const TrShape& s, const uint8_t* image, int it, int d, int t) {
  if (d >= tr_words(s.bits)) return 0;
  const int b = it * 16 + t / 16, i = t % 16;
  uint32_t w = 0;
  for (int bit = 0; bit < 32; ++bit) {
    const int pos = d * 32 + bit, q = pos / s.bits, k = pos % s.bits;
    int j, e;
    tr_src(s.bits, i, q, &j, &e);
    const int src = e * s.bits + k;
    w |= (uint32_t)((image[tr_addr(s, b, j) + src / 8] >> (src % 8)) & 1u) << bit;
  }
  return w;
}
// The image: element c of row r is its own position mixed to the element width - 16-bit: the
// element's index in the image (13 bits) under 3 hash bits; 8-bit: (r % 16) << 4 | c % 16,
// distinct within any block; 6- and 4-bit elements cannot all differ within a block of 256, so
// theirs differ along every row and every column ((5 r + 3 c + r / 16) mod 2^bits, with 2 (c / 8)
// more bits for 6) - xored per block-sized tile with a hash. Bytes no slot covers are hash bytes.
inline std::vector<uint8_t> tr_make_image(int bits, int rows, int stride, uint32_t seed) {
  std::vector<uint8_t> img((size_t)rows * stride);
  for (size_t i = 0; i < img.size(); ++i) img[i] = (uint8_t)h32(seed + (uint32_t)i * 0x9E3779B9u);
  TrShape s;
  if (!tr_shape(bits, rows, stride, &s)) return img;
  const int E = tr_elems(bits), sb = tr_slot_bytes(bits), cols = s.width / sb * E;
  for (int r = 0; r < rows; ++r)
    for (int c = 0; c < cols; ++c) {
      const uint32_t tile = h32(seed ^ (uint32_t)((r / 16) * 64 + c / 16 + 1));
      uint32_t v;
      if (bits == 16) v = (uint32_t)((r * cols + c) & 0x1FFF) | (tile & 0xE000u);
      else if (bits == 8) v = (uint32_t)(((r & 15) << 4) | (c & 15)) ^ (tile & 0xFFu);
      else if (bits == 6) v = (uint32_t)((5 * r + 3 * c + r / 16 + 16 * ((c >> 3) & 3)) & 63) ^ (tile & 63u);
      else v = (uint32_t)((5 * r + 3 * c + r / 16) & 15) ^ (tile & 15u);
      const size_t base = (size_t)r * stride + (size_t)(c / E) * sb;
      for (int k = 0; k < bits; ++k) {
        const int pos = (c % E) * bits + k;
        uint8_t& byte = img[base + pos / 8];
        byte = (uint8_t)((byte & ~(1u << (pos % 8))) | (((v >> k) & 1u) << (pos % 8)));
      }
    }
  return img;
}

// ------------------------------------------------------------------ sfu
constexpr int kSfuExp = 0, kSfuLog = 1, kSfuRcp = 2, kSfuRsq = 3, kSfuSqrt = 4, kSfuSin = 5, kSfuCos = 6, kSfuOps = 7;
inline const char* sfu_name(int op) {
  static const char* const n[kSfuOps] = {"v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32"};
  return op >= 0 && op < kSfuOps ? n[op] : "?";
}
// The bound D on the distance of a result from its bracket, per instruction; kSfuNoBound =
// judged for consistency only. Source of every value: profiles/wave/README.md.
constexpr uint32_t kSfuNoBound = ~0u;
// exp, log, rcp, rsq, sqrt: measured, the largest distance over the whole input list is 0 (every
// result is one of the two neighbours of the true value); sine, cosine: measured 9, not a claim
// in steps, so consistency only.
constexpr uint32_t kSfuBound[kSfuOps] = {0, 0, 0, 0, 0, kSfuNoBound, kSfuNoBound};

inline float f32_of(uint32_t u) {
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline uint32_t bits_of(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
inline bool normal_bits(uint32_t u) {
  const uint32_t e = (u >> 23) & 0xFFu;
  return e != 0 && e != 0xFF;
}
inline long double sfu_true(int op, float xf) {
  const long double x = xf, two_pi = 2.0L * 3.14159265358979323846264338327950288L;
  switch (op) {
    case kSfuExp: return exp2l(x);
    case kSfuLog: return log2l(x);
    case kSfuRcp: return 1.0L / x;
    case kSfuRsq: return 1.0L / sqrtl(x);
    case kSfuSqrt: return sqrtl(x);
    case kSfuSin: return sinl(two_pi * x);
    default: return cosl(two_pi * x);
  }
}
// normal in, normal out, away from overflow and underflow; sine and cosine: revolutions in
// [-256, 256] whose true result is at least 2^-20 in magnitude (nearer a zero the error of
// the instruction is absolute and a distance in steps says nothing)
inline bool sfu_in_domain(int op, uint32_t bits) {
  if (!normal_bits(bits)) return false;
  const float x = f32_of(bits), ax = std::fabs(x);
  const float lo = std::ldexp(1.0f, -120), hi = std::ldexp(1.0f, 120);
  switch (op) {
    case kSfuExp: return ax <= 120.0f;
    case kSfuLog: return x >= lo && x <= hi && x != 1.0f;
    case kSfuRcp: return ax >= lo && ax <= hi;
    case kSfuRsq:
    case kSfuSqrt: return x >= lo && x <= hi;
    default: return ax <= 256.0f && fabsl(sfu_true(op, x)) >= ldexpl(1.0L, -20);
  }
}
struct SfuList {
  std::vector<uint32_t> x;  // input bits; the exact cases are x[exact_from ..]
  size_t exact_from = 0;
};
// every fp32 in the domain whose low 16 bits are zero; the 2^12 floats on each side of 1.0;
// the exact cases (exp: integers; log, rcp: powers of two; sqrt: n^2 for n = 1 .. 4096 and
// powers of 4; rsq: powers of 4; sine, cosine: none)
inline SfuList sfu_inputs(int op) {
  SfuList L;
  auto add = [&](uint32_t b) {
    if (sfu_in_domain(op, b)) L.x.push_back(b);
  };
  for (uint32_t h = 0; h < 65536u; ++h) add(h << 16);
  for (uint32_t k = 1; k <= 4096u; ++k) add(0x3F800000u - k), add(0x3F800000u + k);
  L.exact_from = L.x.size();
  if (op == kSfuExp)
    for (int k = -120; k <= 120; ++k)
      if (k) add(bits_of((float)k));
  if (op == kSfuLog || op == kSfuRcp)
    for (int k = -120; k <= 120; ++k) add(bits_of(std::ldexp(1.0f, k)));
  if (op == kSfuSqrt)
    for (uint32_t n = 1; n <= 4096u; ++n) add(bits_of((float)(n * n)));
  if (op == kSfuSqrt || op == kSfuRsq)
    for (int k = -60; k <= 60; ++k) add(bits_of(std::ldexp(1.0f, 2 * k)));
  return L;
}
// the two neighbouring fp32 values with lo <= true <= hi (lo == hi when the result is exact)
inline void sfu_bracket(int op, uint32_t xbits, uint32_t* lo, uint32_t* hi) {
  const long double t = sfu_true(op, f32_of(xbits));
  const float f = (float)t;
  if ((long double)f == t) *lo = *hi = bits_of(f);
  else if ((long double)f < t) *lo = bits_of(f), *hi = bits_of(std::nextafterf(f, INFINITY));
  else *hi = bits_of(f), *lo = bits_of(std::nextafterf(f, -INFINITY));
}
// ordered-integer space: a monotone map of fp32 bit patterns onto unsigned integers
NTM_HD inline uint32_t ordered(uint32_t u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
// steps outside [lo, hi]; 0 inside
NTM_HD inline uint32_t sfu_distance(uint32_t y, uint32_t lo, uint32_t hi) {
  const uint32_t oy = ordered(y), ol = ordered(lo), oh = ordered(hi);
  return oy < ol ? ol - oy : oy > oh ? oy - oh : 0u;
}
// the digest: thread t folds the result words of inputs t, t + 256, .. in order, the workgroup
// adds the mixed per-thread values
NTM_HD inline uint64_t digest_step(uint64_t acc, uint32_t word) { return (acc ^ word) * 0x100000001B3ull; }
NTM_HD inline uint64_t digest_mix(uint64_t acc, uint32_t t) {
  uint64_t z = acc + 0x9E3779B97F4A7C15ull * (t + 1u);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
constexpr uint64_t kDigestInit = 0xCBF29CE484222325ull;
inline uint64_t sfu_digest_of(const uint32_t* y, size_t n) {
  uint64_t sum = 0;
  for (uint32_t t = 0; t < (uint32_t)kThreads; ++t) {
    uint64_t acc = kDigestInit;
    for (size_t i = t; i < n; i += kThreads) acc = digest_step(acc, y[i]);
    sum += digest_mix(acc, t);
  }
  return sum;
}
struct SfuDistance {  // what the compare kernel reports; initialise with distance_init
  uint32_t max_d, max_index;  // largest distance and the smallest index that has it
  uint32_t beyond;            // results further than the bound
  uint32_t first_beyond;      // smallest index of one; all ones = none
};
inline void distance_init(SfuDistance& d) { d.max_d = 0, d.max_index = ~0u, d.beyond = 0, d.first_beyond = ~0u; }

// ------------------------------------------------------------------ valu
// v_bitop3_b32: bit i of the result = bit ((a_i << 2) | (b_i << 1) | c_i) of the 8-entry table
NTM_HD inline uint32_t bitop3_expected(uint32_t a, uint32_t b, uint32_t c, uint32_t table) {
  uint32_t r = 0;
  for (int i = 0; i < 32; ++i) {
    const uint32_t idx = (((a >> i) & 1u) << 2) | (((b >> i) & 1u) << 1) | ((c >> i) & 1u);
    r |= ((table >> idx) & 1u) << i;
  }
  return r;
}
// fp32 -> bf16, round to nearest even, in integers (finite inputs)
NTM_HD inline uint32_t bf16_rne(uint32_t f) { return (f + 0x7FFFu + ((f >> 16) & 1u)) >> 16; }
NTM_HD inline uint32_t cvt_pk_expected(uint32_t lo, uint32_t hi) { return (bf16_rne(lo) & 0xFFFFu) | (bf16_rne(hi) << 16); }
// inputs of the conversion: every rounding boundary of bf16 (the tie, one below, one above, for
// both parities of the kept mantissa's last bit and every kept mantissa's low 3 bits) in the
// binades 2^-100, 2^-1, 2^0, 2^1, 2^100 and both signs, the largest finite values that round to
// finite, then hashed words whose result is finite
inline bool cvt_finite(uint32_t f) { return ((bf16_rne(f) >> 7) & 0xFFu) != 0xFFu; }
inline std::vector<uint32_t> cvt_inputs(uint32_t seed, size_t hashed) {
  std::vector<uint32_t> v;
  for (int e : {27, 126, 127, 128, 227})
    for (uint32_t sign = 0; sign < 2; ++sign)
      for (uint32_t m = 0; m < 128u; m += (m < 8 || m >= 120) ? 1 : 17)
        for (uint32_t low : {0x0000u, 0x0001u, 0x7FFFu, 0x8000u, 0x8001u, 0xFFFFu})
          v.push_back((sign << 31) | ((uint32_t)e << 23) | (m << 16) | low);
  v.push_back(0x7F7F7FFFu), v.push_back(0xFF7F7FFFu), v.push_back(0x7F7F0000u);
  for (uint32_t i = 0; v.size() % 2 || hashed; ++i) {
    const uint32_t w = h32(seed + 0x51u + i * 0x9E3779B9u);
    if (!cvt_finite(w) || !normal_bits(w)) continue;
    v.push_back(w);
    if (hashed) --hashed;
  }
  return v;
}
constexpr int kValuBitop = 0, kValuCvt = 1;

// ------------------------------------------------------------------ record, verdict, messages
// One per workgroup of a sweep launch; the kernel writes hw_id .. wg and digest[] with plain
// stores, bad .. got stay as the host zeroed them unless a compare fails.
struct Record {
  uint32_t hw_id, xcc_id;
  uint8_t simd[kWaves];
  uint32_t magic, wg;
  uint32_t bad;         // result words that differ from the expected table
  uint32_t first;       // 0 = none; else the complement of the smallest index in the table of one
  uint32_t expected, got;
  uint32_t pad;
  uint64_t digest[kSfuOps];  // sfu only
};
static_assert(sizeof(Record) == 96, "one 96-byte record per workgroup");

// word index of a family's table -> what the message names
// lane: index = op * 256 + t; ldstr: per form f, (it * 3 + d) * 256 + t after the forms before;
// valu: table * 256 + t for bitop3, then the conversion's words
struct Where {
  unsigned xcc, se, sh, cu, simd;
};
inline Where where_of(const Record& r, unsigned thread) {
  const cus::CuId id = cus::decode(r.hw_id, r.xcc_id);
  return Where{id.xcc, id.se, id.sh, id.cu, (unsigned)(r.simd[(thread / 64) & 3] & 3u)};
}
inline std::string hex32(uint32_t v) {
  char b[16];
  std::snprintf(b, sizeof b, "0x%08x", v);
  return b;
}
// "gpu2: wave lane row_shr:3 bound_ctrl:0: xcd 1 se 0 sh 0 cu 4 simd 2 lane 19: expected 0x...,
// got 0x..., bad bits 0x00000400" - `what` is the op and its control, `unit` "lane" or "element"
inline std::string failure_message(int gpu, int family, const std::string& what, const Where& w, const char* unit,
                                   unsigned index, uint32_t expected, uint32_t got) {
  std::string m = "gpu" + std::to_string(gpu) + ": wave " + family_name(family) + " " + what + ": xcd " +
                  std::to_string(w.xcc) + " se " + std::to_string(w.se) + " sh " + std::to_string(w.sh) + " cu " +
                  std::to_string(w.cu) + " simd " + std::to_string(w.simd) + " " + unit + " " + std::to_string(index) +
                  ": expected " + hex32(expected) + ", got " + hex32(got) + ", bad bits " + hex32(expected ^ got);
  if (m.size() > 199) m.resize(199);
  return m;
}
inline std::string lane_failure(int gpu, const Record& r) {
  const unsigned idx = ~r.first, t = idx % kThreads;
  return failure_message(gpu, kFamLane, lane_op_name(lane_op((int)(idx / kThreads))), where_of(r, t), "lane", t % 64,
                         r.expected, r.got);
}
inline std::string indexed_failure(int gpu, int family, const std::string& what, const Record& r) {
  const unsigned idx = ~r.first;
  return failure_message(gpu, family, what, where_of(r, idx % kThreads), "element", idx, r.expected, r.got);
}

// "gpu2: wave sfu v_exp_f32: xcd 1 se 0 sh 0 cu 4 simd 2 element 17 input 0x3f800000: expected
// 0x..., got 0x..., bad bits 0x..." - what the second launch found: `rec` is the record of the
// workgroup that ran again on the CU, expected the word of a workgroup on another CU
inline std::string sfu_failure(int gpu, int op, const Record& rec, uint32_t index, uint32_t input, uint32_t expected,
                               uint32_t got) {
  const Where w = where_of(rec, index % kThreads);
  std::string m = "gpu" + std::to_string(gpu) + ": wave sfu " + sfu_name(op) + ": xcd " + std::to_string(w.xcc) + " se " +
                  std::to_string(w.se) + " sh " + std::to_string(w.sh) + " cu " + std::to_string(w.cu) + " simd " +
                  std::to_string(w.simd) + " element " + std::to_string(index) + " input " + hex32(input) + ": expected " +
                  hex32(expected) + ", got " + hex32(got) + ", bad bits " + hex32(expected ^ got);
  if (m.size() > 199) m.resize(199);
  return m;
}
// the line when the second launch did not show the difference again
inline std::string sfu_digest_failure(int gpu, int op, const Record& rec, uint64_t want, const char* why) {
  const Where w = where_of(rec, 0);
  return "gpu" + std::to_string(gpu) + ": wave sfu " + sfu_name(op) + ": xcd " + std::to_string(w.xcc) + " se " +
         std::to_string(w.se) + " sh " + std::to_string(w.sh) + " cu " + std::to_string(w.cu) + ": digest " +
         cus::hex(rec.digest[op]) + " differs from " + cus::hex(want) + " of the other workgroups (" + why + ")";
}

// the digest most workgroups agree on (ties: the smallest)
inline uint64_t majority_digest(const std::vector<Record>& recs, int op) {
  std::map<uint64_t, size_t> votes;
  for (auto& r : recs)
    if (r.magic == kMagic) ++votes[r.digest[op]];
  uint64_t best = 0;
  size_t n = 0;
  for (auto& kv : votes)
    if (kv.second > n) best = kv.first, n = kv.second;
  return best;
}

}  // namespace wave
}  // namespace ntm
