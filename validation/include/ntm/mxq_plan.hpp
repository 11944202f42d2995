// K11 (device-side MX quantise / dequantise) host side: the scale rule, the
// element rounding and the inverse as integer bit arithmetic, the generators
// of the conversion sweeps, the block-quantise rows and the grid inputs, and
// the failure message. Pure C++ - no HIP - on top of ntm/mx_plan.hpp (formats,
// packers, hash32, Mismatch). The functions marked NTM_MXQ_HD are the ones the
// reference kernels of ntm/mxq.hpp run on the device too.
//
// Semantics (OCP MX v1.0): a block is 32 consecutive elements of a row and has
// one E8M0 scale byte = clamp(floor(log2(amax)) - emax_elem + 127, 1, 254), 127
// for an all-zero block. code = RNE(x * 2^(127 - byte)) in the element format,
// ties to the even code, subnormals kept, a finite magnitude above the largest
// finite value saturating to it. Dequantise: code value * 2^(byte - 127) in
// fp32; bf16 output is that value rounded RNE.
//
// Outside the judged domain, and what this arithmetic does there: an fp32
// denormal input counts as zero; Inf / NaN inputs saturate like any large
// magnitude; a dequantised value below the smallest normal fp32 becomes a
// signed zero and one above the largest becomes infinity; the NaN / Inf codes
// of e4m3 / e5m2 dequantise as if they were finite codes.
#pragma once

#include <algorithm>

#include "ntm/mx_plan.hpp"

#if defined(__HIPCC__)
#define NTM_MXQ_HD __host__ __device__
#else
#define NTM_MXQ_HD
#endif

namespace ntm {
namespace mxq {

constexpr int kF32 = 0, kBf16 = 1;  // source / destination dtype
constexpr int kRne = 0, kStochastic = 1;
constexpr uint32_t kStreamSr = 11, kStreamRows = 12, kStreamRowBase = 13, kStreamTop = 14;

// floor(log2(largest finite value))
constexpr int kEmaxElem[mx::kFormats] = {8, 15, 2, 4, 2};
inline int emax_elem(int fmt) { return kEmaxElem[fmt]; }
// the largest finite magnitude code: e4m3 0x7E (0x7F is NaN), e5m2 0x7B, else all ones
constexpr int kMaxCode[mx::kFormats] = {0x7E, 0x7B, 0x1F, 0x1F, 0x07};

inline bool shape_ok(int R, int K, int ldx) { return R > 0 && K > 0 && K % mx::kBlock == 0 && ldx >= K; }

// ---- the arithmetic, on bit patterns only
// amax_bits: the largest (bits & 0x7fffffff) of the block
NTM_MXQ_HD inline int scale_byte(uint32_t amax_bits, int emax) {
  const int e = (int)(amax_bits >> 23);
  if (e == 0) return mx::kScaleBias;  // zero (or fp32 denormals only)
  const int b = e - emax;
  return b < 1 ? 1 : b > 254 ? 254 : b;
}

// fp32 bits -> the code of x * 2^(127 - byte): bits / mb / bias describe the
// format, max_code its largest finite magnitude.
NTM_MXQ_HD inline int quantize_code(int bits, int mb, int bias, int max_code, uint32_t x, int byte) {
  const int sign = (int)(x >> 31) << (bits - 1);
  const int E = (int)((x >> 23) & 0xFF);
  if (E == 0) return sign;
  if (E == 255) return sign | max_code;
  const uint32_t sig = (x & 0x7FFFFFu) | 0x800000u;
  const int e = E - byte;  // unbiased exponent of the scaled value
  const int emin = 1 - bias;
  int shift = 23 - mb, base = 0;
  if (e >= emin) {
    if (e - emin >= (1 << (bits - 1 - mb))) return sign | max_code;
    base = (e - emin) << mb;
  } else {
    shift += emin - e;
    if (shift >= 25) return sign;
  }
  uint32_t q = sig >> shift;
  const uint32_t rem = sig & ((1u << shift) - 1), half = 1u << (shift - 1);
  if (rem > half || (rem == half && (q & 1))) ++q;
  const int mag = base + (int)q;  // the hidden bit of q raises the exponent field by one
  return sign | (mag > max_code ? max_code : mag);
}

// code -> fp32 bits of its value * 2^(byte - 127)
NTM_MXQ_HD inline uint32_t dequantize_bits(int bits, int mb, int bias, int code, int byte) {
  const uint32_t sign = (uint32_t)((code >> (bits - 1)) & 1) << 31;
  const int m = code & ((1 << mb) - 1);
  const int ef = (code >> mb) & ((1 << (bits - 1 - mb)) - 1);
  int E;
  uint32_t frac;
  if (ef) {
    E = ef - bias + byte;
    frac = (uint32_t)m << (23 - mb);
  } else {
    if (!m) return sign;
    int p = mb - 1;
    while (!((m >> p) & 1)) --p;
    E = p + 1 - bias - mb + byte;
    frac = ((uint32_t)m << (23 - p)) & 0x7FFFFFu;
  }
  if (E <= 0) return sign;
  if (E >= 255) return sign | 0x7F800000u;
  return sign | ((uint32_t)E << 23) | frac;
}

NTM_MXQ_HD inline uint16_t f32_to_bf16_rne(uint32_t b) { return (uint16_t)((b + 0x7FFFu + ((b >> 16) & 1u)) >> 16); }

inline int quantize_code(int fmt, uint32_t x, int byte) {
  const mx::Format& f = mx::kFormatTable[fmt];
  return quantize_code(f.bits, f.man_bits, f.bias, kMaxCode[fmt], x, byte);
}
inline uint32_t dequantize_bits(int fmt, int code, int byte) {
  const mx::Format& f = mx::kFormatTable[fmt];
  return dequantize_bits(f.bits, f.man_bits, f.bias, code, byte);
}

// ---- whole rows on the host. x: R rows of ldx fp32 bit patterns (bf16 sources widened).
struct Quantized {
  std::vector<uint8_t> packed, scales;  // [R][K * bits / 8], [R][K / 32]
};
// given != nullptr: the scale bytes to use (the element-level form) instead of the rule
inline Quantized quantize_rows(int fmt, const uint32_t* x, int R, int K, int ldx, const uint8_t* given = nullptr) {
  Quantized q;
  const size_t rb = mx::row_bytes(fmt, K);
  const int KB = K / mx::kBlock;
  q.packed.assign((size_t)R * rb, 0);
  q.scales.assign((size_t)R * KB, 0);
  std::vector<uint8_t> codes((size_t)K);
  for (int r = 0; r < R; ++r) {
    const uint32_t* row = x + (size_t)r * ldx;
    for (int kb = 0; kb < KB; ++kb) {
      uint32_t amax = 0;
      for (int k = 0; k < mx::kBlock; ++k) amax = std::max(amax, row[kb * mx::kBlock + k] & 0x7FFFFFFFu);
      const int byte = given ? given[(size_t)r * KB + kb] : scale_byte(amax, emax_elem(fmt));
      q.scales[(size_t)r * KB + kb] = (uint8_t)byte;
      for (int k = 0; k < mx::kBlock; ++k)
        codes[kb * mx::kBlock + k] = (uint8_t)quantize_code(fmt, row[kb * mx::kBlock + k], byte);
    }
    mx::pack_row(fmt, codes.data(), K, q.packed.data() + (size_t)r * rb);
  }
  return q;
}
// -> fp32 bit patterns [R][K]
inline std::vector<uint32_t> dequantize_rows(int fmt, const uint8_t* packed, const uint8_t* scales, int R, int K) {
  const size_t rb = mx::row_bytes(fmt, K);
  const int KB = K / mx::kBlock;
  std::vector<uint32_t> y((size_t)R * K);
  for (int r = 0; r < R; ++r)
    for (int k = 0; k < K; ++k)
      y[(size_t)r * K + k] =
          dequantize_bits(fmt, mx::unpack_code(fmt, packed + r * rb, k), scales[(size_t)r * KB + k / mx::kBlock]);
  return y;
}

// ---- generators. A sweep is a list of blocks: 32 fp32 bit patterns and one scale byte each.
struct Sweep {
  std::vector<uint32_t> x;      // [blocks][32]
  std::vector<uint8_t> scales;  // [blocks]
  int blocks() const { return (int)scales.size(); }
};

inline std::vector<int> magnitude_codes(int fmt) {  // finite, ascending value: 0 .. kMaxCode
  std::vector<int> c;
  for (int i = 0; i <= kMaxCode[fmt]; ++i) c.push_back(i);
  return c;
}

// (a) conversion sweep, down, fp32 source. Per pair of adjacent magnitudes: lower, the
// midpoint, its two fp32 neighbours, upper; then the saturation points: max finite,
// max + half a step and its two neighbours, 2 * max. Both signs. One block per scale byte
// and 32 values; the bytes used are every byte 1 .. 254 for which every value of the block
// times 2^(byte - 127) is a normal fp32 - thinned to byte % 11 == 1 plus both ends.
inline std::vector<uint32_t> down_points(int fmt) {  // fp32 bits of the unscaled points (byte 127)
  std::vector<uint32_t> pts;
  auto val = [&](int code) { return dequantize_bits(fmt, code, mx::kScaleBias); };
  auto f = [](uint32_t b) { float v; std::memcpy(&v, &b, 4); return v; };
  auto bits = [](float v) { uint32_t b; std::memcpy(&b, &v, 4); return b; };
  const int top = kMaxCode[fmt];
  for (int c = 0; c < top; ++c) {
    const uint32_t lo = val(c), hi = val(c + 1), mid = bits((f(lo) + f(hi)) * 0.5f);  // exact: few bits
    for (uint32_t p : {lo, mid - 1, mid, mid + 1, hi}) pts.push_back(p);
  }
  const float mx_ = f(val(top)), step = mx_ - f(val(top - 1));
  const uint32_t over = bits(mx_ + step * 0.5f);
  for (uint32_t p : {val(top), over - 1, over, over + 1, bits(mx_ * 2.0f)}) pts.push_back(p);
  const size_t n = pts.size();
  for (size_t i = 0; i < n; ++i) pts.push_back(pts[i] | 0x80000000u);
  return pts;
}
inline std::vector<int> down_bytes(int fmt) {
  // a point's fp32 exponent field is 127 + its exponent; the smallest non-zero point is the
  // half of the smallest subnormal, the largest 2 * max: both must stay in 1 .. 254 after scaling
  const mx::Format& f = mx::kFormatTable[fmt];
  const int lo_exp = 1 - f.bias - f.man_bits - 2, hi_exp = emax_elem(fmt) + 1;
  std::vector<int> out;
  for (int b = 1; b <= 254; ++b) {
    const int d = b - mx::kScaleBias;
    if (127 + lo_exp + d < 1 || 127 + hi_exp + d > 254) continue;
    out.push_back(b);
  }
  std::vector<int> thin;
  for (size_t i = 0; i < out.size(); ++i)
    if (i == 0 || i + 1 == out.size() || out[i] % 11 == 1) thin.push_back(out[i]);
  return thin;
}
inline uint32_t scale_f32(uint32_t x, int d) {  // x * 2^d for a zero or a normal x staying normal
  return (x & 0x7FFFFFFFu) ? x + ((uint32_t)d << 23) : x;
}
inline Sweep make_down_sweep(int fmt) {
  Sweep s;
  std::vector<uint32_t> pts = down_points(fmt);
  while (pts.size() % mx::kBlock) pts.push_back(0);
  for (int b : down_bytes(fmt))
    for (size_t i = 0; i < pts.size(); i += mx::kBlock) {
      for (int k = 0; k < mx::kBlock; ++k) s.x.push_back(scale_f32(pts[i + k], b - mx::kScaleBias));
      s.scales.push_back((uint8_t)b);
    }
  return s;
}

// (a) bf16 source, exhaustive: every finite normal bf16 code and +-0. The binades j of the
// scaled value: emax_elem, 0, the subnormal binade (-bias), and two below the smallest
// subnormal's (1 - bias - man_bits - 2). byte = e - j, kept in 1 .. 254. x holds bf16 << 16.
inline std::vector<int> bf16_binades(int fmt) {
  const mx::Format& f = mx::kFormatTable[fmt];
  std::vector<int> j = {emax_elem(fmt), 0, -f.bias, 1 - f.bias - f.man_bits - 2};
  std::sort(j.begin(), j.end());
  j.erase(std::unique(j.begin(), j.end()), j.end());
  return j;
}
inline Sweep make_down_bf16(int fmt) {
  Sweep s;
  for (int e = 1; e <= 254; ++e)
    for (int j : bf16_binades(fmt)) {
      const int byte = e - (127 + j) + 127;  // scaled exponent field e - byte + 127 = 127 + j
      if (byte < 1 || byte > 254) continue;
      for (int blk = 0; blk < 8; ++blk) {
        for (int k = 0; k < mx::kBlock; ++k) {
          const uint32_t i = (uint32_t)(blk * 32 + k);  // sign, mantissa
          s.x.push_back(((i >> 7) << 31) | ((uint32_t)e << 23) | ((i & 127u) << 16));
        }
        s.scales.push_back((uint8_t)byte);
      }
    }
  // +-0 at three scale bytes
  for (int byte : {1, 127, 254}) {
    for (int k = 0; k < mx::kBlock; ++k) s.x.push_back((k & 1) ? 0x80000000u : 0u);
    s.scales.push_back((uint8_t)byte);
  }
  return s;
}

// (b) conversion sweep, up: every finite code x every scale byte 1 .. 254, one row of all
// codes (padded with code 0 to whole blocks) per byte. up_kept() says which cells are judged:
// the result is zero or a normal fp32. A cell that is not kept holds code 0 instead, so every
// word of the result is compared.
inline bool up_kept(int fmt, int code, int byte) {
  if (mx::is_nonfinite(fmt, code)) return false;
  const uint32_t v = dequantize_bits(fmt, code, mx::kScaleBias);
  if (!(v & 0x7FFFFFFFu)) return true;
  const int E = (int)((v >> 23) & 0xFF) + byte - mx::kScaleBias;
  return E >= 1 && E <= 254;
}
inline int up_row_len(int fmt) { return std::max(mx::format_codes(fmt), mx::kBlock); }
struct UpSweep {
  std::vector<uint8_t> packed, scales;  // 254 rows of up_row_len codes; [254][len / 32]
  int R = 254, K = 0;
};
inline UpSweep make_up_sweep(int fmt) {
  UpSweep u;
  u.K = up_row_len(fmt);
  const size_t rb = mx::row_bytes(fmt, u.K);
  std::vector<uint8_t> codes((size_t)u.K, 0);
  u.packed.assign(254 * rb, 0);
  for (int r = 0; r < 254; ++r) {
    for (int c = 0; c < mx::format_codes(fmt); ++c) codes[c] = up_kept(fmt, c, r + 1) ? (uint8_t)c : 0;
    mx::pack_row(fmt, codes.data(), u.K, u.packed.data() + r * rb);
  }
  for (int r = 0; r < 254; ++r)
    for (int kb = 0; kb < u.K / mx::kBlock; ++kb) u.scales.push_back((uint8_t)(r + 1));
  return u;
}

// (c) block quantise rows: fp32 bit patterns [R][ldx] (the padding holds 0x7FC0DEAD, which a
// correct kernel never reads into a result). Row r has a base exponent field 64 .. 190; every
// element is a hashed sign and 23-bit (bf16: 7-bit) fraction with an exponent field of base -
// (0 .. 7); one hashed element per block sits in the top binade. Special blocks, by
// (row * KB + kb) % 16: 3 = all zero, 5 = a single non-zero, 7 = tiny (exponent fields 1 ..
// emax_elem, so the byte clamps at 1), 9 = amax an exact power of two.
constexpr uint32_t kPad = 0x7FC0DEADu;
inline std::vector<uint32_t> make_block_rows(int fmt, int R, int K, int ldx, uint64_t seed, bool bf16) {
  std::vector<uint32_t> x((size_t)R * ldx, kPad);
  const int KB = K / mx::kBlock;
  const uint32_t keep = bf16 ? 0xFFFF0000u : 0xFFFFFFFFu;
  for (int r = 0; r < R; ++r) {
    const int base = 64 + (int)((mx::hash32(seed, kStreamRowBase, (uint64_t)r) >> 8) % 127u);
    for (int kb = 0; kb < KB; ++kb) {
      const uint64_t blk = (uint64_t)r * KB + kb;
      const int special = (int)(blk % 16);
      const int top = (int)((mx::hash32(seed, kStreamTop, blk) >> 8) % 32u);
      for (int k = 0; k < mx::kBlock; ++k) {
        const uint32_t h = mx::hash32(seed, kStreamRows, blk * mx::kBlock + k);
        int e = base - (int)((h >> 24) & 7u);
        uint32_t frac = h & 0x7FFFFFu;
        if (k == top) e = base;
        if (special == 7) e = 1 + (int)((h >> 24) & 7u) % emax_elem(fmt);
        if (special == 9 && k == top) frac = 0;
        uint32_t v = ((h >> 31) << 31) | ((uint32_t)e << 23) | frac;
        if (special == 3 || (special == 5 && k != top)) v = 0;
        x[(size_t)r * ldx + kb * mx::kBlock + k] = v & keep;
      }
    }
  }
  return x;
}

// (d) grid inputs: the dequantised values of one side of mx::make_dense after every block got
// a top-binade element, so that quantising them gives the side's packed bytes and scale bytes
// back exactly. Top binade: the exponent field is the format's largest finite one (e5m2: 30).
// Element (hash % 32) of a block whose elements all lie below it gets its exponent raised.
struct Grid {
  std::vector<uint8_t> packed, scales;  // as mx_gemm takes them
  std::vector<uint32_t> x;              // fp32 bits [rows][K], exact in bf16 too
};
inline bool in_top_binade(int fmt, int code) {
  const mx::Format& f = mx::kFormatTable[fmt];
  const int ef = (code >> f.man_bits) & ((1 << f.exp_bits) - 1);
  return ef == (kMaxCode[fmt] >> f.man_bits);
}
inline Grid make_grid(int fmt, const std::vector<uint8_t>& packed, const std::vector<uint8_t>& scales, int rows,
                      int K, uint64_t seed) {
  Grid g;
  const mx::Format& f = mx::kFormatTable[fmt];
  const size_t rb = mx::row_bytes(fmt, K);
  const int KB = K / mx::kBlock;
  g.packed.assign(packed.size(), 0);
  g.scales = scales;
  std::vector<uint8_t> codes((size_t)K);
  for (int r = 0; r < rows; ++r) {
    for (int k = 0; k < K; ++k) codes[k] = (uint8_t)mx::unpack_code(fmt, packed.data() + r * rb, k);
    for (int kb = 0; kb < KB; ++kb) {
      bool has = false;
      for (int k = 0; k < mx::kBlock; ++k) has = has || in_top_binade(fmt, codes[kb * mx::kBlock + k]);
      if (has) continue;
      uint8_t& c = codes[kb * mx::kBlock + (mx::hash32(seed, kStreamTop, (uint64_t)r * KB + kb) >> 8) % 32u];
      const int low = c & ((1 << f.man_bits) - 1), sign = c & (1 << (f.bits - 1));
      c = (uint8_t)(sign | (((kMaxCode[fmt] >> f.man_bits) << f.man_bits) + low));
      if ((c & (mx::format_codes(fmt) / 2 - 1)) > kMaxCode[fmt]) c = (uint8_t)(sign | kMaxCode[fmt]);
    }
    mx::pack_row(fmt, codes.data(), K, g.packed.data() + r * rb);
  }
  g.x = dequantize_rows(fmt, g.packed.data(), g.scales.data(), rows, K);
  return g;
}

// "gpu3: mxq e2m1 block: 1 bad word(s), first at row 5 element 64: expected 0x00000021, got
// 0x00000031, bad bits 0x00000010" - one line under 200 characters. `sub` is down, up, block,
// scale or e2e; the compared 32-bit words hold elements of `elem_bits` bits and a row has
// `row_words` of them: row and element name the first element the differing word holds (in
// the sweeps the row is the block, or the scale byte - 1 of the up sweep).
inline std::string failure_message(int gpu, int fmt, const char* sub, const mx::Mismatch& m, size_t row_words,
                                   int elem_bits) {
  const uint64_t w = row_words ? row_words : 1;
  return "gpu" + std::to_string(gpu) + ": mxq " + mx::format_name(fmt) + " " + sub + ": " +
         std::to_string((unsigned long long)m.count) + " bad word(s), first at row " +
         std::to_string((unsigned long long)(m.first_index / w)) + " element " +
         std::to_string((unsigned long long)(m.first_index % w * 32 / (uint64_t)elem_bits)) + ": expected " +
         mx::hex32(m.expected) + ", got " + mx::hex32(m.got) + ", bad bits " + mx::hex32(m.expected ^ m.got);
}

}  // namespace mxq
}  // namespace ntm
