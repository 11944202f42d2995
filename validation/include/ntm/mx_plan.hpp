// K7 (MX block-scaled matrix check) host side: the element formats of the
// f8f6f4 matrix instruction, the packers, the two input generators, the
// exactness bound, a host reference for small shapes, the mismatch record and
// the failure message. Pure C++ - no HIP - so the Job, the kernels' header
// (ntm/mx_gemm.hpp) and a CPU-only test program share it.
//
// C[M x N] (fp32) = A[M x K] * B[N x K]^T with A and B in one MX element
// format, row-major packed, and one E8M0 scale byte per 32 consecutive k of a
// row: SA[M][K/32], SB[N][K/32], value 2^(byte - 127).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

// hash32 also runs in the K11 kernels (ntm/mxq.hpp)
#if defined(__HIPCC__)
#define NTM_MX_HD __host__ __device__
#else
#define NTM_MX_HD
#endif

namespace ntm {
namespace mx {

// ---- the formats, by the instruction's cbsz / blgp codes
constexpr int kFmtE4M3 = 0, kFmtE5M2 = 1, kFmtE2M3 = 2, kFmtE3M2 = 3, kFmtE2M1 = 4;
constexpr int kFormats = 5;
constexpr int kBlock = 32;       // k per scale byte
constexpr int kScaleBias = 127;  // E8M0: 2^(byte - 127); byte 255 is NaN
constexpr int kTile = 128;       // M, N and K are multiples of this

struct Format {
  const char* name;
  int bits;       // per element: 8, 6 or 4
  int exp_bits;
  int man_bits;
  int bias;
  int one_point_five;  // the code of 1.5
};
constexpr Format kFormatTable[kFormats] = {
    {"e4m3", 8, 4, 3, 7, 0x3C},  {"e5m2", 8, 5, 2, 15, 0x3E}, {"e2m3", 6, 2, 3, 1, 0x0C},
    {"e3m2", 6, 3, 2, 3, 0x0E},  {"e2m1", 4, 2, 1, 1, 0x03},
};

inline bool format_ok(int fmt) { return fmt >= 0 && fmt < kFormats; }
inline int format_bits(int fmt) { return kFormatTable[fmt].bits; }
inline int format_codes(int fmt) { return 1 << kFormatTable[fmt].bits; }
inline const char* format_name(int fmt) { return format_ok(fmt) ? kFormatTable[fmt].name : "?"; }

// e4m3: 0x7F / 0xFF are NaN; e5m2: exponent 31 is inf / NaN (0x7C-0x7F,
// 0xFC-0xFF). The 6- and 4-bit formats have no non-finite code.
inline bool is_nonfinite(int fmt, int code) {
  if (fmt == kFmtE4M3) return (code & 0x7F) == 0x7F;
  if (fmt == kFmtE5M2) return (code & 0x7C) == 0x7C;
  return false;
}

// value = mant * 2^exp2, exactly; mant carries the sign.
struct Decoded {
  int mant;
  int exp2;
};
inline Decoded decode(int fmt, int code) {
  const Format& f = kFormatTable[fmt];
  const int m = code & ((1 << f.man_bits) - 1);
  const int e = (code >> f.man_bits) & ((1 << f.exp_bits) - 1);
  const int s = (code >> (f.bits - 1)) & 1;
  Decoded d;
  if (e == 0) {
    d.mant = m;
    d.exp2 = 1 - f.bias - f.man_bits;
  } else {
    d.mant = m | (1 << f.man_bits);
    d.exp2 = e - f.bias - f.man_bits;
  }
  if (s) d.mant = -d.mant;
  return d;
}
// The format's quantum: every finite value is an integer multiple of 2^quantum_exp.
inline int quantum_exp(int fmt) { return 1 - kFormatTable[fmt].bias - kFormatTable[fmt].man_bits; }
// value / 2^quantum_exp as an integer
inline int64_t quanta(int fmt, int code) {
  const Decoded d = decode(fmt, code);
  return (int64_t)d.mant * ((int64_t)1 << (d.exp2 - quantum_exp(fmt)));
}
inline int64_t max_quanta(int fmt) {
  int64_t m = 0;
  for (int c = 0; c < format_codes(fmt); ++c)
    if (!is_nonfinite(fmt, c) && quanta(fmt, c) > m) m = quanta(fmt, c);
  return m;
}

// ---- the exactness bound: with K products of at most max_quanta^2 product
// quanta each, scaled by at most 2^(2W) over the smallest scale of the dot
// product, every partial sum in every order is an integer below 2^24 times one
// power of two, so fp32 accumulation never rounds.
inline uint64_t dense_worst_sum(int fmt, int K, int W) {
  const uint64_t q = (uint64_t)max_quanta(fmt);
  return (uint64_t)K * q * q << (2 * W);
}
inline bool dense_exact(int fmt, int K, int W) {
  if (!format_ok(fmt) || K <= 0 || W < 0 || W > 8) return false;
  const uint64_t q = (uint64_t)max_quanta(fmt);
  if (q * q >= (1ull << 24)) return false;
  return dense_worst_sum(fmt, K, W) < (1ull << 24);
}
// The largest W in 0 .. 3 for which the dense run is exact; -1 when none is.
inline int dense_max_spread(int fmt, int K) {
  for (int W = 3; W >= 0; --W)
    if (dense_exact(fmt, K, W)) return W;
  return -1;
}

inline bool shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && M % kTile == 0 && N % kTile == 0 && K % kTile == 0;
}

// ---- packing. Row-major; a row of K elements takes K * bits / 8 bytes.
// FP8: one byte per value. FP4: two per byte, low nibble first. FP6: the codes
// of a row as one little-endian bit string, 32 values in 24 bytes.
inline size_t row_bytes(int fmt, int K) { return (size_t)K * format_bits(fmt) / 8; }

inline void pack_row(int fmt, const uint8_t* codes, int K, uint8_t* out) {
  const int bits = format_bits(fmt);
  std::memset(out, 0, row_bytes(fmt, K));
  for (int k = 0; k < K; ++k) {
    const unsigned c = codes[k] & ((1u << bits) - 1);
    const size_t bit = (size_t)k * bits;
    out[bit >> 3] |= (uint8_t)(c << (bit & 7));
    if ((bit & 7) + bits > 8) out[(bit >> 3) + 1] |= (uint8_t)(c >> (8 - (bit & 7)));
  }
}
inline int unpack_code(int fmt, const uint8_t* row, int k) {
  const int bits = format_bits(fmt);
  const size_t bit = (size_t)k * bits;
  unsigned v = row[bit >> 3] >> (bit & 7);
  if ((bit & 7) + bits > 8) v |= (unsigned)row[(bit >> 3) + 1] << (8 - (bit & 7));
  return (int)(v & ((1u << bits) - 1));
}

// ---- the generators: K4's counter hash (hbm_pattern.hpp HASH) of a word
// index, one stream per array.
NTM_MX_HD inline uint32_t hash32(uint64_t seed, uint32_t stream, uint64_t idx) {
  const uint64_t w = ((uint64_t)stream << 32) + idx;
  const uint64_t s = seed + (uint64_t)stream * 0x9E3779B97F4A7C15ull;
  uint32_t x = (uint32_t)w + (uint32_t)s;
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x ^= (uint32_t)(w >> 32) * 0x9E3779B9u;
  return x;
}
constexpr uint32_t kStreamA = 1, kStreamB = 2, kStreamSA = 3, kStreamSB = 4, kStreamBaseA = 5,
                   kStreamBaseB = 6;

struct Inputs {
  int fmt = 0, M = 0, N = 0, K = 0;
  std::vector<uint8_t> a, b;    // packed rows
  std::vector<uint8_t> sa, sb;  // [M][K/32], [N][K/32]
};

// A finite code from a hash word: every code of the format, a non-finite one
// moved to a finite one by its top exponent bit.
inline int finite_code(int fmt, uint32_t h) {
  int c = (int)((h >> 8) & (uint32_t)(format_codes(fmt) - 1));
  if (is_nonfinite(fmt, c)) c ^= 0x40;
  return c;
}

constexpr int kBaseSpread = 65;  // row / column base exponents in -32 .. 32

// Dense: hashed codes (different streams for A and B), scale byte = a base per
// row (127 - 32 .. 127 + 32) + a hashed delta in 0 .. W per k-block. With
// dense_exact() every result is exact and, unless it is zero, a normal fp32
// between 2^-100 and 2^100 for e2m1 / e2m3.
inline Inputs make_dense(int fmt, int M, int N, int K, uint64_t seed, int W) {
  Inputs in;
  in.fmt = fmt, in.M = M, in.N = N, in.K = K;
  const size_t rb = row_bytes(fmt, K);
  const int KB = K / kBlock;
  in.a.assign((size_t)M * rb, 0);
  in.b.assign((size_t)N * rb, 0);
  in.sa.assign((size_t)M * KB, 0);
  in.sb.assign((size_t)N * KB, 0);
  std::vector<uint8_t> codes((size_t)K);
  auto fill = [&](std::vector<uint8_t>& data, std::vector<uint8_t>& scale, int rows,
                  uint32_t s_data, uint32_t s_scale, uint32_t s_base) {
    for (int r = 0; r < rows; ++r) {
      for (int k = 0; k < K; ++k) codes[k] = (uint8_t)finite_code(fmt, hash32(seed, s_data, (uint64_t)r * K + k));
      pack_row(fmt, codes.data(), K, data.data() + (size_t)r * rb);
      const int base = kScaleBias - 32 + (int)((hash32(seed, s_base, (uint64_t)r) >> 8) % kBaseSpread);
      for (int kb = 0; kb < KB; ++kb)
        scale[(size_t)r * KB + kb] =
            (uint8_t)(base + (int)((hash32(seed, s_scale, (uint64_t)r * KB + kb) >> 8) % (uint32_t)(W + 1)));
    }
  };
  fill(in.a, in.sa, M, kStreamA, kStreamSA, kStreamBaseA);
  fill(in.b, in.sb, N, kStreamB, kStreamSB, kStreamBaseB);
  return in;
}

// Decode sweep: row i of A holds code i mod 2^bits (a non-finite one moved to
// a finite one) at k = decode_position(i, K) and zeros elsewhere; B is 1.5
// everywhere. `window` 0 .. 14 selects the A scale bytes 17 * window ..
// 17 * window + 16 (15 windows cover 0 .. 254); B's byte puts the combined
// exponent at -8 .. 8. One non-zero product per dot product.
constexpr int kDecodeWindows = 15;
inline int decode_position(int i, int K) {
  return (37 * (i % 128) + 11 * (i / 128)) % 128 + 128 * ((i / 128) % (K / 128));
}
inline Inputs make_decode(int fmt, int M, int N, int K, int window) {
  Inputs in;
  in.fmt = fmt, in.M = M, in.N = N, in.K = K;
  const size_t rb = row_bytes(fmt, K);
  const int KB = K / kBlock;
  window = ((window % kDecodeWindows) + kDecodeWindows) % kDecodeWindows;
  in.a.assign((size_t)M * rb, 0);
  in.b.assign((size_t)N * rb, 0);
  in.sa.assign((size_t)M * KB, 0);
  in.sb.assign((size_t)N * KB, (uint8_t)(246 - 17 * window));
  std::vector<uint8_t> codes((size_t)K);
  for (int i = 0; i < M; ++i) {
    std::fill(codes.begin(), codes.end(), (uint8_t)0);
    int c = i & (format_codes(fmt) - 1);
    if (is_nonfinite(fmt, c)) c ^= 0x40;
    codes[decode_position(i, K)] = (uint8_t)c;
    pack_row(fmt, codes.data(), K, in.a.data() + (size_t)i * rb);
    for (int kb = 0; kb < KB; ++kb) in.sa[(size_t)i * KB + kb] = (uint8_t)(17 * window + (i + 5 * kb) % 17);
  }
  std::fill(codes.begin(), codes.end(), (uint8_t)kFormatTable[fmt].one_point_five);
  for (int j = 0; j < N; ++j) pack_row(fmt, codes.data(), K, in.b.data() + (size_t)j * rb);
  return in;
}

// ---- the host reference (small shapes): every product in integer quanta, the
// k-blocks shifted to the smallest combined scale of the dot product, summed
// in 128 bits, then one conversion to fp32 (exact below 2^24, else nearest
// even). Returns false when a sum cannot be held (a scale spread above 60).
inline bool host_reference(const Inputs& in, std::vector<uint32_t>& c_bits) {
  const int fmt = in.fmt, M = in.M, N = in.N, K = in.K, KB = K / kBlock;
  const size_t rb = row_bytes(fmt, K);
  std::vector<int64_t> qa((size_t)M * K), qb((size_t)N * K);
  for (int i = 0; i < M; ++i)
    for (int k = 0; k < K; ++k) qa[(size_t)i * K + k] = quanta(fmt, unpack_code(fmt, in.a.data() + i * rb, k));
  for (int j = 0; j < N; ++j)
    for (int k = 0; k < K; ++k) qb[(size_t)j * K + k] = quanta(fmt, unpack_code(fmt, in.b.data() + j * rb, k));
  c_bits.assign((size_t)M * N, 0);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      int smin = 1 << 20, smax = 0;
      for (int kb = 0; kb < KB; ++kb) {
        const int s = in.sa[(size_t)i * KB + kb] + in.sb[(size_t)j * KB + kb];
        smin = s < smin ? s : smin;
        smax = s > smax ? s : smax;
      }
      if (smax - smin > 60) return false;
      __int128 acc = 0;
      for (int kb = 0; kb < KB; ++kb) {
        int64_t p = 0;
        for (int k = kb * kBlock; k < (kb + 1) * kBlock; ++k) p += qa[(size_t)i * K + k] * qb[(size_t)j * K + k];
        const int s = in.sa[(size_t)i * KB + kb] + in.sb[(size_t)j * KB + kb];
        acc += (__int128)p * ((__int128)1 << (s - smin));
      }
      const bool neg = acc < 0;
      unsigned __int128 mag = neg ? (unsigned __int128)(-acc) : (unsigned __int128)acc;
      // fold to 64 bits keeping a sticky bit, so the double below rounds once at most
      int shift = 0;
      while (mag >> 53) {
        mag = (mag >> 1) | (mag & 1);
        ++shift;
      }
      const double v = std::ldexp((double)(uint64_t)mag, shift + smin - 2 * kScaleBias + 2 * quantum_exp(fmt));
      const float f = (float)(neg ? -v : v);
      std::memcpy(&c_bits[(size_t)i * N + j], &f, 4);
    }
  return true;
}

// ---- the mismatch record mx_compare_kernel fills. Touched only on a
// mismatch. Initialise with mismatch_init().
struct Mismatch {
  uint64_t count;        // 32-bit words that differ
  uint64_t first_index;  // smallest index of one; all ones = none
  uint32_t expected;
  uint32_t got;
};
static_assert(sizeof(Mismatch) == 24, "Mismatch is three 8-byte words");
inline void mismatch_init(Mismatch& m) {
  m.count = 0;
  m.first_index = ~0ull;
  m.expected = m.got = 0;
}

inline std::string hex32(uint32_t v) {
  char b[16];
  std::snprintf(b, sizeof b, "0x%08x", v);
  return b;
}

// "gpu3: mx e2m1 dense: 1 bad element(s), first at row 5 col 7: expected
// 0x41200000, got 0x41200001" - one line under 200 characters (the termination
// message cuts there). `mode` is "dense" or "decode"; N is C's row length.
inline std::string failure_message(int gpu, int fmt, const char* mode, const Mismatch& m, int N) {
  const uint64_t n = N > 0 ? (uint64_t)N : 1;
  return "gpu" + std::to_string(gpu) + ": mx " + format_name(fmt) + " " + mode + ": " +
         std::to_string((unsigned long long)m.count) + " bad element(s), first at row " +
         std::to_string((unsigned long long)(m.first_index / n)) + " col " +
         std::to_string((unsigned long long)(m.first_index % n)) + ": expected " + hex32(m.expected) +
         ", got " + hex32(m.got);
}

}  // namespace mx
}  // namespace ntm
