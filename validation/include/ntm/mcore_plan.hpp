// K10 (fp64 / fp32 / fp16 / int8 / 2:4-sparse matrix-core check) host side: the format
// table, the 2:4 packers, the exactness bound, the two input generators, a host reference
// for small shapes, the mismatch record and the failure message. Pure C++ - no HIP - so the
// Job, the kernels' header (ntm/mcore.hpp) and a CPU-only test program share it.
//
// C[M x N] = A[M x K] * B[N x K]^T, row-major, M, N and K multiples of 128. A sparse A is
// stored compressed: Ac[M][K/2] holds the two kept values of each group of four consecutive
// k in k order, Ai[M][K/4] one byte per group, p0 | p1 << 2 with p0 < p1 the kept positions.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "ntm/mx_plan.hpp"  // hash32: K4's counter hash

namespace ntm {
namespace mc {

constexpr int kF64 = 0, kF32 = 1, kF16 = 2, kI8 = 3, kSpBf16 = 4, kSpI8 = 5;
constexpr int kFormats = 6;
constexpr int kTile = 128;

struct Format {
  const char* name;
  int elem_bytes;  // of A and B
  int acc_bytes;   // of C
  int acc_bits;    // P: integers below 2^P are exact in the accumulator
  bool sparse;     // A is 2:4 compressed
  bool integer;    // int8 in, int32 out
  int cap_abits;   // the widest operand the element format holds (8 = int8's full range)
};
constexpr Format kFormatTable[kFormats] = {
    {"f64", 8, 8, 53, false, false, 21},    {"f32", 4, 4, 24, false, false, 7},
    {"f16", 2, 4, 24, false, false, 7},     {"i8", 1, 4, 31, false, true, 8},
    {"sp_bf16", 2, 4, 24, true, false, 7},  {"sp_i8", 1, 4, 31, true, true, 8},
};
inline bool format_ok(int fmt) { return fmt >= 0 && fmt < kFormats; }
inline const char* format_name(int fmt) { return format_ok(fmt) ? kFormatTable[fmt].name : "?"; }
inline bool shape_ok(int M, int N, int K) {
  return M > 0 && N > 0 && K > 0 && M % kTile == 0 && N % kTile == 0 && K % kTile == 0;
}
// bytes of one row of A (dense, or Ac), of Ai and of B
inline size_t a_row_bytes(int fmt, int K) {
  return (size_t)(kFormatTable[fmt].sparse ? K / 2 : K) * kFormatTable[fmt].elem_bytes;
}
inline size_t ai_row_bytes(int fmt, int K) { return kFormatTable[fmt].sparse ? (size_t)K / 4 : 0; }
inline size_t b_row_bytes(int fmt, int K) { return (size_t)K * kFormatTable[fmt].elem_bytes; }

// ---- the exactness bound. Operands are integers of magnitude at most 2^abits - 1 (int8
// with abits = 8: its full range, magnitude 128), times one power of two per dot product.
// With Kp products (K dense, K / 2 sparse) below 2^P in sum, every partial sum in every
// order is an exact integer, so no tolerance is needed.
inline uint64_t max_magnitude(int fmt, int abits) {
  return kFormatTable[fmt].integer && abits >= 8 ? 128u : (1ull << abits) - 1;
}
inline bool mcore_exact(int fmt, int K, int abits) {
  if (!format_ok(fmt) || K <= 0 || abits < 1 || abits > kFormatTable[fmt].cap_abits) return false;
  const uint64_t kp = kFormatTable[fmt].sparse ? (uint64_t)K / 2 : (uint64_t)K, m = max_magnitude(fmt, abits);
  return (unsigned __int128)kp * m * m < ((unsigned __int128)1 << kFormatTable[fmt].acc_bits);
}
// The largest exact abits up to the format's cap; 0 when none is.
inline int mcore_max_abits(int fmt, int K) {
  if (!format_ok(fmt)) return 0;
  for (int a = kFormatTable[fmt].cap_abits; a >= 1; --a)
    if (mcore_exact(fmt, K, a)) return a;
  return 0;
}

// ---- 2:4 packing of one row of int32 values (the generators and tests work on integers)
constexpr int kPairs[6][2] = {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}};
inline uint8_t pair_byte(int pair) { return (uint8_t)(kPairs[pair][0] | kPairs[pair][1] << 2); }
// false when a group of four holds more than two non-zeros. A group with fewer keeps the
// lowest free positions as well, so p0 < p1 always.
inline bool compress_2of4(const int32_t* dense, int K, int32_t* ac, uint8_t* ai) {
  for (int g = 0; g < K / 4; ++g) {
    int pos[4], n = 0;
    for (int p = 0; p < 4; ++p)
      if (dense[4 * g + p]) pos[n++] = p;
    if (n > 2) return false;
    for (int p = 0; p < 4 && n < 2; ++p) {
      bool used = false;
      for (int q = 0; q < n; ++q) used = used || pos[q] == p;
      if (!used) pos[n++] = p;
    }
    const int p0 = pos[0] < pos[1] ? pos[0] : pos[1], p1 = pos[0] < pos[1] ? pos[1] : pos[0];
    ac[2 * g] = dense[4 * g + p0];
    ac[2 * g + 1] = dense[4 * g + p1];
    ai[g] = (uint8_t)(p0 | p1 << 2);
  }
  return true;
}
inline void expand_2of4(const int32_t* ac, const uint8_t* ai, int K, int32_t* dense) {
  for (int g = 0; g < K / 4; ++g) {
    for (int p = 0; p < 4; ++p) dense[4 * g + p] = 0;
    dense[4 * g + (ai[g] & 3)] = ac[2 * g];
    dense[4 * g + ((ai[g] >> 2) & 3)] = ac[2 * g + 1];
  }
}

// ---- element encoders: sign, exponent and fraction written as bits, no host half type
inline uint16_t f16_bits(int sign, int exp2, unsigned man10) { return (uint16_t)(sign << 15 | (exp2 + 15) << 10 | man10); }
inline uint16_t bf16_bits(int sign, int exp2, unsigned man7) { return (uint16_t)(sign << 15 | (exp2 + 127) << 7 | man7); }
inline uint32_t f32_bits(int sign, int exp2, uint32_t man23) { return (uint32_t)sign << 31 | (uint32_t)(exp2 + 127) << 23 | man23; }
inline uint64_t f64_bits(int sign, int exp2, uint64_t man52) { return (uint64_t)sign << 63 | (uint64_t)(exp2 + 1023) << 52 | man52; }

// element `idx` of a row-major array of format fmt's elements := v * 2^e (v an integer the
// element format holds exactly; e ignored by the integer formats)
inline void store_int(int fmt, uint8_t* base, size_t idx, int64_t v, int e) {
  if (kFormatTable[fmt].integer) {
    base[idx] = (uint8_t)(int8_t)v;
    return;
  }
  if (fmt == kF64) {
    const double d = std::ldexp((double)v, e);
    std::memcpy(base + idx * 8, &d, 8);
    return;
  }
  const float f = std::ldexp((float)v, e);
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if (fmt == kF32) {
    std::memcpy(base + idx * 4, &u, 4);
    return;
  }
  uint16_t h = (uint16_t)(u >> 16);  // bf16: |v| <= 127 has at most 7 fraction bits
  if (fmt == kF16 && v) {
    const int ex = (int)((u >> 23) & 0xFF) - 127;
    h = f16_bits((int)(u >> 31), ex, (u >> 13) & 0x3FF);
  } else if (fmt == kF16) {
    h = 0;
  }
  std::memcpy(base + idx * 2, &h, 2);
}
// the value of element idx as a double (exact: every element format fits)
inline double load_value(int fmt, const uint8_t* base, size_t idx) {
  if (kFormatTable[fmt].integer) return (double)(int8_t)base[idx];
  if (fmt == kF64) {
    double d;
    std::memcpy(&d, base + idx * 8, 8);
    return d;
  }
  if (fmt == kF32) {
    float f;
    std::memcpy(&f, base + idx * 4, 4);
    return f;
  }
  uint16_t h;
  std::memcpy(&h, base + idx * 2, 2);
  if (fmt == kSpBf16) {
    const uint32_t u = (uint32_t)h << 16;
    float f;
    std::memcpy(&f, &u, 4);
    return f;
  }
  const int s = h >> 15, e = (h >> 10) & 31, m = h & 1023;
  const double v = e ? std::ldexp((double)(m | 1024), e - 25) : std::ldexp((double)m, -24);
  return s ? -v : v;
}

struct Inputs {
  int fmt = 0, M = 0, N = 0, K = 0;
  std::vector<uint8_t> a;   // A, or Ac of a sparse format
  std::vector<uint8_t> ai;  // Ai, empty for a dense format
  std::vector<uint8_t> b;
};
inline Inputs make_empty(int fmt, int M, int N, int K) {
  Inputs in;
  in.fmt = fmt, in.M = M, in.N = N, in.K = K;
  in.a.assign((size_t)M * a_row_bytes(fmt, K), 0);
  in.ai.assign((size_t)M * ai_row_bytes(fmt, K), 0);
  in.b.assign((size_t)N * b_row_bytes(fmt, K), 0);
  return in;
}

constexpr uint32_t kStreamA = 11, kStreamB = 12, kStreamEa = 13, kStreamEb = 14, kStreamIdx = 15,
                   kStreamM1 = 16, kStreamM2 = 17, kStreamM3 = 18;

// a signed integer of abits bits from a hash word
inline int64_t hashed_int(int fmt, uint32_t h, int abits) {
  if (kFormatTable[fmt].integer && abits >= 8) return (int8_t)((h >> 8) & 0xFF);
  const int64_t m = (int64_t)max_magnitude(fmt, abits);
  return (int64_t)((h >> 8) % (uint32_t)(2 * m + 1)) - m;
}
inline int hashed_exp(uint32_t h) { return (int)((h >> 8) % 17u) - 8; }

// Dense: hashed signed integers of abits bits; for the float formats every row of A and
// every column of B is scaled by 2^e, e in -8 .. 8 (one scale per dot product: exactness
// holds and the exponent path is exercised; 127 * 2^8 and 1 * 2^-8 are normal fp16). A
// sparse A has hashed kept values and a hashed pair per group.
inline Inputs make_dense(int fmt, int M, int N, int K, uint64_t seed, int abits) {
  Inputs in = make_empty(fmt, M, N, K);
  const bool sp = kFormatTable[fmt].sparse;
  const int ka = sp ? K / 2 : K;
  for (int i = 0; i < M; ++i) {
    const int e = hashed_exp(mx::hash32(seed, kStreamEa, (uint64_t)i));
    for (int k = 0; k < ka; ++k) {
      const size_t idx = (size_t)i * ka + k;
      store_int(fmt, in.a.data(), idx, hashed_int(fmt, mx::hash32(seed, kStreamA, idx), abits), e);
    }
    for (int g = 0; sp && g < K / 4; ++g) {
      const size_t idx = (size_t)i * (K / 4) + g;
      in.ai[idx] = pair_byte((int)((mx::hash32(seed, kStreamIdx, idx) >> 8) % 6u));
    }
  }
  for (int j = 0; j < N; ++j) {
    const int e = hashed_exp(mx::hash32(seed, kStreamEb, (uint64_t)j));
    for (int k = 0; k < K; ++k) {
      const size_t idx = (size_t)j * K + k;
      store_int(fmt, in.b.data(), idx, hashed_int(fmt, mx::hash32(seed, kStreamB, idx), abits), e);
    }
  }
  return in;
}

// Decode sweep: row i of A holds one non-zero, at k = decode_position(i, K) (for a sparse A:
// in that k's group, at the position the row's pair and slot give), zeros elsewhere. B[j][k]
// is the power of two 2^(((j + k) % 5) - 2) for the float formats and 1 << ((j + k) % 7) for
// int8: it changes with k, so a non-zero that meets the wrong k shows. One non-zero product
// per dot product, so the expected result is that value rescaled.
// With n = window * M + i the non-zero is
//   f64 / f32  a hashed sign, exponent (-300 .. 300 / -40 .. 40) and fraction with the lowest
//              bit set: all 53 / 24 significant bits in use;
//   f16        code number n % 61442 of the 61440 normal codes and the two zeros;
//   i8, sp_i8  the int8 code n & 255;
//   sp_bf16    sign (n >> 7) & 1, fraction n & 127, exponent ((n >> 8) + i) % 17 - 8.
// Sparse rows take combination (i + window) % 12 of the six pairs and the two kept slots;
// the row's other groups step through the pairs from there.
constexpr int kDecodeRows = 256;
constexpr int kF16DecodeCodes = 61442;
constexpr uint64_t kDecodeSeed = 0x4B3Aull;
inline int decode_windows(int fmt) {
  constexpr int w[kFormats] = {4, 4, (kF16DecodeCodes + kDecodeRows - 1) / kDecodeRows, 1, 12, 12};
  return format_ok(fmt) ? w[fmt] : 0;
}
inline int decode_position(int i, int K) {
  return (37 * (i % 128) + 11 * (i / 128)) % 128 + 128 * ((i / 128) % (K / 128));
}
inline uint16_t f16_decode_code(uint32_t n) {
  n %= (uint32_t)kF16DecodeCodes;
  if (n >= 61440u) return (uint16_t)((n - 61440u) << 15);
  return (uint16_t)((n / 30720u) << 15 | (n % 30720u + 1024u));
}
inline Inputs make_decode(int fmt, int M, int N, int K, int window) {
  Inputs in = make_empty(fmt, M, N, K);
  const Format& f = kFormatTable[fmt];
  for (int i = 0; i < M; ++i) {
    const uint32_t n = (uint32_t)window * (uint32_t)M + (uint32_t)i;
    const int pos = decode_position(i, K);
    size_t idx = (size_t)i * K + pos;
    if (f.sparse) {
      const int combo = (i + window) % 12, gi = pos / 4;
      for (int g = 0; g < K / 4; ++g) in.ai[(size_t)i * (K / 4) + g] = pair_byte((combo % 6 + (g ^ gi)) % 6);
      idx = (size_t)i * (K / 2) + 2 * gi + combo / 6;
    }
    const uint32_t h1 = mx::hash32(kDecodeSeed, kStreamM1, n), h2 = mx::hash32(kDecodeSeed, kStreamM2, n),
                   h3 = mx::hash32(kDecodeSeed, kStreamM3, n);
    const int sign = (int)((h3 >> 8) & 1);
    if (fmt == kF64) {
      const uint64_t v = f64_bits(sign, (int)((h3 >> 9) % 601u) - 300, ((uint64_t)(h1 & 0xFFFFFu) << 32 | h2) | 1u);
      std::memcpy(in.a.data() + idx * 8, &v, 8);
    } else if (fmt == kF32) {
      const uint32_t v = f32_bits(sign, (int)((h3 >> 9) % 81u) - 40, ((h1 >> 8) & 0x7FFFFFu) | 1u);
      std::memcpy(in.a.data() + idx * 4, &v, 4);
    } else if (fmt == kF16) {
      const uint16_t v = f16_decode_code(n);
      std::memcpy(in.a.data() + idx * 2, &v, 2);
    } else if (fmt == kSpBf16) {
      const uint16_t v = bf16_bits((int)((n >> 7) & 1), (int)(((n >> 8) + (uint32_t)i) % 17u) - 8, n & 127u);
      std::memcpy(in.a.data() + idx * 2, &v, 2);
    } else {
      in.a[idx] = (uint8_t)(n & 255u);
    }
  }
  for (int j = 0; j < N; ++j)
    for (int k = 0; k < K; ++k)
      store_int(fmt, in.b.data(), (size_t)j * K + k, f.integer ? 1 << ((j + k) % 7) : 1, ((j + k) % 5) - 2);
  return in;
}

// ---- the host reference (small shapes): a double (float formats) or int64 (int8) sum in k
// order, exact under mcore_exact and for the decode sweep, then one conversion to the
// accumulator type. c_bits holds 4- or 8-byte words widened to 64 bits.
inline void host_reference(const Inputs& in, std::vector<uint64_t>& c_bits) {
  const Format& f = kFormatTable[in.fmt];
  const int M = in.M, N = in.N, K = in.K;
  std::vector<double> a((size_t)M * K, 0.0), b((size_t)N * K);
  for (int i = 0; i < M; ++i)
    for (int k = 0; k < K; ++k) {
      if (!f.sparse) {
        a[(size_t)i * K + k] = load_value(in.fmt, in.a.data(), (size_t)i * K + k);
        continue;
      }
      const uint8_t ib = in.ai[(size_t)i * (K / 4) + k / 4];
      const int p = k & 3, slot = p == (ib & 3) ? 0 : p == ((ib >> 2) & 3) ? 1 : -1;
      if (slot >= 0) a[(size_t)i * K + k] = load_value(in.fmt, in.a.data(), (size_t)i * (K / 2) + 2 * (k / 4) + slot);
    }
  for (size_t x = 0; x < b.size(); ++x) b[x] = load_value(in.fmt, in.b.data(), x);
  c_bits.assign((size_t)M * N, 0);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < N; ++j) {
      double acc = 0;
      int64_t iacc = 0;
      for (int k = 0; k < K; ++k) {
        if (f.integer) iacc += (int64_t)a[(size_t)i * K + k] * (int64_t)b[(size_t)j * K + k];
        else acc += a[(size_t)i * K + k] * b[(size_t)j * K + k];
      }
      uint64_t bits = 0;
      if (f.integer) {
        bits = (uint32_t)(int32_t)iacc;
      } else if (f.acc_bytes == 8) {
        std::memcpy(&bits, &acc, 8);
      } else {
        const float v = (float)acc;
        uint32_t u;
        std::memcpy(&u, &v, 4);
        bits = u;
      }
      c_bits[(size_t)i * N + j] = bits;
    }
}

// ---- the mismatch record mcore_compare_kernel fills. Touched only on a mismatch.
struct Mismatch {
  uint64_t count;        // words that differ
  uint64_t first_index;  // smallest index of one; all ones = none
  uint64_t expected;     // the words there (4-byte words zero-extended)
  uint64_t got;
};
static_assert(sizeof(Mismatch) == 32, "Mismatch is four 8-byte words");
inline void mismatch_init(Mismatch& m) {
  m.count = 0;
  m.first_index = ~0ull;
  m.expected = m.got = 0;
}

inline std::string hex_word(uint64_t v, int bytes) {
  char b[24];
  if (bytes == 8) std::snprintf(b, sizeof b, "0x%016llx", (unsigned long long)v);
  else std::snprintf(b, sizeof b, "0x%08llx", (unsigned long long)(v & 0xFFFFFFFFull));
  return b;
}
// "gpu3: mcore: f64 dense: row 5 col 7: expected 0x..., got 0x..., bad bits 0x200; 1 differ"
inline std::string failure_message(int gpu, int fmt, const char* mode, const Mismatch& m, int N) {
  const uint64_t n = N > 0 ? (uint64_t)N : 1;
  const int wb = format_ok(fmt) ? kFormatTable[fmt].acc_bytes : 4;
  char bad[24];
  std::snprintf(bad, sizeof bad, "0x%llx", (unsigned long long)(m.expected ^ m.got));
  return "gpu" + std::to_string(gpu) + ": mcore: " + format_name(fmt) + " " + mode + ": row " +
         std::to_string((unsigned long long)(m.first_index / n)) + " col " +
         std::to_string((unsigned long long)(m.first_index % n)) + ": expected " + hex_word(m.expected, wb) +
         ", got " + hex_word(m.got, wb) + ", bad bits " + bad + "; " + std::to_string((unsigned long long)m.count) +
         " differ";
}

}  // namespace mc
}  // namespace ntm
