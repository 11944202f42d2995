"""K7 on the host, in numpy: the MX element formats of the f8f6f4 matrix instruction, the
packers, the two input generators, the exactness bound and an exact integer reference.

Written from the formats' definitions (OCP MX: e4m3, e5m2, e2m3, e3m2, e2m1 elements, E8M0
scales, 32 elements per scale), not from ``validation/include/ntm/mx_plan.hpp``;
``tests/test_mx_cpu.py`` pins the two to the same bytes and the same result bits through a
stand-alone program. Arrays:

* ``a`` [M, K*bits/8] / ``b`` [N, K*bits/8] uint8 - row-major packed codes: FP8 one per
  byte, FP4 two per byte (low nibble first), FP6 a row's codes as one little-endian bit
  string (32 values in 24 bytes);
* ``sa`` [M, K/32] / ``sb`` [N, K/32] uint8 - E8M0, value 2^(byte - 127), 255 is NaN;
* C = A @ B.T in fp32, returned as its uint32 bit patterns.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

MX_FORMATS = ("e4m3", "e5m2", "e2m3", "e3m2", "e2m1")      # index = the instruction's format code
MX_BLOCK = 32
MX_TILE = 128
MX_SCALE_BIAS = 127
MX_DECODE_WINDOWS = 15
# (bits, exponent bits, mantissa bits, bias, the code of 1.5)
_LAYOUT = {"e4m3": (8, 4, 3, 7, 0x3C), "e5m2": (8, 5, 2, 15, 0x3E), "e2m3": (6, 2, 3, 1, 0x0C),
           "e3m2": (6, 3, 2, 3, 0x0E), "e2m1": (4, 2, 1, 1, 0x03)}
_GOLDEN = 0x9E3779B97F4A7C15


def mx_format_id(fmt) -> int:
    if isinstance(fmt, str):
        if fmt not in MX_FORMATS:
            raise ValueError(f"unknown MX format {fmt!r}; one of {MX_FORMATS}")
        return MX_FORMATS.index(fmt)
    if isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool) and 0 <= int(fmt) < len(MX_FORMATS):
        return int(fmt)
    raise ValueError(f"unknown MX format {fmt!r}; one of {MX_FORMATS} or 0 .. 4")


def mx_bits(fmt) -> int:
    return _LAYOUT[MX_FORMATS[mx_format_id(fmt)]][0]


def mx_nonfinite_codes(fmt) -> tuple:
    name = MX_FORMATS[mx_format_id(fmt)]
    if name == "e4m3":
        return (0x7F, 0xFF)
    if name == "e5m2":
        return (0x7C, 0x7D, 0x7E, 0x7F, 0xFC, 0xFD, 0xFE, 0xFF)
    return ()


def mx_code_value(fmt, code: int) -> Fraction:
    """The exact value of a finite code."""
    bits, eb, mb, bias, _ = _LAYOUT[MX_FORMATS[mx_format_id(fmt)]]
    m, e, s = code & (2**mb - 1), (code >> mb) & (2**eb - 1), code >> (bits - 1) & 1
    v = Fraction(m, 2**mb) * Fraction(2) ** (1 - bias) if e == 0 else \
        (1 + Fraction(m, 2**mb)) * Fraction(2) ** (e - bias)
    return -v if s else v


def _quantum_exp(fmt) -> int:
    _, _, mb, bias, _ = _LAYOUT[MX_FORMATS[mx_format_id(fmt)]]
    return 1 - bias - mb


def mx_quanta_table(fmt) -> np.ndarray:
    """int64 [2^bits]: each code's value in units of the format's smallest subnormal
    (0 for the non-finite codes, which no generator emits)."""
    f = mx_format_id(fmt)
    unit = Fraction(2) ** _quantum_exp(f)
    bad = mx_nonfinite_codes(f)
    out = []
    for c in range(2 ** mx_bits(f)):
        q = Fraction(0) if c in bad else mx_code_value(f, c) / unit
        assert q.denominator == 1
        out.append(int(q))
    return np.asarray(out, dtype=np.int64)


def mx_worst_sum(fmt, K: int, W: int) -> int:
    q = int(mx_quanta_table(fmt).max())
    return K * q * q * 4**W


def mx_dense_exact(fmt, K: int, W: int) -> bool:
    """True when a dense run of depth ``K`` with scale deltas 0 .. ``W`` is exact in every
    order of fp32 accumulation: K * (max |qa * qb|) * 2^(2W) < 2^24 product quanta."""
    if K <= 0 or not 0 <= W <= 8:
        return False
    return mx_worst_sum(fmt, K, W) < 2**24


def mx_max_spread(fmt, K: int) -> int:
    """The largest W in 0 .. 3 with ``mx_dense_exact``; -1 when there is none."""
    return next((w for w in (3, 2, 1, 0) if mx_dense_exact(fmt, K, w)), -1)


def mx_shape_ok(M: int, N: int, K: int) -> bool:
    return min(M, N, K) > 0 and M % MX_TILE == 0 and N % MX_TILE == 0 and K % MX_TILE == 0


# ------------------------------------------------------------------- packing
def mx_pack(codes: np.ndarray, fmt) -> np.ndarray:
    """uint8 codes [rows, K] (K*bits a multiple of 8; FP6: K a multiple of 4) -> packed
    [rows, K*bits/8]."""
    bits = mx_bits(fmt)
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    if codes.ndim != 2 or (codes.shape[1] * bits) % 8:
        raise ValueError("mx_pack needs a 2-D array whose rows fill whole bytes")
    if int(codes.max(initial=0)) >= 2**bits:
        raise ValueError(f"code out of range for {bits}-bit elements")
    if bits == 8:
        return codes.copy()
    if bits == 4:
        return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)
    # 6 bits: four codes -> three bytes, little-endian bit string
    c = codes.reshape(codes.shape[0], -1, 4).astype(np.uint32)
    word = c[..., 0] | (c[..., 1] << 6) | (c[..., 2] << 12) | (c[..., 3] << 18)
    out = np.stack([word & 0xFF, (word >> 8) & 0xFF, (word >> 16) & 0xFF], axis=-1)
    return out.reshape(codes.shape[0], -1).astype(np.uint8)


def mx_unpack(packed: np.ndarray, fmt) -> np.ndarray:
    """The inverse of ``mx_pack``: packed [rows, bytes] -> uint8 codes [rows, K]."""
    bits = mx_bits(fmt)
    packed = np.ascontiguousarray(packed, dtype=np.uint8)
    if packed.ndim != 2 or (bits == 6 and packed.shape[1] % 3):
        raise ValueError("mx_unpack needs a 2-D array of whole packed groups")
    if bits == 8:
        return packed.copy()
    if bits == 4:
        out = np.empty((packed.shape[0], packed.shape[1] * 2), dtype=np.uint8)
        out[:, 0::2], out[:, 1::2] = packed & 15, packed >> 4
        return out
    p = packed.reshape(packed.shape[0], -1, 3).astype(np.uint32)
    word = p[..., 0] | (p[..., 1] << 8) | (p[..., 2] << 16)
    out = np.stack([(word >> s) & 63 for s in (0, 6, 12, 18)], axis=-1)
    return out.reshape(packed.shape[0], -1).astype(np.uint8)


# ---------------------------------------------------------------- generators
def _hash_words(seed: int, stream: int, n: int) -> np.ndarray:
    """K4's HASH pattern word (ops.reference.hbm_pattern_words) at 64-bit word indices
    (stream << 32) .. + n, with seed + stream * 0x9E3779B97F4A7C15."""
    s = (seed + stream * _GOLDEN) & (2**64 - 1)
    w = np.arange(n, dtype=np.uint64)
    x = (w + np.uint64(s & 0xFFFFFFFF)).astype(np.uint32)
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    return x ^ np.uint32((stream * 0x9E3779B9) & 0xFFFFFFFF)


def _finite(fmt: int, codes: np.ndarray) -> np.ndarray:
    bad = np.isin(codes, np.asarray(mx_nonfinite_codes(fmt), dtype=codes.dtype))
    return np.where(bad, codes ^ 0x40, codes).astype(np.uint8)


def mx_decode_position(i, K: int):
    """The k of row i's only non-zero in the decode sweep."""
    return (37 * (i % 128) + 11 * (i // 128)) % 128 + 128 * ((i // 128) % (K // 128))


def mx_make_inputs(kind: str, fmt, M: int, N: int, K: int, seed: int = 0, W: int = 0) -> dict:
    """Deterministic inputs of the MX check: dict(a, b, sa, sb, fmt, M, N, K), numpy uint8.

    ``kind="dense"``: hashed codes (every finite code of the format; A and B from different
    streams), scale byte = a per-row base in 95 .. 159 plus a hashed delta in 0 .. ``W``
    per k-block. ``kind="decode"``: row i of A holds code ``i mod 2^bits`` at
    ``mx_decode_position(i, K)`` and zeros elsewhere, B is 1.5 everywhere; ``seed`` mod 15
    selects the window of A scale bytes ``17 * window .. 17 * window + 16`` (the 15
    windows cover 0 .. 254), and B's byte keeps the combined exponent in -8 .. 8."""
    f = mx_format_id(fmt)
    if not mx_shape_ok(M, N, K):
        raise ValueError("MX check needs M, N and K to be positive multiples of 128")
    bits, KB = mx_bits(f), K // MX_BLOCK
    mask = 2**bits - 1
    if kind == "dense":
        if not 0 <= W <= 8:
            raise ValueError("W must be in 0 .. 8")

        def side(rows, s_data, s_scale, s_base):
            codes = _finite(f, ((_hash_words(seed, s_data, rows * K) >> np.uint32(8)) & np.uint32(mask))
                            .astype(np.uint8)).reshape(rows, K)
            base = 127 - 32 + (_hash_words(seed, s_base, rows) >> np.uint32(8)) % np.uint32(65)
            delta = (_hash_words(seed, s_scale, rows * KB) >> np.uint32(8)) % np.uint32(W + 1)
            return mx_pack(codes, f), (base[:, None] + delta.reshape(rows, KB)).astype(np.uint8)

        a, sa = side(M, 1, 3, 5)
        b, sb = side(N, 2, 4, 6)
    elif kind == "decode":
        window = seed % MX_DECODE_WINDOWS
        i = np.arange(M)
        codes = np.zeros((M, K), dtype=np.uint8)
        codes[i, mx_decode_position(i, K)] = _finite(f, (i & mask).astype(np.uint8))
        a = mx_pack(codes, f)
        b = mx_pack(np.full((N, K), _LAYOUT[MX_FORMATS[f]][4], dtype=np.uint8), f)
        sa = (17 * window + (i[:, None] + 5 * np.arange(KB)[None, :]) % 17).astype(np.uint8)
        sb = np.full((N, KB), 246 - 17 * window, dtype=np.uint8)
    else:
        raise ValueError(f"unknown MX input kind {kind!r}; 'dense' or 'decode'")
    return {"a": a, "b": b, "sa": sa, "sb": sb, "fmt": f, "M": M, "N": N, "K": K}


# ----------------------------------------------------------------- reference
def mx_matmul_bits(a: np.ndarray, b: np.ndarray, sa: np.ndarray, sb: np.ndarray, fmt) -> np.ndarray:
    """The exact product as fp32 bit patterns, uint32 [M, N]: table decode to integer quanta,
    an integer dot per k-block, the blocks shifted to the smallest combined scale of each
    dot product and summed as integers, then one conversion to fp32 (exact below 2^24)."""
    f = mx_format_id(fmt)
    table = mx_quanta_table(f)
    qa, qb = table[mx_unpack(a, f)], table[mx_unpack(b, f)]
    M, K = qa.shape
    N = qb.shape[0]
    KB = K // MX_BLOCK
    if qb.shape[1] != K or K % MX_BLOCK or sa.shape != (M, KB) or sb.shape != (N, KB):
        raise ValueError("operand and scale shapes do not agree")
    if np.any(sa == 255) or np.any(sb == 255):
        raise ValueError("scale byte 255 is NaN")
    s = sa.astype(np.int64)[:, None, :] + sb.astype(np.int64)[None, :, :]          # [M, N, KB]
    smin = s.min(axis=2)
    shift = s - smin[:, :, None]
    if MX_BLOCK * int(np.abs(qa).max(initial=0)) * int(np.abs(qb).max(initial=0)) >= 2**62:
        raise ValueError("element products too large for int64")
    blocks = [qa[:, kb * MX_BLOCK:(kb + 1) * MX_BLOCK] @ qb[:, kb * MX_BLOCK:(kb + 1) * MX_BLOCK].T
              for kb in range(KB)]
    pmax = max(int(np.abs(p).max(initial=0)) for p in blocks)
    if KB * pmax * 2 ** int(shift.max(initial=0)) < 2**53:
        total = np.zeros((M, N), dtype=np.int64)
        for kb, p in enumerate(blocks):
            total += p << shift[:, :, kb]
        as_double = total.astype(np.float64)
    else:   # wide scale spread: Python integers, then a double that must hold the sum exactly
        total = np.zeros((M, N), dtype=object)
        for kb, p in enumerate(blocks):
            total = total + p.astype(object) * (2 ** shift[:, :, kb].astype(object))
        flat = [int(v) for v in total.ravel()]
        as_double = np.asarray([float(v) for v in flat], dtype=np.float64).reshape(M, N)
        if any(int(d) != v for d, v in zip(as_double.ravel(), flat)):
            raise ValueError("sum has more than 53 significant bits")
    exp = smin - 2 * MX_SCALE_BIAS + 2 * _quantum_exp(f)
    with np.errstate(over="ignore", under="ignore"):
        c = np.ldexp(as_double, exp.astype(np.int64)).astype(np.float32)
    return c.view(np.uint32)
