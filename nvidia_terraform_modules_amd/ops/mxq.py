"""K11 on the host, in numpy: MX quantise / dequantise by the OCP MX v1.0 rules, the generators
of the conversion sweeps, the block-quantise rows and the grid inputs.

Written from the definitions in exact float64 arithmetic (a scaled fp32 is exact in a double;
``np.rint`` rounds half to even), not from the bit arithmetic of
``validation/include/ntm/mxq_plan.hpp``; ``tests/test_mxq_cpu.py`` pins the two to the same
bytes through a stand-alone program.

* A block is 32 consecutive elements of a row; scale byte = clamp(floor(log2(amax)) - emax_elem
  + 127, 1, 254), 127 for an all-zero block.
* code = RNE(x * 2^(127 - byte)) in the element format, ties to the even code, subnormals kept,
  finite overflow saturating to the largest finite value.
* dequantise: code value * 2^(byte - 127) in fp32; bf16 is that rounded RNE.

Outside the judged domain: an fp32 denormal input counts as zero, Inf / NaN inputs saturate, a
dequantised value below the smallest normal fp32 becomes a signed zero, one above the largest
becomes infinity, and the NaN / Inf codes of e4m3 / e5m2 dequantise as if they were finite.

fp32 / bf16 data crosses as bit patterns: uint32 (a bf16 widened: bits << 16) and uint16.
"""
from __future__ import annotations

import numpy as np

from .mx import (MX_BLOCK, MX_FORMATS, MX_SCALE_BIAS, _LAYOUT, _hash_words, mx_bits, mx_format_id,  # noqa: F401
                 mx_make_inputs, mx_nonfinite_codes, mx_pack, mx_unpack)

MXQ_EMAX = {"e4m3": 8, "e5m2": 15, "e2m3": 2, "e3m2": 4, "e2m1": 2}
MXQ_MAX_CODE = {"e4m3": 0x7E, "e5m2": 0x7B, "e2m3": 0x1F, "e3m2": 0x1F, "e2m1": 0x07}
MXQ_DTYPES = ("float32", "bfloat16")
MXQ_ROUNDING = ("rne", "stochastic")
MXQ_PAD = 0x7FC0DEAD
_S_ROWS, _S_ROW_BASE, _S_TOP = 12, 13, 14


def _name(fmt) -> str:
    return MX_FORMATS[mx_format_id(fmt)]


def mxq_shape_ok(R: int, K: int, ldx: int) -> bool:
    return R > 0 and K > 0 and K % MX_BLOCK == 0 and ldx >= K


def mxq_value_table(fmt) -> np.ndarray:
    """float64 [2^bits]: the value every code decodes to (the NaN / Inf codes as if finite)."""
    bits, eb, mb, bias, _ = _LAYOUT[_name(fmt)]
    c = np.arange(2**bits)
    m, e, s = c & (2**mb - 1), (c >> mb) & (2**eb - 1), c >> (bits - 1)
    v = np.where(e == 0, m / 2**mb * 2.0 ** (1 - bias), (1 + m / 2**mb) * 2.0 ** (e - bias))
    return np.where(s == 1, -v, v)


def mxq_scale_bytes(xbits: np.ndarray, fmt) -> np.ndarray:
    """uint32 fp32 bits [R, K] -> uint8 [R, K/32]."""
    x = np.asarray(xbits, dtype=np.uint32)
    amax = (x & np.uint32(0x7FFFFFFF)).reshape(x.shape[0], -1, MX_BLOCK).max(axis=2)
    e = (amax >> np.uint32(23)).astype(np.int64)            # 127 + floor(log2(amax)) for a normal amax
    return np.where(e == 0, MX_SCALE_BIAS, np.clip(e - MXQ_EMAX[_name(fmt)], 1, 254)).astype(np.uint8)


def mxq_quantize_codes(xbits, scale_bytes, fmt) -> np.ndarray:
    """Element-wise: fp32 bits and a scale byte per element -> uint8 codes."""
    name = _name(fmt)
    bits, eb, mb, bias, _ = _LAYOUT[name]
    x = np.asarray(xbits, dtype=np.uint32)
    byte = np.broadcast_to(np.asarray(scale_bytes), x.shape).astype(np.int64)
    E = (x >> np.uint32(23)) & np.uint32(0xFF)
    mags = np.abs(mxq_value_table(name)[:MXQ_MAX_CODE[name] + 1])          # ascending, code = index
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.abs(x.view(np.float32).astype(np.float64))
    v = np.where(E == 0, 0.0, np.where(E == 255, mags[-1], np.ldexp(np.where(E == 255, 0.0, v), MX_SCALE_BIAS - byte)))
    _, ex = np.frexp(v)                                                      # v = f * 2^ex, f in [0.5, 1)
    qe = np.maximum(ex - 1, 1 - bias) - mb                                   # the exponent of the quantum at v
    r = np.minimum(np.ldexp(np.rint(np.ldexp(v, -qe)), qe), mags[-1])
    code = np.searchsorted(mags, r)
    assert np.array_equal(mags[code], r)
    return (code | ((x >> np.uint32(31)).astype(np.int64) << (bits - 1))).astype(np.uint8)


def mxq_quantize_bits(xbits: np.ndarray, fmt, scales: np.ndarray | None = None):
    """fp32 bits [R, K] -> (packed uint8 [R, K*bits/8], scales uint8 [R, K/32]) as ``mx_gemm``
    takes them. ``scales`` given: use these bytes (the element-level form) instead of the rule."""
    x = np.asarray(xbits, dtype=np.uint32)
    if x.ndim != 2 or x.shape[1] % MX_BLOCK or not x.shape[1]:
        raise ValueError("MX quantise needs a 2-D array with K a positive multiple of 32")
    s = mxq_scale_bytes(x, fmt) if scales is None else np.asarray(scales, dtype=np.uint8).reshape(x.shape[0], -1)
    codes = mxq_quantize_codes(x, np.repeat(s, MX_BLOCK, axis=1), fmt)
    return mx_pack(codes, fmt), s


def bf16_round_bits(f32bits: np.ndarray) -> np.ndarray:
    b = np.asarray(f32bits, dtype=np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)).astype(np.uint16)


def mxq_dequantize_bits(packed: np.ndarray, scales: np.ndarray, fmt, dtype: str = "float32") -> np.ndarray:
    """-> fp32 bits uint32 [R, K], or bf16 bits uint16 for ``dtype="bfloat16"``."""
    if dtype not in MXQ_DTYPES:
        raise ValueError(f"dtype must be one of {MXQ_DTYPES}")
    codes = mx_unpack(packed, fmt)
    byte = np.repeat(np.asarray(scales, dtype=np.uint8), MX_BLOCK, axis=1).astype(np.int64)
    v = np.ldexp(mxq_value_table(fmt)[codes], byte - MX_SCALE_BIAS)
    neg = (codes >> (mx_bits(fmt) - 1)).astype(bool)
    mag = np.abs(v)
    mag = np.where(mag < 2.0**-126, 0.0, np.where(mag >= 2.0**128, np.inf, mag))
    out = mag.astype(np.float32).view(np.uint32) | (neg.astype(np.uint32) << np.uint32(31))
    return bf16_round_bits(out) if dtype == "bfloat16" else out


# ------------------------------------------------------------------------------ generators
def mxq_down_points(fmt) -> np.ndarray:
    """fp32 bits of the down sweep's points at scale 2^0: per pair of adjacent magnitudes lower,
    midpoint - 1 ulp, midpoint, midpoint + 1 ulp, upper; then max finite, max + half a step and
    its two neighbours, 2 * max; then all of them negated."""
    name = _name(fmt)
    mags = np.abs(mxq_value_table(name)[:MXQ_MAX_CODE[name] + 1]).astype(np.float32)
    pts = []
    for lo, hi in zip(mags[:-1], mags[1:]):
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2).view(np.uint32)
        pts += [lo.view(np.uint32), mid - 1, mid, mid + 1, hi.view(np.uint32)]
    over = np.float32(np.float64(mags[-1]) + (np.float64(mags[-1]) - np.float64(mags[-2])) / 2).view(np.uint32)
    pts += [mags[-1].view(np.uint32), over - 1, over, over + 1, np.float32(2 * mags[-1]).view(np.uint32)]
    p = np.asarray(pts, dtype=np.uint32)
    return np.concatenate([p, p | np.uint32(0x80000000)])


def mxq_down_bytes(fmt) -> list:
    """The scale bytes of the fp32 down sweep: those at which every point stays a normal fp32,
    thinned to both ends and every byte with byte % 11 == 1."""
    _, _, mb, bias, _ = _LAYOUT[_name(fmt)]
    lo, hi = 1 - bias - mb - 2, MXQ_EMAX[_name(fmt)] + 1
    ok = [b for b in range(1, 255) if 127 + lo + b - 127 >= 1 and 127 + hi + b - 127 <= 254]
    return [b for i, b in enumerate(ok) if i in (0, len(ok) - 1) or b % 11 == 1]


def _scaled(pts: np.ndarray, d: int) -> np.ndarray:
    return np.where(pts & np.uint32(0x7FFFFFFF), pts + np.uint32((d << 23) & 0xFFFFFFFF), pts).astype(np.uint32)


def mxq_down_sweep(fmt):
    """-> (x uint32 [blocks, 32], scales uint8 [blocks]): ``mxq_down_points`` at every byte of
    ``mxq_down_bytes``, a block's values all scaled by its byte."""
    pts = mxq_down_points(fmt)
    pts = np.concatenate([pts, np.zeros(-pts.size % MX_BLOCK, np.uint32)]).reshape(-1, MX_BLOCK)
    bs = mxq_down_bytes(fmt)
    x = np.concatenate([_scaled(pts, b - MX_SCALE_BIAS) for b in bs])
    return x, np.repeat(np.asarray(bs, dtype=np.uint8), pts.shape[0])


def mxq_bf16_binades(fmt) -> list:
    _, _, mb, bias, _ = _LAYOUT[_name(fmt)]
    return sorted({MXQ_EMAX[_name(fmt)], 0, -bias, 1 - bias - mb - 2})


def mxq_down_bf16(fmt):
    """The exhaustive bf16 source sweep -> (x uint32 [blocks, 32] = bf16 bits << 16, scales)."""
    i = np.arange(256, dtype=np.uint32)
    xs, ss = [], []
    for e in range(1, 255):
        for j in mxq_bf16_binades(fmt):
            byte = e - j
            if 1 <= byte <= 254:
                xs.append((((i >> np.uint32(7)) << np.uint32(31)) | np.uint32(e << 23) | ((i & np.uint32(127)) << np.uint32(16))).reshape(8, 32))
                ss += [byte] * 8
    zero = np.where(np.arange(32) & 1, np.uint32(0x80000000), np.uint32(0)).astype(np.uint32)[None, :]
    for byte in (1, 127, 254):
        xs.append(zero)
        ss.append(byte)
    return np.concatenate(xs).astype(np.uint32), np.asarray(ss, dtype=np.uint8)


def mxq_up_sweep(fmt):
    """-> (packed [254, len*bits/8], scales [254, len/32], kept bool [254, len]): row r holds every
    code (padded with code 0 to 32) at scale byte r + 1; ``kept`` marks the judged cells: a finite
    code whose result is zero or a normal fp32. A cell that is not kept holds code 0 instead."""
    n = 2 ** mx_bits(fmt)
    K = max(n, MX_BLOCK)
    codes = np.zeros((254, K), np.uint8)
    codes[:, :n] = np.arange(n, dtype=np.uint8)
    scales = np.repeat(np.arange(1, 255, dtype=np.uint8)[:, None], K // MX_BLOCK, axis=1)
    v = np.abs(np.ldexp(mxq_value_table(fmt)[codes], scales[:, :1].astype(np.int64) - MX_SCALE_BIAS))
    kept = (v == 0) | ((v >= 2.0**-126) & (v < 2.0**128))
    kept &= ~np.isin(codes, np.asarray(mx_nonfinite_codes(fmt), dtype=np.uint8))
    kept[:, n:] = False
    return mx_pack(np.where(kept, codes, 0).astype(np.uint8), fmt), scales, kept


def mxq_block_rows(fmt, R: int, K: int, ldx: int | None = None, seed: int = 0, bf16: bool = False) -> np.ndarray:
    """uint32 fp32 bits [R, ldx] (padding = ``MXQ_PAD``): hashed signs and fractions, a per-row
    base exponent, one element per block in the top binade; by (block index) % 16: 3 all zero,
    5 a single non-zero, 7 tiny (the byte clamps at 1), 9 amax a power of two."""
    ldx = K if ldx is None else ldx
    if not mxq_shape_ok(R, K, ldx):
        raise ValueError("MX quantise needs K a positive multiple of 32 and ldx >= K")
    KB = K // MX_BLOCK
    h = _hash_words(seed, _S_ROWS, R * K).reshape(R, KB, MX_BLOCK)
    base = (64 + (_hash_words(seed, _S_ROW_BASE, R) >> np.uint32(8)) % np.uint32(127)).astype(np.int64)[:, None, None]
    top = ((_hash_words(seed, _S_TOP, R * KB) >> np.uint32(8)) % np.uint32(32)).reshape(R, KB, 1)
    special = (np.arange(R * KB) % 16).reshape(R, KB, 1)
    is_top = np.arange(MX_BLOCK)[None, None, :] == top
    low3 = ((h >> np.uint32(24)) & np.uint32(7)).astype(np.int64)
    e = np.where(is_top, base, base - low3)
    e = np.where(special == 7, 1 + low3 % MXQ_EMAX[_name(fmt)], e)
    frac = np.where((special == 9) & is_top, 0, h & np.uint32(0x7FFFFF)).astype(np.uint32)
    v = ((h >> np.uint32(31)) << np.uint32(31)) | (e.astype(np.uint32) << np.uint32(23)) | frac
    v = np.where((special == 3) | ((special == 5) & ~is_top), 0, v).astype(np.uint32)
    if bf16:
        v &= np.uint32(0xFFFF0000)
    out = np.full((R, ldx), MXQ_PAD, dtype=np.uint32)
    out[:, :K] = v.reshape(R, K)
    return out


def mxq_grid(fmt, packed: np.ndarray, scales: np.ndarray, seed: int = 0):
    """Generator (d) for one operand of ``mx_make_inputs("dense", ...)``: in every block without
    an element in the format's top binade one hashed element has its exponent raised to it.
    -> (packed, scales, x uint32 [rows, K]) with ``mxq_quantize_bits(x) == (packed, scales)``."""
    name = _name(fmt)
    bits, eb, mb, bias, _ = _LAYOUT[name]
    codes = mx_unpack(packed, fmt)
    R, K = codes.shape
    KB = K // MX_BLOCK
    top_field = MXQ_MAX_CODE[name] >> mb
    c3 = codes.reshape(R, KB, MX_BLOCK).copy()
    has = (((c3 >> mb) & (2**eb - 1)) == top_field).any(axis=2)
    pick = ((_hash_words(seed, _S_TOP, R * KB) >> np.uint32(8)) % np.uint32(32)).reshape(R, KB)
    r, kb = np.nonzero(~has)
    old = c3[r, kb, pick[r, kb]].astype(np.int64)
    sign = old & (1 << (bits - 1))
    mag = np.minimum((top_field << mb) + (old & (2**mb - 1)), MXQ_MAX_CODE[name])
    c3[r, kb, pick[r, kb]] = (sign | mag).astype(np.uint8)
    p = mx_pack(c3.reshape(R, K), fmt)
    s = np.asarray(scales, dtype=np.uint8).copy()
    return p, s, mxq_dequantize_bits(p, s, fmt)


def mxq_make_inputs(kind: str, fmt, R: int = 0, K: int = 0, ldx: int | None = None, seed: int = 0,
                    bf16: bool = False, N: int = 0, W: int = 0) -> dict:
    """Deterministic inputs of the MX quantise check, numpy.

    ``down`` / ``down_bf16``: dict(x [blocks, 32] fp32 bits, scales [blocks]) for ``mxq_cvt``;
    ``up``: dict(packed, scales, kept); ``block``: dict(x [R, ldx]); ``grid``: both operands of
    ``mx_make_inputs("dense", fmt, R, N, K, seed, W)`` through ``mxq_grid``: dict(a, sa, xa, b,
    sb, xb)."""
    if kind == "down":
        x, s = mxq_down_sweep(fmt)
        return {"x": x, "scales": s}
    if kind == "down_bf16":
        x, s = mxq_down_bf16(fmt)
        return {"x": x, "scales": s}
    if kind == "up":
        p, s, k = mxq_up_sweep(fmt)
        return {"packed": p, "scales": s, "kept": k}
    if kind == "block":
        return {"x": mxq_block_rows(fmt, R, K, ldx, seed, bf16)}
    if kind == "grid":
        d = mx_make_inputs("dense", fmt, R, N, K, seed=seed, W=W)
        a, sa, xa = mxq_grid(fmt, d["a"], d["sa"], seed)
        b, sb, xb = mxq_grid(fmt, d["b"], d["sb"], seed + 1)
        return {"a": a, "sa": sa, "xa": xa, "b": b, "sb": sb, "xb": xb, "fmt": mx_format_id(fmt), "M": R, "N": N, "K": K}
    raise ValueError(f"unknown MX quantise input kind {kind!r}")


def mxq_failure_message(gpu: int, fmt, sub: str, count: int, first_index: int, expected: int, got: int,
                        row_words: int, elem_bits: int) -> str:
    """The Job's line (``mxq_plan.hpp`` failure_message)."""
    w = row_words or 1
    return (f"gpu{gpu}: mxq {_name(fmt)} {sub}: {count} bad word(s), first at row {first_index // w} element "
            f"{first_index % w * 32 // elem_bits}: expected 0x{expected:08x}, got 0x{got:08x}, bad bits 0x{expected ^ got:08x}")
