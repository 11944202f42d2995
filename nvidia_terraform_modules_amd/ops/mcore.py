"""K10 on the host, in numpy: the formats of the matrix-core check (fp64, fp32, fp16 and int8
MFMA, 2:4-sparse bf16 and int8 SMFMAC), the 2:4 packers, the exactness bound, the two input
generators and an exact reference.

``tests/test_mcore_cpu.py`` pins this module to ``validation/include/ntm/mcore_plan.hpp``
(same bytes, same result bits) through a stand-alone program. Arrays, all row-major:

* ``a`` [M, K] and ``b`` [N, K] in the format's element type: float64, float32, float16,
  int8; bf16 as its uint16 bit patterns;
* a sparse A as ``a`` = Ac [M, K/2] (the two kept values of each group of four consecutive k,
  in k order) and ``ai`` [M, K/4] uint8, ``p0 | p1 << 2`` with ``p0 < p1`` the kept positions;
* C = A @ B.T as bit patterns: uint64 for f64, uint32 otherwise.
"""
from __future__ import annotations

import numpy as np

from .mx import _hash_words

MCORE_FORMATS = ("f64", "f32", "f16", "i8", "sp_bf16", "sp_i8")
MCORE_TILE = 128
MCORE_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
MCORE_DECODE_ROWS = 256
MCORE_F16_DECODE_CODES = 61442          # 61440 normal codes and the two zeros
MCORE_DECODE_SEED = 0x4B3A
# (element dtype, element bytes, accumulator bytes, accumulator bits P, sparse, integer, cap)
_TABLE = {"f64": (np.float64, 8, 8, 53, False, False, 21), "f32": (np.float32, 4, 4, 24, False, False, 7),
          "f16": (np.float16, 2, 4, 24, False, False, 7), "i8": (np.int8, 1, 4, 31, False, True, 8),
          "sp_bf16": (np.uint16, 2, 4, 24, True, False, 7), "sp_i8": (np.int8, 1, 4, 31, True, True, 8)}
_PAIR_BYTES = np.asarray([p0 | p1 << 2 for p0, p1 in MCORE_PAIRS], dtype=np.uint8)


def mcore_format_id(fmt) -> int:
    if isinstance(fmt, str):
        if fmt not in MCORE_FORMATS:
            raise ValueError(f"unknown matrix-core format {fmt!r}; one of {MCORE_FORMATS}")
        return MCORE_FORMATS.index(fmt)
    if isinstance(fmt, (int, np.integer)) and not isinstance(fmt, bool) and 0 <= int(fmt) < len(MCORE_FORMATS):
        return int(fmt)
    raise ValueError(f"unknown matrix-core format {fmt!r}; one of {MCORE_FORMATS} or 0 .. 5")


def mcore_format(fmt) -> dict:
    """The format table's row: name, dtype, elem_bytes, acc_bytes, acc_bits, sparse, integer, cap_abits."""
    name = MCORE_FORMATS[mcore_format_id(fmt)]
    keys = ("dtype", "elem_bytes", "acc_bytes", "acc_bits", "sparse", "integer", "cap_abits")
    return {"name": name, **dict(zip(keys, _TABLE[name]))}


def mcore_shape_ok(M: int, N: int, K: int) -> bool:
    return min(M, N, K) > 0 and M % MCORE_TILE == 0 and N % MCORE_TILE == 0 and K % MCORE_TILE == 0


def _max_magnitude(f: dict, abits: int) -> int:
    return 128 if f["integer"] and abits >= 8 else 2**abits - 1


def mcore_exact(fmt, K: int, abits: int) -> bool:
    """True when Kp * (2^abits - 1)^2 < 2^P (Kp = K, or K / 2 for a sparse A; int8 with abits
    8 is its full range, magnitude 128): every partial sum in every order is an exact integer
    times one power of two, so the check needs no tolerance."""
    f = mcore_format(fmt)
    if K <= 0 or not 1 <= abits <= f["cap_abits"]:
        return False
    kp = K // 2 if f["sparse"] else K
    return kp * _max_magnitude(f, abits) ** 2 < 2 ** f["acc_bits"]


def mcore_max_abits(fmt, K: int) -> int:
    """The largest ``abits`` up to the element format's cap with ``mcore_exact``; 0 if none."""
    return next((a for a in range(mcore_format(fmt)["cap_abits"], 0, -1) if mcore_exact(fmt, K, a)), 0)


# ------------------------------------------------------------------- packing
def mcore_compress(dense: np.ndarray):
    """[rows, K] with at most two non-zeros in every group of four consecutive k ->
    (Ac [rows, K/2], Ai [rows, K/4] uint8). A group with fewer non-zeros keeps its lowest
    free positions too. ValueError on a group with three or four."""
    dense = np.asarray(dense)
    if dense.ndim != 2 or dense.shape[1] % 4:
        raise ValueError("mcore_compress needs a 2-D array with K a multiple of 4")
    grp = dense.reshape(dense.shape[0], -1, 4)
    nz = grp != 0
    if int(nz.sum(axis=2).max(initial=0)) > 2:
        raise ValueError("a group of four holds more than two non-zeros: not 2:4 sparse")
    # kept positions: the non-zeros first, then the lowest zeros; a stable sort does both
    order = np.argsort(~nz, axis=2, kind="stable")[:, :, :2]
    order.sort(axis=2)
    ac = np.take_along_axis(grp, order, axis=2).reshape(dense.shape[0], -1)
    ai = (order[:, :, 0] | order[:, :, 1] << 2).astype(np.uint8)
    return np.ascontiguousarray(ac), ai


def mcore_expand(ac: np.ndarray, ai: np.ndarray) -> np.ndarray:
    """The inverse of ``mcore_compress``: (Ac [rows, K/2], Ai [rows, K/4]) -> [rows, K]."""
    ac, ai = np.asarray(ac), np.asarray(ai)
    if ac.ndim != 2 or ai.ndim != 2 or ac.shape[0] != ai.shape[0] or ac.shape[1] != 2 * ai.shape[1]:
        raise ValueError("mcore_expand needs Ac [rows, K/2] and Ai [rows, K/4]")
    rows, groups = ai.shape
    out = np.zeros((rows, groups, 4), dtype=ac.dtype)
    pair = ac.reshape(rows, groups, 2)
    p0, p1 = (ai & 3).astype(np.int64), ((ai >> 2) & 3).astype(np.int64)
    if np.any(p0 >= p1):
        raise ValueError("an index byte needs p0 < p1")
    np.put_along_axis(out, p0[:, :, None], pair[:, :, 0:1], axis=2)
    np.put_along_axis(out, p1[:, :, None], pair[:, :, 1:2], axis=2)
    return out.reshape(rows, groups * 4)


# ---------------------------------------------------------------- generators
def _bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 values with at most 8 significant bits -> bf16 bit patterns."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def _bf16_values(bits: np.ndarray) -> np.ndarray:
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def _encode(f: dict, ints: np.ndarray, exp: np.ndarray) -> np.ndarray:
    """ints * 2^exp (exp broadcast against ints) in the format's element type."""
    if f["integer"]:
        return ints.astype(np.int8)
    v = np.ldexp(ints.astype(np.float64), np.asarray(exp).astype(np.int64))
    return _bf16_bits(v) if f["name"] == "sp_bf16" else v.astype(f["dtype"])


def _hashed_ints(f: dict, h: np.ndarray, abits: int) -> np.ndarray:
    if f["integer"] and abits >= 8:
        return ((h >> np.uint32(8)) & np.uint32(0xFF)).astype(np.uint8).view(np.int8).astype(np.int64)
    m = _max_magnitude(f, abits)
    return ((h >> np.uint32(8)) % np.uint32(2 * m + 1)).astype(np.int64) - m


def mcore_decode_windows(fmt) -> int:
    """Windows of the decode sweep (at its 256 rows)."""
    return (4, 4, -(-MCORE_F16_DECODE_CODES // MCORE_DECODE_ROWS), 1, 12, 12)[mcore_format_id(fmt)]


def mcore_decode_position(i, K: int):
    """The k (of the dense A) of row i's only non-zero in the decode sweep, before a sparse
    row moves it inside its group of four."""
    return (37 * (i % 128) + 11 * (i // 128)) % 128 + 128 * ((i // 128) % (K // 128))


def mcore_f16_decode_code(n):
    n = np.asarray(n, dtype=np.uint32) % np.uint32(MCORE_F16_DECODE_CODES)
    normal = ((n // np.uint32(30720)) << np.uint32(15)) | (n % np.uint32(30720) + np.uint32(1024))
    zero = (n - np.uint32(61440)) << np.uint32(15)
    return np.where(n >= 61440, zero, normal).astype(np.uint16)


def mcore_make_inputs(kind: str, fmt, M: int, N: int, K: int, seed: int = 0, abits: int | None = None) -> dict:
    """Deterministic inputs of the matrix-core check: dict(a, ai, b, fmt, M, N, K), numpy;
    ``ai`` is None for a dense format.

    ``kind="dense"``: hashed signed integers of ``abits`` bits (default: ``mcore_max_abits``);
    for the float formats every row of A and every column of B is scaled by 2^e, e in
    -8 .. 8; a sparse A has hashed kept values and a hashed pair per group.
    ``kind="decode"``: ``seed`` is the window; row i of A holds one non-zero at
    ``mcore_decode_position`` (a sparse row: in that group, at the position its pair and slot
    give, combination ``(i + window) % 12``), B[j, k] is 2^(((j + k) % 5) - 2), for int8
    ``1 << ((j + k) % 7)``, so a non-zero that meets the wrong k shows. With n = window * M + i the non-zero is: f64 / f32 a hashed sign,
    exponent and full-width fraction; f16 code number n of the normal codes and zeros; int8
    the code n & 255; sp_bf16 sign, fraction and exponent from n."""
    fid = mcore_format_id(fmt)
    f = mcore_format(fid)
    if not mcore_shape_ok(M, N, K):
        raise ValueError("the matrix-core check needs M, N and K to be positive multiples of 128")
    ka = K // 2 if f["sparse"] else K
    ai = None
    if kind == "dense":
        abits = mcore_max_abits(fid, K) if abits is None else abits
        if not 1 <= abits <= f["cap_abits"]:
            raise ValueError(f"abits must be in 1 .. {f['cap_abits']} for {f['name']}")
        ea = ((_hash_words(seed, 13, M) >> np.uint32(8)) % np.uint32(17)).astype(np.int64) - 8
        eb = ((_hash_words(seed, 14, N) >> np.uint32(8)) % np.uint32(17)).astype(np.int64) - 8
        a = _encode(f, _hashed_ints(f, _hash_words(seed, 11, M * ka), abits).reshape(M, ka), ea[:, None])
        b = _encode(f, _hashed_ints(f, _hash_words(seed, 12, N * K), abits).reshape(N, K), eb[:, None])
        if f["sparse"]:
            ai = _PAIR_BYTES[((_hash_words(seed, 15, M * (K // 4)) >> np.uint32(8)) % np.uint32(6)).astype(np.int64)]
            ai = ai.reshape(M, K // 4)
    elif kind == "decode":
        window = int(seed)
        i = np.arange(M)
        n = (window * M + i).astype(np.uint32)
        pos = mcore_decode_position(i, K)
        col = pos
        if f["sparse"]:
            combo, gi = (i + window) % 12, pos // 4
            g = np.arange(K // 4)
            ai = _PAIR_BYTES[(combo[:, None] % 6 + (g[None, :] ^ gi[:, None])) % 6]
            col = 2 * gi + combo // 6
        h1, h2, h3 = (_hash_words(MCORE_DECODE_SEED, st, int(n[-1]) + 1)[n] for st in (16, 17, 18))
        sign = ((h3 >> np.uint32(8)) & np.uint32(1)).astype(np.uint64)
        name = f["name"]
        if name == "f64":
            e = ((h3 >> np.uint32(9)) % np.uint32(601)).astype(np.int64) - 300
            man = ((h1 & np.uint32(0xFFFFF)).astype(np.uint64) << np.uint64(32)) | h2.astype(np.uint64) | np.uint64(1)
            bits = (sign << np.uint64(63)) | ((e + 1023).astype(np.uint64) << np.uint64(52)) | man
            a = np.zeros((M, ka), dtype=np.uint64)
        elif name == "f32":
            e = ((h3 >> np.uint32(9)) % np.uint32(81)).astype(np.int64) - 40
            man = ((h1 >> np.uint32(8)) & np.uint32(0x7FFFFF)) | np.uint32(1)
            bits = (sign.astype(np.uint32) << np.uint32(31)) | ((e + 127).astype(np.uint32) << np.uint32(23)) | man
            a = np.zeros((M, ka), dtype=np.uint32)
        elif name == "f16":
            bits = mcore_f16_decode_code(n)
            a = np.zeros((M, ka), dtype=np.uint16)
        elif name == "sp_bf16":
            e = (((n >> np.uint32(8)) + i.astype(np.uint32)) % np.uint32(17)).astype(np.int64) - 8
            bits = ((((n >> np.uint32(7)) & np.uint32(1)) << np.uint32(15)) | ((e + 127).astype(np.uint32) << np.uint32(7))
                    | (n & np.uint32(127))).astype(np.uint16)
            a = np.zeros((M, ka), dtype=np.uint16)
        else:
            bits = (n & np.uint32(255)).astype(np.uint8)
            a = np.zeros((M, ka), dtype=np.uint8)
        a[i, col] = bits
        a = a if name == "sp_bf16" else a.view(f["dtype"])
        jk = np.arange(N)[:, None] + np.arange(K)[None, :]
        ones = np.ones((N, K), dtype=np.int64)
        b = _encode(f, ones << (jk % 7) if f["integer"] else ones, jk % 5 - 2)
    else:
        raise ValueError(f"unknown matrix-core input kind {kind!r}; 'dense' or 'decode'")
    return {"a": np.ascontiguousarray(a), "ai": ai, "b": np.ascontiguousarray(b), "fmt": fid, "M": M, "N": N, "K": K}


# ----------------------------------------------------------------- reference
def mcore_values(x: np.ndarray, fmt) -> np.ndarray:
    """The elements' values: int64 for the int8 formats, float64 (exact) otherwise."""
    f = mcore_format(fmt)
    if f["integer"]:
        return np.asarray(x).astype(np.int64)
    return (_bf16_values(np.asarray(x)) if f["name"] == "sp_bf16" else np.asarray(x)).astype(np.float64)


def mcore_matmul_bits(a: np.ndarray, b: np.ndarray, fmt, ai: np.ndarray | None = None) -> np.ndarray:
    """C = A @ B.T as the accumulator's bit patterns, [M, N] uint64 (f64) or uint32: an int64
    matmul for the int8 formats, a float64 matmul otherwise, which is exact in every order
    under ``mcore_exact`` (all partial sums of a dot product are integers below 2^53 times
    one power of two) and for the decode sweep (one non-zero product per dot product)."""
    f = mcore_format(fmt)
    va, vb = mcore_values(a, fmt), mcore_values(b, fmt)
    if f["sparse"]:
        if ai is None:
            raise ValueError("a sparse format needs ai")
        va = mcore_expand(va, ai)
    if va.ndim != 2 or vb.ndim != 2 or va.shape[1] != vb.shape[1]:
        raise ValueError("operand shapes do not agree")
    c = va @ vb.T
    if f["integer"]:
        return c.astype(np.int32).view(np.uint32)
    return c.view(np.uint64) if f["acc_bytes"] == 8 else c.astype(np.float32).view(np.uint32)


def mcore_failure_message(gpu: int, fmt, mode: str, count: int, first_index: int, expected: int, got: int,
                          N: int) -> str:
    """The Job's line for a mismatch (``ntm::mc::failure_message``)."""
    f = mcore_format(fmt)
    width = 16 if f["acc_bytes"] == 8 else 8
    return (f"gpu{gpu}: mcore: {f['name']} {mode}: row {first_index // N} col {first_index % N}: "
            f"expected 0x{expected:0{width}x}, got 0x{got:0{width}x}, bad bits 0x{expected ^ got:x}; {count} differ")
