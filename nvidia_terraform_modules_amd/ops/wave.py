"""K12 wave data-path and special-function check: the host side in numpy, a mirror of
``validation/include/ntm/wave_paths_plan.hpp`` (the op list of the ``lane`` family and its lane
map, the transposed-read maps and image generator, the ``sfu`` input lists and brackets in
``np.longdouble``, the truth-table evaluator and bf16 rounding). ``tests/test_wave_cpu.py`` pins
the two to equal bytes through a stand-alone program."""
from __future__ import annotations

import numpy as np

WAVE_FAMILIES = ("lane", "ldstr", "sfu", "valu")
WAVE_THREADS, WAVE_LANES = 256, 64
WAVE_OLD, WAVE_ZERO, WAVE_SKIP = -1, -2, -3
WAVE_FAULT_BIT = 1 << 10
WAVE_SFU_OPS = ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32")
# the bound D per instruction; None = judged for consistency only (profiles/wave/README.md)
WAVE_SFU_BOUND = {n: (0 if i < 5 else None) for i, n in enumerate(WAVE_SFU_OPS)}
WAVE_TR_BITS = (16, 8, 4, 6)
WAVE_SWEEP_ROWS = 64


def wave_sweep_stride(bits: int) -> int:
    """Row stride of the per-CU sweep's image: 136 bytes, 144 for the 6-bit form (16-byte aligned)."""
    return 144 if bits == 6 else 136


_M32 = 0xFFFFFFFF


def _h32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x.astype(np.uint32)


def wave_hash32(seed, stream, w, r, l):
    k = ((((np.uint64(stream) * 4 + np.asarray(w, np.uint64)) << np.uint64(8)) | (np.asarray(r, np.uint64) & 255)) << np.uint64(6)
         | np.asarray(l, np.uint64)) + 1
    return _h32((np.uint64(seed) + np.uint64(0x9E3779B9) * k) & _M32)


# ---------------------------------------------------------------- lane
_QUAD = (0xE4, 0x1B, 0x00, 0x55, 0xAA, 0xFF, 0xB1, 0x4E)
_SWIZZLE = (0x041F, 0x401F, 0x7C1F, 0x003E, 0x1070, 0x801B, 0x8000, 0x80B1)
_DPP_CTRLS = (list(_QUAD) + [0x101 + i for i in range(15)] + [0x111 + i for i in range(15)] + [0x121 + i for i in range(15)]
              + [0x130, 0x134, 0x138, 0x13C] + [0x140, 0x141, 0x142, 0x143] + [0x150 + i for i in range(16)])


def wave_lane_ops() -> list[tuple]:
    """The op list: (kind, ctrl, bound_ctrl, row_mask, bank_mask), in the header's order."""
    ops = []
    for rm, bm in ((0xF, 0xF), (0x5, 0xF), (0xF, 0x6)):
        for b in (0, 1):
            ops += [("dpp", c, b, rm, bm) for c in _DPP_CTRLS]
    ops += [("bpermute", v, 0, 0xF, 0xF) for v in range(3)]
    ops += [("permute", v, 0, 0xF, 0xF) for v in range(2)]
    ops += [("swizzle", v, 0, 0xF, 0xF) for v in _SWIZZLE]
    ops += [("swap16", v, 0, 0xF, 0xF) for v in range(2)]
    ops += [("swap32", v, 0, 0xF, 0xF) for v in range(2)]
    ops += [("readlane", v, 0, 0xF, 0xF) for v in range(64)]
    ops += [("readfirst", 0, 0, 0xF, 0xF), ("readfirst_branch", 5, 0, 0xF, 0xF), ("readfirst_branch", 37, 0, 0xF, 0xF),
            ("bpermute_branch", 0, 0, 0xF, 0xF)]
    return ops


def wave_dpp_name(c: int) -> str:
    if c < 0x100:
        return f"quad_perm:[{c & 3},{(c >> 2) & 3},{(c >> 4) & 3},{(c >> 6) & 3}]"
    for lo, name in ((0x100, "row_shl"), (0x110, "row_shr"), (0x120, "row_ror")):
        if lo < c <= lo + 15:
            return f"{name}:{c & 15}"
    fixed = {0x130: "wave_shl:1", 0x134: "wave_rol:1", 0x138: "wave_shr:1", 0x13C: "wave_ror:1", 0x140: "row_mirror",
             0x141: "row_half_mirror", 0x142: "row_bcast:15", 0x143: "row_bcast:31"}
    return fixed.get(c, f"row_newbcast:{c & 15}")


def wave_lane_op_name(op: tuple) -> str:
    kind, ctrl, bound, rm, bm = op
    if kind == "dpp":
        s = f"{wave_dpp_name(ctrl)} bound_ctrl:{bound}"
        s += f" row_mask:0x{rm:x}" if rm != 0xF else ""
        return s + (f" bank_mask:0x{bm:x}" if bm != 0xF else "")
    return {"bpermute": f"ds_bpermute {ctrl}", "permute": f"ds_permute {ctrl}", "swizzle": f"ds_swizzle 0x{ctrl:04x}",
            "swap16": f"permlane16_swap {ctrl}", "swap32": f"permlane32_swap {ctrl}", "readlane": f"readlane {ctrl}",
            "readfirst": "readfirstlane", "readfirst_branch": f"readfirstlane branch {ctrl}",
            "bpermute_branch": "ds_bpermute branch"}[kind]


def wave_lane_op_index(name: str) -> int:
    """Index of the op whose ``wave_lane_op_name`` is ``name``; ValueError if there is none."""
    for i, op in enumerate(wave_lane_ops()):
        if wave_lane_op_name(op) == name:
            return i
    raise ValueError(f"no lane op named {name!r}")


def wave_bpermute_index(variant: int, l: int) -> int:
    if variant == 0:
        return (((l * 37 + 11) & 63) ^ 0x15) << 2
    if variant == 1:
        return (int(_h32(0xB5 + l)) & 60) << 2
    return (((l * 29 + 5) & 63) << 2) | (int(_h32(0x99 + l)) & 0xFFFFFF03)


def _dpp_src(c: int, l: int) -> int:
    row, i, n = l & ~15, l & 15, c & 15
    if c < 0x100:
        return (l & ~3) | ((c >> (2 * (l & 3))) & 3)
    if 0x101 <= c <= 0x10F:
        return l + n if i + n < 16 else WAVE_OLD
    if 0x111 <= c <= 0x11F:
        return l - n if i >= n else WAVE_OLD
    if 0x121 <= c <= 0x12F:
        return row | ((i - n) & 15)
    if c == 0x130:
        return l + 1 if l < 63 else WAVE_OLD
    if c == 0x134:
        return (l + 1) & 63
    if c == 0x138:
        return l - 1 if l > 0 else WAVE_OLD
    if c == 0x13C:
        return (l - 1) & 63
    if c == 0x140:
        return row | (15 - i)
    if c == 0x141:
        return (l & ~7) | (7 - (l & 7))
    if c == 0x142:
        return row - 1 if l >= 16 else WAVE_SKIP
    if c == 0x143:
        return 31 if l >= 32 else WAVE_SKIP
    return row | n


def wave_src_lane(op: tuple) -> np.ndarray:
    """int8[64]: where every lane's output word comes from - 0 .. 63 lane of x, 64 .. 127 lane of
    y, -1 the lane's own y (old), -2 zero, -3 not judged (zero in both kernels)."""
    kind, ctrl, bound, rm, bm = op
    out = np.zeros(64, np.int16)
    for l in range(64):
        if kind == "dpp":
            if not (rm >> (l >> 4)) & 1 or not (bm >> ((l & 15) >> 2)) & 1:
                s = WAVE_OLD
            else:
                s = _dpp_src(ctrl, l)
                if s == WAVE_OLD and bound:
                    s = WAVE_ZERO
        elif kind == "bpermute":
            s = (wave_bpermute_index(ctrl, l) >> 2) & 63
        elif kind == "permute":
            s = [k for k in range(64) if (wave_bpermute_index(2 if ctrl else 0, k) >> 2) & 63 == l][0]
        elif kind == "swizzle":
            if ctrl & 0x8000:
                s = (l & ~3) | ((ctrl >> (2 * (l & 3))) & 3)
            else:
                s = (l & 32) | ((((l & 31) & (ctrl & 31)) | ((ctrl >> 5) & 31)) ^ ((ctrl >> 10) & 31))
        elif kind == "swap16":
            odd = (l >> 4) & 1
            s = (64 + l - 16 if odd else l) if ctrl == 0 else (64 + l if odd else l + 16)
        elif kind == "swap32":
            s = (l if l < 32 else 64 + l - 32) if ctrl == 0 else (l + 32 if l < 32 else 64 + l)
        elif kind == "readlane":
            s = ctrl & 63
        elif kind == "readfirst":
            s = 0
        elif kind == "readfirst_branch":
            s = ctrl if l >= ctrl else WAVE_OLD
        else:
            s = 32 + ((l * 13 + 7) & 31) if l >= 32 else WAVE_OLD
        out[l] = s
    return out.astype(np.int8) if out.max() < 128 else out


def wave_expected_lane(op: tuple, x, y) -> np.ndarray:
    """The output words of ``op`` on x, y (uint32, a multiple of 64 long; each 64 one wave)."""
    x, y = np.asarray(x, np.uint32).reshape(-1, 64), np.asarray(y, np.uint32).reshape(-1, 64)
    s = wave_src_lane(op).astype(np.int64)
    both = np.concatenate([x, y], axis=1)
    out = both[:, np.clip(s, 0, 127)]
    out = np.where(s == WAVE_OLD, y, out)
    return np.where(s < WAVE_OLD, np.uint32(0), out).astype(np.uint32).reshape(-1)


# ---------------------------------------------------------------- ldstr
def _tr_consts(bits):
    if bits not in WAVE_TR_BITS:
        raise ValueError("transposed reads are 16, 8, 4 or 6 bits wide")
    E = 16 if bits == 6 else 64 // bits
    return E, 16 // E, 16 if bits == 6 else 8, 3 if bits == 6 else 2


def wave_tr_shape(bits, rows, stride):
    """dict of the header's TrShape, or None when it refuses the shape."""
    E, P, sb, _ = _tr_consts(bits)
    if rows <= 0 or stride < 32 or stride % sb or rows % E or rows * stride > 16384:
        return None
    width = min(stride, 128) & ~31
    rb, cb = rows // E, width // (P * sb)
    return {"bits": bits, "rows": rows, "stride": stride, "width": width, "row_blocks": rb, "col_blocks": cb,
            "blocks": rb * cb, "iters": (rb * cb + 15) // 16}


def wave_tr_src(bits, i, q):
    """(j, e): element q of group lane i's result is element e of the slot lane j addressed."""
    E, P, _, _ = _tr_consts(bits)
    return q * P + i // E, i % E


def _tr_addr(s, b, j):
    E, P, sb, _ = _tr_consts(s["bits"])
    b = min(b, s["blocks"] - 1)
    rb, cb = divmod(b, s["col_blocks"])
    return (rb * E + j // P) * s["stride"] + (cb * P + j % P) * sb


def wave_make_image(bits, rows, stride, seed) -> np.ndarray:
    """uint8[rows * stride]: the header's tr_make_image."""
    n = rows * stride
    img = (_h32((np.uint64(seed) + np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B9)) & _M32) & 0xFF).astype(np.uint8)
    s = wave_tr_shape(bits, rows, stride)
    if s is None:
        return img
    E, _, sb, _ = _tr_consts(bits)
    cols = s["width"] // sb * E
    bitsv = np.unpackbits(img, bitorder="little")
    for r in range(rows):
        for c in range(cols):
            tile = int(_h32(seed ^ ((r // 16) * 64 + c // 16 + 1)))
            if bits == 16:
                v = ((r * cols + c) & 0x1FFF) | (tile & 0xE000)
            elif bits == 8:
                v = (((r & 15) << 4) | (c & 15)) ^ (tile & 0xFF)
            elif bits == 6:
                v = ((5 * r + 3 * c + r // 16 + 16 * ((c >> 3) & 3)) & 63) ^ (tile & 63)
            else:
                v = ((5 * r + 3 * c + r // 16) & 15) ^ (tile & 15)
            at = (r * stride + (c // E) * sb) * 8 + (c % E) * bits
            for k in range(bits):
                bitsv[at + k] = (v >> k) & 1
    return np.packbits(bitsv, bitorder="little")


def wave_expected_tr_read(bits, image, rows, stride) -> np.ndarray:
    """uint32[iters * 3 * 256] in the kernel's layout: word d of thread t in iteration it at
    [(it * 3 + d) * 256 + t]."""
    s = wave_tr_shape(bits, rows, stride)
    if s is None:
        raise ValueError("bad transposed-read shape")
    E, _, _, words = _tr_consts(bits)
    ib = np.unpackbits(np.asarray(image, np.uint8), bitorder="little")
    out = np.zeros((s["iters"], 3, 256), np.uint32)
    for it in range(s["iters"]):
        for t in range(256):
            b, i = it * 16 + t // 16, t % 16
            res = np.zeros(96, np.uint8)
            for q in range(E):
                j, e = wave_tr_src(bits, i, q)
                at = _tr_addr(s, b, j) * 8 + e * bits
                res[q * bits:(q + 1) * bits] = ib[at:at + bits]
            w = np.packbits(res, bitorder="little").view(np.uint32)
            out[it, :words, t] = w[:words]
    return out.reshape(-1)


# ---------------------------------------------------------------- sfu
_LD = np.longdouble
_TWO_PI = _LD(2) * _LD("3.14159265358979323846264338327950288")


def _sfu_true(op: int, xbits) -> np.ndarray:
    x = np.asarray(xbits, np.uint32).view(np.float32).astype(_LD)
    with np.errstate(all="ignore"):
        return (np.exp2(x), np.log2(x), _LD(1) / x, _LD(1) / np.sqrt(x), np.sqrt(x), np.sin(_TWO_PI * x), np.cos(_TWO_PI * x))[op]


def _normal(bits):
    e = (np.asarray(bits, np.uint32) >> 23) & 0xFF
    return (e != 0) & (e != 0xFF)


def _sfu_in_domain(op: int, bits) -> np.ndarray:
    bits = np.asarray(bits, np.uint32)
    x = bits.view(np.float32)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        lo, hi = np.float32(2.0) ** -120, np.float32(2.0) ** 120
        if op == 0:
            ok = ax <= 120
        elif op == 1:
            ok = (x >= lo) & (x <= hi) & (x != 1)
        elif op == 2:
            ok = (ax >= lo) & (ax <= hi)
        elif op in (3, 4):
            ok = (x >= lo) & (x <= hi)
        else:
            ok = (ax <= 256) & (np.abs(_sfu_true(op, bits)) >= _LD(2) ** -20)
    return ok & _normal(bits)


def wave_sfu_inputs(op) -> tuple[np.ndarray, int]:
    """(input bits uint32, index the exact cases start at) of instruction ``op`` (name or id)."""
    op = WAVE_SFU_OPS.index(op) if isinstance(op, str) else int(op)
    low = np.arange(65536, dtype=np.uint32) << 16
    k = np.arange(1, 4097, dtype=np.uint32)
    near = np.stack([np.uint32(0x3F800000) - k, np.uint32(0x3F800000) + k], 1).reshape(-1)
    first = np.concatenate([low, near])
    first = first[_sfu_in_domain(op, first)]
    exact = []
    ks = np.arange(-120, 121)
    if op == 0:
        exact.append(ks[ks != 0].astype(np.float32).view(np.uint32))
    if op in (1, 2):
        exact.append(np.ldexp(np.float32(1), ks).astype(np.float32).view(np.uint32))
    if op == 4:
        n = np.arange(1, 4097, dtype=np.uint32)
        exact.append((n * n).astype(np.float32).view(np.uint32))
    if op in (3, 4):
        exact.append(np.ldexp(np.float32(1), 2 * np.arange(-60, 61)).astype(np.float32).view(np.uint32))
    ex = np.concatenate(exact) if exact else np.zeros(0, np.uint32)
    ex = ex[_sfu_in_domain(op, ex)] if ex.size else ex
    return np.concatenate([first, ex]).astype(np.uint32), int(first.size)


def wave_sfu_brackets(op, xbits) -> tuple[np.ndarray, np.ndarray]:
    """(lo, hi) fp32 bit patterns with lo <= true <= hi, neighbours or equal."""
    op = WAVE_SFU_OPS.index(op) if isinstance(op, str) else int(op)
    t = _sfu_true(op, xbits)
    f = t.astype(np.float32)
    fl = f.astype(_LD)
    up, down = np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))
    lo = np.where(fl <= t, f, down)
    hi = np.where(fl >= t, f, up)
    return lo.view(np.uint32), hi.view(np.uint32)


def wave_ordered(u) -> np.ndarray:
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def wave_expected_sfu_distance(y, lo, hi) -> np.ndarray:
    oy, ol, oh = (wave_ordered(v).astype(np.int64) for v in (y, lo, hi))
    return np.where(oy < ol, ol - oy, np.where(oy > oh, oy - oh, 0)).astype(np.uint32)


# ---------------------------------------------------------------- valu
def wave_expected_bitop3(a, b, c, table: int) -> np.ndarray:
    a, b, c = (np.asarray(v, np.uint32) for v in (a, b, c))
    r = np.zeros_like(a)
    for idx in range(8):
        if (table >> idx) & 1:
            r |= (a if idx & 4 else ~a) & (b if idx & 2 else ~b) & (c if idx & 1 else ~c)
    return r


def wave_bf16_rne(f) -> np.ndarray:
    f = np.asarray(f, np.uint32).astype(np.uint64)
    return (((f + 0x7FFF + ((f >> np.uint64(16)) & 1)) >> np.uint64(16)) & _M32).astype(np.uint32)


def wave_expected_cvt_pk(lo, hi) -> np.ndarray:
    return ((wave_bf16_rne(lo) & 0xFFFF) | (wave_bf16_rne(hi) << 16)).astype(np.uint32)


def wave_cvt_inputs(seed: int, hashed: int) -> np.ndarray:
    v = []
    for e in (27, 126, 127, 128, 227):
        for sign in (0, 1):
            m = 0
            while m < 128:
                for low in (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF):
                    v.append((sign << 31) | (e << 23) | (m << 16) | low)
                m += 1 if (m < 8 or m >= 120) else 17
    v += [0x7F7F7FFF, 0xFF7F7FFF, 0x7F7F0000]
    i = 0
    while len(v) % 2 or hashed:
        w = int(_h32((seed + 0x51 + i * 0x9E3779B9) & _M32))
        i += 1
        if ((int(wave_bf16_rne(w)) >> 7) & 0xFF) == 0xFF or not bool(_normal(w)):
            continue
        v.append(w)
        hashed -= 1 if hashed else 0
    return np.asarray(v, np.uint32)


def wave_failure_message(gpu, family, what, where, unit, index, expected, got) -> str:
    """The Job's line; ``where`` = (xcd, se, sh, cu, simd)."""
    m = (f"gpu{gpu}: wave {family} {what}: xcd {where[0]} se {where[1]} sh {where[2]} cu {where[3]} simd {where[4]} "
         f"{unit} {index}: expected 0x{expected:08x}, got 0x{got:08x}, bad bits 0x{expected ^ got:08x}")
    return m[:199]
