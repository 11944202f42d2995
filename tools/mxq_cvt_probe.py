#!/usr/bin/env python3
"""K11: what the gfx950 scaled-conversion instructions (v_cvt_scalef32_*) do, measured with the
one-instruction probe of libntm_experimental.so (``ntm_mxq_cvt_probe``). Needs one MI355X.

    python tools/mxq_cvt_probe.py > profiles/mxq/cvt_probe.log

Six questions, one section each: the scale operand; element order and selectors; tie rounding;
finite overflow; element subnormals; the random word of the ``sr_`` forms. Every section ends
with a line starting ``=>`` that states the finding; ``ops.mxq`` (the numpy mirror of
``mxq_plan.hpp``) is the expectation where one is printed.
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nvidia_terraform_modules_amd.ops import mxq  # noqa: E402
from nvidia_terraform_modules_amd.ops._lib import check, lib_experimental, stream_handle  # noqa: E402

OPS = {"pk_fp4_f32": 0, "pk_fp4_bf16": 1, "pk_fp8_f32": 2, "pk_bf8_f32": 3, "2xpk16_fp6_f32": 4,
       "2xpk16_bf6_f32": 5, "pk_f32_fp4": 6, "pk_f32_fp8": 7, "pk_f32_bf8": 8, "pk32_f32_fp6": 9,
       "pk32_f32_bf6": 10, "sr_pk_fp4_f32": 11, "sr_fp8_f32": 12}
DOWN = {"e2m1": "pk_fp4_f32", "e4m3": "pk_fp8_f32", "e5m2": "pk_bf8_f32", "e2m3": "2xpk16_fp6_f32",
        "e3m2": "2xpk16_bf6_f32"}
UP = {"e2m1": "pk_f32_fp4", "e4m3": "pk_f32_fp8", "e5m2": "pk_f32_bf8", "e2m3": "pk32_f32_fp6", "e3m2": "pk32_f32_bf6"}


def run(op, src, scale, sel=0, rnd=0, old=0):
    """src [n, <=32] fp32 values or uint32 bits; scale / rnd / old scalars or [n] -> uint32 [n, 32]."""
    src = np.asarray(src)
    n = src.shape[0]
    full = np.zeros((n, 32), np.uint32)
    full[:, :src.shape[1]] = src.view(np.uint32) if src.dtype in (np.float32, np.uint32) else src.astype(np.float32).view(np.uint32)
    dev = torch.device("cuda")

    def col(v):
        return torch.from_numpy(np.broadcast_to(np.asarray(v, dtype=np.uint32), (n,)).astype(np.int64).astype(np.int32, casting="unsafe").copy()).to(dev)
    t_src = torch.from_numpy(full.view(np.int32).copy()).to(dev)
    t_scale, t_rnd, t_old = col(scale), col(rnd), col(old)
    out = torch.zeros((n, 32), dtype=torch.int32, device=dev)
    check(lib_experimental().ntm_mxq_cvt_probe(OPS[op], sel, t_src.data_ptr(), t_scale.data_ptr(), t_rnd.data_ptr(),
                                               t_old.data_ptr(), out.data_ptr(), n, stream_handle()), "ntm_mxq_cvt_probe")
    return out.cpu().numpy().view(np.uint32)


def f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def down_codes(fmt, x, scale_bits):
    """One value per lane through the format's down instruction -> its code."""
    x = np.asarray(x, dtype=np.float32).reshape(-1, 1)
    if fmt in ("e2m3", "e3m2"):
        return run(DOWN[fmt], x, scale_bits)[:, 0] & 63
    return run(DOWN[fmt], np.concatenate([x, np.zeros_like(x)], 1), scale_bits)[:, 0] & (15 if fmt == "e2m1" else 255)


def section_scale():
    print("== 1. the scale operand")
    for fmt in mxq.MX_FORMATS:
        x = np.full(5, 1.5, np.float32) * np.float32(2.0) ** np.arange(-2, 3)
        for sb in (126 << 23, 127 << 23, 128 << 23, (128 << 23) | 0x7FFFFF, (128 << 23) | 0x80000000):
            got = down_codes(fmt, x, sb)
            print(f"  down {fmt} x=1.5*2^(-2..2) scale bits {sb:#010x}: codes {[hex(c) for c in got]}")
    one_five = {f: mxq._LAYOUT[f][4] for f in mxq.MX_FORMATS}
    for fmt in mxq.MX_FORMATS:
        for sb in (126 << 23, 127 << 23, 128 << 23, (128 << 23) | 0x7FFFFF, (128 << 23) | 0x80000000):
            r = run(UP[fmt], np.full((1, 6), one_five[fmt], np.uint32), sb)[0, 0]
            print(f"  up   {fmt} code of 1.5 scale bits {sb:#010x}: {f32(r)} ({r:#010x})")
    print("=> expected if down divides and up multiplies by 2^(exponent field - 127), fraction and sign ignored:"
          " down codes of 1.5*2^(-1..3), 1.5*2^(-2..2), 1.5*2^(-3..1), and the last two rows as the third; up 0.75, 1.5, 3, 3, 3")


def section_order():
    print("== 2. element order, selectors, 2xpk16 interleave")
    for op in ("pk_fp4_f32", "pk_fp8_f32", "pk_bf8_f32"):
        for sel in range(4 if op == "pk_fp4_f32" else 2):
            r = run(op, np.array([[1.0, -2.0]], np.float32), 127 << 23, sel=sel, old=0xAAAAAAAA)[0, 0]
            print(f"  {op} (1.0, -2.0) sel {sel} old 0xaaaaaaaa -> {r:#010x}")
    a = np.array([[1.0, -2.0]], np.float32)
    packed = (bits(a)[0, 0] >> 16) | (bits(a)[0, 1] & 0xFFFF0000)
    for sel in range(4):
        r = run("pk_fp4_bf16", np.array([[packed]], np.uint32), 127 << 23, sel=sel, old=0xAAAAAAAA)[0, 0]
        print(f"  pk_fp4_bf16 (lo 1.0, hi -2.0) sel {sel} old 0xaaaaaaaa -> {r:#010x}")
    for fmt in ("e2m3", "e3m2"):
        src = np.zeros((32, 32), np.float32)
        src[np.arange(32), np.arange(32)] = 1.5          # lane i: only input i (0..15 src0, 16..31 src1) is 1.5
        r = run(DOWN[fmt], src, 127 << 23)[:, :6]
        codes = mxq.mx_unpack(r.view(np.uint8).reshape(32, 24), fmt)
        where = [int(np.flatnonzero(c)[0]) if np.count_nonzero(c) == 1 else None for c in codes]
        print(f"  {DOWN[fmt]}: input i -> slot {where}")
        up = run(UP[fmt], r.astype(np.uint32), 127 << 23)
        back = [int(np.flatnonzero(f32(u))[0]) if np.count_nonzero(f32(u)) == 1 else None for u in up]
        print(f"  {UP[fmt]}: slot of input i -> output element {back}")
    for op, word in (("pk_f32_fp4", 0x76543210), ("pk_f32_fp8", 0x44403C38), ("pk_f32_bf8", 0x46423E3A)):
        for sel in range(4 if op == "pk_f32_fp4" else 2):
            r = run(op, np.array([[word]], np.uint32), 127 << 23, sel=sel)[0, :2]
            print(f"  {op} src {word:#010x} sel {sel} -> {f32(r)}")
    print("=> see above: which nibble / byte / half each source lands in, and whether `old` is kept elsewhere")


def section_values(title, fmt_points):
    print(title)
    for fmt in mxq.MX_FORMATS:
        pts = fmt_points(fmt)
        got = down_codes(fmt, f32(pts), 127 << 23)
        want = mxq.mxq_quantize_codes(pts, np.full(pts.shape, 127), fmt)
        bad = np.flatnonzero(got != want)
        print(f"  {fmt}: {pts.size} points, {bad.size} differ from the mirror")
        for i in bad[:12]:
            print(f"    x {f32(pts[i])} ({pts[i]:#010x}): got {got[i]:#04x}, mirror {want[i]:#04x}")
    print("=> 0 differ: the instruction agrees with the mirror on these points")


def sweep_points(fmt, which):
    s = mxq.mxq_down_points(fmt)
    n = s.size // 2
    per = s[:n - 5].reshape(-1, 5)
    if which == "ties":
        p = per[:, 1:4].ravel()
    elif which == "grid":
        p = per[:, [0, 4]].ravel()
    elif which == "sub":
        sub = 2 ** mxq._LAYOUT[fmt][2]
        p = per[:sub].ravel()
    else:
        p = s[n - 5:n]
    return np.concatenate([p, p | np.uint32(0x80000000)])


def section_sr():
    print("== 6. the random word of the sr_ forms")
    for op, mant, name in (("sr_pk_fp4_f32", 1, "e2m1"), ("sr_fp8_f32", 3, "e4m3")):
        D = 23 - mant                                    # fp32 fraction bits dropped for a normal result
        for el in ((0, 1) if op == "sr_pk_fp4_f32" else (0,)):
            pos = []
            for b in range(32):
                # x = 1 + (2^D - 2^j) / 2^23 rounds up with one-hot random bit b iff that bit is added at weight >= 2^j
                j = np.arange(D + 1)
                frac = ((1 << D) - (1 << j)).astype(np.uint32)
                x = f32(np.uint32(127 << 23) | frac)
                src = np.zeros((j.size, 2), np.float32)
                src[:, el] = x
                r = run(op, src, 127 << 23, rnd=1 << b)[:, 0]
                code = (r >> (4 * el)) & (15 if name == "e2m1" else 255)
                one = {"e2m1": 2, "e4m3": 0x38}[name]
                up = code != one
                pos.append(int(j[up].max()) if up.any() else None)
            print(f"  {op} element {el}: one-hot random bit b acts at fraction weight 2^j, j = {pos}")
        x = np.zeros((4, 2), np.float32)
        x[:, 0] = [1.0, 1.5, -1.0, 0.0]
        for rnd in (0, 0xFFFFFFFF):
            r = run(op, x, 127 << 23, rnd=rnd)[:, 0]
            print(f"  {op} exact inputs (1, 1.5, -1, 0) rnd {rnd:#010x}: {[hex(v) for v in r]}")
    print("=> j = None: the bit is not used; a bit with j acts as value 2^j against the dropped fraction bits")


def main():
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    print(torch.cuda.get_device_name(0))
    section_scale()
    section_order()
    section_values("== 3. tie rounding: midpoints of adjacent codes and their fp32 neighbours, scale 2^0",
                   lambda f: sweep_points(f, "ties"))
    section_values("== 4. finite overflow: max, max + half a step and its neighbours, 2 * max (mirror saturates)",
                   lambda f: sweep_points(f, "over"))
    section_values("== 5. element subnormals: every point of the subnormal range", lambda f: sweep_points(f, "sub"))
    section_sr()


if __name__ == "__main__":
    main()
