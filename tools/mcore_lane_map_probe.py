#!/usr/bin/env python3
"""K10: operand lane maps of the fp64 / fp32 / fp16 / int8 MFMAs and the 2:4-sparse bf16 /
int8 SMFMACs, measured with the one-instruction probe of libntm_experimental.so
(``ntm_mcore_mfma_probe``) and exact integer data. Needs one MI355X.

    python tools/mcore_lane_map_probe.py > profiles/mcore/lane_map_probe.log

A "slot" is (lane group g = lane >> 4, element e of the lane's fragment). Dense formats: for
every A slot, which B slot it is multiplied with, and that rows and columns of C/D sit where
the kernel expects them. Sparse formats: for every slot of the compressed A, which 2-bit
field of the index VGPR moves it and which B slot it meets for the field's values 0 .. 3;
then which index bits the instruction's cbsz / abid immediates select.
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nvidia_terraform_modules_amd.ops._lib import check, lib_experimental, stream_handle  # noqa: E402

FORMATS = ("f64", "f32", "f16", "i8", "sp_bf16", "sp_i8")
ELEM = {"f64": np.float64, "f32": np.float32, "f16": np.float16, "i8": np.int8, "sp_bf16": np.uint16, "sp_i8": np.int8}
ACC = {"f64": np.float64, "f32": np.float32, "f16": np.float32, "i8": np.int32, "sp_bf16": np.float32, "sp_i8": np.int32}
A_SLOTS = {"f64": 1, "f32": 1, "f16": 8, "i8": 16, "sp_bf16": 8, "sp_i8": 16}
B_SLOTS = {"f64": 1, "f32": 1, "f16": 8, "i8": 16, "sp_bf16": 16, "sp_i8": 32}


def enc(fmt, values):
    v = np.asarray(values)
    if fmt == "sp_bf16":
        return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    return v.astype(ELEM[fmt])


def run(fmt, a, b, idx=None, cbsz=0, abid=0):
    """a [64, A_SLOTS], b [64, B_SLOTS] values, idx [64] -> C [16, 16] by the kernel's C/D map."""
    dev = torch.device("cuda")
    sa, sb = np.zeros((64, 16), np.uint8), np.zeros((64, 32), np.uint8)
    ea, eb = enc(fmt, a), enc(fmt, b)
    sa[:, :ea.shape[1] * ea.itemsize] = ea.view(np.uint8).reshape(64, -1)
    sb[:, :eb.shape[1] * eb.itemsize] = eb.view(np.uint8).reshape(64, -1)
    ix = np.zeros(64, np.uint32) if idx is None else np.asarray(idx, dtype=np.uint32)
    ta, tb, ti = (torch.from_numpy(x.view(np.uint8).copy()).to(dev) for x in (sa, sb, ix))
    d = torch.zeros(64 * 32, dtype=torch.uint8, device=dev)
    check(lib_experimental().ntm_mcore_mfma_probe(FORMATS.index(fmt), ta.data_ptr(), tb.data_ptr(), ti.data_ptr(),
                                                  cbsz, abid, d.data_ptr(), stream_handle()), "ntm_mcore_mfma_probe")
    raw = d.cpu().numpy().reshape(64, 32)
    regs = raw.view(ACC[fmt]).reshape(64, -1)[:, :4]
    c = np.zeros((16, 16), dtype=np.float64)
    for lane in range(64):
        g = lane >> 4
        for r in range(4):
            c[g + 4 * r if fmt == "f64" else 4 * g + r, lane & 15] = regs[lane, r]
    return c


def b_codes(fmt):
    """A distinct non-zero value per B slot, the same in every column: [64, B_SLOTS]."""
    n = B_SLOTS[fmt]
    v = np.arange(4 * n).reshape(4, n)
    v = np.where(v < 64, v - 64, v - 63) if fmt in ("i8", "sp_i8") and 4 * n > 64 else v + 1
    return np.repeat(v, 16, axis=0), {int(x): (g, e) for g in range(4) for e, x in enumerate(v[g])}


def dense(fmt):
    na = A_SLOTS[fmt]
    codes, where = b_codes(fmt)
    print(f"== {fmt}: A slot (g, e) -> B slot it multiplies; rows / columns of C/D")
    ok = True
    for g in range(4):
        for e in range(na):
            a = np.zeros((64, na))
            a[16 * g:16 * g + 16, e] = np.arange(1, 17)          # row r holds r + 1
            c = run(fmt, a, codes)
            per_row = c[:, 0] / np.arange(1, 17)
            uniform = np.all(c == c[:, :1]) and np.all(per_row == per_row[0])
            hit = where.get(int(per_row[0])) if uniform else None
            ok = ok and hit == (g, e)
            print(f"  A({g},{e:2d}) -> B{hit}  rows {'ok' if uniform else 'WRONG'}")
    a = np.zeros((64, na))
    a[:16, 0] = 1
    b = np.zeros((64, B_SLOTS[fmt]))
    b[:16, 0] = np.arange(1, 17)                                 # column c holds c + 1
    c = run(fmt, a, b)
    cols = bool(np.all(c == np.arange(1, 17)[None, :]))
    print(f"  columns {'ok' if cols else 'WRONG'}; A and B slots pair one to one: {ok}")


def sparse(fmt):
    na, nb = A_SLOTS[fmt], B_SLOTS[fmt]
    fields = na                                                   # 2 bits per kept value
    codes, where = b_codes(fmt)
    print(f"== {fmt}: compressed A slot (g, e) -> index field that moves it, B slot met for field value 0..3")

    def landing(g, e, idx, cbsz=0, abid=0):
        a = np.zeros((64, na))
        a[16 * g:16 * g + 16, e] = 1
        c = run(fmt, a, codes, np.full(64, idx, np.uint32), cbsz, abid)
        return where.get(int(c[0, 0])) if np.all(c == c[0, 0]) else None

    for g in range(4):
        for e in range(na):
            base = landing(g, e, 0)
            moved = [f for f in range(fields) if landing(g, e, 3 << (2 * f)) != base]
            row = [landing(g, e, v << (2 * moved[0])) for v in range(4)] if len(moved) == 1 else None
            print(f"  Ac({g},{e:2d}) field {moved} -> B {row if row else base}")
    print(f"   {fmt}: cbsz / abid with one pattern per index byte (field 0 of byte n = n) and per half (1, 3):")
    for cbsz in (0, 1):
        for abid in range(4):
            per_byte = [landing(g, 0, 0x03020100, cbsz, abid) for g in (0, 1)]
            per_half = [landing(g, 0, 0x00030001, cbsz, abid) for g in (0, 1)]
            print(f"   cbsz {cbsz} abid {abid}: Ac(0,0) / Ac(1,0) meet B {per_byte} (bytes), {per_half} (halves)")


def main():
    if not torch.cuda.is_available():
        sys.exit("needs a GPU")
    print(torch.cuda.get_device_name(0))
    for fmt in FORMATS[:4]:
        dense(fmt)
    for fmt in FORMATS[4:]:
        sparse(fmt)


if __name__ == "__main__":
    main()
