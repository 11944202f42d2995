#!/usr/bin/env python3
"""K12: the lane maps of the gfx950 transposed LDS reads (ds_read_b64_tr_b16 / _tr_b8 / _tr_b4,
ds_read_b96_tr_b6), measured with the one-instruction probe of libntm_experimental.so
(``ntm_wave_tr_probe``). Needs one MI355X.

    python tools/wave_lane_map_probe.py > profiles/wave/lane_map_probe.log
    python tools/wave_lane_map_probe.py --misaligned-b6    # once only, see below

The probe reads a 4 KiB LDS image with one wave. Pass k fills the image so that bit b of it is
bit k of b; 15 passes and their complements give, for every result bit of every lane, the image
bit it came from (a bit that does not follow the complement is a constant). The source bit is
then named by the lane whose address covers it. Every section ends with lines starting ``=>``;
the hypothesis printed beside them is the one of ``wave_paths_plan.hpp``: element q of group
lane i is element i % E of the slot of group lane q P + i // E, with E elements per slot and
P = 16 // E lanes per row.

``--misaligned-b6`` adds two sections that issue ds_read_b96_tr_b6 at addresses 8 mod 16 (every
slot moved up by 8 bytes; 24-byte rows). That is how the 16-byte requirement of the 6-bit form was
found; the reads return other lanes' data and do not fault. It was a once-only measurement, kept in
``profiles/wave/lane_map_probe_b6_alignment.log``: do not re-run it routinely. No kernel of the check
issues such a read (``tr_shape`` refuses the strides that would).
"""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nvidia_terraform_modules_amd.ops._lib import check, lib_experimental, stream_handle  # noqa: E402

IMAGE_BITS = 4096 * 8
FORMS = {16: (4, 8, 2), 8: (8, 8, 2), 4: (16, 8, 2), 6: (16, 16, 3)}   # bits: (E, slot bytes, result dwords)


def run(bits, image_bytes, addr):
    dev = torch.device("cuda")
    im = torch.from_numpy(np.frombuffer(image_bytes, dtype=np.int32).copy()).to(dev)
    ad = torch.from_numpy(np.asarray(addr, dtype=np.int32).copy()).to(dev)
    out = torch.zeros(64 * 3, dtype=torch.int32, device=dev)
    check(lib_experimental().ntm_wave_tr_probe(bits, im.data_ptr(), ad.data_ptr(), out.data_ptr(), stream_handle()),
          "ntm_wave_tr_probe")
    return out.cpu().numpy().view(np.uint32).reshape(64, 3)


def source_bits(bits, addr):
    """[64, 96] image bit index each result bit came from; -1 = a constant."""
    idx = np.arange(IMAGE_BITS, dtype=np.uint32)
    src = np.zeros((64, 96), np.int64)
    follows = np.ones((64, 96), bool)
    for k in range(15):
        plane = ((idx >> k) & 1).astype(np.uint8)
        got = [run(bits, np.packbits(p, bitorder="little").tobytes(), addr) for p in (plane, 1 - plane)]
        b = [np.unpackbits(g.view(np.uint8).reshape(64, 12), axis=1, bitorder="little") for g in got]
        follows &= b[0] != b[1]
        src |= b[0].astype(np.int64) << k
    src[~follows] = -1
    return src


def describe(bits, addr, label):
    E, slot, words = FORMS[bits]
    P = 16 // E
    src = source_bits(bits, addr)
    used = words * 32
    print(f"  {label}: result bits that are constants: {(src[:, :used] < 0).sum()} of {64 * used}"
          f"; beyond bit {used}: {(src[:, used:] >= 0).sum()} sourced")
    addr = np.asarray(addr) & 0xFF8
    ok_hyp, within_group, in_order = True, True, True
    rows = []
    for lane in range(64):
        g, i = lane // 16, lane % 16
        for q in range(used // bits):
            sb = src[lane, q * bits:(q + 1) * bits]
            if (sb < 0).any():
                ok_hyp = False
                continue
            if not (np.diff(sb) == 1).all():
                in_order = False
            # the lane whose slot covers the element's first bit
            owner = [j for j in range(64) if addr[j] * 8 <= sb[0] < addr[j] * 8 + slot * 8]
            j = owner[0] if owner else -1
            e = (sb[0] - addr[j] * 8) // bits if owner else -1
            if j // 16 != g:
                within_group = False
            if j != g * 16 + q * P + i // E or e != i % E:
                ok_hyp = False
            if lane < 16:
                rows.append((i, q, j, e))
    for i in sorted({0, 1, 2, E - 1, min(E, 15), 15}):
        print(f"    lane {i:2d}: " + " ".join(f"el{q}<-lane{j}.el{e}" for (ii, q, j, e) in rows if ii == i))
    print(f"  => {label}: every element's bits are consecutive image bits in order: {in_order}")
    print(f"  => {label}: every source lies in a slot of the reader's own 16-lane group: {within_group}")
    print(f"  => {label}: element q of group lane i is element i % {E} of the slot of group lane {P} q + i // {E}: {ok_hyp}")
    return ok_hyp


def block_addrs(bits, stride, base_step=1024, offset=0):
    """Group g reads one block at g * base_step: lane j of it supplies row j // P, slot j % P."""
    E, slot, _ = FORMS[bits]
    P = 16 // E
    return [g * base_step + offset + (j // P) * stride + (j % P) * slot for g in range(4) for j in range(16)]


def main():
    print(f"# {torch.cuda.get_device_name(0)}; ROCm {torch.version.hip}")
    for bits in (16, 8, 4, 6):
        E, slot, words = FORMS[bits]
        name = f"ds_read_b{words * 32}_tr_b{bits}"
        print(f"== {name}: {E} elements per lane, block of {E} rows x 16 columns")
        for stride in (32, 64) if bits != 4 else (32, 48):
            if (E - 1) * stride + 16 > 1024:
                continue
            describe(bits, block_addrs(bits, stride), f"{name} stride {stride}")
        if bits == 6 and "--misaligned-b6" in sys.argv[1:]:
            print("  -- addresses 8 mod 16 (every slot moved up by 8 bytes)")
            describe(bits, block_addrs(bits, 32, offset=8), f"{name} at 8 mod 16")
            print("  -- row stride 24: rows 8-byte aligned, alternately 0 and 8 mod 16")
            describe(bits, block_addrs(bits, 24), f"{name} stride 24")
    return 0


if __name__ == "__main__":
    sys.exit(main())
