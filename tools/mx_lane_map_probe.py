"""Which lane group's scale byte applies to slot (lane group g, value j) of an operand?
One-hot A (or B) rows, the other operand 1.5 everywhere with unit scales, the one-hot
operand's lane group g' carries scale 2^g'. Prints, per format and side, the scale group
seen for every (g, j)."""
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from nvidia_terraform_modules_amd import ops
from nvidia_terraform_modules_amd.ops import mx
from nvidia_terraform_modules_amd.ops._lib import lib_experimental, stream_handle

lanes = np.arange(64)
ONE = {"e4m3": 0x38, "e5m2": 0x3C, "e2m3": 0x08, "e3m2": 0x0C, "e2m1": 0x02}


def stage(codes, fmt):
    """codes [16 rows, 4 groups, 32 slots] -> register image [64, 32 B]"""
    frag = 4 * mx.mx_bits(fmt)
    packed = ops.mx_pack(codes.reshape(16 * 4, 32), fmt).reshape(16, 4, frag)
    img = np.zeros((64, 32), dtype=np.uint8)
    img[:, :frag] = packed[lanes & 15, lanes >> 4]
    return torch.from_numpy(img).cuda()


for fmt in ops.MX_FORMATS:
    f = ops.MX_FORMATS.index(fmt)
    for side in ("A", "B"):
        seen = np.full((4, 32), -1)
        for launch in range(8):
            hot = np.zeros((16, 4, 32), dtype=np.uint8)
            slots = [(launch * 16 + r) for r in range(16)]
            for r, sidx in enumerate(slots):
                hot[r, sidx // 32, sidx % 32] = ONE[fmt]
            dense = np.full((16, 4, 32), mx._LAYOUT[fmt][4], dtype=np.uint8)
            tag = torch.from_numpy((127 + (lanes >> 4)).astype(np.int32)).cuda()
            unit = torch.full((64,), 127, dtype=torch.int32).cuda()
            d = torch.empty((64, 4), dtype=torch.float32, device="cuda")
            if side == "A":
                args = (stage(hot, fmt), stage(dense, fmt), tag, unit)
            else:
                args = (stage(dense, fmt), stage(hot, fmt), unit, tag)
            rc = lib_experimental().ntm_mx_mfma_probe(f, *(t.data_ptr() for t in args), d.data_ptr(),
                                                     stream_handle())
            assert rc == 0
            torch.cuda.synchronize()
            dc = d.cpu().numpy()
            got = np.empty((16, 16), dtype=np.float32)
            for lane in range(64):
                got[4 * (lane >> 4):4 * (lane >> 4) + 4, lane & 15] = dc[lane]
            for r, sidx in enumerate(slots):
                v = got[r, 0] if side == "A" else got[0, r]
                seen[sidx // 32, sidx % 32] = int(round(np.log2(v / 1.5))) if v > 0 else -9
        print(fmt, side)
        for g in range(4):
            print("  group", g, "".join(str(x) if x >= 0 else "?" for x in seen[g]))
