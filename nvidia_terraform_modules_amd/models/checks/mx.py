"""K7: the Job's MX block-scaled matrix check."""
from __future__ import annotations

import time

import numpy as np
import torch

from ...ops import mx
from .._timing import _wall_time
from ._common import begin, device_context


def mx_check(device: torch.device, size: int = 512, iters: int = 3, backend=None,
             corrupt: bool = False) -> dict:
    """K7, the Job's MX block-scaled matrix check (``amdgpu-validate --mx-check``) on
    ``device``: the decode sweep of all five formats (256 x 128 x 128, all 15 scale windows)
    against the exact integer table, dense e2m3 (``size`` x ``size`` x 512) and dense e2m1
    (``size``^3) with the largest exact scale spread against the reference kernel, every
    element compared bitwise, then ``iters`` timed e2m1 products. ``corrupt`` flips one bit
    of one element of the dense e2m1 result before its compare.

    Unlike the Job, which times with events after a settle, the timing here is a host clock
    around a synchronise: the Job's ``mx_fp4_tflops`` is the rate to quote. With
    ``backend=ops.reference`` (CPU) every product is the integer reference itself and the
    rate means nothing."""
    o, device, _ = begin(device, backend)
    t_begin = time.perf_counter()
    out = {"size": size, "formats": [], "bad_elements": 0, "first": None, "failed_step": None,
           "fp4_tflops": 0.0, "scale_spread": mx.mx_max_spread("e2m1", size)}
    clean = {f: True for f in mx.MX_FORMATS}

    def put(i: dict) -> dict:
        return {k: torch.from_numpy(i[k]).to(device) for k in ("a", "b", "sa", "sb")}

    def judge(rep, fmt: str, mode: str, n_cols: int) -> None:
        if rep.ok:
            return
        out["bad_elements"] += rep.count
        clean[fmt] = False
        if out["first"] is None:
            out["failed_step"] = f"{fmt} {mode}"
            out["first"] = {"format": fmt, "mode": mode, "row": rep.first_index // n_cols,
                            "col": rep.first_index % n_cols, "expected": rep.expected, "got": rep.got}

    with device_context(device):
        for fmt in mx.MX_FORMATS:
            for window in range(mx.MX_DECODE_WINDOWS):
                i = mx.mx_make_inputs("decode", fmt, 256, 128, 128, seed=window)
                want = torch.from_numpy(mx.mx_matmul_bits(i["a"], i["b"], i["sa"], i["sb"], fmt)
                                        .view(np.int32)).to(device)
                d = put(i)
                judge(o.mx_compare(want, o.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], fmt)), fmt, "decode", 128)
        w6 = mx.mx_max_spread("e2m3", 512)
        d = put(mx.mx_make_inputs("dense", "e2m3", size, size, 512, seed=0x4B37, W=w6))
        judge(o.mx_compare(o.mx_reference_gpu(d["a"], d["b"], d["sa"], d["sb"], "e2m3"),
                           o.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m3")), "e2m3", "dense", size)
        if out["scale_spread"] < 0:
            raise ValueError(f"no exact scale spread for e2m1 at size {size}")
        d = put(mx.mx_make_inputs("dense", "e2m1", size, size, size, seed=0x4B37, W=out["scale_spread"]))
        c = o.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m1")
        if corrupt:
            c.view(torch.int32).view(-1)[c.numel() // 2 + 5] ^= 1 << 3
        judge(o.mx_compare(o.mx_reference_gpu(d["a"], d["b"], d["sa"], d["sb"], "e2m1"), c),
              "e2m1", "dense", size)
        secs = _wall_time(lambda: o.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m1", out=c), iters, device)
        out["fp4_tflops"] = 2.0 * size**3 * iters / secs / 1e12
    out["formats"] = [f for f in mx.MX_FORMATS if clean[f]]
    out["ok"] = out["bad_elements"] == 0
    out["seconds"] = time.perf_counter() - t_begin
    return out
