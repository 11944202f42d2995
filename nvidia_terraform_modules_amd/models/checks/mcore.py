"""K10: the Job's matrix-core check of the formats K1 and K7 never issue."""
from __future__ import annotations

import time

import torch

from .._timing import _wall_time
from ._common import begin, device_context, verdict


def mcore_check(device: torch.device, size: int = 512, big: int = 0, iters: int = 3, backend=None,
                corrupt: bool = False, seed: int = 0x4B3A, max_windows: int | None = None) -> dict:
    """K10, the Job's matrix-core check of the formats K1 and K7 never issue
    (``NTM_MCORE_CHECK=1``) on ``device``, in the Job's sequence: per format of
    ``ops.MCORE_FORMATS`` the decode sweep (256 x 128 x 128, every window) and a dense
    ``size``^3 with the widest operands ``mcore_exact`` allows, each against the reference
    kernel, bitwise; then, with ``big`` > 0 (the Job: 4096), a verified dense ``big``^3 for
    f64 and i8 and ``iters`` timed launches of it. ``corrupt`` flips bit 9 of one element of
    the dense f64 result before its compare; ``max_windows`` cuts every format's decode sweep
    short (the Job runs them all). Returns ``ok``, ``failures`` (the Job's lines),
    ``bad`` per format, ``f64_tflops`` / ``i8_tops`` (host clock around a synchronise: the
    Job's figures are the ones to quote) and ``seconds``. With ``backend=ops.reference`` (CPU)
    every product is the numpy reference itself."""
    o, device, gpu = begin(device, backend)
    t_begin = time.perf_counter()
    out = {"size": size, "bad": {f: 0 for f in o.MCORE_FORMATS}, "failures": [], "f64_tflops": 0.0, "i8_tops": 0.0}

    def product(i: dict, mode: str, flip: bool = False):
        d = o.mcore_to_device(i, device)
        fmt = o.MCORE_FORMATS[i["fmt"]]
        c = o.mcore_gemm(d["a"], d["b"], fmt, d["ai"])
        if flip:
            c.view(torch.int32).view(-1)[2 * (c.numel() // 2 + 5)] ^= 1 << 9
        rep = o.mcore_compare(o.mcore_reference_gpu(d["a"], d["b"], fmt, d["ai"]), c)
        if not rep.ok:
            out["bad"][fmt] += rep.count
            if not any(f.startswith(f"gpu{gpu}: mcore: {fmt} {mode}:") for f in out["failures"]):
                out["failures"].append(o.mcore_failure_message(gpu, fmt, mode, rep.count, rep.first_index,
                                                               rep.expected, rep.got, i["N"]))
        return d, c

    with device_context(device):
        for fmt in o.MCORE_FORMATS:
            for window in range(min(o.mcore_decode_windows(fmt), max_windows or 1 << 30)):
                product(o.mcore_make_inputs("decode", fmt, 256, 128, 128, seed=window), "decode")
            product(o.mcore_make_inputs("dense", fmt, size, size, size, seed=seed), "dense",
                    flip=corrupt and fmt == "f64")
        for fmt, key in (("f64", "f64_tflops"), ("i8", "i8_tops")) if big else ():
            d, c = product(o.mcore_make_inputs("dense", fmt, big, big, big, seed=seed), "dense")
            secs = _wall_time(lambda: o.mcore_gemm(d["a"], d["b"], fmt, d["ai"], out=c), iters, device)
            out[key] = 2.0 * big**3 * iters / secs / 1e12
    return verdict(out, t_begin)
