"""K8: the Job's per-XCD sweep."""
from __future__ import annotations

import time

import numpy as np
import torch

from ._common import begin


def xcd_sweep_check(device: torch.device, hbm_mib: int = 256, ratio: float = 0.0, seed: int = 0x4B38,
                    slow_xcd: int | None = None, slow_factor: int = 4, corrupt_xcd: int | None = None,
                    levels=("l2", "mall", "hbm", "mfma"), backend=None) -> dict:
    """K8, the Job's per-XCD sweep (``amdgpu-validate --xcd-sweep``) on ``device``: a buffer of
    ``xcds x hbm_mib`` MiB filled with K4's hash pattern; per level (``l2`` 1 MiB, ``mall``
    16 MiB, ``hbm`` ``hbm_mib`` per XCD) every XCD reads and verifies its own slice alone (one
    launch per XCD) and together (one launch); ``mfma`` is the clock probe under matrix load.
    Each cell runs once to warm up and to size its passes for spans of at least 100 us, then
    for the record. Returns ``ok``, ``failures``, ``seconds``, ``xcds`` and ``cells``: the
    summaries of ``ops.xcd_sweep_summarize`` keyed ``"<level>/<mode>"``, each with ``passes``.
    The ratio applies to the cells ``ops.xcd_sweep_gated`` names; the others are reported.
    ``corrupt_xcd`` flips one bit of that XCD's ``hbm`` slice before the ``hbm`` level."""
    o, device, gpu = begin(device, backend)
    xcds = o.xcd_sweep_xcds(device)
    t0 = time.perf_counter()
    buf = torch.empty(xcds * hbm_mib << 20, dtype=torch.uint8, device=device)
    o.hbm_pattern_write(buf, "hash", seed)
    slow = dict(slow_xcd=slow_xcd, slow_factor=slow_factor if slow_xcd is not None else 1)
    cells, failures = {}, []

    def run(level, mode, passes, r):
        masks = [1 << x for x in range(xcds)] if mode == "alone" else [(1 << xcds) - 1]
        if level == "mfma":
            recs = [o.xcd_sweep_mfma(device, batches=passes, xcd_mask=m, **slow) for m in masks]
            expected = 0
        else:
            mib = min({"l2": 1, "mall": 16}.get(level, hbm_mib), hbm_mib)
            part = buf[: xcds * mib << 20]
            recs = [o.xcd_sweep_read(part, "hash", seed, m, passes, **slow) for m in masks]
            expected = passes * (mib << 20) // (64 * 1024)
        out = o.xcd_sweep_summarize(np.concatenate(recs), level, mode, xcds, ratio=r, gpu=gpu,
                                    expected_tiles=expected)
        out["passes"] = passes
        return out

    for level in levels:
        if level == "hbm" and corrupt_xcd is not None:
            off = (corrupt_xcd * hbm_mib << 20) + (hbm_mib << 19) + 40
            buf[off] ^= 2
        for mode in ("alone", "together"):
            if level == "mfma" and mode == "alone":
                continue
            passes = {"l2": 64, "mall": 4, "hbm": 1, "mfma": 16}[level]
            def timed(c):       # the XCDs that timed something; one that ran nothing fails on its own
                return [p["span_ticks"] for p in c["per_xcd"] if p["span_ticks"]]

            cell = run(level, mode, passes, 0.0)
            for _ in range(2):
                spans = timed(cell)
                if spans and min(spans) < 10000:
                    passes = min(-(-passes * 2 * 10000 // min(spans)), 65536 if level == "mfma" else 1 << 20)
                cell = run(level, mode, passes, ratio if o.xcd_sweep_gated(level, mode) else 0.0)
                if not timed(cell) or min(timed(cell)) >= 10000:
                    break
            cells[f"{level}/{mode}"] = cell
            failures += cell["failures"]
    torch.cuda.synchronize(device)
    return {"ok": not failures, "failures": failures, "message": failures[0] if failures else "",
            "xcds": xcds, "hbm_mib": hbm_mib, "ratio": ratio, "cells": cells,
            "seconds": time.perf_counter() - t0}
