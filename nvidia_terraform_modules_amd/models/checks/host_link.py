"""K6: the Job's host-link (PCIe) check."""
from __future__ import annotations

import time

import numpy as np
import torch

from ...ops import reference
from .._timing import _wall_time
from ._common import begin, device_context


def host_link_check(device: torch.device, nbytes: int = 64 << 20, iters: int = 3,
                    backend=None) -> dict:
    """K6, the Job's host-link (PCIe) check (``amdgpu-validate --host-link-mib``) on
    ``device`` with one pinned host buffer and one HBM buffer of ``nbytes``: push the HASH
    pattern (device->host), pull and verify it on the device (host->device), push into one
    half while pulling from the other on two streams, ``copy_`` (hipMemcpyAsync) both ways
    on the same buffers, then the pointer chase over 1024 slots and 4096 hops. Rates are
    medians of ``iters``.

    Unlike the Job, which times each kernel with events and reads the error record once
    per pull, this model synchronises per call, as ``hbm_memtest`` documents for K4: each
    ``host_link_pull`` allocates its own record and copies it to the host, and the timings
    are host clocks around a synchronise. The rates therefore read a little low at small
    ``nbytes``; the Job's ``host_link_*_GBps`` are the rates to quote. With
    ``backend=ops.reference`` (CPU) nothing crosses a link and the rates mean nothing."""
    o, device, _ = begin(device, backend)
    gpu = device.type == "cuda"
    nbytes = max(nbytes // 32 * 32, 1024 * reference.HOST_LINK_SLOT_BYTES)
    half = nbytes // 2
    seed = 0x4B36
    t_begin = time.perf_counter()
    host = torch.empty(nbytes // 4, dtype=torch.int32, pin_memory=gpu)
    dev_buf = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
    out = {"bytes": nbytes, "bad_words": 0, "bad_bits": 0, "first_bad_offset": None, "records": [],
           "failed_step": None, "duplex_GBps": 0.0, "h2d_copy_GBps": 0.0, "d2h_copy_GBps": 0.0,
           "read_latency_us": 0.0, "chase_ok": None}

    def timed(fn) -> float:
        return _wall_time(fn, 1, device)

    def bad(rep, step: str) -> bool:
        if rep.ok:
            return False
        out.update(bad_words=rep.bad_words, bad_bits=rep.bad_bits, records=rep.records,
                   first_bad_offset=rep.first_bad_offset, failed_step=step)
        return True

    def rate(n: int, secs: list) -> float:
        return n / float(np.median(secs)) / 1e9

    with device_context(device):
        out["d2h_GBps"] = rate(nbytes, [timed(lambda: o.host_link_push(host, 1, seed=seed))
                                        for _ in range(iters)])
        secs, reps = [], []
        for _ in range(iters):
            secs.append(timed(lambda: reps.append(o.host_link_pull(host, 1, seed=seed))))
            if bad(reps[-1], "pull"):
                break
        out["h2d_GBps"] = rate(nbytes, secs)
        if out["failed_step"] is None:
            lo, hi = host[: half // 4], host[half // 4:]
            side = torch.cuda.Stream(device) if gpu else None

            def duplex():
                o.host_link_push(lo, 1, seed=seed)
                if side is None:
                    reps.append(o.host_link_pull(hi, 1, seed=seed, base=half))
                else:
                    with torch.cuda.stream(side):
                        reps.append(o.host_link_pull(hi, 1, seed=seed, base=half))

            secs = [timed(duplex) for _ in range(iters)]
            out["duplex_GBps"] = rate(2 * half, secs)
            bad(reps[-1], "duplex pull")
            out["h2d_copy_GBps"] = rate(nbytes, [timed(lambda: dev_buf.copy_(host, non_blocking=True))
                                                 for _ in range(iters)])
            out["d2h_copy_GBps"] = rate(nbytes, [timed(lambda: host.copy_(dev_buf, non_blocking=True))
                                                 for _ in range(iters)])
            table = reference.host_link_chase_table(1024, seed)
            slots = host[: table.size * 2]
            slots.view(torch.int64).copy_(torch.from_numpy(table.view(np.int64).reshape(-1)))
            final, ns = o.host_link_chase(slots, 4096)
            want, _ = reference.host_link_chase(slots, 4096)
            out["chase_ok"] = final == want
            out["read_latency_us"] = ns / 1e3
            if final != want and out["failed_step"] is None:
                out["failed_step"] = "chase"
    del host, dev_buf
    out["ok"] = out["bad_words"] == 0 and out["failed_step"] is None
    out["seconds"] = time.perf_counter() - t_begin
    return out
