"""Synchronise and time on a device: shared by the flagship workload and the opt-in checks."""
from __future__ import annotations

import time

import torch


def _sync(device: torch.device) -> None:
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def _wall_time(fn, iters: int, device: torch.device) -> float:
    """Seconds ``iters`` calls take by the host clock, a synchronise before and after."""
    _sync(device)
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    _sync(device)
    return time.perf_counter() - t0


def _time_loop(fn, iters: int, device: torch.device) -> float:
    """Seconds per call: events on the current stream (wall clock on CPU)."""
    if device.type != "cuda":
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) / iters
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize(device)
    return s.elapsed_time(e) / 1e3 / iters
