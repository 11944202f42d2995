"""The lines every opt-in check opens and closes with."""
from __future__ import annotations

import contextlib
import time

import torch

from ... import ops as native


def begin(device, backend=None) -> tuple:
    """(the ops backend, native unless given; ``device`` as a torch.device; its index for ``gpu<N>:`` lines)."""
    device = torch.device(device)
    return backend or native, device, device.index if device.index is not None else 0


def device_context(device: torch.device):
    """``torch.cuda.device(device)`` on a GPU, nothing on the CPU backend."""
    return torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()


def verdict(out: dict, t_begin: float, seconds: str = "seconds") -> dict:
    """Closes a check's report: ``ok``, ``message`` (the first of ``failures``) and the elapsed time."""
    out["ok"] = not out["failures"]
    out["message"] = out["failures"][0] if out["failures"] else ""
    out[seconds] = time.perf_counter() - t_begin
    return out
