"""K5: per-CU compute sweep (validation/include/ntm/cu_sweep.hpp, cu_sweep_plan.hpp)."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import torch

from .._lib import check, lib, stream_handle
from ..reference import cu_sweep_expected

CU_SWEEP_SUBTESTS = ("lds", "valu", "mfma_bf16", "mfma_fp8")
CU_SWEEP_MAGIC = 0x4B355357
CU_SWEEP_MAX_LAUNCHES = 8      # cap of the coverage loop
CU_SWEEP_GRID_PER_CU = 4       # workgroups per CU and launch
CU_SWEEP_FAULT_OFF = 0xFFFFFFFF


def cu_sweep_record_dtype():
    """numpy dtype of the 64-byte per-workgroup record (ntm::cus::Record)."""
    dt = np.dtype([("hw_id", "<u4"), ("xcc_id", "<u4"), ("simd", "u1", (4,)), ("magic", "<u4"),
                   ("wg", "<u4"), ("bad", "<u4", (4,)), ("first", "<u4"), ("first_round", "<u4"),
                   ("first_elem", "<u4"), ("expected", "<u8"), ("got", "<u8")])
    assert dt.itemsize == 64
    return dt


def cu_sweep_subtest_id(subtest: int | str) -> int:
    s = CU_SWEEP_SUBTESTS.index(subtest) if subtest in CU_SWEEP_SUBTESTS else subtest
    if s not in (0, 1, 2, 3):
        raise ValueError(f"unknown CU sweep sub-test {subtest!r} {CU_SWEEP_SUBTESTS}")
    return s


def cu_sweep_max_lds_bytes(device=None) -> int:
    """The per-block LDS maximum the runtime reports for ``device``: the default ``lds_bytes``."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    n = lib().ntm_cu_sweep_max_lds_bytes(dev.index if dev.index is not None else torch.cuda.current_device())
    if n <= 0:
        raise RuntimeError("cannot read the device's per-block LDS maximum")
    return n


def cu_sweep(device=None, iters: int = 2, lds_bytes: int | None = None, grid: int | None = None,
             seed: int = 0, fault_key: int | None = None, fault_subtest: int | str | None = None):
    """K5: one launch of the per-CU compute sweep; returns the workgroups' records (a numpy
    structured array, ``cu_sweep_record_dtype``). ``lds_bytes`` defaults to the device's
    per-block maximum, ``grid`` to 4 workgroups per CU. ``fault_key`` (a packed CU key of
    ``cu_sweep_decode``) makes the workgroups on that CU flip one bit of one computed value of
    ``fault_subtest`` before the compare. Expected values come from ``reference.cu_sweep_expected``."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("cu_sweep needs a GPU device")
    limit = cu_sweep_max_lds_bytes(dev)
    lds_bytes = limit if lds_bytes is None else int(lds_bytes)
    if lds_bytes < 16 or lds_bytes % 16 or lds_bytes > limit:
        raise ValueError(f"lds_bytes must be a multiple of 16 in 16 .. {limit}, got {lds_bytes}")
    if grid is None:
        grid = CU_SWEEP_GRID_PER_CU * torch.cuda.get_device_properties(dev).multi_processor_count
    if grid < 1 or not 1 <= iters <= 1024:
        raise ValueError("cu_sweep needs grid >= 1 and 1 <= iters <= 1024")
    if (fault_key is None) != (fault_subtest is None):
        raise ValueError("fault_key and fault_subtest go together")
    key = CU_SWEEP_FAULT_OFF if fault_key is None else int(fault_key) & 0xFFFFFFFF
    sub = 0 if fault_subtest is None else cu_sweep_subtest_id(fault_subtest)
    table = cu_sweep_expected(iters, seed, lds_bytes)["table"]
    with torch.cuda.device(dev):
        exp = torch.from_numpy(table.view(np.int32).copy()).to(dev)
        rec = torch.empty(grid * 16, dtype=torch.int32, device=dev)
        rc = lib().ntm_cu_sweep_launch(rec.data_ptr(), exp.data_ptr(), grid, iters, lds_bytes,
                                       seed & 0xFFFFFFFF, key, sub, stream_handle())
        check(rc, "ntm_cu_sweep_launch")
        raw = rec.cpu().numpy()            # synchronises; exp stays alive until here
    return raw.view(cu_sweep_record_dtype()).copy()


def cu_sweep_decode(hw_id: int, xcc_id: int) -> dict:
    """HW_REG_HW_ID / HW_REG_XCC_ID words -> xcd, se, sh, cu, simd and the packed CU key."""
    out = (ctypes.c_uint * 6)()
    lib().ntm_cu_sweep_decode(int(hw_id) & 0xFFFFFFFF, int(xcc_id) & 0xFFFFFFFF, out)
    return dict(zip(("xcd", "se", "sh", "cu", "simd", "key"), (int(v) for v in out)))


def cu_sweep_summarize(records, cus: int, launches: int = 1, gpu: int = 0) -> dict:
    """Aggregate records (of one or more launches, concatenated) per CU: coverage, workgroups
    per CU, the bad CUs with their first mismatch, ``ok`` and the Job's failure ``message``."""
    recs = np.ascontiguousarray(records, dtype=cu_sweep_record_dtype())
    buf = recs.tobytes()
    n = lib().ntm_cu_sweep_summarize(buf, len(recs), cus, launches, gpu, None, 0)
    out = ctypes.create_string_buffer(n + 1)
    lib().ntm_cu_sweep_summarize(buf, len(recs), cus, launches, gpu, out, n + 1)
    return json.loads(out.value.decode())
