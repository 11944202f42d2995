"""K5: the Job's per-CU compute sweep."""
from __future__ import annotations

import time

import numpy as np
import torch

from ...ops.gpu.cu_sweep import CU_SWEEP_MAX_LAUNCHES
from ._common import begin


def cu_sweep_check(device: torch.device, iters: int = 16, lds_bytes: int | None = None,
                   seed: int = 0, max_launches: int | None = None, fault_key: int | None = None,
                   fault_subtest=None, backend=None) -> dict:
    """K5, the Job's per-CU compute sweep (``amdgpu-validate --cu-sweep``) on ``device``:
    launches of 4 workgroups per CU, each running ``iters`` rounds of the known-answer
    lds / valu / mfma_bf16 / mfma_fp8 sub-tests, until every CU ran a workgroup or
    ``max_launches`` (8) are spent - a cap, not a retry. Returns the summary of
    ``ops.cu_sweep_summarize`` (``ok``, ``cus``, ``cus_covered``, ``simds_covered``,
    ``launches``, ``bad_cus``, ``message`` ...) plus ``lds_bytes`` and ``seconds``. A CU that
    ran nothing fails the check; SIMD coverage is reported only."""
    o, device, gpu = begin(device, backend)
    cap = CU_SWEEP_MAX_LAUNCHES if max_launches is None else max_launches
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    lds = o.cu_sweep_max_lds_bytes(device) if lds_bytes is None else lds_bytes
    t0 = time.perf_counter()
    recs, launches = [], 0
    for launch in range(cap):
        recs.append(o.cu_sweep(device, iters=iters, lds_bytes=lds, seed=seed + launch,
                               fault_key=fault_key, fault_subtest=fault_subtest))
        launches += 1
        if o.cu_sweep_summarize(np.concatenate(recs), cus, launches)["cus_covered"] >= cus:
            break
    out = o.cu_sweep_summarize(np.concatenate(recs), cus, launches, gpu=gpu)
    out["lds_bytes"] = lds
    out["iters"] = iters
    out["seconds"] = time.perf_counter() - t0
    return out
