#!/usr/bin/env python3
"""K5 measurements on one MI355X (profiles/cu_sweep/README.md): launches needed to
cover every CU and workgroups per CU, SIMD coverage, time per launch over iters and
LDS size (lds_bytes = 16 leaves the valu + MFMA sub-tests, the difference to the full
size is the lds sub-test), the largest dynamic LDS the runtime grants, the Job's sweep
seconds, and the default-off verdict time against another binary (--parent-bin).

  python tools/cu_sweep_report.py [--out DIR] [--iters 16] [--parent-bin PATH] [--ab-runs 7]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from nvidia_terraform_modules_amd import ops  # noqa: E402
from nvidia_terraform_modules_amd.ops import reference  # noqa: E402
from nvidia_terraform_modules_amd.ops.gpu import cu_sweep as k5  # noqa: E402
from nvidia_terraform_modules_amd.ops._lib import lib, stream_handle  # noqa: E402

BIN = ROOT / "validation" / "build" / "amdgpu-validate"


def keys(rec):
    return ((rec["xcc_id"] & 0xF).astype(np.int64) << 8 | ((rec["hw_id"] >> 13) & 7) << 5 |
            ((rec["hw_id"] >> 12) & 1) << 4 | (rec["hw_id"] >> 8) & 0xF)


def coverage(cus, iters, trials):
    rows = []
    for t in range(trials):
        recs, launches = [], 0
        first = None
        while launches < k5.CU_SWEEP_MAX_LAUNCHES:
            recs.append(ops.cu_sweep("cuda:0", iters=iters, seed=launches))
            launches += 1
            s = ops.cu_sweep_summarize(np.concatenate(recs), cus, launches)
            first = first or dict(s)
            if s["cus_covered"] >= cus:
                break
        simds = {}
        for r in np.concatenate(recs):
            simds.setdefault(int(keys(r[None])[0]), set()).update(int(x) for x in r["simd"])
        rows.append({"trial": t, "launches": launches, "ok": s["ok"],
                     "first_launch_cus_covered": first["cus_covered"],
                     "first_launch_wg_per_cu": [first["wg_per_cu_min"], first["wg_per_cu_max"]],
                     "wg_per_cu": [s["wg_per_cu_min"], s["wg_per_cu_max"]],
                     "simds_covered": s["simds_covered"],
                     "cus_with_4_simds": sum(len(v) == 4 for v in simds.values()),
                     "waves_on_distinct_simds": int(sum(len(set(r["simd"].tolist())) == 4
                                                        for r in recs[0])), "workgroups": len(recs[0])})
    return rows


def time_launch(cus, iters, lds_bytes, grid, reps=7):
    """Median milliseconds of one launch (events around the C ABI call: memset + kernel)."""
    table = reference.cu_sweep_expected(iters, 0, lds_bytes)["table"]
    exp = torch.from_numpy(table.view(np.int32).copy()).cuda()
    rec = torch.empty(grid * 16, dtype=torch.int32, device="cuda")
    ms = []
    for i in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = lib().ntm_cu_sweep_launch(rec.data_ptr(), exp.data_ptr(), grid, iters, lds_bytes, 0,
                                       0xFFFFFFFF, 0, stream_handle())
        e1.record()
        torch.cuda.synchronize()
        if rc:
            return None
        if i >= 2:
            ms.append(e0.elapsed_time(e1))
    assert not rec.cpu().numpy().view(ops.cu_sweep_record_dtype())["bad"].any()
    return round(statistics.median(ms), 4)


def run_job(binary, *args):
    t0 = time.perf_counter()
    p = subprocess.run([str(binary), "--gpus", "1", "--size", "8192", "--json", *args],
                       capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        raise RuntimeError(f"{binary} exited {p.returncode}: {p.stderr[-400:]}")
    return json.loads(p.stdout.strip().splitlines()[-1]), wall


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--iters", type=int, default=16)
    ap.add_argument("--parent-bin", default="")
    ap.add_argument("--ab-runs", type=int, default=7)
    ap.add_argument("--trials", type=int, default=3)
    a = ap.parse_args()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lds = ops.cu_sweep_max_lds_bytes("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "cus": cus, "lds_bytes_attribute": lds,
           "iters": a.iters}
    # the largest dynamic LDS: the attribute's value must launch, 16 bytes more must be refused
    rec = torch.zeros(16, dtype=torch.int32, device="cuda")
    exp = torch.from_numpy(reference.cu_sweep_expected(1, 0, 16)["table"].view(np.int32).copy()).cuda()
    over = lib().ntm_cu_sweep_launch(rec.data_ptr(), exp.data_ptr(), 1, 1, lds + 16, 0, 0xFFFFFFFF, 0,
                                     stream_handle())
    torch.cuda.synchronize()
    out["launch_rc_at_attribute_plus_16"] = over
    out["coverage"] = coverage(cus, a.iters, a.trials)
    print(json.dumps({"coverage": out["coverage"]}), flush=True)
    grid = k5.CU_SWEEP_GRID_PER_CU * cus
    timing = []
    for it in sorted({1, 2, 4, 8, a.iters, 2 * a.iters}):
        full, small = time_launch(cus, it, lds, grid), time_launch(cus, it, 16, grid)
        one = time_launch(cus, it, lds, cus)
        timing.append({"iters": it, "launch_ms_full_lds": full, "launch_ms_lds16": small,
                       "lds_subtest_ms": round(full - small, 4), "launch_ms_grid_1_per_cu": one,
                       "us_per_workgroup_round": round(one * 1e3 / it, 2)})
        print(json.dumps(timing[-1]), flush=True)
    out["timing"] = timing
    if BIN.exists():
        jobs = []
        for _ in range(3):
            j, wall = run_job(BIN, "--cu-sweep", "--cu-sweep-iters", str(a.iters))
            g = j["gpus"][0]
            jobs.append({"verdict_s": j["phases_s"]["end"], "wall_s": round(wall, 3),
                         **{k: v for k, v in g.items() if k.startswith("cu_sweep")}})
        out["job_with_sweep"] = jobs
        print(json.dumps({"job_with_sweep": jobs}), flush=True)
        if a.parent_bin:
            ab = {"parent": [], "new": []}
            for i in range(a.ab_runs):
                order = [("parent", a.parent_bin), ("new", BIN)]
                for name, b in (order if i % 2 == 0 else order[::-1]):
                    ab[name].append(run_job(b)[0]["phases_s"]["end"])
            out["default_off_ab"] = {
                k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                    "max": round(max(v), 4), "runs": [round(x, 4) for x in v]} for k, v in ab.items()}
            print(json.dumps({"default_off_ab": out["default_off_ab"]}), flush=True)
    if a.out:
        Path(a.out).mkdir(parents=True, exist_ok=True)
        (Path(a.out) / "report.json").write_text(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
