#!/usr/bin/env python3
"""K8 XCD sweep report: runs ``amdgpu-validate --xcd-sweep`` N times and prints, per level
and mode, every XCD's rate and clock and min / median, the passes chosen and the spans they
gave, and the seconds the stage adds; ``--parent BIN`` interleaves default (flag-off) runs
of this build with another binary and compares the verdict times.

    python tools/xcd_sweep_report.py --runs 5 --out profiles/xcd_sweep/run1 [--parent BIN]
"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
BASE = ["--gpus", "1", "--size", "1024", "--iters", "5", "--no-fp8"]
CELLS = ("l2_alone", "l2_together", "mall_alone", "mall_together", "hbm_alone", "hbm_together",
         "mfma_together")


def run(binary, *args, timeout=600):
    t0 = time.perf_counter()
    p = subprocess.run([str(binary), *BASE, *args], capture_output=True, text=True, timeout=timeout)
    dt = time.perf_counter() - t0
    if p.returncode not in (0, 1):
        sys.exit(f"{binary} exited {p.returncode}: {p.stderr[-400:]}")
    return json.loads(p.stdout.strip().splitlines()[-1]), dt, p.returncode


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mib", type=int, default=256, help="--xcd-sweep-mib")
    ap.add_argument("--parent", help="another amdgpu-validate for the flag-off comparison")
    ap.add_argument("--out", help="directory for report.json")
    a = ap.parse_args()
    if not BIN.exists():
        sys.exit("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    runs = []
    for i in range(a.runs):
        rep, dt, rc = run(BIN, "--xcd-sweep", "--xcd-sweep-mib", str(a.mib))
        g = rep["gpus"][0]
        runs.append({"wall_s": dt, "rc": rc, "verdict_s": rep["phases_s"]["end"],
                     **{k: v for k, v in g.items() if k.startswith("xcd_sweep")}})
    out = {"mib": a.mib, "runs": runs, "cells": {}}
    print(f"{a.runs} runs, {a.mib} MiB per XCD at hbm; rates in GB/s (mfma: GMFMA/s), last run shown")
    for c in CELLS:
        mm = [r[f"xcd_sweep_{c}_min_over_median"] for r in runs]
        last = runs[-1]
        out["cells"][c] = {"min_over_median": mm, "lowest": min(mm), "range": max(mm) - min(mm),
                           "passes": [r[f"xcd_sweep_{c}_passes"] for r in runs],
                           "span_us": [r[f"xcd_sweep_{c}_span_us"] for r in runs]}
        print(f"{c:14s} rate {' '.join(f'{v:7.1f}' for v in last[f'xcd_sweep_{c}_rate'])}  "
              f"clock {' '.join(f'{v:4.2f}' for v in last[f'xcd_sweep_{c}_clock_ghz'])}  "
              f"min/median {' '.join(f'{v:.3f}' for v in mm)}  lowest {min(mm):.3f} range {max(mm) - min(mm):.3f}  "
              f"passes {last[f'xcd_sweep_{c}_passes']} span_us {last[f'xcd_sweep_{c}_span_us']}")
    out["stage_s"] = [r["xcd_sweep_s"] for r in runs]
    print(f"stage seconds: {' '.join(f'{v:.3f}' for v in out['stage_s'])}  median "
          f"{statistics.median(out['stage_s']):.3f}; failures: {sum(len(r['xcd_sweep_failures']) for r in runs)}")
    if a.parent:
        mine, theirs = [], []
        for i in range(max(a.runs, 5)):                     # interleaved
            theirs.append(run(a.parent)[0]["phases_s"]["end"])
            mine.append(run(BIN)[0]["phases_s"]["end"])
        out["flag_off"] = {"this_s": mine, "parent_s": theirs}
        inside = min(theirs) <= statistics.median(mine) <= max(theirs)
        print(f"flag off, verdict seconds: this {' '.join(f'{v:.3f}' for v in mine)} median "
              f"{statistics.median(mine):.3f}; parent {' '.join(f'{v:.3f}' for v in theirs)} median "
              f"{statistics.median(theirs):.3f} range {min(theirs):.3f}-{max(theirs):.3f}; "
              f"this median inside the parent's range: {inside}")
    if a.out:
        d = Path(a.out)
        d.mkdir(parents=True, exist_ok=True)
        (d / "report.json").write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
