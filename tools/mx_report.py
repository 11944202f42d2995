"""K7 measurements with the Job binary (profiles/mx/README.md): the MXFP4 rate beside K1-fp8's
at 4096^3 and 8192^3 in one process each, the stage's seconds over 5 runs, and the
default-off verdict time (``phases_s.end``) against another binary, 5 runs each, interleaved.

    python tools/mx_report.py --out DIR [--parent-bin PATH]
"""
import argparse
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "validation" / "build" / "amdgpu-validate"


def run(binary, *args):
    p = subprocess.run([str(binary), "--gpus", "1", "--json", *args], capture_output=True, text=True,
                       timeout=600)
    if p.returncode != 0:
        sys.exit(f"{binary} {' '.join(args)}: exit {p.returncode}\n{p.stdout[-2000:]}{p.stderr[-2000:]}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", required=True)
    ap.add_argument("--parent-bin")
    a = ap.parse_args()
    out = Path(a.out)
    out.mkdir(parents=True, exist_ok=True)
    rep = {"rates": [], "stage_s": [], "flag_off_end_s": {"this": [], "parent": []}}
    for size in (4096, 8192):
        g = run(BIN, "--size", str(size), "--mx-check", "--mx-size", str(size))["gpus"][0]
        row = {"size": size, "mx_fp4_tflops": g["mx_fp4_tflops"], "gemm_fp8_tflops": g["gemm_fp8_tflops"],
               "gemm_bf16_tflops": g.get("gemm_tflops"), "mx_scale_spread": g["mx_scale_spread"],
               "mx_bad_elements": g["mx_bad_elements"], "mx_s": g["mx_s"]}
        rep["rates"].append(row)
        print(row, flush=True)
    for _ in range(5):
        g = run(BIN, "--size", "8192", "--mx-check")["gpus"][0]
        rep["stage_s"].append(g["mx_s"])
    print("stage mx_s (default --mx-size 4096):", rep["stage_s"], "median",
          statistics.median(rep["stage_s"]), flush=True)
    if a.parent_bin:
        for _ in range(5):
            rep["flag_off_end_s"]["parent"].append(run(a.parent_bin, "--size", "8192")["phases_s"]["end"])
            rep["flag_off_end_s"]["this"].append(run(BIN, "--size", "8192")["phases_s"]["end"])
        for k, v in rep["flag_off_end_s"].items():
            print(f"flag off, {k}: median {statistics.median(v):.3f} s ({min(v):.3f} - {max(v):.3f})", flush=True)
    (out / "report.json").write_text(json.dumps(rep, indent=1) + "\n")


if __name__ == "__main__":
    main()
