#!/usr/bin/env python3
"""Record what the built ``amdgpu-validate`` does with its command line, and the
shape of its report, as fixtures.

Run it BEFORE a change to the Job binary's host code (validation/src/validate/);
the tests then hold the changed binary to the recording:

    python tools/validate_cli_table.py                 # tests/fixtures/validate_cli.json
    python tools/validate_cli_table.py --report-shape  # + validate_report_shape.json (MI355X)

``validate_cli.json`` (no GPU: every vector returns before the first HIP call):
  help           stderr of ``--help``
  describe       stdout of ``--describe-sweep`` for two ``--allreduce-max-mib`` values
  vectors        [argv, env, exit status, first line of stderr]; a vector that parses
                 cleanly carries ``--describe-sweep`` so that it ends there
  tests/test_validate_cli.py replays it and demands byte equality.

``validate_report_shape.json`` (one run with every check on at its smallest size):
  json_paths     the ordered key paths of the JSON document
  prometheus     the ordered ``HELP`` / ``TYPE`` / sample names with their label keys,
                 consecutive repeats counted
  termination    the keys of the termination message
  values         every value that depends on neither time nor rate
  tests/test_validate_report_shape.py runs the same arguments and demands equality.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
FIXTURES = ROOT / "tests" / "fixtures"

VALUED = ["--gpus", "--size", "--iters", "--tflops-floor", "--min-hbm-gb", "--hbm-floor-gbps",
          "--hbm-test-gb", "--hbm-test-passes", "--cu-sweep-iters", "--host-link-mib",
          "--host-link-floor-gbps", "--mx-size", "--mx-tflops-floor", "--xcd-sweep-mib", "--xcd-ratio",
          "--allreduce-max-mib", "--xgmi-sim", "--settle-s", "--fp8-tflops-floor", "--p2p-mib",
          "--p2p-floor-gbps", "--rccl-busbw-floor-gbps", "--xgmi-busbw-floor-gbps", "--xgmi-nblk",
          "--xgmi-one-shot-max", "--out", "--termination-log", "--prom-out", "--fault-inject",
          "--pushgateway"]
SWITCHES = ["--cu-sweep", "--mx-check", "--xcd-sweep", "--rccl", "--no-rccl", "--no-xgmi", "--no-fp8",
            "--no-p2p", "--p2p-loopback", "--xgmi-tune", "--require-host-prep", "--require-iommu-pt",
            "--json"]
# flag -> values on both sides of every bound of the range expression (and the C2 knobs)
BOUNDS = {
    "--size": ["0", "1", "-256"],
    "--iters": ["0", "1"],
    "--p2p-mib": ["0", "1"],
    "--allreduce-max-mib": ["0", "1"],
    "--xgmi-sim": ["-1", "0", "8", "9"],
    "--settle-s": ["-0.001", "0"],
    "--hbm-test-passes": ["0", "1"],
    "--hbm-test-gb": ["nan", "inf", "-1", "0.5"],
    "--cu-sweep-iters": ["0", "1", "1024", "1025"],
    "--host-link-mib": ["-1", "0", "1048576", "1048577"],
    "--host-link-floor-gbps": ["-1", "0"],
    "--mx-size": ["0", "100", "128", "16384", "16512"],
    "--mx-tflops-floor": ["-1", "0"],
    "--xcd-sweep-mib": ["0", "1", "4096", "4097"],
    "--xcd-ratio": ["-0.01", "0", "0.99", "1"],
    "--xgmi-nblk": ["0", "1", "1024", "1025"],
    "--xgmi-one-shot-max": ["-1", "0"],
}
DESCRIBE_MIB = ("1", "8192")

# the run behind validate_report_shape.json: everything on, at the smallest sizes
SHAPE_ARGS = ["--gpus", "1", "--size", "1024", "--iters", "5", "--settle-s", "0", "--hbm-test-gb", "1", "--cu-sweep",
              "--cu-sweep-iters", "1", "--host-link-mib", "16", "--mx-check", "--mx-size", "128",
              "--xcd-sweep", "--xcd-sweep-mib", "16", "--xgmi-sim", "2", "--p2p-loopback", "--p2p-mib", "16",
              "--rccl", "--allreduce-max-mib", "16"]
SHAPE_NODE = "gpu-node-shape"
# keys whose value depends on time, rate or the machine: their VALUES stay out of the fixture
UNSTABLE = re.compile(
    r"(_s|_ms|_us|GBps|gbps|tflops|_rate|_clock_ghz|_median|_min_over_median|_passes|_err|seconds|"
    r"time_us|hbm_total_gb|launches|simds_covered|tflops_aggregate)$|epoch|^(phases_s|host_prep|s)$")
# objects whose keys depend on what the machine lets the process read
OPAQUE = {"host_link_pcie"}


def vectors() -> list[tuple[list[str], dict]]:
    """Every argument vector of the table with its extra environment."""
    out: list[tuple[list[str], dict]] = [(["--definitely-not-an-option"], {})]
    out += [([f], {}) for f in VALUED]                                    # a missing value
    out += [(["--size", "512", f], {}) for f in ("--gpus", "--fault-inject")]  # ... after other flags
    for flag, values in BOUNDS.items():
        out += [([flag, v, "--describe-sweep"], {}) for v in values]
    out.append(([*SWITCHES, "--describe-sweep"], {}))
    out.append((["--gpus", "x", "--size"], {}))
    for kind in ("slow_xcd", "corrupt_xcd"):
        out.append((["--fault-inject", kind], {}))                        # needs --xcd-sweep: exit 2
        out.append(([], {"NTM_FAULT_INJECT": kind}))
        out.append((["--fault-inject", kind, "--xcd-sweep", "--describe-sweep"], {}))
    return out


def run(binary: Path, argv: list[str], env: dict | None = None, timeout: int = 60):
    e = {k: v for k, v in os.environ.items() if k not in ("NTM_FAULT_INJECT", "NODE_NAME")}
    e.update(env or {})
    p = subprocess.run([str(binary), *argv], capture_output=True, text=True, timeout=timeout, env=e)
    return p.returncode, p.stdout, p.stderr


def cli_table(binary: Path) -> dict:
    rc, _, err = run(binary, ["--help"])
    assert rc == 0, err
    table = {"help": err, "describe": {}, "vectors": []}
    for mib in DESCRIBE_MIB:
        rc, out, err = run(binary, ["--describe-sweep", "--allreduce-max-mib", mib])
        assert rc == 0, err
        table["describe"][mib] = out
    for argv, env in vectors():
        rc, _, err = run(binary, argv, env)
        assert rc in (0, 2), (argv, rc)       # a vector that got as far as a GPU is a mistake here
        table["vectors"].append([argv, env, rc, err.splitlines()[0] if err else ""])
    return table


def _paths(v, at: str, paths: list, values: dict) -> None:
    if isinstance(v, dict) and at.rsplit(".", 1)[-1] not in OPAQUE:
        for k, x in v.items():
            _paths(x, f"{at}.{k}" if at else k, paths, values)
    elif isinstance(v, list) and v and all(isinstance(x, dict) for x in v):
        for i, x in enumerate(v):
            _paths(x, f"{at}[{i}]", paths, values)
    else:
        paths.append(at)
        key = re.sub(r"\[\d+\]$", "", at).rsplit(".", 1)[-1]
        top = at.split(".", 1)[0]
        if not UNSTABLE.search(key) and not UNSTABLE.search(top) and key not in OPAQUE:
            values[at] = v


def prometheus_shape(text: str) -> list:
    out: list = []
    for line in text.splitlines():
        if line.startswith("# "):
            kind, name = line.split()[1:3]
            entry = f"{kind} {name}"
        else:
            m = re.match(r"([a-zA-Z_:][\w:]*)(?:\{([^}]*)\})? ", line)
            entry = m.group(1) + "{" + ",".join(re.findall(r"(\w+)=\"", m.group(2) or "")) + "}"
        if out and out[-1][0] == entry:
            out[-1][1] += 1
        else:
            out.append([entry, 1])
    return out


def report_shape(binary: Path, timeout: int = 120) -> dict:
    """Run SHAPE_ARGS once (needs an MI355X) and reduce the three outputs to their shape."""
    with tempfile.TemporaryDirectory() as d:
        term, prom = Path(d) / "term", Path(d) / "m.prom"
        rc, out, err = run(binary, [*SHAPE_ARGS, "--termination-log", str(term), "--prom-out", str(prom)],
                           {"NODE_NAME": SHAPE_NODE}, timeout=timeout)
        if rc != 0:
            raise RuntimeError(f"exit {rc}: {out[-2000:]} {err[-2000:]}")
        paths: list = []
        values: dict = {}
        _paths(json.loads(out.strip().splitlines()[-1]), "", paths, values)
        return {"args": SHAPE_ARGS, "exit": rc, "json_paths": paths, "values": values,
                "prometheus": prometheus_shape(prom.read_text()),
                "termination": list(json.loads(term.read_text()))}


def main(argv: list[str] | None = None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--bin", default=str(BIN), help="the amdgpu-validate to record")
    ap.add_argument("--out-dir", default=str(FIXTURES))
    ap.add_argument("--report-shape", action="store_true",
                    help="also run the binary once on the GPU and record validate_report_shape.json")
    args = ap.parse_args(argv)
    out = Path(args.out_dir)
    out.mkdir(parents=True, exist_ok=True)
    t = cli_table(Path(args.bin))
    (out / "validate_cli.json").write_text(json.dumps(t, indent=1) + "\n")
    print(f"{out / 'validate_cli.json'}: {len(t['vectors'])} vectors")
    if args.report_shape:
        s = report_shape(Path(args.bin))
        (out / "validate_report_shape.json").write_text(json.dumps(s, indent=1) + "\n")
        print(f"{out / 'validate_report_shape.json'}: {len(s['json_paths'])} paths, {len(s['values'])} values")
    return 0


if __name__ == "__main__":
    sys.exit(main())
