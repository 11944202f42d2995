"""``NTM_MXQ_CHECK=1 amdgpu-validate``: stage K11, MX quantise / dequantise on the device, in the
Job binary - a clean run with its keys and gauges, the injection, and a default run in which
the check is invisible."""
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
BASE = ("--gpus", "1", "--size", "1024", "--iters", "2", "--no-fp8")
FORMATS = ("e4m3", "e5m2", "e2m3", "e3m2", "e2m1")
SUBS = ("down", "up", "block", "e2e")


def _run(*args, on=True, timeout=300):
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = {k: v for k, v in os.environ.items() if k not in ("NTM_FAULT_INJECT", "NODE_NAME", "NTM_MXQ_CHECK")}
    if on:
        e["NTM_MXQ_CHECK"] = "1"
    p = subprocess.run([str(BIN), *BASE, *args], capture_output=True, text=True, timeout=timeout, env=e)
    return p.returncode, p.stdout, p.stderr


def _last_json(out):
    return json.loads(out.strip().splitlines()[-1])


def test_clean_run_passes_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run("--prom-out", str(prom))
    g0 = _last_json(out)["gpus"][0]
    print({k: v for k, v in g0.items() if k.startswith("mxq_") or k == "hbm_copy_GBps"})
    assert rc == 0, out + err
    assert g0["mxq_formats"] == list(FORMATS)
    for fmt in FORMATS:
        for sub in SUBS:
            assert g0[f"mxq_{fmt}_{sub}_bad"] == 0
    assert g0["mxq_quantize_GBps"] > 0 and g0["mxq_seconds"] > 0
    metrics = prom.read_text()
    for fmt in FORMATS:
        assert f'amdgpu_validate_mxq_bad{{gpu="0",format="{fmt}"}} 0' in metrics
    assert 'amdgpu_validate_mxq_quantize_gbps{gpu="0"} ' in metrics
    assert 'amdgpu_validate_mxq_seconds{gpu="0"} ' in metrics


def test_corrupt_mxq_names_format_subtest_row_and_element():
    rc, out, err = _run("--fault-inject", "corrupt_mxq")
    assert rc == 1, out + err
    rep = _last_json(out)
    assert len(rep["failures"]) == 1, rep["failures"]
    line = rep["failures"][0]
    m = re.match(r"gpu0: mxq e2m1 block: 1 bad word\(s\), first at row (\d+) element (\d+): expected "
                 r"(0x[0-9a-f]{8}), got (0x[0-9a-f]{8}), bad bits (0x[0-9a-f]{8})$", line)
    assert m and len(line) < 200, line
    flipped = int(m.group(3), 16) ^ int(m.group(4), 16)
    assert flipped == int(m.group(5), 16) and bin(flipped).count("1") == 1, line
    g0 = rep["gpus"][0]
    assert g0["mxq_e2m1_block_bad"] == 1
    assert sum(g0[f"mxq_{fmt}_{sub}_bad"] for fmt in FORMATS for sub in SUBS) == 1


def test_fault_without_the_variable_is_refused():
    rc, out, err = _run("--fault-inject", "corrupt_mxq", on=False)
    assert rc == 2 and "fault-inject corrupt_mxq needs NTM_MXQ_CHECK=1" in err and out == ""


def test_without_the_variable_nothing_mentions_the_check(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run("--prom-out", str(prom), "--termination-log", str(term), on=False)
    assert rc == 0, out + err
    assert "mxq" not in out.strip().splitlines()[-1]
    assert "mxq" not in prom.read_text() and "mxq" not in term.read_text()
