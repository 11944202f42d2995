"""``NTM_MCORE_CHECK=1 amdgpu-validate``: stage K10, the fp64 / fp32 / fp16 / int8 / 2:4-sparse
matrix-core check, in the Job binary - a clean run with its keys and gauges, the injection,
and a default run in which the check is invisible."""
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
FORMATS = ("f64", "f32", "f16", "i8", "sp_bf16", "sp_i8")


def _run(*args, on=True, timeout=300):
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = {k: v for k, v in os.environ.items() if k not in ("NTM_FAULT_INJECT", "NODE_NAME", "NTM_MCORE_CHECK")}
    if on:
        e["NTM_MCORE_CHECK"] = "1"
    p = subprocess.run([str(BIN), *BASE, *args], capture_output=True, text=True, timeout=timeout, env=e)
    return p.returncode, p.stdout, p.stderr


def _last_json(out):
    return json.loads(out.strip().splitlines()[-1])


def test_clean_run_passes_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run("--prom-out", str(prom))
    g0 = _last_json(out)["gpus"][0]
    print({k: v for k, v in g0.items() if k.startswith("mcore_")})
    assert rc == 0, out + err
    assert g0["mcore_formats"] == list(FORMATS)
    for fmt in FORMATS:
        assert g0[f"mcore_{fmt}_bad"] == 0
    assert g0["mcore_f64_tflops"] > 0 and g0["mcore_i8_tops"] > 0 and g0["mcore_seconds"] > 0
    metrics = prom.read_text()
    for fmt in FORMATS:
        assert f'amdgpu_validate_mcore_bad{{gpu="0",format="{fmt}"}} 0' in metrics
    assert 'amdgpu_validate_mcore_rate{gpu="0",format="f64"} ' in metrics
    assert 'amdgpu_validate_mcore_rate{gpu="0",format="i8"} ' in metrics


def test_corrupt_mcore_names_format_row_and_column():
    rc, out, err = _run("--fault-inject", "corrupt_mcore")
    assert rc == 1, out + err
    rep = _last_json(out)
    assert len(rep["failures"]) == 1, rep["failures"]
    m = re.match(r"gpu0: mcore: f64 dense: row (\d+) col (\d+): expected (0x[0-9a-f]{16}), got (0x[0-9a-f]{16}), "
                 r"bad bits 0x200; 1 differ$", rep["failures"][0])
    assert m and int(m.group(3), 16) ^ int(m.group(4), 16) == 0x200, rep["failures"][0]
    g0 = rep["gpus"][0]
    assert g0["mcore_f64_bad"] == 1 and sum(g0[f"mcore_{fmt}_bad"] for fmt in FORMATS) == 1


def test_fault_without_the_variable_is_refused():
    rc, out, err = _run("--fault-inject", "corrupt_mcore", on=False)
    assert rc == 2 and "fault-inject corrupt_mcore needs NTM_MCORE_CHECK=1" in err and out == ""


def test_without_the_variable_nothing_mentions_the_check(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run("--prom-out", str(prom), "--termination-log", str(term), on=False)
    assert rc == 0, out + err
    assert "mcore" not in out.strip().splitlines()[-1]
    assert "mcore" not in prom.read_text() and "mcore" not in term.read_text()
