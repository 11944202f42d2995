"""``NTM_WAVE_CHECK=1 amdgpu-validate``: stage K12, wave data paths and the special-function unit,
in the Job binary - a clean run with its keys and gauges, the injection, and a default run in
which the check is invisible."""
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
KEYS = ("wave_lane_bad", "wave_ldstr_bad", "wave_valu_bad", "wave_sfu_inconsistent", "wave_sfu_max_distance",
        "wave_sfu_beyond_bound", "wave_cus_covered", "wave_seconds")
SFU = ("v_exp_f32", "v_log_f32", "v_rcp_f32", "v_rsq_f32", "v_sqrt_f32", "v_sin_f32", "v_cos_f32")


def _run(*args, on=True, timeout=300):
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = {k: v for k, v in os.environ.items() if k not in ("NTM_FAULT_INJECT", "NODE_NAME", "NTM_WAVE_CHECK")}
    if on:
        e["NTM_WAVE_CHECK"] = "1"
    p = subprocess.run([str(BIN), *BASE, *args], capture_output=True, text=True, timeout=timeout, env=e)
    return p.returncode, p.stdout, p.stderr


def _last_json(out):
    return json.loads(out.strip().splitlines()[-1])


def test_clean_run_passes_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run("--prom-out", str(prom))
    g0 = _last_json(out)["gpus"][0]
    print({k: v for k, v in g0.items() if k.startswith("wave_")})
    assert rc == 0, out + err
    assert all(k in g0 for k in KEYS)
    assert g0["wave_lane_bad"] == g0["wave_ldstr_bad"] == g0["wave_valu_bad"] == g0["wave_sfu_inconsistent"] == 0
    assert g0["wave_sfu_beyond_bound"] == 0 and g0["wave_cus_covered"] > 0 and g0["wave_seconds"] > 0
    assert set(g0["wave_sfu_max_distance"]) == set(SFU)
    metrics = prom.read_text()
    for fam in ("lane", "ldstr", "sfu", "valu"):
        assert f'amdgpu_validate_wave_bad{{gpu="0",family="{fam}"}} 0' in metrics
    assert 'amdgpu_validate_wave_seconds{gpu="0"} ' in metrics


def test_corrupt_wave_names_cu_op_and_lane():
    rc, out, err = _run("--fault-inject", "corrupt_wave")
    assert rc == 1, out + err
    rep = _last_json(out)
    assert len(rep["failures"]) == 1, rep["failures"]
    line = rep["failures"][0]
    m = re.match(r"gpu0: wave lane row_shr:3 bound_ctrl:0: xcd (\d+) se (\d+) sh (\d+) cu (\d+) simd (\d+) lane 19: expected "
                 r"(0x[0-9a-f]{8}), got (0x[0-9a-f]{8}), bad bits 0x00000400$", line)
    assert m and len(line) < 200, line
    assert int(m.group(6), 16) ^ int(m.group(7), 16) == 0x400
    assert rep["gpus"][0]["wave_lane_bad"] == 1


def test_corrupt_wave_sfu_names_cu_instruction_and_input():
    rc, out, err = _run("--fault-inject", "corrupt_wave_sfu")
    assert rc == 1, out + err
    rep = _last_json(out)
    assert len(rep["failures"]) == 1, rep["failures"]
    line = rep["failures"][0]
    m = re.match(r"gpu0: wave sfu v_exp_f32: xcd \d+ se \d+ sh \d+ cu \d+ simd \d+ element 1000 input (0x[0-9a-f]{8}): expected "
                 r"(0x[0-9a-f]{8}), got (0x[0-9a-f]{8}), bad bits 0x00000400$", line)
    assert m and len(line) < 200, line
    g0 = rep["gpus"][0]
    assert g0["wave_sfu_inconsistent"] >= 1 and g0["wave_lane_bad"] == 0 and g0["wave_sfu_beyond_bound"] == 0


@pytest.mark.parametrize("fault", ["corrupt_wave", "corrupt_wave_sfu"])
def test_fault_without_the_variable_is_refused(fault):
    rc, out, err = _run("--fault-inject", fault, on=False)
    assert rc == 2 and f"fault-inject {fault} needs NTM_WAVE_CHECK=1" in err and out == ""


def test_without_the_variable_nothing_mentions_the_check(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run("--prom-out", str(prom), "--termination-log", str(term), on=False)
    assert rc == 0, out + err
    assert "wave" not in out.strip().splitlines()[-1]
    assert "wave" not in prom.read_text() and "wave" not in term.read_text()
    on_help = subprocess.run([str(BIN), "--help"], capture_output=True, text=True, timeout=60,
                             env={**os.environ, "NTM_WAVE_CHECK": "1"})
    off_help = subprocess.run([str(BIN), "--help"], capture_output=True, text=True, timeout=60)
    assert on_help.stdout + on_help.stderr == off_help.stdout + off_help.stderr
    assert "wave" not in (off_help.stdout + off_help.stderr).lower()
