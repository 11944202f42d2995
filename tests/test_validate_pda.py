"""``NTM_PDA_CHECK=1 amdgpu-validate``: stage K14, the paged-KV decode attention check, in the Job
binary - a clean run with its keys and gauges, the injection, and a default run in which the check
is invisible."""
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
KEYS = ("pda_exact_bad", "pda_dense_bad", "pda_dense_worst_err_over_a", "pda_cus_covered", "pda_launches", "pda_splits",
        "pda_kv_gbps", "pda_seconds")


def _run(*args, on=True, timeout=300):
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = {k: v for k, v in os.environ.items() if k not in ("NTM_FAULT_INJECT", "NODE_NAME", "NTM_PDA_CHECK")}
    if on:
        e["NTM_PDA_CHECK"] = "1"
    p = subprocess.run([str(BIN), *BASE, *args], capture_output=True, text=True, timeout=timeout, env=e)
    return p.returncode, p.stdout, p.stderr


def _last_json(out):
    return json.loads(out.strip().splitlines()[-1])


def test_clean_run_passes_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run("--prom-out", str(prom))
    g0 = _last_json(out)["gpus"][0]
    print({k: v for k, v in g0.items() if k.startswith("pda_")})
    assert rc == 0, out + err
    assert all(k in g0 for k in KEYS)
    assert g0["pda_exact_bad"] == 0 and g0["pda_dense_bad"] == 0
    assert 0 < g0["pda_dense_worst_err_over_a"] < 2.0 ** -7
    assert g0["pda_cus_covered"] > 0 and 2 <= g0["pda_launches"] <= 16 and 1 <= g0["pda_splits"] <= 64
    assert g0["pda_kv_gbps"] > 0 and g0["pda_seconds"] > 0
    metrics = prom.read_text()
    assert 'amdgpu_validate_pda_bad{gpu="0"} 0' in metrics
    assert 'amdgpu_validate_pda_kv_gbps{gpu="0"} ' in metrics and 'amdgpu_validate_pda_seconds{gpu="0"} ' in metrics


def test_corrupt_pda_names_sequence_head_token_column_cus_and_bits():
    rc, out, err = _run("--fault-inject", "corrupt_pda")
    assert rc == 1, out + err
    rep = _last_json(out)
    assert len(rep["failures"]) == 1, rep["failures"]
    line = rep["failures"][0]
    m = re.match(r"gpu0: pda exact T1 O: seq (\d+) head (\d+) tok 0 col (\d+): cu( \d+\.\d+\.\d+\.\d+){2} \(xcd\.se\.sh\.cu\): "
                 r"expected (0x[0-9a-f]{8}), got (0x[0-9a-f]{8}), bad bits 0x00080000; 1 differ$", line)
    assert m and len(line) < 200, line
    assert int(m.group(5), 16) ^ int(m.group(6), 16) == 0x80000
    assert rep["gpus"][0]["pda_exact_bad"] == 1 and rep["gpus"][0]["pda_dense_bad"] == 0


def test_fault_without_the_variable_is_refused():
    rc, out, err = _run("--fault-inject", "corrupt_pda", on=False)
    assert rc == 2 and "fault-inject corrupt_pda needs NTM_PDA_CHECK=1" in err and out == ""


def test_without_the_variable_nothing_mentions_the_check(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run("--prom-out", str(prom), "--termination-log", str(term), on=False)
    assert rc == 0, out + err
    assert "pda" not in out.strip().splitlines()[-1]
    assert "pda" not in prom.read_text() and "pda" not in term.read_text()
    on_help = subprocess.run([str(BIN), "--help"], capture_output=True, text=True, timeout=60,
                             env={**os.environ, "NTM_PDA_CHECK": "1"})
    off_help = subprocess.run([str(BIN), "--help"], capture_output=True, text=True, timeout=60)
    assert on_help.stdout + on_help.stderr == off_help.stdout + off_help.stderr
    assert "pda" not in (off_help.stdout + off_help.stderr).lower()
