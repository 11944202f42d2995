"""``amdgpu-validate --cu-sweep``: stage K5, the per-CU compute sweep, in the Job
binary - a clean run, the native fault injection that must fail the Job naming
exactly one CU, and a default run in which the sweep is invisible."""
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
BASE = ("--gpus", "1", "--size", "1024", "--iters", "5", "--no-fp8")


def _run(*args, timeout=300):
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = dict(os.environ)
    e.pop("NTM_FAULT_INJECT", None)
    e.pop("NODE_NAME", None)
    p = subprocess.run([str(BIN), *args], capture_output=True, text=True, timeout=timeout, env=e)
    return p.returncode, p.stdout, p.stderr


def _last_json(out):
    return json.loads(out.strip().splitlines()[-1])


def test_cu_sweep_passes_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run(*BASE, "--cu-sweep", "--prom-out", str(prom))
    assert rc == 0, out + err
    g0 = _last_json(out)["gpus"][0]
    for k in ("cu_sweep_cus", "cu_sweep_cus_covered", "cu_sweep_simds_covered", "cu_sweep_launches",
              "cu_sweep_bad_cus", "cu_sweep_lds_bytes", "cu_sweep_s"):
        assert k in g0, k
    print({k: v for k, v in g0.items() if k.startswith("cu_sweep")})
    assert g0["cu_sweep_cus"] > 0 and g0["cu_sweep_cus_covered"] == g0["cu_sweep_cus"]
    assert g0["cu_sweep_bad_cus"] == [] and 1 <= g0["cu_sweep_launches"] <= 8
    assert g0["cu_sweep_lds_bytes"] >= 64 * 1024 and g0["cu_sweep_s"] > 0
    assert g0["cu_sweep_simds_covered"] <= 4 * g0["cu_sweep_cus"]
    metrics = prom.read_text()
    assert f'amdgpu_validate_cu_sweep_cus_covered{{gpu="0"}} {g0["cu_sweep_cus"]}' in metrics
    assert 'amdgpu_validate_cu_sweep_bad_cus{gpu="0"} 0' in metrics


def test_bad_cu_injection_fails_the_job_and_names_the_cu(tmp_path):
    term = tmp_path / "term"
    rc, out, err = _run(*BASE, "--cu-sweep", "--fault-inject", "bad_cu", "--termination-log", str(term))
    assert rc == 1, out + err
    rep = _last_json(out)
    assert not rep["passed"]
    t = json.loads(term.read_text())
    assert t["passed"] is False
    msg = [f for f in t["failures"] if f.startswith("gpu0: CU sweep:")]
    assert len(msg) == 1 and len(msg[0]) < 200, t
    m = re.search(r"1 bad CU of \d+: xcd (\d+) se (\d+) sh (\d+) cu (\d+) \(simd (\d)\) mfma_bf16 round 0 "
                  r"elem \d+: expected (0x[0-9a-f]+), got (0x[0-9a-f]+); (\d+) of (\d+) workgroups", msg[0])
    assert m, msg[0]
    bad = rep["gpus"][0]["cu_sweep_bad_cus"]
    assert len(bad) == 1
    assert [bad[0][k] for k in ("xcd", "se", "sh", "cu")] == [int(x) for x in m.groups()[:4]]
    flipped = int(m.group(6), 16) ^ int(m.group(7), 16)
    assert flipped and flipped & (flipped - 1) == 0
    assert m.group(8) == m.group(9) and bad[0]["bad_workgroups"] == int(m.group(8))
    assert rep["gpus"][0]["cu_sweep_cus_covered"] == rep["gpus"][0]["cu_sweep_cus"]


def test_default_run_does_not_mention_the_cu_sweep(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run(*BASE, "--prom-out", str(prom), "--termination-log", str(term))
    assert rc == 0, out + err
    assert "cu_sweep" not in out.strip().splitlines()[-1]
    assert "cu_sweep" not in prom.read_text() and "cu_sweep" not in term.read_text()
