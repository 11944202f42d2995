"""``amdgpu-validate --hbm-test-gb``: stage K4, the HBM pattern test, in the Job
binary - off by default and then invisible in every output, a clean run, and
the native fault injection that must fail the Job naming GPU, offset and bit."""
import json
import os
import re
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
BASE = ("--gpus", "1", "--size", "1024", "--iters", "5", "--no-fp8")


def _have_bin():
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")


def _run(*args, timeout=300):
    e = dict(os.environ)
    e.pop("NTM_FAULT_INJECT", None)
    e.pop("NODE_NAME", None)
    p = subprocess.run([str(BIN), *args], capture_output=True, text=True, timeout=timeout, env=e)
    return p.returncode, p.stdout, p.stderr


def _last_json(out):
    return json.loads(out.strip().splitlines()[-1])


def test_hbm_test_gb_needs_a_value():
    _have_bin()
    rc, _, err = _run("--hbm-test-gb", timeout=60)
    assert rc == 2 and "missing value for --hbm-test-gb" in err and "usage" in err
    rc, _, err = _run("--hbm-test-gb", "4", "--hbm-test-passes", "0", timeout=60)
    assert rc == 2
    rc, _, err = _run("--help", timeout=60)
    assert rc == 0 and "--hbm-test-gb" in err and "corrupt_hbm" in err


@pytest.mark.gpu
def test_hbm_test_passes_on_4_gb(tmp_path):
    _have_bin()
    prom = tmp_path / "m.prom"
    rc, out, err = _run(*BASE, "--hbm-test-gb", "4", "--prom-out", str(prom))
    assert rc == 0, out + err
    g0 = _last_json(out)["gpus"][0]
    assert 3.9 < g0["hbm_test_gb"] < 4.1 and 3.9 < g0["hbm_test_requested_gb"] < 4.1, g0
    assert g0["hbm_test_bad_words"] == 0 and g0["hbm_test_bad_bits"] == 0
    assert g0["hbm_test_write_GBps"] > 0 and g0["hbm_test_verify_GBps"] > 0 and g0["hbm_test_s"] > 0
    assert [s["step"] for s in g0["hbm_test_steps"]] == [
        "addr write", "addr verify+invert", "addr inverted verify", "hash write", "hash verify"]
    metrics = prom.read_text()
    assert re.search(r'^amdgpu_validate_hbm_test_gb\{gpu="0"\} (3\.9|4)', metrics, re.M)
    assert 'amdgpu_validate_hbm_test_bad_words{gpu="0"} 0' in metrics


@pytest.mark.gpu
def test_hbm_fault_injection_fails_the_job(tmp_path):
    _have_bin()
    term = tmp_path / "term"
    rc, out, err = _run(*BASE, "--hbm-test-gb", "4", "--fault-inject", "corrupt_hbm",
                        "--termination-log", str(term))
    assert rc == 1, out + err
    rep = _last_json(out)
    assert not rep["passed"] and rep["gpus"][0]["hbm_test_bad_words"] == 1
    t = json.loads(term.read_text())
    assert t["passed"] is False
    msg = [f for f in t["failures"] if "HBM pattern" in f]
    assert len(msg) == 1 and msg[0].startswith("gpu0: "), t
    mask = int(re.search(r"bad bits (0x[0-9a-f]{16})", msg[0]).group(1), 16)
    assert mask and mask & (mask - 1) == 0, msg          # exactly one bit
    assert mask == rep["gpus"][0]["hbm_test_bad_bits"]
    m = re.search(r"byte offset (0x[0-9a-f]{16}).*expected (0x[0-9a-f]{16}), got (0x[0-9a-f]{16})", msg[0])
    off, exp, got = (int(x, 16) for x in m.groups())
    assert exp ^ got == mask and exp == off // 8         # the ADDR word names its own address
    assert 0 <= off < 4.1e9


@pytest.mark.gpu
def test_default_run_does_not_mention_the_hbm_test(tmp_path):
    _have_bin()
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run(*BASE, "--prom-out", str(prom), "--termination-log", str(term))
    assert rc == 0, out + err
    rep = _last_json(out)
    assert not [k for g in rep["gpus"] for k in g if k.startswith("hbm_test")]
    assert not [k for k in rep if k.startswith("hbm_test")]
    assert "hbm_test" not in prom.read_text() and "hbm_test" not in term.read_text()
