"""``amdgpu-validate --mx-check``: stage K7, the MX block-scaled matrix check, in the Job
binary - a clean run, the fault injection that must fail the Job with one line naming the
format and the element, a default run in which the stage is invisible, and the argument
check of ``--mx-size``."""
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
MX = ("--mx-check", "--mx-size", "512")
KEYS = ("mx_formats", "mx_bad_elements", "mx_fp4_tflops", "mx_scale_spread", "mx_s")


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


def test_mx_check_passes_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run(*BASE, *MX, "--prom-out", str(prom))
    assert rc == 0, out + err
    g0 = _last_json(out)["gpus"][0]
    for k in KEYS:
        assert k in g0, k
    print({k: v for k, v in g0.items() if k.startswith("mx_")})
    assert g0["mx_formats"] == ["e4m3", "e5m2", "e2m3", "e3m2", "e2m1"]
    assert g0["mx_bad_elements"] == 0 and g0["mx_scale_spread"] == 3
    assert g0["mx_fp4_tflops"] > 0 and g0["mx_s"] > 0
    metrics = prom.read_text()
    assert 'amdgpu_validate_mx_bad_elements{gpu="0"} 0' in metrics
    assert 'amdgpu_validate_mx_formats{gpu="0"} 5' in metrics
    assert 'amdgpu_validate_mx_scale_spread{gpu="0"} 3' in metrics
    assert re.search(r'^amdgpu_validate_mx_fp4_tflops\{gpu="0"\} [0-9.e+]+$', metrics, re.M)
    assert re.search(r'^amdgpu_validate_mx_s\{gpu="0"\} [0-9.e+-]+$', metrics, re.M)


def test_corrupt_mx_fails_the_job_with_one_line(tmp_path):
    term = tmp_path / "term"
    rc, out, err = _run(*BASE, *MX, "--fault-inject", "corrupt_mx", "--termination-log", str(term))
    assert rc == 1, out + err
    rep = _last_json(out)
    assert not rep["passed"]
    g0 = rep["gpus"][0]
    assert g0["mx_bad_elements"] == 1 and "e2m1" not in g0["mx_formats"] and len(g0["mx_formats"]) == 4
    t = json.loads(term.read_text())
    assert t["passed"] is False
    msg = [f for f in t["failures"] if f.startswith("gpu0: mx ")]
    assert len(msg) == 1 and len(msg[0]) < 200 and "\n" not in msg[0], t
    m = re.fullmatch(r"gpu0: mx e2m1 dense: 1 bad element\(s\), first at row (\d+) col (\d+): "
                     r"expected (0x[0-9a-f]{8}), got (0x[0-9a-f]{8})", msg[0])
    assert m, msg[0]
    assert (int(m.group(1)), int(m.group(2))) == (256, 5)       # element 512 * 512 / 2 + 5
    assert int(m.group(3), 16) ^ int(m.group(4), 16) == 1 << 3
    assert msg[0] in rep["failures"]


def test_default_run_does_not_mention_the_mx_check(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run(*BASE, "--prom-out", str(prom), "--termination-log", str(term))
    assert rc == 0, out + err
    assert "mx_" not in out.strip().splitlines()[-1]
    assert "mx_" not in prom.read_text() and "mx_" not in term.read_text()


def test_mx_size_without_a_value_is_a_usage_error():
    rc, out, err = _run(*BASE, "--mx-check", "--mx-size")
    assert rc == 2, out + err
    assert "usage: amdgpu-validate" in err and "--mx-size S" in err
    assert "--mx-tflops-floor" in err and "corrupt_mx" in err
    rc, out, err = _run(*BASE, "--mx-check", "--mx-size", "500")    # no multiple of 128
    assert rc == 2, out + err
