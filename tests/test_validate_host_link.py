"""``amdgpu-validate --host-link-mib``: stage K6, the host-link (PCIe) check, in the Job
binary - a clean run, the fault injection that must fail the Job with one line naming
the direction and the word, a default run in which the stage is invisible, and the
flag's argument check."""
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
KEYS = ("host_link_mib", "host_link_h2d_GBps", "host_link_d2h_GBps", "host_link_h2d_copy_GBps",
        "host_link_d2h_copy_GBps", "host_link_duplex_GBps", "host_link_read_latency_us",
        "host_link_bad_words", "host_link_bad_bits", "host_link_pcie", "host_link_s")


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


def test_host_link_passes_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run(*BASE, "--host-link-mib", "64", "--prom-out", str(prom))
    assert rc == 0, out + err
    g0 = _last_json(out)["gpus"][0]
    for k in KEYS:
        assert k in g0, k
    print({k: v for k, v in g0.items() if k.startswith("host_link")})
    assert g0["host_link_mib"] == 64 and g0["host_link_bad_words"] == 0 and g0["host_link_bad_bits"] == 0
    for k in KEYS[1:7]:
        assert g0[k] > 0, k
    assert g0["host_link_s"] > 0
    pcie = g0["host_link_pcie"]                        # null where sysfs does not show the device
    assert pcie is None or set(pcie) == {"speed_gts", "width", "max_speed_gts", "max_width", "numa_node"}
    metrics = prom.read_text()
    assert re.search(r'^amdgpu_validate_host_link_h2d_gbps\{gpu="0"\} [0-9.e+]+$', metrics, re.M)
    assert re.search(r'^amdgpu_validate_host_link_d2h_gbps\{gpu="0"\} [0-9.e+]+$', metrics, re.M)
    assert 'amdgpu_validate_host_link_bad_words{gpu="0"} 0' in metrics


def test_corrupt_host_link_fails_the_job_with_one_line(tmp_path):
    term = tmp_path / "term"
    rc, out, err = _run(*BASE, "--host-link-mib", "64", "--fault-inject", "corrupt_host_link",
                        "--termination-log", str(term))
    assert rc == 1, out + err
    rep = _last_json(out)
    assert not rep["passed"]
    g0 = rep["gpus"][0]
    assert g0["host_link_bad_words"] == 1 and g0["host_link_bad_bits"] == 1 << 45
    t = json.loads(term.read_text())
    assert t["passed"] is False
    msg = [f for f in t["failures"] if f.startswith("gpu0: host link")]
    assert len(msg) == 1 and len(msg[0]) < 200 and "\n" not in msg[0], t
    # the host flipped the bit, so the pinned buffer itself is wrong: the push side is named
    m = re.fullmatch(r"gpu0: host link device->host write or host memory: 1 bad word\(s\), at byte "
                     r"(0x[0-9a-f]+): expected (0x[0-9a-f]{16}), got (0x[0-9a-f]{16}), bad bits 0x200000000000",
                     msg[0])
    assert m, msg[0]
    assert int(m.group(1), 16) == 32 << 20                      # the middle of 64 MiB
    assert int(m.group(2), 16) ^ int(m.group(3), 16) == 1 << 45
    assert msg[0] in rep["failures"]


def test_default_run_does_not_mention_the_host_link(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run(*BASE, "--prom-out", str(prom), "--termination-log", str(term))
    assert rc == 0, out + err
    assert "host_link" not in out.strip().splitlines()[-1]
    assert "host_link" not in prom.read_text() and "host_link" not in term.read_text()


def test_host_link_mib_without_a_value_is_a_usage_error():
    rc, out, err = _run(*BASE, "--host-link-mib")
    assert rc == 2, out + err
    assert "usage: amdgpu-validate" in err and "--host-link-mib MiB" in err
    assert "--host-link-floor-gbps" in err and "corrupt_host_link" in err
