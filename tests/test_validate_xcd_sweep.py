"""``amdgpu-validate --xcd-sweep``: stage K8, the per-XCD sweep, in the Job binary - a clean
run gated at 0.5, the slow-XCD injection with and without a ratio, the corruption injection
and a default run in which the sweep is invisible."""
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
SWEEP = ("--xcd-sweep", "--xcd-sweep-mib", "32")
CELLS = ("l2_alone", "l2_together", "mall_alone", "mall_together", "hbm_alone", "hbm_together",
         "mfma_together")


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


def test_clean_run_passes_at_ratio_half_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run(*BASE, *SWEEP, "--xcd-ratio", "0.5", "--prom-out", str(prom))
    g0 = _last_json(out)["gpus"][0]
    n = g0["xcd_sweep_xcds"]
    for c in CELLS:
        print(c, "min/median", g0[f"xcd_sweep_{c}_min_over_median"], "passes", g0[f"xcd_sweep_{c}_passes"],
              "span_us", g0[f"xcd_sweep_{c}_span_us"], "rates", g0[f"xcd_sweep_{c}_rate"])
    assert rc == 0, out + err
    for c in CELLS:
        assert len(g0[f"xcd_sweep_{c}_rate"]) == n and len(g0[f"xcd_sweep_{c}_clock_ghz"]) == n
        assert all(r > 0 for r in g0[f"xcd_sweep_{c}_rate"])
        assert all(0.5 < r < 3.0 for r in g0[f"xcd_sweep_{c}_clock_ghz"])
        assert g0[f"xcd_sweep_{c}_span_us"][0] >= 100
    assert g0["xcd_sweep_slow"] == [] and g0["xcd_sweep_bad"] == [] and g0["xcd_sweep_s"] > 0
    metrics = prom.read_text()
    for level, mode in (c.split("_") for c in CELLS):
        for name in ("amdgpu_validate_xcd_rate", "amdgpu_validate_xcd_clock_ghz"):
            assert f'{name}{{gpu="0",xcd="{n - 1}",level="{level}",mode="{mode}"}} ' in metrics


def test_slow_xcd_injection_fails_the_job_and_names_the_xcd(tmp_path):
    term = tmp_path / "term"
    rc, out, err = _run(*BASE, *SWEEP, "--xcd-ratio", "0.5", "--fault-inject", "slow_xcd",
                        "--termination-log", str(term))
    assert rc == 1, out + err
    t = json.loads(term.read_text())
    assert t["passed"] is False and t["xcd_sweep_min_over_median"] < 0.5
    msgs = [f for f in t["failures"] if f.startswith("gpu0: XCD sweep:")]
    print(msgs)
    assert msgs and all(len(m) < 200 for m in msgs)
    assert all(re.match(r"gpu0: XCD sweep: xcd 5 slow at (l2|mall|hbm|mfma)/(alone|together): [\d.]+ G(B|MFMA)/s "
                        r"vs median [\d.]+ \(0\.\d\d < 0\.50\); clock [\d.]+ GHz vs median [\d.]+$", m)
               for m in msgs), msgs
    # the two contended cells are reported, not judged (profiles/xcd_sweep/README.md)
    assert len(msgs) == 5 and not [m for m in msgs if "mall/together" in m or "hbm/together" in m]
    g0 = _last_json(out)["gpus"][0]
    assert {s["xcd"] for s in g0["xcd_sweep_slow"]} == {5} and g0["xcd_sweep_bad"] == []
    assert [c for c in CELLS if not g0[f"xcd_sweep_{c}_gated"]] == ["mall_together", "hbm_together"]
    assert g0["xcd_sweep_hbm_together_min_over_median"] < 0.5      # still visible there


def test_slow_xcd_injection_is_reported_only_at_ratio_zero():
    rc, out, err = _run(*BASE, *SWEEP, "--fault-inject", "slow_xcd")
    assert rc == 0, out + err
    g0 = _last_json(out)["gpus"][0]
    assert g0["xcd_sweep_slow"] == [] and g0["xcd_sweep_failures"] == []
    r = g0["xcd_sweep_hbm_together_rate"]
    print(r, g0["xcd_sweep_hbm_together_min_over_median"])
    assert r[5] == min(r) and g0["xcd_sweep_hbm_together_min_over_median"] < 0.5


def test_corrupt_xcd_injection_names_xcd_3():
    rc, out, err = _run(*BASE, *SWEEP, "--fault-inject", "corrupt_xcd")
    assert rc == 1, out + err
    rep = _last_json(out)
    msgs = [f for f in rep["failures"] if f.startswith("gpu0: XCD sweep:")]
    assert len(msgs) == 2 and all(len(m) < 200 for m in msgs), msgs     # hbm/alone and hbm/together
    m = re.match(r"gpu0: XCD sweep: xcd 3 read wrong data at hbm/alone: slice offset (0x[0-9a-f]+), expected "
                 r"(0x[0-9a-f]+), got (0x[0-9a-f]+), bad bits (0x[0-9a-f]+); \d+ words?$", msgs[0])
    assert m, msgs[0]
    flipped = int(m.group(2), 16) ^ int(m.group(3), 16)
    assert flipped == int(m.group(4), 16) and flipped & (flipped - 1) == 0 and flipped
    assert {b["xcd"] for b in rep["gpus"][0]["xcd_sweep_bad"]} == {3}


def test_injections_need_the_sweep():
    for kind in ("slow_xcd", "corrupt_xcd"):
        rc, out, err = _run(*BASE, "--fault-inject", kind)
        assert rc == 2 and f"fault-inject {kind} needs --xcd-sweep" in err


def test_default_run_does_not_mention_the_xcd_sweep(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run(*BASE, "--prom-out", str(prom), "--termination-log", str(term))
    assert rc == 0, out + err
    assert "xcd_sweep" not in out.strip().splitlines()[-1]
    assert "xcd_rate" not in prom.read_text() and "xcd_clock" not in prom.read_text() and "xcd_sweep" not in term.read_text()
