"""``NTM_ATOMICS_CHECK=1 amdgpu-validate``: stage K9, the atomics and cross-XCD hand-off
check, in the Job binary - a clean run with its keys and gauges, the two injections, and a
default run in which the check is invisible."""
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
OPS = ("add_u32", "add_u64", "and_u32", "or_u32", "xor_u32", "min_i32", "max_i32", "max_u64",
       "cas_u32", "add_f32", "add_f64", "add_bf16x2", "add_f16x2")
KEYS = ("atomics_ops", "atomics_ticket_bad", "atomics_handoff_bad_words", "atomics_handoff_stale_words",
        "atomics_handoff_episodes_per_s", "atomics_xcd_pairs_covered", "atomics_seconds")


def _run(*args, on=True, timeout=300):
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = {k: v for k, v in os.environ.items() if k not in ("NTM_FAULT_INJECT", "NODE_NAME", "NTM_ATOMICS_CHECK")}
    if on:
        e["NTM_ATOMICS_CHECK"] = "1"
    p = subprocess.run([str(BIN), *BASE, *args], capture_output=True, text=True, timeout=timeout, env=e)
    return p.returncode, p.stdout, p.stderr


def _last_json(out):
    return json.loads(out.strip().splitlines()[-1])


def test_clean_run_passes_and_reports(tmp_path):
    prom = tmp_path / "m.prom"
    rc, out, err = _run("--prom-out", str(prom))
    g0 = _last_json(out)["gpus"][0]
    print({k: g0.get(k) for k in KEYS})
    print({op: g0.get(f"atomics_{op}_gops") for op in OPS})
    assert rc == 0, out + err
    assert g0["atomics_ops"] == list(OPS)
    for op in OPS:
        assert g0[f"atomics_{op}_bad"] == 0 and g0[f"atomics_{op}_gops"] > 0
    assert g0["atomics_ticket_bad"] == 0 and g0["atomics_handoff_bad_words"] == 0
    assert g0["atomics_handoff_stale_words"] == 0 and g0["atomics_handoff_episodes_per_s"] > 0
    assert 1 <= g0["atomics_xcd_pairs_covered"] <= 64 and g0["atomics_seconds"] > 0
    metrics = prom.read_text()
    assert 'amdgpu_validate_atomics_gops{gpu="0",op="add_bf16x2"} ' in metrics
    assert 'amdgpu_validate_atomics_handoff_bad_words{gpu="0"} 0' in metrics


def test_corrupt_atomic_names_op_and_slot():
    rc, out, err = _run("--fault-inject", "corrupt_atomic")
    assert rc == 1, out + err
    rep = _last_json(out)
    msgs = [f for f in rep["failures"] if f.startswith("gpu0: atomics:")]
    assert len(msgs) == 1, rep["failures"]
    m = re.match(r"gpu0: atomics: add_f32 slot (\d+): expected (0x[0-9a-f]+), got (0x[0-9a-f]+), bad bits 0x200$", msgs[0])
    assert m and int(m.group(2), 16) ^ int(m.group(3), 16) == 0x200, msgs[0]
    g0 = rep["gpus"][0]
    assert g0["atomics_add_f32_bad"] == 1 and sum(g0[f"atomics_{op}_bad"] for op in OPS) == 1


def test_stale_handoff_is_classed_stale():
    rc, out, err = _run("--fault-inject", "stale_handoff")
    assert rc == 1, out + err
    rep = _last_json(out)
    msgs = [f for f in rep["failures"] if f.startswith("gpu0: atomics:")]
    assert len(msgs) == 1 and len(msgs[0]) < 200, rep["failures"]
    assert re.match(r"gpu0: atomics: handoff: stale word: reader xcd \d+ se \d+ cu \d+, writer xcd \d+ cu \d+ "
                    r"\(workgroup \d+\), episode \d+, offset 0x1100, expected 0x[0-9a-f]+, got 0x[0-9a-f]+; "
                    r"4 bad, 4 stale$", msgs[0]), msgs[0]
    g0 = rep["gpus"][0]
    assert g0["atomics_handoff_bad_words"] == 4 and g0["atomics_handoff_stale_words"] == 4


def test_without_the_variable_nothing_mentions_the_check(tmp_path):
    prom, term = tmp_path / "m.prom", tmp_path / "term"
    rc, out, err = _run("--prom-out", str(prom), "--termination-log", str(term), on=False)
    assert rc == 0, out + err
    assert "atomics" not in out.strip().splitlines()[-1]
    assert "atomics" not in prom.read_text() and "atomics" not in term.read_text()
