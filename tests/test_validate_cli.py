"""The Job binary's command line (validation/src/validate/options.hpp) without a GPU.

* The built binary replays tests/fixtures/validate_cli.json, which
  tools/validate_cli_table.py recorded from the binary before its sources were
  split: the --help text, --describe-sweep, and for every argument vector the exit
  status and the first line of stderr, byte for byte.
* options.hpp alone, in a stand-alone program with its own main built with
  AddressSanitizer and UBSan (host code only; nothing is loaded into Python): every
  flag lands in exactly its field of Opts.
"""
import importlib.util
import json
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
TABLE = json.loads((ROOT / "tests" / "fixtures" / "validate_cli.json").read_text())

_spec = importlib.util.spec_from_file_location("validate_cli_table", ROOT / "tools" / "validate_cli_table.py")
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)


def _have_bin():
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")


def test_the_table_covers_what_it_should():
    vec = [tuple(v[0]) for v in TABLE["vectors"]]
    assert vec == [tuple(a) for a, _ in tool.vectors()]            # the tool still builds this table
    assert ("--definitely-not-an-option",) in vec
    assert all((f,) in vec for f in tool.VALUED) and len(tool.VALUED) == 30
    by = {tuple(v[0]): v[2] for v in TABLE["vectors"]}
    for flag, bad, good in [("--cu-sweep-iters", "0", "1"), ("--cu-sweep-iters", "1025", "1024"),
                            ("--xcd-ratio", "1", "0.99"), ("--mx-size", "100", "128"),
                            ("--host-link-mib", "-1", "0"), ("--xgmi-sim", "9", "8"),
                            ("--xcd-sweep-mib", "4097", "4096"), ("--hbm-test-passes", "0", "1"),
                            ("--xgmi-nblk", "0", "1"), ("--xgmi-nblk", "1025", "1024")]:
        assert by[(flag, bad, "--describe-sweep")] == 2 and by[(flag, good, "--describe-sweep")] == 0, flag
    assert by[("--fault-inject", "slow_xcd")] == 2
    # a vector either fails (2) or ends in --describe-sweep (0): none reaches a GPU
    assert all(v[2] == 2 or (v[2] == 0 and "--describe-sweep" in v[0]) for v in TABLE["vectors"])
    line = max(TABLE["help"].splitlines(), key=len)
    assert len(line) > 140 and "sk_xcc - corrupts the LAST GPU's data" in line   # the over-long line stays


def test_help_and_describe_sweep_are_byte_identical():
    _have_bin()
    rc, out, err = tool.run(BIN, ["--help"])
    assert rc == 0 and out == "" and err == TABLE["help"]
    for mib, want in TABLE["describe"].items():
        rc, out, err = tool.run(BIN, ["--describe-sweep", "--allreduce-max-mib", mib])
        assert (rc, out, err) == (0, want, "")


def test_every_vector_ends_as_recorded():
    _have_bin()
    wrong = []
    for argv, env, rc, first in TABLE["vectors"]:
        got_rc, out, err = tool.run(BIN, argv, env)
        got = [got_rc, err.splitlines()[0] if err else ""]
        if got != [rc, first] or (rc == 0 and out != TABLE["describe"]["8192"] and "--allreduce-max-mib" not in argv):
            wrong.append((argv, env, got, [rc, first]))
        if rc == 2 and first.startswith("usage:"):
            assert err == TABLE["help"], argv          # a range failure prints the usage text alone
    assert not wrong, wrong


# ------------------------------------------------ options.hpp on its own
# flag -> (field of Opts, value passed, value expected), written from the parse() of
# the binary before the split; a switch passes no value
FLAGS = {
    "--gpus": ("gpus", "3", 3), "--size": ("size", "2304", 2304), "--iters": ("iters", "17", 17),
    "--tflops-floor": ("tflops_floor", "123.5", 123.5), "--min-hbm-gb": ("min_hbm_gb", "250.25", 250.25),
    "--hbm-floor-gbps": ("hbm_floor_gbps", "3100.5", 3100.5), "--hbm-test-gb": ("hbm_test_gb", "-1", -1.0),
    "--hbm-test-passes": ("hbm_test_passes", "4", 4), "--cu-sweep": ("cu_sweep", None, True),
    "--cu-sweep-iters": ("cu_sweep_iters", "33", 33), "--host-link-mib": ("host_link_mib", "48", 48),
    "--host-link-floor-gbps": ("host_link_floor_gbps", "41.5", 41.5), "--mx-check": ("mx_check", None, True),
    "--mx-size": ("mx_size", "384", 384), "--mx-tflops-floor": ("mx_tflops_floor", "2000.5", 2000.5),
    "--xcd-sweep": ("xcd_sweep", None, True), "--xcd-sweep-mib": ("xcd_sweep_mib", "77", 77),
    "--xcd-ratio": ("xcd_ratio", "0.85", 0.85), "--allreduce-max-mib": ("allreduce_max_mib", "96", 96),
    "--rccl": ("rccl", None, 1), "--no-rccl": ("rccl", None, 0), "--no-xgmi": ("xgmi", None, False),
    "--xgmi-sim": ("xgmi_sim", "6", 6), "--settle-s": ("settle_s", "0.75", 0.75),
    "--no-fp8": ("fp8", None, False), "--fp8-tflops-floor": ("fp8_tflops_floor", "3000.5", 3000.5),
    "--no-p2p": ("p2p", None, False), "--p2p-loopback": ("p2p_loopback", None, True),
    "--p2p-mib": ("p2p_mib", "72", 72), "--p2p-floor-gbps": ("p2p_floor_gbps", "45.5", 45.5),
    "--rccl-busbw-floor-gbps": ("rccl_busbw_floor_gbps", "301.5", 301.5),
    "--xgmi-busbw-floor-gbps": ("xgmi_busbw_floor_gbps", "302.5", 302.5),
    "--xgmi-nblk": ("xgmi_nblk", "48", 48), "--xgmi-one-shot-max": ("xgmi_one_shot_max", "131072", 131072),
    "--xgmi-tune": ("xgmi_tune", None, True), "--require-host-prep": ("require_host_prep", None, True),
    "--require-iommu-pt": ("require_iommu_pt", None, True), "--describe-sweep": ("describe_sweep", None, True),
    "--json": ("json", None, True), "--out": ("out", "o.json", "o.json"),
    "--termination-log": ("termination_log", "/dev/t\"log", "/dev/t\"log"),
    "--prom-out": ("prom_out", "m.prom", "m.prom"), "--fault-inject": ("fault", "corrupt_mx", "corrupt_mx"),
    "--pushgateway": ("pushgateway", "http://gw:9091/x", "http://gw:9091/x"),
}
DEFAULTS = {
    "gpus": 0, "size": 8192, "iters": 50, "tflops_floor": 0, "min_hbm_gb": 0, "hbm_floor_gbps": 0,
    "hbm_test_gb": 0, "hbm_test_passes": 1, "cu_sweep": False, "cu_sweep_iters": 16, "host_link_mib": 0,
    "host_link_floor_gbps": 0, "mx_check": False, "mx_size": 4096, "mx_tflops_floor": 0, "xcd_sweep": False,
    "xcd_sweep_mib": 256, "xcd_ratio": 0, "allreduce_max_mib": 8192, "xgmi": True, "xgmi_sim": 0, "rccl": -1,
    "settle_s": 0.1, "fp8": True, "fp8_tflops_floor": 0, "p2p": True, "p2p_loopback": False, "p2p_mib": 256,
    "p2p_floor_gbps": 0, "rccl_busbw_floor_gbps": 0, "xgmi_busbw_floor_gbps": 0, "xgmi_nblk": 64,
    "xgmi_one_shot_max": 262144, "xgmi_tune": False, "require_host_prep": False, "require_iommu_pt": False,
    "describe_sweep": False, "json": True, "out": "", "termination_log": "", "prom_out": "", "fault": "",
    "pushgateway": "",
}

OPTIONS_MAIN = r"""
#include "options.hpp"
#include "json.hpp"
using namespace ntm::job;
int main(int argc, char** argv) {
  Opts o;
  const bool ok = parse(argc, argv, o);
  auto b = [](bool v) { return std::string(v ? "true" : "false"); };
  std::string s = "{\"parse\":" + b(ok) + ",\"range_ok\":" + b(range_ok(o)) + ",\"flags\":" +
                  std::to_string(sizeof kFlags / sizeof kFlags[0]);
  auto put = [&](const char* k, const std::string& v) { s += std::string(",\"") + k + "\":" + v; };
#define NUM(f) put(#f, jnum((double)o.f))
#define BOOL(f) put(#f, b(o.f))
#define STR(f) put(#f, jstr(o.f))
  NUM(gpus); NUM(size); NUM(iters); NUM(tflops_floor); NUM(min_hbm_gb); NUM(hbm_floor_gbps);
  NUM(hbm_test_gb); NUM(hbm_test_passes); BOOL(cu_sweep); NUM(cu_sweep_iters); NUM(host_link_mib);
  NUM(host_link_floor_gbps); BOOL(mx_check); NUM(mx_size); NUM(mx_tflops_floor); BOOL(xcd_sweep);
  NUM(xcd_sweep_mib); NUM(xcd_ratio); NUM(allreduce_max_mib); BOOL(xgmi); NUM(xgmi_sim); NUM(rccl);
  NUM(settle_s); BOOL(fp8); NUM(fp8_tflops_floor); BOOL(p2p); BOOL(p2p_loopback); NUM(p2p_mib);
  NUM(p2p_floor_gbps); NUM(rccl_busbw_floor_gbps); NUM(xgmi_busbw_floor_gbps); NUM(xgmi_nblk);
  NUM(xgmi_one_shot_max); BOOL(xgmi_tune); BOOL(require_host_prep); BOOL(require_iommu_pt);
  BOOL(describe_sweep); BOOL(json); STR(out); STR(termination_log); STR(prom_out); STR(fault);
  STR(pushgateway);
  std::puts((s + "}").c_str());
  return ok ? 0 : 2;
}
"""


def build_sanitized(tmp_path, name: str, source: str) -> Path:
    """A stand-alone host program against validation/src/validate/*.hpp under ASan + UBSan."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    src, exe = tmp_path / f"{name}.cpp", tmp_path / name
    src.write_text(source)
    static = (["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) else ["-static-libsan"])
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", *static, f"-I{ROOT / 'validation' / 'include'}",
           f"-I{ROOT / 'validation' / 'src' / 'validate'}", str(src), "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    return exe


@pytest.fixture(scope="module")
def options_exe(tmp_path_factory):
    return build_sanitized(tmp_path_factory.mktemp("opts"), "options_main", OPTIONS_MAIN)


def _opts(exe, *argv):
    p = subprocess.run([str(exe), *argv], capture_output=True, text=True, timeout=60)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr
    return p.returncode, json.loads(p.stdout), p.stderr


def test_defaults(options_exe):
    rc, o, err = _opts(options_exe)
    assert rc == 0 and err == "" and o.pop("parse") and o.pop("range_ok")
    assert o.pop("flags") == len(FLAGS) == 44
    assert o == DEFAULTS and {f for f, _, _ in FLAGS.values()} == set(DEFAULTS)


@pytest.mark.parametrize("flag", sorted(FLAGS))
def test_each_flag_changes_exactly_its_field(options_exe, flag):
    field, value, want = FLAGS[flag]
    rc, o, err = _opts(options_exe, flag, *([value] if value is not None else []))
    assert rc == 0 and err == "" and o["parse"]
    changed = {k: v for k, v in o.items() if k in DEFAULTS and v != DEFAULTS[k]}
    assert changed == ({field: want} if want != DEFAULTS[field] else {})
    assert o[field] == want and isinstance(o[field], bool) == isinstance(want, bool)
    if value is not None:                      # and without its value it says so
        rc, o, err = _opts(options_exe, flag)
        assert rc == 2 and err == f"missing value for {flag}\n" and not o["parse"]
        assert {k: v for k, v in o.items() if k in DEFAULTS} == DEFAULTS


def test_all_flags_at_once_and_the_error_paths(options_exe):
    argv = []
    for flag, (_, value, _) in FLAGS.items():
        if flag != "--rccl":                   # --no-rccl comes later and wins either way
            argv += [flag] + ([value] if value is not None else [])
    rc, o, err = _opts(options_exe, *argv)
    assert rc == 0 and err == ""
    assert {k: o[k] for k in DEFAULTS} == {**DEFAULTS, **{f: w for fl, (f, _, w) in FLAGS.items() if fl != "--rccl"}}
    rc, o, err = _opts(options_exe, "--size", "512", "--nope", "--iters", "3")
    assert rc == 2 and err == "unknown argument --nope\n" and o["size"] == 512 and o["iters"] == 50
    rc, o, err = _opts(options_exe, "--xcd-ratio", "1")
    assert rc == 2 and err == "" and not o["parse"] and not o["range_ok"] and o["xcd_ratio"] == 1
    rc, _, err = _opts(options_exe, "--gpus", "x", "--size")          # malformed arguments
    assert rc == 2 and err == "missing value for --size\n"
