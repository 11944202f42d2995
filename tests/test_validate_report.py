"""The Job binary's report (validation/src/validate/report.hpp).

* Without a GPU: report.hpp in a stand-alone program with its own main built with
  AddressSanitizer and UBSan (host code only; nothing is loaded into Python), on two
  synthetic GPUs with every check marked ran, a hostile device name, a NaN rate and
  100 failures of 300 characters.
* On an MI355X: one run of the built binary with every check on at its smallest
  size, held to tests/fixtures/validate_report_shape.json, which
  tools/validate_cli_table.py recorded from the binary before its sources were split.
"""
import json
import re
import subprocess

import pytest

from test_validate_cli import BIN, ROOT, build_sanitized, tool

SHAPE = json.loads((ROOT / "tests" / "fixtures" / "validate_report_shape.json").read_text())

REPORT_MAIN = r"""
#include <cstdio>
#include "report.hpp"
using namespace ntm::job;

static GpuResult gpu(int dev) {
  GpuResult r;
  r.device = dev;
  r.name = "AMD \"Instinct\"\tMI355X\\";   // a quote, a control character, a backslash
  r.arch = "gfx950:sramecc+:xnack-";
  r.total_gb = 309.2;
  r.k1.ms = 0.7; r.k1.tflops = dev ? 1590.5 : NAN;   // one rate is NaN
  r.k1.bad = 0; r.k1.max_err = 0.001f;
  r.k1.abft_bad_acc = 0; r.k1.abft_bad_store = 0; r.k1.abft_max_rel_acc = 1e-6f; r.k1.abft_tflops = 1500;
  r.fp8.tflops = 2900; r.fp8.bad = 0; r.fp8.max_err = 0.01f; r.fp8.abft_bad = 0;
  r.sk.variant = 54; r.sk.bad = 0; r.sk.ms = 0.4;
  r.k2.copy_gbps = 4300; r.k2.read_gbps = 4800; r.k2.copy_ok = true;
  r.hbm_test.ran = true; r.hbm_test.gb = 1; r.hbm_test.requested_gb = 1; r.hbm_test.bad_words = 3;
  r.hbm_test.steps = "[{\"step\":\"addr write\",\"s\":0.01}]";
  r.hbm_test.failures = {"gpu" + std::to_string(dev) + ": HBM pattern test: " + std::string(300, 'h')};
  r.cu_sweep.ran = true; r.cu_sweep.sum.cus = 256; r.cu_sweep.sum.cus_covered = 255; r.cu_sweep.lds_bytes = 163840;
  r.host_link.ran = true; r.host_link.mib = 16; r.host_link.h2d_gbps = 50; r.host_link.h2d_copy_gbps = 55;
  r.host_link.d2h_gbps = 52; r.host_link.d2h_copy_gbps = 48; r.host_link.bad_words = 1;
  r.mx.ran = true; r.mx.formats = {"e4m3", "e2m1"}; r.mx.bad_elements = 7; r.mx.fp4_tflops = 4000; r.mx.scale_spread = 2;
  r.xcd.ran = true; r.xcd.xcds = 2; r.xcd.mib = 16; r.xcd.ratio = 0.5;
  XcdCell c;
  c.gated = true; c.passes = 4; c.min_span_ticks = 12000; c.max_span_ticks = 15000;
  c.sum.level = ntm::xcs::kLevelHbm; c.sum.mode = ntm::xcs::kModeAlone; c.sum.min_over_median = 0.4 + dev * 0.1;
  c.sum.median_rate = 500; c.sum.rule_ran = true; c.sum.slow = {1};
  c.sum.rows.resize(2);
  c.sum.rows[1].xcd = 1; c.sum.rows[0].rate = 500; c.sum.rows[1].rate = 250; c.sum.rows[0].clock_ghz = 2.4;
  r.xcd.cells.push_back(c);
  r.xcd.failures = {"gpu" + std::to_string(dev) + ": XCD sweep: xcd 1 slow \"quoted\""};
  return r;
}

int main() {
  Report R;
  Opts& o = R.o;
  o.hbm_test_gb = 1; o.cu_sweep = true; o.host_link_mib = 16; o.mx_check = true; o.xcd_sweep = true;
  o.termination_log = "t"; o.pushgateway = "http://gw"; o.tflops_floor = 1600;
  R.node = "node \"7\"";
  R.devs = {0, 1};
  R.gpus = {gpu(0), gpu(1)};
  R.rccl_rows = {{"bf16", 8, 10.0, NAN, 0.0, 0}, {"fp32", 32, 11.0, 2.5, 4.4, 0}};
  R.xgmi_rows = {{"bf16-1shot", 512, 9.0, 3.0, 5.25, 0}};
  R.p2p.n = 2; R.p2p.gbps = {NAN, 60.5, 61.5, NAN}; R.p2p.min_gbps = 60.5;
  R.t_start = 1.7e9; R.t_hip = R.t_start + 0.1; R.t_rccl = R.t_start + 0.5; R.t_end = R.t_start + 0.75;
  R.push_status = "error: \"no\"";
  for (auto& g : R.gpus)
    for (auto& f : gpu_failures(g, o)) R.failures.push_back(f);
  while (R.failures.size() < 100) R.failures.push_back("failure " + std::to_string(R.failures.size()) + " " + std::string(300, 'x'));
  std::puts(report_json(R).c_str());
  std::puts(termination_message(R).c_str());
  std::fputs(prometheus_text(R).c_str(), stdout);
  return 0;
}
"""


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    exe = build_sanitized(tmp_path_factory.mktemp("report"), "report_main", REPORT_MAIN)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stderr == "", p.stderr
    js, term, prom = p.stdout.split("\n", 2)
    return js, term, prom


def test_report_is_valid_json_with_hostile_strings(outputs):
    rep = json.loads(outputs[0])
    assert rep["passed"] is False and rep["node"] == 'node "7"' and rep["n_gpus"] == 2
    g0, g1 = rep["gpus"]
    assert g0["name"] == 'AMD "Instinct"MI355X\\'             # escaped; the control character is dropped
    assert g0["gemm_tflops"] is None and g1["gemm_tflops"] == 1590.5      # the NaN came out as null
    assert rep["gemm_tflops_aggregate"] is None
    assert rep["rccl_allreduce"][0]["algbw_GBps"] is None and rep["xgmi_p2p_GBps"] == [[None, 60.5], [61.5, None]]
    assert g0["xcd_sweep_hbm_alone_rate"] == [500, 250] and g0["xcd_sweep_slow"] == [
        {"xcd": 1, "level": "hbm", "mode": "alone"}]
    assert g1["mx_formats"] == ["e4m3", "e2m1"] and g1["hbm_test_steps"][0]["step"] == "addr write"
    assert rep["pushgateway"] == 'error: "no"' and len(rep["failures"]) == 100
    # every check's own failures arrive, in the report's order, after the K1 / K2 verdicts
    mine = [f for f in rep["failures"] if f.startswith("gpu1: ")]
    assert mine[0] == "gpu1: GEMM 1590.5 TFLOP/s below floor 1600" and len(mine) == 3
    assert mine[1].startswith("gpu1: HBM pattern test: hhh") and mine[2] == 'gpu1: XCD sweep: xcd 1 slow "quoted"'
    assert not [f for f in rep["failures"] if f.startswith("gpu0: GEMM")]      # a NaN rate is below no floor
    assert list(g0)[:6] == ["device", "name", "arch", "hbm_total_gb", "gemm_ms", "gemm_tflops"]
    assert list(rep)[-2:] == ["failures", "pushgateway"]


def test_termination_message_stays_under_the_cap(outputs):
    term = outputs[1]
    t = json.loads(term)
    assert len(term.encode()) + 1 < 4096
    assert t["passed"] is False and t["node"] == 'node "7"' and t["xcd_sweep_min_over_median"] == 0.4
    assert 8 <= len(t["failures"]) < 100 and all(len(f) <= 200 for f in t["failures"])
    assert len(t["failures"][0]) == 200 and t["failures"][0].startswith("gpu0: HBM pattern test: hhh")
    assert t["failures"][1] == 'gpu0: XCD sweep: xcd 1 slow "quoted"' 
    assert list(t) == ["passed", "node", "n_gpus", "gemm_tflops_aggregate", "rccl_peak_busbw_GBps", "seconds",
                       "xcd_sweep_min_over_median", "failures"]


def test_every_prometheus_sample_follows_its_type_line(outputs):
    typed, samples = None, {}
    for line in outputs[2].splitlines():
        if line.startswith("# TYPE "):
            typed = line.split()[2]
            assert line.split()[3] == "gauge" and typed not in samples      # HELP / TYPE once per metric
            samples[typed] = 0
        elif line.startswith("# HELP "):
            assert line.split()[2] not in samples
        else:
            m = re.match(r"([a-z0-9_]+)(\{.*\})? (\S+)$", line)
            assert m and m.group(1) == typed, line
            assert m.group(3) == "null" or float(m.group(3)) == float(m.group(3))
            samples[typed] += 1
    assert samples["amdgpu_validate_gemm_tflops"] == 2 and samples["amdgpu_validate_mx_formats"] == 2
    assert samples["amdgpu_validate_xcd_rate"] == 4 and samples["amdgpu_validate_xgmi_p2p_gbps"] == 2
    assert 'amdgpu_validate_passed{node="node \\"7\\""} 0' in outputs[2]
    assert 'amdgpu_validate_host_link_h2d_gbps{gpu="1"} 55' in outputs[2]      # the faster of the two paths
    assert 'amdgpu_validate_host_link_d2h_gbps{gpu="0"} 52' in outputs[2]
    assert list(samples)[:6] == ["amdgpu_validate_passed", "amdgpu_validate_seconds", "amdgpu_validate_gemm_tflops",
                                 "amdgpu_validate_gemm_fp8_tflops", "amdgpu_validate_hbm_copy_gbps",
                                 "amdgpu_validate_hbm_total_gb"]


# ------------------------------------------------------------------ on the GPU
@pytest.mark.gpu
def test_report_shape_is_the_recorded_one():
    """Key paths and their order, the Prometheus names with label keys, the keys of the
    termination message and every value that depends on neither time nor rate."""
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    assert SHAPE["args"] == tool.SHAPE_ARGS
    got = tool.report_shape(BIN, timeout=120)
    assert got["exit"] == SHAPE["exit"] == 0
    assert got["json_paths"] == SHAPE["json_paths"]
    assert got["prometheus"] == SHAPE["prometheus"]
    assert got["termination"] == SHAPE["termination"]
    assert got["values"] == SHAPE["values"]
    v = SHAPE["values"]      # the recording is of a full, clean run
    assert v["passed"] is True and v["gpus[0].mx_formats"] == ["e4m3", "e5m2", "e2m3", "e3m2", "e2m1"]
    assert v["gpus[0].gemm_wrong"] == 0 and v["gpus[0].hbm_test_bad_words"] == 0 and v["failures"] == []
    assert sum(1 for p in SHAPE["json_paths"] if p.endswith("_gated")) == 7
