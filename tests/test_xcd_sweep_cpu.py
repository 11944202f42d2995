"""K8 without a GPU: the per-XCD aggregation, conservation, verdict and messages of
``ops.xcd_sweep_summarize`` (host code of the native library) on synthetic records, the plan
header in a stand-alone sanitized program, the module variables and the binary's flags."""
import json
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
STACK_DIR = ROOT / "modules" / "amd-gpu-stack"
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
MAGIC = 0x4B385843
TILE = 64 * 1024


@pytest.fixture(scope="module")
def ops():
    from nvidia_terraform_modules_amd import ops as o
    from nvidia_terraform_modules_amd.ops._lib import NativeLibraryMissing, lib
    try:
        lib()
    except NativeLibraryMissing:
        pytest.skip("libntm_validation.so not built (python -m nvidia_terraform_modules_amd.ops.build)")
    return o


def make_records(ops, xcds=8, per_cu=2, tiles=4, ticks=20000, ghz=2.4, start=1_000_000):
    """xcds x 32 CUs x per_cu clean workgroups: CU c of XCD x -> se c // 8, sh 0, cu c % 8; every
    workgroup pulled `tiles` tiles in `ticks` ticks from `start` at `ghz`."""
    rec = np.zeros(xcds * 32 * per_cu, dtype=ops.xcd_sweep_record_dtype())
    for i in range(len(rec)):
        x, c = i % xcds, (i // xcds) % 32
        rec[i]["magic"], rec[i]["wg"], rec[i]["xcc_id"] = MAGIC, i, x
        rec[i]["hw_id"] = (c // 8) << 13 | (c % 8) << 8
        rec[i]["tiles"], rec[i]["rt_ticks"], rec[i]["rt_start"] = tiles, ticks, start
        rec[i]["cycles"] = int(ticks * ghz * 10)
    return rec


def of_xcd(rec, x):
    return (rec["xcc_id"] & 0xF) == x


def test_record_layout(ops):
    from nvidia_terraform_modules_amd.ops._lib import lib
    assert lib().ntm_xcd_sweep_record_bytes() == ops.xcd_sweep_record_dtype().itemsize == 64
    assert lib().ntm_xcd_sweep_tile_bytes() == TILE and lib().ntm_xcd_sweep_mfma_per_batch() == 512


def test_the_two_contended_cells_are_reported_not_judged(ops):
    ungated = {(lv, md) for lv in ops.XCD_SWEEP_LEVELS for md in ops.XCD_SWEEP_MODES
               if not ops.xcd_sweep_gated(lv, md)}
    assert ungated == {("mall", "together"), ("hbm", "together")}


def test_all_equal_is_ok(ops):
    s = ops.xcd_sweep_summarize(make_records(ops), "hbm", "together", 8, ratio=0.85, expected_tiles=256)
    assert s["ok"] and s["message"] == "" and s["failures"] == [] and s["rule_ran"]
    assert s["min_over_median"] == 1.0 and s["slow"] == [] and s["bad"] == []
    # 256 tiles x 64 KiB in 200 us = 83.886 GB/s
    assert all(abs(r - 256 * TILE / 200e-6 / 1e9) < 1e-3 for r in s["rates"])
    assert all(p["workgroups"] == 64 and p["cus"] == 32 and p["bytes"] == 256 * TILE for p in s["per_xcd"])
    assert all(abs(c - 2.4) < 1e-6 for c in s["clocks_ghz"])


def half_rate(ops):
    rec = make_records(ops)
    rec["rt_ticks"][of_xcd(rec, 5)] = 40000          # the same tiles in twice the time ...
    rec["cycles"][of_xcd(rec, 5)] = int(40000 * 2.3 * 10)   # ... at 2.3 GHz
    return rec


def test_one_xcd_at_half_rate_is_named_with_both_clocks(ops):
    s = ops.xcd_sweep_summarize(half_rate(ops), "hbm", "together", 8, ratio=0.85, gpu=3, expected_tiles=256)
    assert not s["ok"] and s["slow"] == [5] and len(s["failures"]) == 1
    assert s["message"] == ("gpu3: XCD sweep: xcd 5 slow at hbm/together: 41.9 GB/s vs median 83.9 "
                            "(0.50 < 0.85); clock 2.30 GHz vs median 2.40")
    assert [p["slow"] for p in s["per_xcd"]] == [x == 5 for x in range(8)]


def test_ratio_zero_reports_without_failing(ops):
    s = ops.xcd_sweep_summarize(half_rate(ops), "hbm", "together", 8, ratio=0, expected_tiles=256)
    assert s["ok"] and s["message"] == "" and not s["rule_ran"] and "report only" in s["rule_skipped"]
    assert s["min_over_median"] == 0.5 and s["slow"] == []


def test_even_count_median_is_the_mean_of_the_middle_two(ops):
    rec = make_records(ops)
    ticks = [10000, 12500, 16000, 20000, 25000, 32000, 40000, 50000]
    for x, t in enumerate(ticks):
        rec["rt_ticks"][of_xcd(rec, x)] = t
    s = ops.xcd_sweep_summarize(rec, "l2", "alone", 8, ratio=0.5, expected_tiles=256)
    gb = 256 * TILE / 1e9
    rates = [gb / (t * 1e-8) for t in ticks]
    median = 0.5 * (rates[3] + rates[4])          # sorted descending: the 4th and 5th
    assert np.allclose(s["rates"], rates, rtol=1e-5) and abs(s["median_rate"] - median) < 1e-3
    assert abs(s["min_over_median"] - rates[7] / median) < 1e-5
    assert s["slow"] == [x for x, r in enumerate(rates) if r < 0.5 * median] == [7]


def test_an_xcd_with_no_record_fails(ops):
    rec = make_records(ops)
    s = ops.xcd_sweep_summarize(rec[~of_xcd(rec, 6)], "mall", "together", 8, gpu=1, expected_tiles=256)
    assert not s["ok"] and s["message"] == "gpu1: XCD sweep: xcd 6 ran no workgroup at mall/together"
    short = rec[~(of_xcd(rec, 2) & (((rec["hw_id"] >> 8) & 0xF) == 7) & ((rec["hw_id"] >> 13) == 3))]
    s = ops.xcd_sweep_summarize(short, "mall", "together", 8, gpu=1)
    assert s["message"] == "gpu1: XCD sweep: xcd 2: 31 of 32 CUs ran a workgroup at mall/together"


@pytest.mark.parametrize("delta", [-1, 1])
def test_a_tile_sum_off_by_one_fails(ops, delta):
    rec = make_records(ops)
    rec["tiles"][np.flatnonzero(of_xcd(rec, 4))[0]] = 4 + delta
    s = ops.xcd_sweep_summarize(rec, "l2", "together", 8, expected_tiles=256)
    assert not s["ok"] and s["failures"] == [
        f"gpu0: XCD sweep: xcd 4 pulled {256 + delta} tiles at l2/together, expected 256"]


def test_a_bad_word_is_reported_with_offset_and_bits(ops):
    rec = make_records(ops)
    i, j = np.flatnonzero(of_xcd(rec, 2))[[3, 9]]
    rec[i]["bad_words"], rec[i]["first_off"] = 2, 0x123458
    rec[i]["expected"], rec[i]["got"] = 0xDEADBEEF00C0FFEE, 0xDEADBEEF00C0FFEE ^ (1 << 40)
    rec[j]["bad_words"], rec[j]["first_off"] = 1, 0x200000          # a later word of the same slice
    rec[j]["expected"], rec[j]["got"] = 1, 3
    s = ops.xcd_sweep_summarize(rec, "mall", "alone", 8, ratio=0.85, gpu=3, expected_tiles=256)
    assert not s["ok"] and s["bad"] == [2] and s["slow"] == []
    assert s["message"] == ("gpu3: XCD sweep: xcd 2 read wrong data at mall/alone: slice offset 0x123458, "
                            "expected 0xdeadbeef00c0ffee, got 0xdeadbfef00c0ffee, bad bits 0x10000000000; 3 words")
    assert s["per_xcd"][2]["first"]["bad_bits"] == hex(1 << 40)


def test_two_xcds_skip_the_rule_with_a_reason(ops):
    rec = make_records(ops, xcds=2)
    rec["rt_ticks"][of_xcd(rec, 1)] = 80000
    s = ops.xcd_sweep_summarize(rec, "hbm", "together", 2, ratio=0.85, expected_tiles=256)
    assert s["ok"] and not s["rule_ran"] and "fewer than 3 XCDs" in s["rule_skipped"]
    assert abs(s["min_over_median"] - 0.4) < 1e-6


def test_every_message_is_under_200_characters(ops):
    rec = make_records(ops)
    rec["bad_words"], rec["first_off"] = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFF8
    rec["expected"], rec["got"] = 0xFFFFFFFFFFFFFFFF, 0
    rec["tiles"], rec["rt_ticks"][of_xcd(rec, 0)] = 0xFFFFFFFF, 0xFFFFFFFF
    s = ops.xcd_sweep_summarize(rec, "mall", "together", 8, ratio=0.99, gpu=15, expected_tiles=2**40)
    assert len(s["failures"]) >= 17 and all(len(f) < 200 for f in s["failures"])
    blank = np.zeros(3, dtype=rec.dtype)
    s = ops.xcd_sweep_summarize(blank, "l2", "alone", 8)
    assert s["unwritten"] == 3 and all(len(f) < 200 for f in s["failures"])


def test_span_uses_only_the_xcds_own_stamps(ops):
    rec = make_records(ops)
    sel = np.flatnonzero(of_xcd(rec, 3))
    rec["rt_start"][sel[:10]] += 5000                   # a late starter widens XCD 3's own span
    base = ops.xcd_sweep_summarize(rec, "hbm", "together", 8, expected_tiles=256)
    assert base["per_xcd"][3]["span_ticks"] == 25000 and base["per_xcd"][0]["span_ticks"] == 20000
    moved = rec.copy()
    moved["rt_start"][of_xcd(moved, 6)] += 987_654_321   # XCD 6's counter far from the others'
    s = ops.xcd_sweep_summarize(moved, "hbm", "together", 8, expected_tiles=256)
    assert s["rates"] == base["rates"] and s["clocks_ghz"] == base["clocks_ghz"]
    # a workgroup that pulled nothing does not stretch the span
    idle = rec.copy()
    idle["tiles"][sel[-1]], idle["rt_start"][sel[-1]] = 0, 1
    assert ops.xcd_sweep_summarize(idle, "hbm", "together", 8)["per_xcd"][3]["span_ticks"] == 25000


def test_alone_launches_concatenate(ops):
    launches = []
    for x in range(8):
        rec = make_records(ops, start=1_000_000 + 50_000 * x)
        rec["tiles"][~of_xcd(rec, x)] = 0
        rec["tiles"][of_xcd(rec, x)] = 4
        launches.append(rec)
    s = ops.xcd_sweep_summarize(np.concatenate(launches), "hbm", "alone", 8, ratio=0.85, expected_tiles=256)
    assert s["ok"] and all(p["tiles"] == 256 and p["span_ticks"] == 20000 for p in s["per_xcd"])
    one = ops.xcd_sweep_summarize(launches[7], "hbm", "alone", 8, ratio=0.85, expected_tiles=256, xcd_mask=1 << 7)
    assert one["ok"] and not one["rule_ran"] and [p["judged"] for p in one["per_xcd"]] == [False] * 7 + [True]


# ------------------------------------------------- the header on its own
PLAN_MAIN = r"""
#include "ntm/xcd_sweep_plan.hpp"
#include <cstdio>
using namespace ntm::xcs;
static Record mk(uint32_t x, uint32_t c, uint32_t i, uint32_t tiles, uint32_t ticks) {
  Record r{};
  r.magic = kMagic, r.xcc_id = x, r.wg = i, r.hw_id = (c / 8) << 13 | (c % 8) << 8;
  r.tiles = tiles, r.rt_ticks = ticks, r.cycles = ticks * 24, r.rt_start = 1000000;
  return r;
}
int main() {
  static_assert(kTileBytes == 65536 && sizeof(Record) == 64, "layout");
  if (gated(kLevelHbm, kModeTogether) || gated(kLevelMall, kModeTogether) || !gated(kLevelHbm, kModeAlone) ||
      !gated(kLevelL2, kModeTogether) || !gated(kLevelMfma, kModeTogether))
    return 4;
  if (tiles_per_slice(4u << 20) != 64 || expected_tiles(4u << 20, 2) != 128 || slice_ok(65536 + 16) ||
      !slice_ok(3 * 65536) || passes_ok(1u << 20, 1u << 30) || grid_of(8, 2) != 512 || full_mask(8) != 0xFF ||
      xcds_expected(256) != 8 || xcds_expected(64) != 2 || level_mib(kLevelMall, 8) != 8 ||
      level_mib(kLevelHbm, 256) != 256 || passes_for_min_span(4, 20000) != 4 || passes_for_min_span(4, 1000) != 80 ||
      passes_for_min_span(7, 0) != 7 || passes_for_min_span(1, 1) != 20000 || median_of({4, 1, 3, 2}) != 2.5 || median_of({}) != 0)
    return 1;
  std::vector<Record> v;
  for (uint32_t x = 0; x < 8; ++x)
    for (uint32_t c = 0; c < 32; ++c)
      for (uint32_t w = 0; w < 2; ++w) v.push_back(mk(x, c, (uint32_t)v.size(), 4, x == 5 ? 40000 : 20000));
  Summary slow = summarize(v.data(), v.size(), kLevelHbm, kModeTogether, 8, 0xFF, 256, 0.85, 3);
  std::puts(failure_message(slow).c_str());
  v[17].bad_words = 1, v[17].first_off = 0x40, v[17].expected = 0x10, v[17].got = 0x30;
  Summary bad = summarize(v.data(), v.size(), kLevelMall, kModeAlone, 8, 0xFF, 256, 0, 3);
  std::puts(failure_message(bad).c_str());
  Summary none = summarize(nullptr, 0, kLevelL2, kModeAlone, 16, ~0u, 1, 0.5, 0);  // 16 XCDs, no record at all
  std::puts(failure_message(none).c_str());
  // sizing: only XCDs that timed something count; with none there is nothing to size from
  std::vector<Record> seven(v.begin() + 64, v.end());  // XCD 0 ran nothing
  Summary gap = summarize(seven.data(), seven.size(), kLevelHbm, kModeTogether, 8, 0xFF, 256, 0, 0);
  if (gap.rows[0].span_ticks != 0 || min_timed_span(gap) != 20000 || min_timed_span(none) != 0 ||
      passes_for_min_span(64, min_timed_span(none)) != 64 || failure_message(gap).find("xcd 0 ran no workgroup") == std::string::npos)
    return 3;
  Summary stray = summarize(v.data(), v.size(), kLevelMfma, kModeTogether, 4, 0xF, 0, 0.5, 0);
  if (stray.strays != 4 * 64 || stray.bad.size() != 1 || stray.failures.size() != 1) return 2;
  std::puts(summary_json(bad).c_str());
  return 0;
}
"""


def test_plan_header_under_sanitizers(tmp_path):
    """Stand-alone program with its own main against xcd_sweep_plan.hpp, built with
    AddressSanitizer and UBSan (host code only; nothing is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "xcd_plan_main.cpp", tmp_path / "xcd_plan_main"
    src.write_text(PLAN_MAIN)
    inc = f"-I{ROOT / 'validation' / 'include'}"
    if cxx:
        static = (["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx)
                  else ["-static-libsan"])
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *static, inc, str(src), "-o", str(exe)]
    elif os.path.exists(hipcc):
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
               "-fsanitize=undefined", "-static-libsan", inc, str(src), "-o", str(exe)]
    else:
        pytest.skip("no C++ compiler")
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    slow, bad, none, js = p.stdout.strip().splitlines()
    assert slow == ("gpu3: XCD sweep: xcd 5 slow at hbm/together: 41.9 GB/s vs median 83.9 (0.50 < 0.85); "
                    "clock 2.40 GHz vs median 2.40")
    assert bad == ("gpu3: XCD sweep: xcd 0 read wrong data at mall/alone: slice offset 0x40, expected 0x10, "
                   "got 0x30, bad bits 0x20; 1 word")
    assert none == "gpu0: XCD sweep: xcd 0 ran no workgroup at l2/alone"
    j = json.loads(js)
    assert j["message"] == bad and j["bad"] == [0] and not j["ok"] and len(j["per_xcd"]) == 8


# ------------------------------------------------------------ the module
def _stack_local(name, **overrides):
    """local.<name> of modules/amd-gpu-stack with variable defaults + overrides."""
    from nvidia_terraform_modules_amd.tfcheck.config import load_module
    from nvidia_terraform_modules_amd.tfcheck.evaluate import Evaluator, Scope, convert

    mod = load_module(STACK_DIR)
    ev = Evaluator()
    variables = {}
    for vn, v in mod.variables.items():
        if vn in overrides:
            variables[vn] = overrides[vn]
        elif not v.required:
            variables[vn] = convert(ev.eval(v.block.body.attr("default"), Scope({}, {})),
                                    v.type_expr)
    scope = Scope(variables, {n: e for n, (e, _, _) in mod.locals.items()}, str(mod.path))
    return ev.eval(mod.locals[name][0], scope)


def test_job_args_carry_the_xcd_sweep_only_when_asked():
    off = _stack_local("validation_args")
    assert not [a for a in off if "xcd" in a]
    assert _stack_local("validation_args", validation_xcd_ratio=0.85) == off     # the ratio alone does nothing
    on = _stack_local("validation_args", validation_xcd_sweep=True)
    i = on.index("--xcd-sweep")
    assert on[i + 1] == "--termination-log" and on[:i] + on[i + 1:] == off
    both = _stack_local("validation_args", validation_xcd_sweep=True, validation_xcd_ratio=0.85)
    i = both.index("--xcd-sweep")
    assert both[i:i + 4] == ["--xcd-sweep", "--xcd-ratio", "0.85", "--termination-log"]
    assert both[:i] + both[i + 3:] == off


def _plan_with(tmp_path, extra):
    from nvidia_terraform_modules_amd.tfcheck.plan import plan

    src = os.path.relpath(STACK_DIR, tmp_path)
    (tmp_path / "main.tf").write_text(
        f'module "stack" {{\n  source = "{src}"\n  cluster_name = "c"\n'
        f'  validation_image = "registry.example/amdgpu-validate:1"\n{extra}}}\n')
    return plan(tmp_path)


def test_stack_plans_with_the_xcd_sweep_on(tmp_path):
    p = _plan_with(tmp_path, "  validation_xcd_sweep = true\n  validation_xcd_ratio = 0.85\n")
    assert not p.errors, p.errors
    assert not [w for w in p.warnings if "no such variable" in w]
    text = (STACK_DIR / "variables.tf").read_text()
    sweep = text.split('variable "validation_xcd_sweep"')[1].split("\n}")[0]
    ratio = text.split('variable "validation_xcd_ratio"')[1].split("\n}")[0]
    assert "profiles/xcd_sweep/README.md" in sweep and "false" in sweep
    assert "profiles/xcd_sweep/README.md" in ratio and "default     = 0" in ratio


@pytest.mark.parametrize("bad", ["1", "-0.1", "1.5"])
def test_ratio_outside_zero_to_one_is_refused(tmp_path, bad):
    p = _plan_with(tmp_path, f"  validation_xcd_sweep = true\n  validation_xcd_ratio = {bad}\n")
    assert any("validation_xcd_ratio must be >= 0 and < 1" in e for e in p.errors), p.errors


# ------------------------------------------------------------ the binary
def _run_bin(*args):
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = dict(os.environ)
    e.pop("NTM_FAULT_INJECT", None)
    p = subprocess.run([str(BIN), *args], capture_output=True, text=True, timeout=60, env=e)
    return p.returncode, p.stderr


def test_binary_help_and_flag_parsing():
    rc, err = _run_bin("--help")
    assert rc == 0
    for word in ("--xcd-sweep", "--xcd-sweep-mib", "--xcd-ratio", "slow_xcd", "corrupt_xcd"):
        assert word in err, word
    rc, err = _run_bin("--xcd-ratio")
    assert rc == 2 and "missing value for --xcd-ratio" in err and "usage" in err
    for bad in (("--xcd-sweep", "--xcd-ratio", "1"), ("--xcd-sweep", "--xcd-ratio", "-0.5"),
                ("--xcd-sweep", "--xcd-sweep-mib", "0"), ("--xcd-sweep", "--xcd-sweep-mib", "99999")):
        assert _run_bin(*bad)[0] == 2, bad
