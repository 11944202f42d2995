"""K5, the per-CU compute sweep, without a GPU: the HW_ID / XCC_ID decode, the
aggregation of synthetic records (``ops.cu_sweep_summarize``), the expected tables
of ``ops.reference`` against numpy matmuls and against the generator in
``validation/include/ntm/cu_sweep_plan.hpp`` (through the C ABI), the header in a
stand-alone sanitized C++ program, the module's ``validation_cu_sweep`` variable and
the Job binary's flags."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nvidia_terraform_modules_amd.ops import reference

ROOT = Path(__file__).resolve().parents[1]
STACK_DIR = ROOT / "modules" / "amd-gpu-stack"
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
MAGIC = 0x4B355357
SUBTESTS = ("lds", "valu", "mfma_bf16", "mfma_fp8")


@pytest.fixture(scope="module")
def ops():
    from nvidia_terraform_modules_amd import ops as o
    from nvidia_terraform_modules_amd.ops._lib import NativeLibraryMissing, lib
    try:
        lib()
    except NativeLibraryMissing:
        pytest.skip("libntm_validation.so not built (python -m nvidia_terraform_modules_amd.ops.build)")
    return o


# ------------------------------------------------------------------ decode
def hw_word(se, sh, cu, simd, wave=0, pipe=0):
    """HW_REG_HW_ID from its fields (gfx9: WAVE 3:0, SIMD 5:4, PIPE 7:6, CU 11:8, SH 12, SE 15:13)."""
    return wave | simd << 4 | pipe << 6 | cu << 8 | sh << 12 | se << 13


@pytest.mark.parametrize("xcc,se,sh,cu,simd", [(0, 0, 0, 0, 0), (15, 7, 1, 15, 3), (5, 2, 0, 7, 1),
                                               (7, 3, 1, 8, 2)])
def test_decode_maps_register_words_to_the_cu(ops, xcc, se, sh, cu, simd):
    # bits outside the fields (wave id, pipe, queue/vm ids above bit 15, XCC_ID's upper bits) are ignored
    hw = hw_word(se, sh, cu, simd, wave=9, pipe=3) | 0xABCD0000
    d = ops.cu_sweep_decode(hw, xcc | 0xFFF0)
    assert (d["xcd"], d["se"], d["sh"], d["cu"], d["simd"]) == (xcc, se, sh, cu, simd)
    assert d["key"] == xcc << 8 | se << 5 | sh << 4 | cu
    # the same CU as tools/experiments/gemm_stamp.py keys it
    assert ((hw >> 8) & 0xF, (hw >> 12) & 1, (hw >> 13) & 7) == (cu, sh, se)


# ------------------------------------------------------------- aggregation
def make_records(ops, cus, per_cu=1):
    """One clean record per (CU, workgroup): CU c -> xcd c // 32, se (c // 8) % 4, sh 0, cu c % 8."""
    rec = np.zeros(cus * per_cu, dtype=ops.cu_sweep_record_dtype())
    for i in range(len(rec)):
        c = i % cus
        rec[i]["hw_id"] = hw_word((c // 8) % 4, 0, c % 8, 0)
        rec[i]["xcc_id"] = c // 32
        rec[i]["simd"] = [0, 1, 2, 3]
        rec[i]["magic"] = MAGIC
        rec[i]["wg"] = i
    return rec


def mark_bad(rec, i, sub, wave, rnd, elem, expected, got, count=1):
    rec[i]["bad"][sub] = count
    rec[i]["first"] = (1 + sub) | wave << 8
    rec[i]["first_round"], rec[i]["first_elem"] = rnd, elem
    rec[i]["expected"], rec[i]["got"] = expected, got


def test_summarize_all_good_full_coverage(ops):
    s = ops.cu_sweep_summarize(make_records(ops, 256, 4), 256, launches=1, gpu=3)
    assert s["ok"] and s["message"] == "" and s["bad_cus"] == []
    assert (s["cus"], s["cus_covered"], s["simds_covered"]) == (256, 256, 1024)
    assert (s["wg_per_cu_min"], s["wg_per_cu_max"], s["workgroups"], s["launches"]) == (4, 4, 1024, 1)


def test_summarize_one_cu_bad_in_all_its_workgroups(ops):
    rec = make_records(ops, 256, 3)
    c = 5 * 32 + 2 * 8 + 7                             # xcd 5 se 2 sh 0 cu 7
    for j, i in enumerate(range(c, len(rec), 256)):
        mark_bad(rec, i, 2, 1, 3 + j, 41, 0x45800000, 0x45800080, count=2)
    s = ops.cu_sweep_summarize(rec, 256, gpu=3)
    assert not s["ok"] and len(s["bad_cus"]) == 1
    b = s["bad_cus"][0]
    assert (b["xcd"], b["se"], b["sh"], b["cu"], b["simd"]) == (5, 2, 0, 7, 1)
    assert (b["workgroups"], b["bad_workgroups"], b["subtests"]) == (3, 3, ["mfma_bf16"])
    assert b["first"] == {"subtest": "mfma_bf16", "round": 3, "elem": 41,
                          "expected": "0x45800000", "got": "0x45800080"}
    assert s["message"] == ("gpu3: CU sweep: 1 bad CU of 256: xcd 5 se 2 sh 0 cu 7 (simd 1) mfma_bf16 "
                            "round 3 elem 41: expected 0x45800000, got 0x45800080; "
                            "3 of 3 workgroups there failed")
    assert len(s["message"]) < 200


def test_summarize_reports_a_cu_that_is_bad_in_one_of_three(ops):
    rec = make_records(ops, 64, 3)
    mark_bad(rec, 64 + 9, 0, 3, 0, 40959, 0x12345678, 0x12345679)
    s = ops.cu_sweep_summarize(rec, 64, gpu=0)
    assert not s["ok"] and len(s["bad_cus"]) == 1
    b = s["bad_cus"][0]
    assert (b["xcd"], b["se"], b["cu"], b["bad_workgroups"], b["workgroups"]) == (0, 1, 1, 1, 3)
    assert b["subtests"] == ["lds"] and b["simd"] == 3
    assert "1 of 3 workgroups there failed" in s["message"] and "lds round 0 elem 40959" in s["message"]
    assert len(s["message"]) < 200


def test_summarize_fails_on_an_uncovered_cu(ops):
    rec = make_records(ops, 256, 2)
    rec = rec[(np.arange(len(rec)) % 256) != 77]       # CU 77 never ran
    s = ops.cu_sweep_summarize(rec, 256, launches=8, gpu=3)
    assert not s["ok"] and s["bad_cus"] == [] and (s["cus"], s["cus_covered"]) == (256, 255)
    assert s["message"] == "gpu3: CU sweep: 1 of 256 CUs ran no workgroup after 8 launches"
    # partial coverage alone marks no CU bad
    part = ops.cu_sweep_summarize(make_records(ops, 8), 256)
    assert part["cus_covered"] == 8 and part["bad_cus"] == [] and not part["ok"]


def test_summarize_counts_an_unwritten_record_and_keeps_messages_short(ops):
    rec = make_records(ops, 256, 4)
    rec[17]["magic"] = 0                               # the workgroup never wrote its record
    s = ops.cu_sweep_summarize(rec, 256, gpu=7)
    assert not s["ok"] and s["unwritten"] == 1 and "1 of 1024 workgroups wrote no record" in s["message"]
    # the longest message: every field at its maximum, 64-bit values
    rec = make_records(ops, 256, 4)
    rec["hw_id"], rec["xcc_id"] = hw_word(7, 1, 15, 3), 15
    for i in range(len(rec)):
        mark_bad(rec, i, 2, 3, 1023, 4294967295, 2**64 - 1, 2**64 - 2)
    worst = ops.cu_sweep_summarize(rec, 256, launches=8, gpu=7)
    assert len(worst["bad_cus"]) == 1 and worst["bad_cus"][0]["workgroups"] == 1024
    assert "expected 0xffffffffffffffff, got 0xfffffffffffffffe" in worst["message"]
    assert len(worst["message"]) < 200


# --------------------------------------------------------------- reference
@pytest.fixture(scope="module")
def expected():
    return reference.cu_sweep_expected(3, 0x1234, 48)


def test_reference_tables_equal_int64_matmuls(expected):
    e = expected
    for name, n, k, lim in (("bf16_16", 16, 128, 8), ("bf16_32", 32, 128, 8), ("fp8", 16, 256, 4)):
        a, b = e[name + "_a"], e[name + "_b"]          # [iters][4][n][k], b by column
        assert a.shape == b.shape == (3, 4, n, k) and a.dtype == np.int64
        assert np.abs(a).max() <= lim and np.abs(b).max() <= lim
        assert a.min() < 0 < a.max() and len(np.unique(a)) == 2 * lim
        d = np.matmul(a, np.swapaxes(b, -1, -2))       # int64
        got = e[name].view(np.float32)
        assert got.shape == (3, 4, n, n) and np.array_equal(got.astype(np.int64), d)
        assert np.array_equal(d.astype(np.float32).view(np.uint32), e[name])
        # every partial sum, in any order, is bounded by the sum of |a * b|
        assert np.matmul(np.abs(a), np.swapaxes(np.abs(b), -1, -2)).max() <= e["peak"] < 2**24
    # rounds and waves differ
    assert not np.array_equal(e["bf16_16"][0], e["bf16_16"][1])
    assert not np.array_equal(e["fp8"][0, 0], e["fp8"][0, 1])


def test_reference_valu_chains_are_exact_and_the_table_is_laid_out(expected):
    e = expected
    f32, f64 = e["f32"].view(np.float32), e["f64"].view(np.float64)
    assert np.abs(f32).max() < 2**24 and np.array_equal(f32, np.round(f32))
    assert np.abs(f64).max() < 2**53 and np.array_equal(f64, np.round(f64))
    assert len(np.unique(e["hash"])) == e["hash"].size and len(np.unique(e["mad"])) == e["mad"].size
    t = e["table"].reshape(3, reference.CU_SWEEP_ROUND_WORDS)
    assert t.dtype == np.uint32
    assert np.array_equal(t[:, :256], e["hash"])
    assert np.array_equal(t[:, 256:768].copy().view(np.uint64), e["mad"])
    assert np.array_equal(t[:, 768:1024], e["f32"])
    assert np.array_equal(t[:, 1024:1536].copy().view(np.uint64), e["f64"])
    assert np.array_equal(t[:, 1536:2560].reshape(3, 4, 16, 16), e["bf16_16"])
    assert np.array_equal(t[:, 2560:6656].reshape(3, 4, 32, 32), e["bf16_32"])
    assert np.array_equal(t[:, 6656:].reshape(3, 4, 16, 16), e["fp8"])
    assert e["lds"].shape == (3, 12) and len(np.unique(e["lds"])) == 36


def test_header_generator_gives_the_same_bytes(ops, expected):
    import ctypes

    from nvidia_terraform_modules_amd.ops._lib import lib
    n = lib().ntm_cu_sweep_expected_bytes(3)
    assert n == 3 * reference.CU_SWEEP_ROUND_WORDS * 4 and lib().ntm_cu_sweep_record_bytes() == 64
    buf = ctypes.create_string_buffer(n)
    assert lib().ntm_cu_sweep_expected(3, 0x1234, buf, n) == 0
    assert buf.raw == expected["table"].tobytes()
    assert lib().ntm_cu_sweep_expected(3, 0x1234, buf, n - 4) != 0       # too small a buffer
    assert lib().ntm_cu_sweep_expected_bytes(0) == 0
    words = (ctypes.c_uint * 12)()
    for rnd in range(3):
        assert lib().ntm_cu_sweep_lds_words(0x1234, rnd, 0, 12, words) == 0
        assert list(words) == expected["lds"][rnd].tolist()
    other = reference.cu_sweep_expected(1, 0x1235, 16)
    assert not np.array_equal(other["table"], expected["table"][:reference.CU_SWEEP_ROUND_WORDS])


# ------------------------------------------------- the plan header, sanitized
PLAN_MAIN = r"""
#include "ntm/cu_sweep_plan.hpp"
#include <cstdlib>
using namespace ntm::cus;
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
static uint32_t hw(unsigned se, unsigned sh, unsigned cu, unsigned simd) {
  return 9u | simd << 4 | 3u << 6 | cu << 8 | sh << 12 | se << 13 | 0xABCD0000u;
}
static Record rec(unsigned xcc, unsigned se, unsigned sh, unsigned cu) {
  Record r{};
  r.hw_id = hw(se, sh, cu, 0);
  r.xcc_id = xcc | 0xF0u;
  for (int w = 0; w < 4; ++w) r.simd[w] = (uint8_t)w;
  r.magic = kMagic;
  return r;
}
int main() {
  const CuId id = decode(hw(7, 1, 15, 3), 0xFFFFu);
  REQUIRE(id.xcc == 15 && id.se == 7 && id.sh == 1 && id.cu == 15 && id.simd == 3);
  REQUIRE(cu_key(hw(7, 1, 15, 3), 0xFFFFu) == 0xFFFu && cu_key(hw(0, 0, 0, 3), 0xF0u) == 0);
  const CuId back = key_to_id(cu_key(hw(2, 0, 7, 1), 5));
  REQUIRE(back.xcc == 5 && back.se == 2 && back.sh == 0 && back.cu == 7);
  for (int v = -4; v <= 3; ++v) {                     // e4m3: 1 = 0x38, sign = 0x80
    const uint32_t c = e4m3_of_small_int(v), m = c & 0x7Fu;
    const int mag = m == 0 ? 0 : (8 + (int)(m & 7)) << ((m >> 3) - 7 + 4) >> 7;
    REQUIRE((v < 0) == ((c & 0x80u) != 0) && mag == (v < 0 ? -v : v));
  }

  // the tables: sizes, and a second call writes the same bytes and nothing beyond them
  REQUIRE(expected_bytes(2) == 2 * 7680 * 4 && expected_bytes(0) == 0);
  std::vector<uint32_t> a(2 * kRoundWords + 1, 0xDEADBEEFu), b(2 * kRoundWords + 1, 0xDEADBEEFu);
  make_expected(a.data(), 2, 77);
  make_expected(b.data(), 2, 77);
  REQUIRE(a == b && a.back() == 0xDEADBEEFu && a[0] != a[kRoundWords]);

  // coverage loop: 8 CUs, launch l covers CUs 0 .. 3 + 2 l: covered after 3 launches
  Sweep sweep;
  int launches = 0;
  REQUIRE(coverage_loop(8, kMaxLaunches, [&](int l, std::vector<Record>& out) {
    ++launches;
    for (unsigned c = 0; c < 4u + 2u * (unsigned)l && c < 8; ++c) out.push_back(rec(c / 4, 0, 0, c % 4));
    return true;
  }, sweep));
  Summary s = sweep.summary(8);
  REQUIRE(launches == 3 && s.launches == 3 && s.ok() && s.cus_covered == 8 && s.simds_covered == 32);
  REQUIRE(s.wg_per_cu_min == 1 && s.wg_per_cu_max == 3 && failure_message(0, s).empty());
  // the cap: a CU that never runs ends the loop after kMaxLaunches
  Sweep capped;
  launches = 0;
  coverage_loop(9, kMaxLaunches, [&](int, std::vector<Record>& out) {
    ++launches;
    for (unsigned c = 0; c < 8; ++c) out.push_back(rec(c / 4, 0, 0, c % 4));
    return true;
  }, capped);
  s = capped.summary(9);
  REQUIRE(launches == kMaxLaunches && !s.ok() && s.bad_cus.empty());
  std::printf("%s\n", failure_message(3, s).c_str());
  // an empty sweep and a failed launch
  REQUIRE(!Sweep().summary(4).ok());
  Sweep none;
  REQUIRE(!coverage_loop(4, 8, [](int, std::vector<Record>&) { return false; }, none));

  Sweep bad;
  std::vector<Record> rs;
  for (int i = 0; i < 4; ++i) {
    Record r = rec(5, 2, 0, 7);
    r.bad[kSubBf16] = 1;
    r.first = (1u + kSubBf16) | 1u << 8;
    r.first_round = 3, r.first_elem = 41, r.expected = 0x45800000u, r.got = 0x45800080u;
    rs.push_back(r);
  }
  rs.push_back(rec(0, 0, 0, 0));
  bad.add(rs.data(), rs.size());
  s = bad.summary(2);
  REQUIRE(s.bad_cus.size() == 1 && s.bad_cus[0].key == cu_key(hw(2, 0, 7, 0), 5));
  std::printf("%s\n", failure_message(3, s).c_str());
  std::printf("%s\n", summary_json(3, s).c_str());
  return 0;
}
"""


def test_plan_header_under_sanitizers(tmp_path):
    """Stand-alone program with its own main against cu_sweep_plan.hpp, built with
    AddressSanitizer and UBSan (host code only; nothing is loaded into Python)."""
    import json
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "cu_plan_main.cpp", tmp_path / "cu_plan_main"
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
    uncovered, bad, js = p.stdout.strip().splitlines()
    assert uncovered == "gpu3: CU sweep: 1 of 9 CUs ran no workgroup after 8 launches"
    assert bad == ("gpu3: CU sweep: 1 bad CU of 2: xcd 5 se 2 sh 0 cu 7 (simd 1) mfma_bf16 round 3 "
                   "elem 41: expected 0x45800000, got 0x45800080; 4 of 4 workgroups there failed")
    assert len(bad) < 200 and len(uncovered) < 200
    j = json.loads(js)
    assert j["message"] == bad and j["bad_cus"][0]["subtests"] == ["mfma_bf16"] and not j["ok"]


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


# local.validation_args at the variables' defaults before validation_cu_sweep existed (the list
# tests/test_hbm_pattern_cpu.py pins)
PARENT_DEFAULT_ARGS = [
    "--gpus", "8", "--size", "8192", "--tflops-floor", "1000", "--min-hbm-gb", "250",
    "--allreduce-max-mib", "1024", "--json", "--fp8-tflops-floor", "2000",
    "--xgmi-tune", "--require-host-prep", "--termination-log", "/dev/termination-log"]


def test_job_args_carry_the_cu_sweep_only_when_asked():
    args = _stack_local("validation_args")
    assert args == PARENT_DEFAULT_ARGS
    on = _stack_local("validation_args", validation_cu_sweep=True)
    i = on.index("--cu-sweep")
    assert on[i + 1] == "--termination-log"
    assert on[:i] + on[i + 1:] == PARENT_DEFAULT_ARGS


def test_stack_plans_with_the_cu_sweep_on(tmp_path):
    from nvidia_terraform_modules_amd.tfcheck.plan import plan

    src = os.path.relpath(STACK_DIR, tmp_path)
    (tmp_path / "main.tf").write_text(
        f'module "stack" {{\n  source = "{src}"\n  cluster_name = "c"\n'
        '  validation_image = "registry.example/amdgpu-validate:1"\n  validation_cu_sweep = true\n}\n')
    p = plan(tmp_path)
    assert not p.errors, p.errors
    assert not [w for w in p.warnings if "no such variable" in w]
    desc = (STACK_DIR / "variables.tf").read_text().split('variable "validation_cu_sweep"')[1].split("}")[0]
    assert "profiles/cu_sweep/README.md" in desc and "false" in desc


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
    assert rc == 0 and "--cu-sweep" in err and "--cu-sweep-iters" in err and "bad_cu" in err
    rc, err = _run_bin("--cu-sweep-iters")
    assert rc == 2 and "missing value for --cu-sweep-iters" in err and "usage" in err
    rc, err = _run_bin("--cu-sweep", "--cu-sweep-iters", "0")
    assert rc == 2
