"""K4, the HBM pattern test, without a GPU: the pattern's definition against
``ops.reference``, the Job's sequence (``models.validation_job.hbm_memtest``)
on the CPU backend, the chunk plan and failure message of
``validation/include/ntm/hbm_test_plan.hpp`` through a stand-alone sanitized
C++ program, and the module's ``validation_hbm_test_gb`` variable."""
import os
import shutil
import subprocess
from pathlib import Path

import pytest
import torch

from nvidia_terraform_modules_amd.ops import reference
from nvidia_terraform_modules_amd.models import validation_job as vj

ROOT = Path(__file__).resolve().parents[1]
STACK_DIR = ROOT / "modules" / "amd-gpu-stack"
M32, M64 = 0xFFFFFFFF, (1 << 64) - 1


# ------------------------------------------------------------------ the oracle
# Typed from the formulas in validation/README.md ("K4: HBM pattern test"), one
# word at a time in Python integers: nothing shared with ops.reference.
def oracle_bytes(nbytes, pattern, seed, invert, base):
    out = bytearray()
    if pattern == 0:                                   # ADDR: 8-byte word = its 8-byte index ^ seed
        for off in range(0, nbytes, 8):
            v = (((base + off) // 8) ^ seed) & M64
            out += ((v ^ M64) if invert else v).to_bytes(8, "little")
    else:                                              # HASH: per 32-bit word
        for off in range(0, nbytes, 4):
            w = (base + off) // 4
            lo, hi = w & M32, w >> 32
            x = (lo + (seed & M32)) & M32
            x ^= x >> 16
            x = (x * 0x7FEB352D) & M32
            x ^= x >> 15
            x ^= (hi * 0x9E3779B9) & M32
            out += ((x ^ M32) if invert else x).to_bytes(4, "little")
    return bytes(out)


@pytest.mark.parametrize("base", [0, 2**35 - 4096], ids=["base0", "base_carry"])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", [0, 1], ids=["addr", "hash"])
def test_reference_matches_the_written_formulas(pattern, invert, base):
    # at byte 4096 of the second base both carries happen: the upper half of the 8-byte index
    # (ADDR) goes 0 -> 1 and the upper half of the 32-bit word index (HASH's hi) 1 -> 2
    n = 8192
    seed = 0x1234_5678_9ABC_DEF1
    t = torch.zeros(n // 4, dtype=torch.int32)
    reference.hbm_pattern_write(t, pattern, seed=seed, invert=invert, base=base)
    assert t.numpy().tobytes() == oracle_bytes(n, pattern, seed, invert, base)
    assert reference.hbm_pattern_verify(t, pattern, seed=seed, invert=invert, base=base).ok
    if base:
        assert ((base + 4088) // 8 >> 32, (base + 4096) // 8 >> 32) == (0, 1)
        assert ((base + 4092) // 4 >> 32, (base + 4096) // 4 >> 32) == (1, 2)


def test_reference_verify_reports_offset_bits_and_inverts_in_place():
    base = 1 << 20
    t = torch.zeros(1024, dtype=torch.int32)
    reference.hbm_pattern_write(t, "hash", seed=3, base=base)
    t[301] ^= 1 << 13                                  # upper half of the 8-byte word at byte 1200
    rep = reference.hbm_pattern_verify(t, "hash", seed=3, base=base, invert_after=True)
    assert not rep.ok and rep.bad_words == 1 and rep.first_bad_offset == base + 1200
    assert rep.bad_bits == 1 << (13 + 32)
    assert rep.records[0]["expected"] ^ rep.records[0]["got"] == 1 << 45
    assert t.numpy().tobytes() == oracle_bytes(4096, 1, 3, True, base)
    assert reference.hbm_pattern_verify(t, "hash", seed=3, invert=True, base=base).ok


def test_reference_rejects_unaligned_sizes_and_bases():
    with pytest.raises(ValueError):
        reference.hbm_pattern_write(torch.zeros(6, dtype=torch.int32), 0)
    with pytest.raises(ValueError):
        reference.hbm_pattern_write(torch.zeros(8, dtype=torch.int32), 0, base=8)
    with pytest.raises(ValueError):
        reference.hbm_pattern_verify(torch.zeros(8, dtype=torch.int32), 2)


# -------------------------------------------------------- the Job's sequence
def test_memtest_passes_on_the_cpu_backend():
    rep = vj.hbm_memtest(torch.device("cpu"), 1 << 20, chunk_bytes=1 << 18, backend=reference)
    assert rep["ok"] and rep["bad_words"] == 0 and rep["first_bad_offset"] is None
    assert rep["bytes"] == 1 << 20 and rep["chunks"] == 4 and rep["passes"] == 1


class _FlipAfterWrite:
    """ops.reference, but one bit of the tested space flips after the first write."""

    def __init__(self, offset, bit):
        self.offset, self.bit, self.done = offset, bit, False

    def hbm_pattern_write(self, t, pattern, seed=0, invert=False, base=0):
        reference.hbm_pattern_write(t, pattern, seed=seed, invert=invert, base=base)
        n = t.numel() * t.element_size()
        if not self.done and base <= self.offset < base + n:
            self.done = True
            t.view(-1).view(torch.uint8)[self.offset - base + self.bit // 8] ^= 1 << (self.bit % 8)
        return t

    hbm_pattern_verify = staticmethod(reference.hbm_pattern_verify)


def test_memtest_finds_one_flipped_bit():
    off, bit = (1 << 18) * 2 + 4096, 37               # in the third chunk
    rep = vj.hbm_memtest(torch.device("cpu"), 1 << 20, chunk_bytes=1 << 18,
                         backend=_FlipAfterWrite(off, bit))
    assert not rep["ok"] and rep["bad_words"] == 1
    assert rep["first_bad_offset"] == off and rep["bad_bits"] == 1 << bit
    assert rep["failed_step"] == "addr verify+invert"
    assert rep["records"] == [{"offset": off, "expected": off // 8, "got": (off // 8) ^ (1 << bit)}]


# ------------------------------------------------- the plan header, sanitized
PLAN_MAIN = r"""
#include "ntm/hbm_test_plan.hpp"
#include <cstdlib>
using namespace ntm::hbm;
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
static uint64_t sum(const TestPlan& p) { uint64_t s = 0; for (auto c : p.chunks) s += c; return s; }
static void common(const TestPlan& p, uint64_t fre) {
  REQUIRE(sum(p) == p.tested_bytes);
  REQUIRE(p.tested_bytes + p.headroom_bytes <= fre || p.tested_bytes == 0);
  for (size_t i = 0; i < p.chunks.size(); ++i) {
    REQUIRE(p.chunks[i] > 0 && p.chunks[i] % 16 == 0 && p.chunks[i] <= 16 * kGiB);
    if (i + 1 < p.chunks.size()) REQUIRE(p.chunks[i] >= kGiB);
  }
}
int main() {
  const uint64_t fre = 286ull * 1000 * 1000 * 1000 + 12345;        // an MI355X after K2
  REQUIRE(default_headroom(fre) == fre / 50);                      // 2 % > 2 GiB
  REQUIRE(default_headroom(8 * kGiB) == 2 * kGiB);
  TestPlan all = make_test_plan(fre, -1);                          // -1 = all
  common(all, fre);
  REQUIRE(all.headroom_bytes == fre / 50);
  REQUIRE(all.tested_bytes == ((fre - fre / 50) & ~15ull));
  REQUIRE(all.requested_bytes == fre - fre / 50);
  REQUIRE(all.chunks.size() == (all.tested_bytes + 16 * kGiB - 1) / (16 * kGiB));
  TestPlan four = make_test_plan(fre, 4);                          // 4 GB = one chunk
  common(four, fre);
  REQUIRE(four.tested_bytes == 4000000000ull && four.chunks.size() == 1);
  TestPlan big = make_test_plan(fre, 1000);                        // above free: clamped
  common(big, fre);
  REQUIRE(big.requested_bytes == 1000000000000ull);
  REQUIRE(big.tested_bytes == all.tested_bytes);
  REQUIRE(make_test_plan(fre, 0).chunks.empty());                  // 0 = off
  REQUIRE(make_test_plan(kGiB, -1).chunks.empty());                // nothing beyond the headroom
  TestPlan small = make_test_plan(fre, 40, default_headroom(fre), 3 * kGiB + 8);
  common(small, fre);
  REQUIRE(small.chunks[0] == 3 * kGiB && small.tested_bytes == 40000000000ull);
  REQUIRE(make_test_plan(fre, 3, 0, 1).chunks[0] == kGiB);         // chunk floor 1 GiB
  REQUIRE(make_test_plan(fre, 40, 0, ~0ull).chunks[0] == 16 * kGiB);
  common(make_test_plan(fre, 1e30), fre);
  // a nonsensical "free" neither overflows nor builds an endless list
  TestPlan huge = make_test_plan(~0ull, 5);
  common(huge, ~0ull);
  REQUIRE(huge.tested_bytes == 5000000000ull && huge.headroom_bytes == ~0ull / 50);
  TestPlan capped = make_test_plan(~0ull, -1);
  common(capped, ~0ull);
  REQUIRE(capped.chunks.size() == kMaxChunks && capped.tested_bytes == kMaxChunks * 16 * kGiB);
  REQUIRE(capped.requested_bytes == ~0ull - ~0ull / 50);

  PatternResult r;
  pattern_result_init(r);
  REQUIRE(r.first_bad_offset == ~0ull && r.bad_words == 0 && sizeof(r) == 128 && alignof(PatternResult) == 64);
  r.bad_words = 2;
  r.bad_bits_or = 0x2000;
  r.first_bad_offset = 0x1234567890ull;
  r.n_records = 7;                                                 // more mismatches than slots
  r.records[0] = {0x2234567890ull, 0x5555, 0x5557};
  r.records[1] = {0x1234567890ull, 0xAAAA00000000ull, 0xAAAA00002000ull};
  const std::string m = failure_message(3, "addr verify+invert", r);
  std::printf("%s\n", m.c_str());
  return 0;
}
"""


def test_plan_header_under_sanitizers(tmp_path):
    """Stand-alone program with its own main against hbm_test_plan.hpp, built with
    AddressSanitizer and UBSan (host code only; nothing is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "plan_main.cpp", tmp_path / "plan_main"
    src.write_text(PLAN_MAIN)
    inc = f"-I{ROOT / 'validation' / 'include'}"
    if cxx:
        # the sanitizer runtimes are linked statically, so the program does not depend on
        # what else the environment has the loader bring in, or in which order
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
    msg = p.stdout.strip()
    assert msg.startswith("gpu3: HBM pattern test (addr verify+invert): 2 bad word(s), first at byte")
    assert "offset 0x0000001234567890" in msg                      # the first bad word ...
    assert "expected 0x0000aaaa00000000, got 0x0000aaaa00002000" in msg   # ... and its record
    assert msg.endswith("bad bits 0x0000000000002000") and len(msg) < 200


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


# local.validation_args at the variables' defaults before validation_hbm_test_gb existed
PARENT_DEFAULT_ARGS = [
    "--gpus", "8", "--size", "8192", "--tflops-floor", "1000", "--min-hbm-gb", "250",
    "--allreduce-max-mib", "1024", "--json", "--fp8-tflops-floor", "2000",
    "--xgmi-tune", "--require-host-prep", "--termination-log", "/dev/termination-log"]


def test_job_args_carry_the_hbm_test_only_when_asked():
    args = _stack_local("validation_args")
    assert "--hbm-test-gb" not in args and args == PARENT_DEFAULT_ARGS
    full = _stack_local("validation_args", validation_hbm_test_gb=-1)
    i = full.index("--hbm-test-gb")
    assert full[i + 1] == "-1" and i < full.index("--termination-log")
    assert [a for j, a in enumerate(full) if j not in (i, i + 1)] == PARENT_DEFAULT_ARGS
    some = _stack_local("validation_args", validation_hbm_test_gb=64)
    assert some[some.index("--hbm-test-gb") + 1] == "64"


def _stack_plan(tmp_path, **kv):
    from nvidia_terraform_modules_amd.tfcheck.plan import plan

    args = "\n".join(f"  {k} = {v!r}" for k, v in kv.items())
    src = os.path.relpath(STACK_DIR, tmp_path)
    (tmp_path / "main.tf").write_text(
        f'module "stack" {{\n  source = "{src}"\n  cluster_name = "c"\n{args}\n}}\n')
    return plan(tmp_path)


def test_hbm_test_gb_below_minus_one_is_rejected(tmp_path):
    bad = _stack_plan(tmp_path, validation_hbm_test_gb=-2)
    assert any("validation_hbm_test_gb must be >= -1" in e for e in bad.errors), bad.errors
    ok = _stack_plan(tmp_path, validation_hbm_test_gb=-1)
    assert not [e for e in ok.errors if "validation_hbm_test_gb" in e], ok.errors
    assert not [e for e in ok.errors + ok.warnings if "no such variable" in e]
    desc = (STACK_DIR / "variables.tf").read_text().split('variable "validation_hbm_test_gb"')[1]
    assert "-1 tests all free HBM" in desc.split("validation {")[0]
    assert "profiles/hbm_memtest/README.md" in desc.split("validation {")[0]
