"""K6, the host-link (PCIe) check, without a GPU: ``ops.reference.host_link_*`` against
``hbm_pattern_words``, the argument checks of ``ops.host_link_*``, the host side in
``validation/include/ntm/host_link_plan.hpp`` through a stand-alone sanitized C++
program, and the module's ``validation_host_link_*`` variables."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import ops
from nvidia_terraform_modules_amd.models import validation_job as vj
from nvidia_terraform_modules_amd.ops import reference

ROOT = Path(__file__).resolve().parents[1]
STACK_DIR = ROOT / "modules" / "amd-gpu-stack"
SEED = 0x1234_5678_9ABC_DEF1


# ------------------------------------------------------------- the reference
@pytest.mark.parametrize("base", [0, 2**35 - 4096], ids=["base0", "base_carry"])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", [0, 1], ids=["addr", "hash"])
def test_reference_push_and_pull_speak_the_hbm_pattern(pattern, invert, base):
    n = 8192
    t = torch.zeros(n // 4, dtype=torch.int32)
    assert reference.host_link_push(t, pattern, seed=SEED, invert=invert, base=base, blocks=3) is t
    want = reference.hbm_pattern_words(n, pattern, SEED, invert, base)
    assert np.array_equal(t.numpy().view(np.uint32), want)
    dst = torch.zeros_like(t)
    rep = reference.host_link_pull(t, pattern, seed=SEED, invert=invert, base=base, dst=dst)
    assert rep.ok and rep.bad_words == 0 and torch.equal(dst, t)


def test_reference_pull_names_offset_expected_got_and_bits():
    base = 1 << 20
    t = torch.zeros(1024, dtype=torch.int32)
    reference.host_link_push(t, "hash", seed=3, base=base)
    exp = reference.hbm_pattern_words(4096, "hash", 3, False, base).view(np.uint64)
    t[301] ^= 1 << 13                                  # upper half of the 8-byte word at byte 1200
    rep = reference.host_link_pull(t, "hash", seed=3, base=base)
    assert not rep.ok and rep.bad_words == 1 and rep.first_bad_offset == base + 1200
    assert rep.bad_bits == 1 << 45
    assert rep.records == [{"offset": base + 1200, "expected": int(exp[150]),
                            "got": int(exp[150]) ^ (1 << 45)}]


def test_reference_chase_is_one_cycle_and_walks_it():
    n = 1024
    nxt = reference.host_link_chase_next(n, seed=7)
    assert sorted(nxt.tolist()) == list(range(n))
    seen, i = 0, 0
    while True:
        i, seen = int(nxt[i]), seen + 1
        if i == 0:
            break
    assert seen == n                                   # a single cycle of the full length
    table = reference.host_link_chase_table(n, seed=7)
    assert table.shape == (n, 8) and table.dtype == np.uint64 and not table[:, 1:].any()
    host = torch.from_numpy(table.view(np.int64).reshape(-1).copy())
    walk = 0
    for _ in range(4096):
        walk = int(nxt[walk])
    assert reference.host_link_chase(host, 4096) == (walk, 0.0)
    assert reference.host_link_chase(host, n)[0] == 0           # once round the cycle
    assert reference.host_link_chase(host, 1, start=5)[0] == int(nxt[5])
    assert not np.array_equal(nxt, reference.host_link_chase_next(n, seed=8))


def test_model_runs_the_sequence_on_the_cpu_backend():
    rep = vj.host_link_check(torch.device("cpu"), 1 << 20, backend=reference)
    assert rep["ok"] and rep["bad_words"] == 0 and rep["chase_ok"] and rep["bytes"] == 1 << 20


# ------------------------------------------------------- the argument checks
def test_ops_refuse_what_is_not_a_pinned_16_byte_multiple():
    plain = torch.zeros(16, dtype=torch.int32)         # 64 bytes, not pinned
    for fn in (ops.host_link_push, ops.host_link_pull):
        with pytest.raises(ValueError, match="pinned"):
            fn(plain, 0)
        with pytest.raises(ValueError, match="% 16"):
            fn(torch.zeros(6, dtype=torch.int32), 0)   # 24 bytes
        with pytest.raises(ValueError, match="% 16"):
            fn(plain, 0, base=8)
        with pytest.raises(ValueError, match="unknown HBM pattern"):
            fn(plain, 2)
        with pytest.raises(ValueError, match="blocks"):
            fn(plain, 0, blocks=0)
    with pytest.raises(ValueError, match="pinned"):
        ops.host_link_chase(plain, 16)
    with pytest.raises(ValueError, match="% 64"):
        ops.host_link_chase(torch.zeros(12, dtype=torch.int32), 16)
    with pytest.raises(ValueError, match="pinned"):
        ops.host_link_push(np.zeros(16, dtype=np.int32), 0)


def test_hbm_pattern_ops_still_refuse_cpu_tensors():
    t = torch.zeros(16, dtype=torch.int32)
    with pytest.raises(ValueError, match="needs a GPU tensor"):
        ops.hbm_pattern_write(t, 0)
    with pytest.raises(ValueError, match="needs a GPU tensor"):
        ops.hbm_pattern_verify(t, 0)


# ------------------------------------------------- the plan header, sanitized
# (pattern, logical byte offset, seed, invert): offsets past 2^34 bytes reach the upper
# half of the 32-bit word index (HASH) and, past 2^35, of the 8-byte index (ADDR)
WORD_CASES = [(p, off, seed, inv)
              for p in (0, 1) for inv in (0, 1)
              for off in (0, 8, 4088, 2**34 + 16, 2**35 - 8, 2**35, 2**36 + 2**20 + 8, 2**40 + 24)
              for seed in (0, SEED)]

PLAN_MAIN = r"""
#include "ntm/host_link_plan.hpp"
using namespace ntm::hostlink;
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
struct Case { int pattern; uint64_t off, seed; int invert; uint64_t want; };
static const Case kCases[] = {
#include "cases.inc"
};
int main(int argc, char** argv) {
  REQUIRE(argc == 2);
  const std::string root = argv[1];
  for (const Case& c : kCases) REQUIRE(pattern_word(c.pattern, c.off, c.seed, c.invert != 0) == c.want);

  // the slow path: a buffer of pattern words with two of them changed
  std::vector<uint64_t> buf(512);
  const uint64_t base = (1ull << 34) + 4096;
  for (size_t i = 0; i < buf.size(); ++i) buf[i] = pattern_word(kPatternHash, base + 8 * i, 9, false);
  PatternResult r;
  REQUIRE(host_check(buf.data(), buf.size() * 8, base, kPatternHash, 9, false, r) == 0);
  REQUIRE(r.first_bad_offset == ~0ull && r.n_records == 0);
  buf[100] ^= 1ull << 45;
  buf[300] ^= 3;
  REQUIRE(host_check(buf.data(), buf.size() * 8, base, kPatternHash, 9, false, r) == 2);
  REQUIRE(r.first_bad_offset == base + 800 && r.bad_bits_or == ((1ull << 45) | 3) && r.n_records == 2);
  REQUIRE(r.records[0].offset == base + 800 && (r.records[0].expected ^ r.records[0].got) == 1ull << 45);
  REQUIRE(r.records[1].offset == base + 2400 && (r.records[1].expected ^ r.records[1].got) == 3);

  // the chase: one cycle of the full length whatever the seed, and the expected final index
  for (uint64_t seed : {0ull, 7ull, ~0ull}) {
    for (uint32_t n : {1u, 2u, 3u, 1000u, kChaseSlots}) {
      const std::vector<uint32_t> next = chase_permutation(n, seed);
      REQUIRE(next.size() == n);
      uint32_t i = 0, len = 0;
      do { REQUIRE(i < n); i = next[i]; ++len; } while (i != 0 && len <= n);
      REQUIRE(i == 0 && len == n);
      REQUIRE(chase_walk(next, 0, n) == 0);
      REQUIRE(chase_walk(next, 0, 1) == next[0]);
    }
  }
  const std::vector<uint32_t> next = chase_permutation(kChaseSlots, 7);
  std::vector<uint64_t> slots(kChaseSlots * (kChaseSlotBytes / 8), ~0ull);
  chase_fill(slots.data(), next);
  uint32_t at = 0;
  for (uint32_t h = 0; h < kChaseHops; ++h) {
    REQUIRE(slots[at * 8 + 1] == 0 && slots[at * 8 + 7] == 0);
    at = (uint32_t)slots[at * 8];
  }
  REQUIRE(at == chase_walk(next, 0, kChaseHops));
  std::printf("chase %u %u %u %u %u\n", next[0], next[1], next[511], next[1023], at);

  // sysfs: a full link, a link trained down, missing files
  const LinkState full = read_link_state(root, "0000:C1:00.0");   // upper case as HIP may print it
  REQUIRE(full.known() && full.speed_gts == 32.0 && full.width == 16 && full.max_speed_gts == 32.0);
  REQUIRE(full.max_width == 16 && full.numa_known && full.numa_node == 1);
  const LinkState down = read_link_state(root, "0000:05:00.0");
  REQUIRE(down.known() && down.speed_gts == 16.0 && down.width == 8 && down.max_width == 16);
  REQUIRE(down.numa_known && down.numa_node == -1);
  const LinkState part = read_link_state(root, "0000:06:00.0");   // only max_* present
  REQUIRE(!part.known() && part.max_speed_gts == 32.0 && part.max_width == 16 && !part.numa_known);
  REQUIRE(link_string(part).empty() && link_json(part) != "null");
  const LinkState none = read_link_state(root + "/nowhere", "0000:c1:00.0");
  REQUIRE(!none.known() && none.width == -1 && none.max_speed_gts < 0 && !none.numa_known);
  REQUIRE(link_string(none).empty() && link_json(none) == "null");
  std::printf("%s\n%s\n", link_json(full).c_str(), link_json(down).c_str());

  // the messages
  pattern_result_init(r);
  r.bad_words = 1;
  r.bad_bits_or = 0x2000;
  r.first_bad_offset = 0x4000008;
  r.n_records = 1;
  r.records[0] = {0x4000008, 0xAAAA00000000ull, 0xAAAA00002000ull};
  std::printf("%s\n", data_failure_message(3, kDirPull, r).c_str());
  r.bad_words = 2;                                                 // the first bad word won no slot
  r.bad_bits_or = ~0ull;
  r.first_bad_offset = (1ull << 40) + 8;
  r.n_records = 9;
  r.records[0] = {(1ull << 41), 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull};
  std::printf("%s\n", data_failure_message(15, kDirPush, r).c_str());
  r.bad_words = ~0ull;                                             // ... with every field at its widest
  r.first_bad_offset = ~0ull - 0xF7;
  r.records[0].offset = ~0ull - 0xEF;
  std::printf("%s\n", data_failure_message(15, kDirPush, r).c_str());
  r.records[1] = {r.first_bad_offset, 0x5555555555555555ull, 0xAAAAAAAAAAAAAAAAull};
  std::printf("%s\n", data_failure_message(15, kDirPush, r).c_str());
  std::printf("%s\n", rate_failure_message(3, "host->device", 13.14, 40, down).c_str());
  std::printf("%s\n", rate_failure_message(0, "device->host", 48.26, 50.5, none).c_str());
  return 0;
}
"""


def _fake_sysfs(root: Path) -> None:
    def dev(bus, **files):
        d = root / "bus" / "pci" / "devices" / bus
        d.mkdir(parents=True)
        for name, text in files.items():
            (d / name).write_text(text + "\n")

    dev("0000:c1:00.0", current_link_speed="32.0 GT/s PCIe", current_link_width="16",
        max_link_speed="32.0 GT/s PCIe", max_link_width="16", numa_node="1")
    dev("0000:05:00.0", current_link_speed="16.0 GT/s PCIe", current_link_width="8",
        max_link_speed="32.0 GT/s PCIe", max_link_width="16", numa_node="-1")
    dev("0000:06:00.0", max_link_speed="32.0 GT/s PCIe", max_link_width="16",
        current_link_speed="Unknown", current_link_width="0")


def test_plan_header_under_sanitizers(tmp_path):
    """Stand-alone program with its own main against host_link_plan.hpp, built with
    AddressSanitizer and UBSan (host code only; nothing is loaded into Python)."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "link_main.cpp", tmp_path / "link_main"
    src.write_text(PLAN_MAIN)
    lines = []
    for p, off, seed, inv in WORD_CASES:
        want = reference.hbm_pattern_words(8, p, seed, bool(inv), off).view(np.uint64)[0]
        lines.append(f"{{{p}, {off}ull, {seed}ull, {inv}, {int(want)}ull}},")
    (tmp_path / "cases.inc").write_text("\n".join(lines) + "\n")
    _fake_sysfs(tmp_path / "sys")
    inc = [f"-I{ROOT / 'validation' / 'include'}", f"-I{tmp_path}"]
    if cxx:
        # the sanitizer runtimes are linked statically, so the program does not depend on
        # what else the environment has the loader bring in, or in which order
        static = (["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx)
                  else ["-static-libsan"])
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *static, *inc, str(src), "-o", str(exe)]
    elif os.path.exists(hipcc):
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
               "-fsanitize=undefined", "-static-libsan", *inc, str(src), "-o", str(exe)]
    else:
        pytest.skip("no C++ compiler")
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([str(exe), str(tmp_path / "sys")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout + p.stderr
    chase, full, down, pull, other, push, first, slow, slow_unknown = p.stdout.strip().splitlines()
    # the header's permutation is the one ops.reference builds
    nxt = reference.host_link_chase_next(1024, seed=7)
    table = torch.from_numpy(reference.host_link_chase_table(1024, 7).view(np.int64).reshape(-1).copy())
    assert [int(x) for x in chase.split()[1:]] == [
        int(nxt[0]), int(nxt[1]), int(nxt[511]), int(nxt[1023]), reference.host_link_chase(table, 4096)[0]]
    assert full == '{"speed_gts":32.0,"width":16,"max_speed_gts":32.0,"max_width":16,"numa_node":1}'
    assert down == '{"speed_gts":16.0,"width":8,"max_speed_gts":32.0,"max_width":16,"numa_node":-1}'
    assert pull == ("gpu3: host link host->device read: 1 bad word(s), at byte 0x4000008: "
                    "expected 0x0000aaaa00000000, got 0x0000aaaa00002000, bad bits 0x2000")
    # every field at its widest: another word's record is left out to stay under 200
    assert push == ("gpu15: host link device->host write or host memory: 18446744073709551615 bad "
                    "word(s), at byte 0xffffffffffffff08, bad bits 0xffffffffffffffff")
    assert other == ("gpu15: host link device->host write or host memory: 2 bad word(s), at byte "
                     "0x10000000008; at 0x20000000000: expected 0x5555555555555555, got "
                     "0xaaaaaaaaaaaaaaaa, bad bits 0xffffffffffffffff")
    assert first == ("gpu15: host link device->host write or host memory: 18446744073709551615 bad "
                     "word(s), at byte 0xffffffffffffff08: expected 0x5555555555555555, got "
                     "0xaaaaaaaaaaaaaaaa, bad bits 0xffffffffffffffff")
    assert slow == ("gpu3: host link 13.1 GB/s host->device below floor 40 "
                    "(PCIe 16.0 GT/s x8, max 32.0 GT/s x16)")
    assert slow_unknown == "gpu0: host link 48.3 GB/s device->host below floor 50.5"
    for line in (pull, other, push, first, slow, slow_unknown):
        assert len(line) < 200 and "\n" not in line


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


# local.validation_args at the variables' defaults before validation_host_link_mib existed
# (the list pinned in tests/test_hbm_pattern_cpu.py and tests/test_cu_sweep_cpu.py)
PARENT_DEFAULT_ARGS = [
    "--gpus", "8", "--size", "8192", "--tflops-floor", "1000", "--min-hbm-gb", "250",
    "--allreduce-max-mib", "1024", "--json", "--fp8-tflops-floor", "2000",
    "--xgmi-tune", "--require-host-prep", "--termination-log", "/dev/termination-log"]


def test_job_args_carry_the_host_link_check_only_when_asked():
    args = _stack_local("validation_args")
    assert not [a for a in args if "host-link" in a] and args == PARENT_DEFAULT_ARGS
    on = _stack_local("validation_args", validation_host_link_mib=256)
    i = on.index("--host-link-mib")
    assert on[i + 1] == "256" and i < on.index("--termination-log")
    assert "--host-link-floor-gbps" not in on
    assert [a for j, a in enumerate(on) if j not in (i, i + 1)] == PARENT_DEFAULT_ARGS
    both = _stack_local("validation_args", validation_host_link_mib=256,
                        validation_host_link_floor_gbps=40)
    j = both.index("--host-link-floor-gbps")
    assert both[j + 1] == "40" and both.index("--host-link-mib") < j < both.index("--termination-log")
    # the floor alone asks for nothing
    assert _stack_local("validation_args", validation_host_link_floor_gbps=40) == PARENT_DEFAULT_ARGS


def _stack_plan(tmp_path, **kv):
    from nvidia_terraform_modules_amd.tfcheck.plan import plan

    args = "\n".join(f"  {k} = {v!r}" for k, v in kv.items())
    src = os.path.relpath(STACK_DIR, tmp_path)
    (tmp_path / "main.tf").write_text(
        f'module "stack" {{\n  source = "{src}"\n  cluster_name = "c"\n{args}\n}}\n')
    return plan(tmp_path)


@pytest.mark.parametrize("name", ["validation_host_link_mib", "validation_host_link_floor_gbps"])
def test_negative_host_link_values_are_rejected(tmp_path, name):
    bad = _stack_plan(tmp_path, **{name: -1})
    assert any(f"{name} must be >= 0" in e for e in bad.errors), bad.errors
    ok = _stack_plan(tmp_path, validation_host_link_mib=256, validation_host_link_floor_gbps=40)
    assert not [e for e in ok.errors if "host_link" in e], ok.errors
    assert not [e for e in ok.errors + ok.warnings if "no such variable" in e]
    desc = (STACK_DIR / "variables.tf").read_text().split(f'variable "{name}"')[1]
    assert "profiles/host_link/README.md" in desc.split("validation {")[0]
