"""K9 without a GPU: ``atomics_plan.hpp`` against a numpy mirror through a stand-alone
sanitized program (the k -> slot / operand map, the expected tables of every op, the
exactness bounds), the verdicts of ``ops.atomics_summarize`` on synthetic tables, tickets
and hand-off records, ``AtomicsResult`` in the report writers, the module variable and the
binary's refusal of an injection without the switch."""
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
INC = ROOT / "validation" / "include"
OPS = ("add_u32", "add_u64", "and_u32", "or_u32", "xor_u32", "min_i32", "max_i32", "max_u64",
       "cas_u32", "add_f32", "add_f64", "add_bf16x2", "add_f16x2")
MAGIC = 0x4B394154
SLOTS, TOTAL, SEED = 64, 4096, 0x5EED
MAX_ABS = {"add_f32": 255, "add_f64": 1000003, "add_bf16x2": 7, "add_f16x2": 63}   # 64 adds per slot, 32 per cell
M64 = (1 << 64) - 1


# ------------------------------------------------------------ the numpy mirror
def hash64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15))
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def op_hash(k, seed):
    return hash64(np.uint64(seed * 0x100000001B3 & M64) ^ hash64(k))


def float_operand(k, seed, max_abs):
    return (op_hash(k, seed) % np.uint64(2 * max_abs + 1)).astype(np.int64) - max_abs


def half_bits(v, dtype_bits):
    """bits of small integers in bf16 (via float32) or fp16"""
    if dtype_bits == "bf16":
        return (v.astype(np.float32).view(np.uint32) >> 16).astype(np.uint64)
    return v.astype(np.float16).view(np.uint16).astype(np.uint64)


def mirror_table(op, slots=SLOTS, total=TOTAL, seed=SEED, max_abs=1):
    with np.errstate(over="ignore"):
        k = np.arange(total, dtype=np.uint64).reshape(-1, slots)      # column s: k = s, s + slots, ...
        h = op_hash(k, seed)
        lo = h & np.uint64(0xFFFFFFFF)
        bit = (h >> np.uint64(8)) & np.uint64(31)
        idle = ((h >> np.uint64(13)) & np.uint64(7)) != 0          # seven operations in eight change no bit
        if op == "add_u32":
            return (lo.sum(axis=0) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        if op == "add_u64":
            return h.sum(axis=0, dtype=np.uint64)
        if op == "and_u32":
            return np.bitwise_and.reduce(np.where(idle, np.uint32(0xFFFFFFFF), ~(np.uint32(1) << bit.astype(np.uint32))), axis=0)
        if op == "or_u32":
            return np.bitwise_or.reduce(np.where(idle, np.uint32(0), np.uint32(1) << bit.astype(np.uint32)), axis=0)
        if op == "xor_u32":
            return np.bitwise_xor.reduce(lo.astype(np.uint32), axis=0)
        if op in ("min_i32", "max_i32"):
            s = lo.astype(np.uint32).view(np.int32)
            return (s.min(axis=0) if op == "min_i32" else s.max(axis=0)).view(np.uint32)
        if op == "max_u64":
            return h.max(axis=0)
        if op == "cas_u32":
            return (np.uint64(1) << np.uint64(32)) | (np.arange(slots, dtype=np.uint64) + np.uint64(1))
        v = float_operand(k, seed, max_abs)
        if op == "add_f32":
            return v.sum(axis=0).astype(np.float32).view(np.uint32)
        if op == "add_f64":
            return v.sum(axis=0).astype(np.float64).view(np.uint64)
        kind = "bf16" if op == "add_bf16x2" else "f16"
        cell0, cell1 = v[0::2].sum(axis=0), v[1::2].sum(axis=0)       # op k adds to cell (k / slots) & 1
        return (half_bits(cell0, kind) | (half_bits(cell1, kind) << np.uint64(16))).astype(np.uint32)


def mirror_operand_bits(op, k, slots=SLOTS, seed=SEED, max_abs=1):
    with np.errstate(over="ignore"):
        k = np.asarray(k, dtype=np.uint64)
        h = op_hash(k, seed)
        bit = ((h >> np.uint64(8)) & np.uint64(31)).astype(np.uint32)
        idle = ((h >> np.uint64(13)) & np.uint64(7)) != 0
        if op in ("add_u32", "xor_u32", "min_i32", "max_i32"):
            return h & np.uint64(0xFFFFFFFF)
        if op in ("add_u64", "max_u64"):
            return h
        if op == "and_u32":
            return np.where(idle, np.uint32(0xFFFFFFFF), ~(np.uint32(1) << bit)).astype(np.uint64)
        if op == "or_u32":
            return np.where(idle, np.uint32(0), np.uint32(1) << bit).astype(np.uint64)
        if op == "cas_u32":
            return (k + np.uint64(1)) & np.uint64(0xFFFFFFFF)
        v = float_operand(k, seed, max_abs)
        if op == "add_f32":
            return v.astype(np.float32).view(np.uint32).astype(np.uint64)
        if op == "add_f64":
            return v.astype(np.float64).view(np.uint64)
        b = half_bits(v, "bf16" if op == "add_bf16x2" else "f16")
        return np.where((k // np.uint64(slots)) & np.uint64(1), b << np.uint64(16), b)


# ------------------------------------------------------------ stand-alone sanitized programs
def build_sanitized(tmp_path, name, source, extra_inc=()):
    """Compile `source` (with its own main) with AddressSanitizer and UBSan and return the
    program's path: host code only, nothing is loaded into Python."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / f"{name}.cpp", tmp_path / name
    src.write_text(source)
    inc = [f"-I{INC}", *[f"-I{p}" for p in extra_inc]]
    if cxx:
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
    return exe


PLAN_MAIN = r"""
#include "ntm/atomics_plan.hpp"
#include <cstdio>
using namespace ntm::atm;
int main(int argc, char** argv) {
  static_assert(sizeof(Record) == 96 && kSlabWords == 256, "layout");
  const unsigned long long max_abs[kOps] = {1, 1, 1, 1, 1, 1, 1, 1, 1, 255, 1000003, 7, 63};
  for (int op = 0; op < kOps; ++op) {
    std::printf("%s %u", op_name(op), slot_bytes(op));
    for (uint64_t s = 0; s < 64; ++s)
      std::printf(" %llx", (unsigned long long)expected_slot(op, s, 64, 4096, 0x5EED, max_abs[op]));
    std::printf("\n%s", op_name(op));
    for (uint64_t k = 4000; k < 4010; ++k)
      std::printf(" %llu:%llx", (unsigned long long)slot_of(k, 64),
                  (unsigned long long)operand_bits(op, k, 0x5EED, max_abs[op], 64));
    std::printf("\n");
  }
  // the bounds, at and just past each
  struct { int op; uint64_t adds, max_abs; bool ok; } b[] = {
      {kAddF32, 256, 65535, true}, {kAddF32, 256, 65536, false}, {kAddF32, (1u << 24) - 1, 1, true}, {kAddF32, 1u << 24, 1, false},
      {kAddF64, 256, (1ull << 45) - 1, true}, {kAddF64, 256, 1ull << 45, false}, {kAddF64, ~0ull, ~0ull, false},
      {kAddBf16x2, 510, 1, true}, {kAddBf16x2, 511, 1, false}, {kAddBf16x2, 2, 255, true}, {kAddBf16x2, 2, 256, false},
      {kAddF16x2, 4094, 1, true}, {kAddF16x2, 4095, 1, false}, {kAddF16x2, 178, 23, true}, {kAddF16x2, 179, 23, false},
      {kAddU32, ~0ull, ~0ull, true}, {kCasU32, 5, 0, true}, {kAddF32, 4, 0, false}, {kOps, 1, 1, false}, {-1, 1, 1, false}};
  for (auto& c : b)
    if (atomics_exact(c.op, c.adds, c.max_abs) != c.ok) return 1 + (int)(&c - b);
  if (!rmw_shape_ok(kAddF32, 64, 16, 4, 65535) || rmw_shape_ok(kAddF32, 64, 16, 4, 65536) || rmw_shape_ok(kAddU32, 60, 16, 4, 1) ||
      rmw_shape_ok(kAddBf16x2, 64, 16, 4, 2) || !rmw_shape_ok(kAddBf16x2, 256, 255, 2, 1) || !rmw_shape_ok(kAddF16x2, 128, 89, 1, 23))
    return 40;
  if (f16_bits_of_int(1) != 0x3C00 || f16_bits_of_int(-2047) != 0xE7FF || f16_bits_of_int(2048) != 0x6800 ||
      bf16_bits_of_int(255) != 0x437F || bf16_bits_of_int(-1) != 0xBF80 || cas_canonical(65 + 1, 1, 64, 4096) != 2 ||
      cas_canonical(66 + 1, 1, 64, 4096) != 67 || cas_canonical(0, 1, 64, 4096) != 0 || cas_canonical(4097 + 64, 0, 64, 4096) != 4161)
    return 41;
  if (ticket_head(5, 2, 4) != 3 || tickets_per_head(2, 16, 4) != 8192 || !ticket_shape_ok(2, 16, 4) || ticket_shape_ok(3, 16, 4) ||
      !handoff_shape_ok(4, 8) || handoff_shape_ok(4, 1) || handoff_shape_ok(4, 65) || handoff_slab_bytes(4, 8) != 131072 ||
      round_seed(9, 3) == round_seed(9, 2) || sleep_count(7, 1, 2) > 7)
    return 42;
  (void)argc, (void)argv;
  return 0;
}
"""


@pytest.fixture(scope="module")
def plan_output(tmp_path_factory):
    exe = build_sanitized(tmp_path_factory.mktemp("atomics_plan"), "atomics_plan_main", PLAN_MAIN)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, f"exit {p.returncode}\n{p.stdout[-400:]}{p.stderr[-2000:]}"
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 2 * len(OPS)
    return {lines[2 * i].split()[0]: (lines[2 * i].split()[1:], lines[2 * i + 1].split()[1:]) for i in range(len(OPS))}


@pytest.mark.parametrize("op", OPS)
def test_plan_header_matches_the_numpy_mirror(plan_output, op):
    table, operands = plan_output[op]
    wide = op in ("add_u64", "max_u64", "cas_u32", "add_f64")
    assert int(table[0]) == (8 if wide else 4)
    want = mirror_table(op, max_abs=MAX_ABS.get(op, 1))
    assert [int(x, 16) for x in table[1:]] == [int(x) for x in want]
    ks = np.arange(4000, 4010, dtype=np.uint64)
    bits = mirror_operand_bits(op, ks, max_abs=MAX_ABS.get(op, 1))
    assert operands == [f"{int(k) % SLOTS}:{int(b):x}" for k, b in zip(ks, bits)]


def test_float_tables_are_not_trivial():
    for op in ("add_f32", "add_f64", "add_bf16x2", "add_f16x2"):
        t = mirror_table(op, max_abs=MAX_ABS[op])
        assert len(set(t.tolist())) > SLOTS // 2, op


# ------------------------------------------------------------ the verdicts (host code of the library)
@pytest.fixture(scope="module")
def ops():
    from nvidia_terraform_modules_amd import ops as o
    from nvidia_terraform_modules_amd.ops._lib import NativeLibraryMissing, lib
    try:
        lib()
    except NativeLibraryMissing:
        pytest.skip("libntm_validation.so not built (python -m nvidia_terraform_modules_amd.ops.build)")
    return o


def test_op_list_and_host_tables_match_the_mirror(ops):
    from nvidia_terraform_modules_amd.ops._lib import lib
    assert ops.ATOMIC_OPS == OPS and lib().ntm_atomics_ops() == len(OPS)
    assert [lib().ntm_atomics_op_name(i).decode() for i in range(len(OPS))] == list(OPS)
    assert lib().ntm_atomics_record_bytes() == ops.atomics_record_dtype().itemsize == 96
    for op in OPS:
        got = ops.atomics_rmw_expected(op, SLOTS, TOTAL, SEED, MAX_ABS.get(op, 1))
        assert (got == mirror_table(op, max_abs=MAX_ABS.get(op, 1))).all(), op


def test_exact_bounds_through_python(ops):
    assert ops.atomics_exact("add_f32", 256, 65535) and not ops.atomics_exact("add_f32", 256, 65536)
    assert ops.atomics_exact("add_f64", 256, 2**45 - 1) and not ops.atomics_exact("add_f64", 256, 2**45)
    assert ops.atomics_exact("add_bf16x2", 510, 1) and not ops.atomics_exact("add_bf16x2", 511, 1)
    assert ops.atomics_exact("add_f16x2", 4094, 1) and not ops.atomics_exact("add_f16x2", 4095, 1)
    assert ops.atomics_exact("xor_u32", 10**12, 10**12)


def test_rmw_clean_and_one_wrong_slot(ops):
    exp = ops.atomics_rmw_expected("add_f32", SLOTS, TOTAL, SEED, 255)
    s = ops.atomics_summarize("rmw", 2, op="add_f32", got=exp, expected=exp)
    assert s["ok"] and s["message"] == "" and s["bad_slots"] == 0 and s["first"] is None
    got = exp.copy()
    got[37] ^= 1 << 9
    s = ops.atomics_summarize("rmw", 2, op="add_f32", got=got, expected=exp)
    assert not s["ok"] and s["bad_slots"] == 1 and s["first"]["slot"] == 37
    assert s["message"] == (f"gpu2: atomics: add_f32 slot 37: expected {int(exp[37]):#x}, got {int(got[37]):#x}, "
                            "bad bits 0x200")
    wide = ops.atomics_rmw_expected("max_u64", SLOTS, TOTAL, SEED)
    bad = wide.copy()
    bad[:20] ^= np.uint64(1 << 63)
    s = ops.atomics_summarize("rmw", 0, op="max_u64", got=bad, expected=wide)
    assert s["bad_slots"] == 20 and len(s["failures"]) == 8 and all(len(f) < 200 for f in s["failures"])


def clean_tickets(heads=2, grid=16, iters=4):
    per = grid * 256 // heads * iters
    claim = np.zeros((heads, per), dtype=np.uint32)
    for h in range(heads):
        gids = [g for it in range(iters) for g in range(grid * 256) if (g + it) % heads == h]
        claim[h] = gids
    counters = np.zeros(heads * 32, dtype=np.uint32)
    counters[::32] = per
    return dict(counters=counters, claim=claim, grid=grid, iters=iters)


def test_tickets_clean_missing_duplicate_and_short(ops):
    t = clean_tickets()
    s = ops.atomics_summarize("tickets", 1, **t)
    assert s["ok"] and s["bad"] == 0
    miss = clean_tickets()
    miss["claim"][1, 77] = 0xFFFFFFFF
    s = ops.atomics_summarize("tickets", 1, **miss)
    assert not s["ok"] and s["missing"] == 1 and s["duplicate"] == 0
    assert s["message"] == "gpu1: atomics: ticket: head 1 ticket 77 missing: nobody wrote the entry"
    dup = clean_tickets()
    owner, other = int(dup["claim"][0, 100]), int(dup["claim"][0, 4000])
    dup["claim"][0, 4000] = owner                       # `owner` holds a fifth entry, `other` only three
    s = ops.atomics_summarize("tickets", 1, **dup)
    assert not s["ok"] and s["duplicate"] == 1 and s["missing"] == 0 and owner != other
    assert s["message"].startswith("gpu1: atomics: ticket: head ") and " duplicate: thread " in s["message"]
    assert f"thread {owner} holds 5 entries, expected 4" in s["message"]
    short = clean_tickets()
    short["counters"][32] -= 1
    s = ops.atomics_summarize("tickets", 1, **short)
    assert not s["ok"] and s["short_counters"] == 1
    assert s["message"] == "gpu1: atomics: ticket: head 1 counter short: 8191, expected 8192"
    bad = clean_tickets()
    bad["claim"][0, 5] = 16 * 256
    assert ops.atomics_summarize("tickets", 1, **bad)["invalid"] == 1


def make_records(ops, episodes=4, e=8, xcds=8, spread=True):
    """One clean launch: workgroup w sits on XCD w % xcds (or all on XCD 0), the last of each
    episode is the reader and saw every writer's XCD."""
    rec = np.zeros(episodes * e, dtype=ops.atomics_record_dtype())
    for w in range(len(rec)):
        x = w % xcds if spread else 0
        rec[w]["magic"], rec[w]["wg"], rec[w]["episode"] = MAGIC, w, w // e
        rec[w]["xcc_id"], rec[w]["hw_id"] = x, (w % 4) << 13 | (w % 8) << 8
        if w % e == e - 1:
            rec[w]["episodes_read"], rec[w]["words_checked"] = 1, e * 256
            rec[w]["writer_mask"] = sum({1 << ((w - j) % xcds if spread else 0) for j in range(e)})
    return rec


def summarize(ops, rec, episodes=4, e=8, xcds=8, launches=1, gpu=0):
    return ops.atomics_summarize("handoff", gpu, records=rec, episodes=episodes, episode_size=e, xcds=xcds,
                                 launches=launches)


def test_handoff_clean_counts_pairs(ops):
    s = summarize(ops, make_records(ops))
    assert s["ok"] and s["readers"] == 4 and s["words_checked"] == s["expected_words"] == 4 * 8 * 256
    assert s["xcd_pairs_covered"] == 8 and s["cross_xcd_pairs"] == 7        # every writer XCD -> reader XCD 7
    assert [row[7] for row in s["pairs"]] == [1] * 8
    two = np.concatenate([make_records(ops), make_records(ops)])
    assert summarize(ops, two, launches=2)["ok"]


@pytest.mark.parametrize("cls,name", [(1, "stale"), (2, "corrupt")])
def test_handoff_bad_word_is_classified_and_named(ops, cls, name):
    rec = make_records(ops)
    r = rec[15]
    r["bad_words"], r["stale_words"], r["first_class"] = 4, 4 if cls == 1 else 0, cls
    r["writer_hw"], r["writer_xcc"], r["writer_wg"], r["first_off"] = 3 << 8, 2, 10, 2 * 4096 + 256
    r["expected"], r["got"] = 0xAAAA, 0xBBBB
    s = summarize(ops, rec, gpu=3)
    assert not s["ok"] and s["bad_words"] == 4 and s["stale_words"] == (4 if cls == 1 else 0)
    assert s["message"] == (f"gpu3: atomics: handoff: {name} word: reader xcd 7 se 3 cu 7, writer xcd 2 cu 3 "
                            f"(workgroup 10), episode 1, offset 0x2100, expected 0xaaaa, got 0xbbbb; 4 bad, "
                            f"{4 if cls == 1 else 0} stale")


def test_handoff_conservation(ops):
    two = make_records(ops)
    two[9]["episodes_read"], two[9]["words_checked"] = 1, 8 * 256
    s = summarize(ops, two)
    assert not s["ok"] and "gpu0: atomics: handoff: episode 1 had 2 readers, expected 1" in s["failures"]
    assert any("words checked, expected 8192" in f for f in s["failures"])
    none = make_records(ops)
    none[23]["episodes_read"], none[23]["words_checked"] = 0, 0
    s = summarize(ops, none)
    assert not s["ok"] and s["failures"][0] == "gpu0: atomics: handoff: episode 2 had 0 readers, expected 1"
    blank = make_records(ops)
    blank[3]["magic"] = 0
    assert "1 of 32 workgroups wrote no record" in summarize(ops, blank)["message"]


def test_handoff_no_cross_xcd_pair_fails_only_with_several_xcds(ops):
    rec = make_records(ops, spread=False)
    s = summarize(ops, rec, xcds=8)
    assert not s["ok"] and s["cross_xcd_pairs"] == 0 and s["xcd_pairs_covered"] == 1
    assert s["message"] == "gpu0: atomics: handoff: no cross-XCD pair was checked on 8 XCDs: the run proved nothing"
    assert summarize(ops, rec, xcds=1)["ok"]


# ------------------------------------------------------------ the report writers
REPORT_MAIN = r"""
#include "report.hpp"
#include <iostream>
using namespace ntm::job;
int main(int argc, char**) {
  Report R;
  R.gpus.resize(2);
  for (int i = 0; i < 2; ++i) {
    GpuResult& g = R.gpus[i];
    g.device = i, g.name = "gpu", g.arch = "gfx950", g.k1.bad = 0, g.k1.abft_bad_acc = 0, g.k1.abft_bad_store = 0;
    g.k2.copy_ok = true;
    if (argc > 1) continue;  // any argument: the check did not run
    g.atomics.ran = true;
    for (int op = 0; op < ntm::atm::kOps; ++op) g.atomics.ops.push_back({op, op == 9 && i == 1 ? 1ull : 0ull, 1.5 + op});
    g.atomics.xcds = 2, g.atomics.pairs.assign(256, 0), g.atomics.pairs[1] = 1, g.atomics.xcd_pairs_covered = 1;
    g.atomics.episodes_per_s = 1e6, g.atomics.seconds = 0.05;
    if (i == 1) g.atomics.failures.push_back("gpu1: atomics: add_f32 slot 3: expected 0x1, got 0x3, bad bits 0x2");
  }
  R.o.atomics_check = argc == 1;
  R.o.fp8 = false;
  for (auto& g : R.gpus)
    for (auto& f : gpu_failures(g, R.o)) R.failures.push_back(f);
  std::cout << report_json(R) << "\n" << prometheus_text(R);
  return 0;
}
"""


@pytest.fixture(scope="module")
def report_exe(tmp_path_factory):
    return build_sanitized(tmp_path_factory.mktemp("atomics_report"), "atomics_report_main", REPORT_MAIN,
                           extra_inc=[ROOT / "validation" / "src" / "validate"])


def test_report_with_the_check_ran(report_exe):
    p = subprocess.run([str(report_exe)], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    first, prom = p.stdout.split("\n", 1)
    rep = json.loads(first)
    g0, g1 = rep["gpus"]
    assert g0["atomics_ops"] == list(OPS) and g1["atomics_add_f32_bad"] == 1 and g0["atomics_add_f32_bad"] == 0
    for op in OPS:
        assert g0[f"atomics_{op}_gops"] > 0
    for key in ("atomics_ticket_bad", "atomics_handoff_bad_words", "atomics_handoff_stale_words",
                "atomics_handoff_episodes_per_s", "atomics_xcd_pairs_covered", "atomics_seconds"):
        assert key in g0, key
    assert g0["atomics_xcd_pairs"] == [[0, 1], [0, 0]]
    assert rep["passed"] is False and rep["failures"] == ["gpu1: atomics: add_f32 slot 3: expected 0x1, got 0x3, bad bits 0x2"]
    types = [ln.split()[2] for ln in prom.splitlines() if ln.startswith("# TYPE ")]
    assert len(types) == len(set(types)), "a gauge is typed twice"
    atom = [t for t in types if t.startswith("amdgpu_validate_atomics_")]
    assert len(atom) == 8 and 'amdgpu_validate_atomics_gops{gpu="1",op="add_f16x2"} 13.5' in prom


def test_report_without_the_check_has_no_key(report_exe):
    p = subprocess.run([str(report_exe), "off"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "atomics" not in p.stdout and json.loads(p.stdout.split("\n", 1)[0])["passed"] is True


# ------------------------------------------------------------ the module
def _stack_local(name, **overrides):
    from nvidia_terraform_modules_amd.tfcheck.config import load_module
    from nvidia_terraform_modules_amd.tfcheck.evaluate import Evaluator, Scope, convert

    mod = load_module(STACK_DIR)
    ev = Evaluator()
    variables = {}
    for vn, v in mod.variables.items():
        if vn in overrides:
            variables[vn] = overrides[vn]
        elif not v.required:
            variables[vn] = convert(ev.eval(v.block.body.attr("default"), Scope({}, {})), v.type_expr)
    scope = Scope(variables, {n: e for n, (e, _, _) in mod.locals.items()}, str(mod.path))
    return ev.eval(mod.locals[name][0], scope)


def test_module_sets_the_variable_only_when_asked():
    off, on = _stack_local("validation_env"), _stack_local("validation_env", validation_atomics_check=True)
    assert "NTM_ATOMICS_CHECK" not in off and on["NTM_ATOMICS_CHECK"] == "1"
    assert {k: v for k, v in on.items() if k != "NTM_ATOMICS_CHECK"} == off
    args = _stack_local("validation_args")
    assert _stack_local("validation_args", validation_atomics_check=True) == args
    assert not [a for a in args if "atomics" in a]
    text = (STACK_DIR / "variables.tf").read_text()
    block = text.split('variable "validation_atomics_check"')[1].split("\n}")[0]
    assert "bool" in block and "false" in block and "profiles/atomics/README.md" in block


# ------------------------------------------------------------ the binary
@pytest.mark.parametrize("kind", ["stale_handoff", "corrupt_atomic"])
def test_injection_without_the_switch_is_refused(kind):
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = {k: v for k, v in os.environ.items() if k not in ("NTM_FAULT_INJECT", "NTM_ATOMICS_CHECK")}
    p = subprocess.run([str(BIN), "--gpus", "1", "--fault-inject", kind], capture_output=True, text=True,
                       timeout=60, env=e)
    assert p.returncode == 2 and f"fault-inject {kind} needs NTM_ATOMICS_CHECK=1" in p.stderr
    assert p.stdout == ""
