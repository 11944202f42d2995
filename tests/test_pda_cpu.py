"""K14 without a GPU: the numpy side of the paged-KV decode attention check (``ops.pda``) - the split
plan, the page-table generator, scatter and gather, the float32 twin of the split arithmetic and
its merge against the reference on exact inputs - and the plan header in a sanitized stand-alone
program that the numpy twin is held to."""
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest

from nvidia_terraform_modules_amd.ops import attn as A
from nvidia_terraform_modules_amd.ops import pda as P

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "validation" / "include"

# (Hq, Hkv, T, lens, S): the shapes of tests/test_pda_gpu.py
SHAPES = [(8, 2, 1, [257, 1], 4), (4, 1, 4, [191], 1), (32, 1, 1, [300], 2), (2, 2, 1, [64, 1000], 3),
          (32, 8, 4, [5, 130], 2), (16, 2, 1, [2048], 8)]


def _u32(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@pytest.mark.parametrize("length", [1, 63, 64, 65, 257, 1000, 2048, 65536])
@pytest.mark.parametrize("S", [1, 2, 3, 4, 7, 8, 64])
def test_split_ranges_tile_the_steps_and_empty_splits_appear_only_on_overshoot(length, S):
    steps = P.pda_key_steps(length)
    per = -(-steps // S)
    ranges = [P.pda_split_range(length, s, S) for s in range(S)]
    walked = [st for b, e in ranges for st in range(b, e)]
    assert walked == list(range(steps))                        # tiles [0, steps): no gap, no overlap
    empty = [s for s, (b, e) in enumerate(ranges) if b >= e]
    assert bool(empty) == (S * per - steps >= per)              # exactly when S * per overshoots by a whole split
    assert empty == list(range(S - len(empty), S))              # and they are the last ones
    for s, (b, e) in enumerate(ranges):                         # the waves of a split tile its range
        by_wave = sorted(st for w in range(P.PDA_WAVES) for st in P.pda_wave_steps(length, s, S, w))
        assert by_wave == list(range(b, e))


def test_default_splits_at_pinned_points():
    assert P.pda_splits(32, 8, 8192, 256) == 2      # the Job's timed shape: 256 (b, kv head) pairs, 2 per CU at S 2
    assert P.pda_splits(1, 8, 8192, 256) == 32      # capped by 4 steps per split: 128 steps / 4
    assert P.pda_splits(1, 1, 65536, 256) == 64     # capped by kMaxSplits
    assert P.pda_splits(4, 8, 255, 256) == 1        # 4 steps: one split
    assert P.pda_splits(4, 8, 512, 256) == 2        # 8 steps
    assert P.pda_splits(1024, 8, 8192, 256) == 1    # the grid is large enough already
    assert P.pda_splits(1, 1, 1, 1) == 1


def test_scatter_then_gather_is_the_identity_and_poison_is_never_referenced_below_len():
    lens = [257, 1, 64, 1000, 16, 17]
    pt = P.pda_make_page_table(lens, seed=5, shared_pairs=0)
    assert pt["pages"] == sum(P.pda_pages_of(n) for n in lens) + 1 and pt["max_pages"] == 63
    used = np.concatenate([pt["table"][b, :P.pda_pages_of(n)] for b, n in enumerate(lens)])
    assert len(set(used.tolist())) == len(used) and pt["poison"] not in used        # a permutation, poison apart
    assert ((pt["table"] >= 0) & (pt["table"] < pt["pages"])).all()
    for b, n in enumerate(lens):
        assert (pt["table"][b, P.pda_pages_of(n):] == pt["poison"]).all()
    assert (np.diff(pt["table"][3, :63]) != 1).mean() > 0.9                          # shuffled: neighbours are not adjacent
    rng = np.random.default_rng(0)
    pool = np.full((pt["pages"], 2, 16, 128), 0x7FC0, dtype=np.uint16)
    src = [rng.integers(0, 0x7F00, (2, n, 128)).astype(np.uint16) for n in lens]
    for b in range(len(lens)):
        P.pda_scatter_to_pages(pt, b, src[b], pool)
    for b in range(len(lens)):
        assert (P.pda_gather_from_pages(pt, b, pool) == src[b]).all()
    assert (pool[pt["poison"]] == 0x7FC0).all()
    # prefix sharing: sequence 1 reads sequence 0's first pages, sequence 3 those of sequence 2
    sh = P.pda_make_page_table([257, 130, 64, 1000], seed=5, shared_pairs=2)
    assert (sh["table"][1, :4] == sh["table"][0, :4]).all() and sh["table"][1, 4] != sh["table"][0, 4]
    assert (sh["table"][3, :2] == sh["table"][2, :2]).all() and sh["table"][3, 2] != sh["table"][2, 2]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s[:3])) + "_" + "_".join(map(str, s[3])))
def test_every_gpu_shape_passes_the_exact_predicate_per_sequence(shape):
    Hq, Hkv, T, lens, S = shape
    pr = P.pda_make_problem("exact", Hq, Hkv, T, lens, seed=0x14 + sum(lens), shared_pairs=0)
    assert P.pda_exact(pr)
    assert pr["k_pool"][pr["pt"]["poison"]].min() == 0x7FC0     # NaN poison page
    n = lens[0]
    if n % 16:                                                  # NaN page tail past len
        last = pr["block_table"][0, (n - 1) // 16]
        assert (pr["v_pool"][last, :, n % 16:] == 0x7FC0).all() and (pr["v_pool"][last, :, :n % 16] != 0x7FC0).all()


@pytest.mark.parametrize("shape", [(8, 2, 1, [257, 1], 4), (4, 1, 4, [191], 1), (2, 2, 1, [64, 1000], 3),
                                   (32, 8, 4, [5, 130], 2), (8, 2, 2, [200, 150], 3)],
                         ids=lambda s: "x".join(map(str, s[:3])) + "_" + "_".join(map(str, s[3])) + "_S" + str(s[4]))
def test_float32_twin_of_the_merge_equals_the_reference_bitwise_on_exact_inputs(shape):
    Hq, Hkv, T, lens, S = shape
    shared = 1 if len(lens) > 1 and min(lens) >= 64 else 0
    pr = P.pda_make_problem("exact", Hq, Hkv, T, lens, seed=0x14 + sum(lens), shared_pairs=shared)
    assert P.pda_exact(pr)
    got, ref = P.pda_emulate(pr, S), P.pda_reference_f32(pr)
    assert (got["o"] == ref["o"]).all()
    assert (_u32(got["m"]) == _u32(ref["m"])).all() and (_u32(got["l"]) == _u32(ref["l"])).all()
    assert np.isfinite(ref["m"]).all() and (ref["l"] > 0).all()
    one = P.pda_emulate(pr, 1)                                  # and the number of splits does not matter
    assert (one["o"] == got["o"]).all() and (_u32(one["l"]) == _u32(got["l"])).all()
    if shared:                                                  # the shared prefix really is the same keys
        n = min(lens) // 16 // 2 * 16
        assert n and (pr["seqs"][0]["k"][:, :, :n] == pr["seqs"][1]["k"][:, :, :n]).all()


def test_twin_on_dense_inputs_is_within_the_tolerance_and_nan_never_leaks():
    pr = P.pda_make_problem("dense", 8, 2, 1, [320, 77, 513], seed=3)
    got, ref = P.pda_emulate(pr, 3), P.pda_reference_f32(pr)
    assert not np.isnan(A.bf16_to_f32(got["o"])).any()
    err = np.abs(A.bf16_to_f32(got["o"]).astype(np.float64) - ref["o32"])
    print("worst err / a", (err / ref["a"]).max())
    assert (err <= P.pda_tolerance(ref["a"])).all()


PLAN_MAIN = r"""
#include <cstdio>
#include "ntm/pda_plan.hpp"
namespace pd = ntm::pda;
namespace at = ntm::attn;
int main() {
  static_assert(pd::kLdsBytes == 4 * 64 * 272 + 8 * 64 * 16, "one V stage per wave, and Q^T");
  static_assert(pd::kPartialFloats == 32 * 128 + 64, "acc, m, l");
  int bad = 0;
  struct Shape { long long B, Hq, Hkv, T, mp, pages, S; bool ok; };
  const Shape shapes[] = {{2, 8, 2, 1, 17, 19, 4, true},  {1, 4, 1, 4, 12, 13, 1, true},  {1, 32, 1, 1, 19, 20, 2, true},
                          {1, 64, 1, 1, 19, 20, 2, false}, {1, 32, 2, 4, 19, 20, 2, false}, {1, 4, 1, 5, 12, 13, 1, false},
                          {1, 3, 2, 1, 12, 13, 1, false},  {1, 4, 1, 1, 4097, 13, 1, false}, {1, 4, 1, 1, 4096, 13, 64, true},
                          {1, 4, 1, 1, 12, 13, 65, false}, {0, 4, 1, 1, 12, 13, 1, false},  {1, 4, 1, 1, 12, 0, 1, false}};
  for (const Shape& s : shapes)
    if (pd::shape_ok(s.B, s.Hq, s.Hkv, s.T, s.mp, s.pages, s.S) != s.ok) ++bad, std::printf("shape %lld %lld %lld\n", s.Hq, s.T, s.S);
  // the split plan: the ranges tile [0, steps)
  const int lens_t[] = {1, 63, 64, 65, 257, 1000, 2048, 65536};
  for (int len : lens_t)
    for (int S = 1; S <= 64; ++S) {
      int next = 0;
      for (int s = 0; s < S; ++s) {
        const pd::Range r = pd::split_range(len, s, S);
        if (r.begin < r.end) { if (r.begin != next) ++bad; next = r.end; }
      }
      if (next != pd::key_steps(len)) ++bad, std::printf("tile %d %d\n", len, S);
    }
  // scatter then gather is the identity; the poison page keeps its fill
  const std::vector<int32_t> lens = {257, 130, 64, 1000, 16, 17};
  pd::PageTable pt = pd::make_page_table(lens, 5, 0);
  std::vector<uint16_t> pool((size_t)pt.pages * 2 * 16 * 128, 0x7FC0);
  std::vector<std::vector<uint16_t>> src;
  for (int b = 0; b < pt.B; ++b) {
    std::vector<uint16_t> v((size_t)2 * lens[b] * 128);
    for (size_t i = 0; i < v.size(); ++i) v[i] = (uint16_t)(at::attn_hash(9, (uint32_t)b, (uint32_t)i) & 0x7EFF);
    pd::scatter_to_pages(pt, b, 2, v.data(), pool);
    src.push_back(v);
  }
  for (int b = 0; b < pt.B; ++b)
    if (pd::gather_from_pages(pt, b, 2, pool) != src[b]) ++bad, std::printf("gather %d\n", b);
  for (size_t i = 0; i < (size_t)2 * 16 * 128; ++i)
    if (pool[(size_t)pt.poison * 2 * 16 * 128 + i] != 0x7FC0) { ++bad; break; }
  // exact inputs of one sequence pass the predicate, alone and behind a shared prefix
  at::Inputs in = pd::exact_sequence(7, 1, 4, 2, 2, 37);
  if (!at::attn_exact(in.q.data(), in.k.data(), in.v.data(), 1, 4, 2, 2, 37, 1)) ++bad, std::printf("exact\n");
  // line 1: the message; line 2: sizes and splits; line 3: the shared table; then the generator's dump
  const uint32_t table[8] = {0, 0, 0, 0, 0x0300u | (1u << 13) | (1u << 12), 2, 0x0700u, 5};
  std::printf("%s\n", pd::failure_message(3, "exact T4", "O", 2, (uint64_t)((0 * 8 + 5) * 4 + 3) * 64 + 3, 0x3f803f80u,
                                          0x3f803f81u, 8, 2, 4, 2, table + 0).c_str());
  const int32_t l3[3] = {100, 1, 8192};
  std::printf("%zu %zu %.0f %d %d %d %d %d %d\n", pd::workspace_bytes(2, 8, 3), pd::table_bytes(2, 8, 3), pd::kv_bytes(l3, 3, 8),
              pd::pda_splits(32, 8, 8192, 256), pd::pda_splits(1, 8, 8192, 256), pd::pda_splits(1, 1, 65536, 256),
              pd::pda_splits(4, 8, 255, 256), pd::pda_splits(4, 8, 512, 256), pd::pda_splits(1024, 8, 8192, 256));
  pt = pd::make_page_table({257, 130, 64, 1000}, 5, 2);
  std::printf("%d %d %d", pt.pages, pt.max_pages, pt.poison);
  for (int32_t v : pt.table) std::printf(" %d", v);
  std::printf("\n");
  for (int d = 0; d < 128; ++d)
    std::printf("%d %d %d %d %u\n", in.q[(3 * 2 + 1) * 128 + d], in.k[d], in.k[(37 + 36) * 128 + d], in.v[(37 + 1) * 128 + d],
                (unsigned)in.kb[(37 + 36) * 128 + d]);
  return bad;
}
"""


def test_plan_header_in_a_sanitized_program_and_the_numpy_twin():
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "plan.cpp").write_text(PLAN_MAIN)
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{INCLUDE}", str(Path(d) / "plan.cpp"), "-o", str(Path(d) / "plan")], check=True, timeout=300)
        p = subprocess.run([str(Path(d) / "plan")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    word = ((0 * 8 + 5) * 4 + 3) * 64 + 3
    table = np.array([0, 0, 0, 0, 0x0300 | 1 << 13 | 1 << 12, 2, 0x0700, 5], dtype=np.uint32)
    assert lines[0] == P.pda_failure_message(3, "exact T4", "O", 2, word, 0x3F803F80, 0x3F803F81, 8, 2, 4, 2, table)
    assert lines[0] == ("gpu3: pda exact T4 O: seq 0 head 5 tok 3 col 6: cu 2.1.1.3 5.0.0.7 (xcd.se.sh.cu): expected 0x3f803f80, "
                        "got 0x3f803f81, bad bits 0x00000001; 2 differ")
    assert len(lines[0]) < 200
    nums = [int(x) for x in lines[1].split()]
    assert nums[0] == P.pda_workspace_bytes(2, 8, 3) == 2 * 8 * 3 * (32 * 128 + 64) * 4
    assert nums[1] == P.pda_table_bytes(2, 8, 3) == 2 * 8 * 3 * 8
    assert nums[2] == P.pda_kv_bytes([100, 1, 8192], 8) == 8293 * 8 * 128 * 4
    assert nums[3:] == [P.pda_splits(*a) for a in ((32, 8, 8192, 256), (1, 8, 8192, 256), (1, 1, 65536, 256), (4, 8, 255, 256),
                                                   (4, 8, 512, 256), (1024, 8, 8192, 256))]
    pt = P.pda_make_page_table([257, 130, 64, 1000], seed=5, shared_pairs=2)
    assert [int(x) for x in lines[2].split()] == [pt["pages"], pt["max_pages"], pt["poison"]] + pt["table"].reshape(-1).tolist()
    qi, ki, vi = P.pda_exact_sequence(7, 1, 4, 2, 2, 37)
    rows = np.array([[int(x) for x in ln.split()] for ln in lines[3:131]])
    assert (rows[:, 0] == qi[3, 1]).all() and (rows[:, 1] == ki[0, 0]).all() and (rows[:, 2] == ki[1, 36]).all()
    assert (rows[:, 3] == vi[1, 1]).all() and (rows[:, 4] == A.f32_to_bf16_bits(ki[1, 36].astype(np.float32))).all()
    assert P.PDA_LDS_BYTES == 4 * 64 * 272 + 8192 <= 80 * 1024 and P.PDA_PARTIAL_FLOATS == 32 * 128 + 64
