"""K13 without a GPU: the numpy side of the fused attention check (``ops.attn``) - the emulation of
the kernel's arithmetic contract against float64 attention, the exact-input predicate and why it
makes the answer independent of summation order - the plan header in a sanitized stand-alone
program, and ``models.checks.attn.attn_check`` on the CPU backend."""
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nvidia_terraform_modules_amd.models.checks.attn import attn_check
from nvidia_terraform_modules_amd.ops import attn as A

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "validation" / "include"


@pytest.fixture(scope="module")
def exact():
    return A.attn_make_inputs("exact", 1, 4, 2, 129, 191, seed=7)


@pytest.mark.parametrize("S", [128, 320, 1024])
@pytest.mark.parametrize("causal", [False, True])
def test_contract_emulation_is_within_the_derived_bound_of_float64(S, causal):
    d = A.attn_make_inputs("dense", 1, 2, 1, S, S, seed=S)
    got, ref = A.attn_emulate(d, causal), A.attn_reference(d, causal)
    err = np.abs(A.bf16_to_f32(got["o"]).astype(np.float64) - ref["o"])
    print("worst err / a", (err / ref["a"]).max())
    assert (err <= A.attn_tolerance(ref["a"])).all()
    assert np.allclose(got["m"], ref["m"], rtol=1e-5, atol=1e-5) and np.allclose(got["l"], ref["l"], rtol=1e-4)


@pytest.mark.parametrize("causal", [False, True])
def test_exact_inputs_are_accepted_and_make_the_emulation_bitwise(exact, causal):
    assert A.attn_exact(exact["qi"], exact["ki"], exact["vi"], causal)
    got, ref = A.attn_emulate(exact, causal), A.attn_reference_f32(exact, causal)
    assert (got["o"] == ref["o"]).all()
    assert (got["m"].view(np.uint32) == ref["m"].view(np.uint32)).all()
    assert (got["l"].view(np.uint32) == ref["l"].view(np.uint32)).all()
    # both kinds of key occur: rows whose sum is more than one near key, and results that are not all zero
    assert ref["l"].max() > 2 and (ref["o"] != 0).mean() > 0.5


def test_exact_predicate_rejects_what_breaks_it(exact):
    qi, ki, vi = exact["qi"], exact["ki"], exact["vi"]
    # a score 50 below the row maximum: one near key's gap product 10 * 21 becomes 10 * 16
    near = int(np.flatnonzero(ki[0, 0, :, 5] == 21)[0])
    k2 = ki.copy()
    k2[0, 0, near, 5] = 16
    assert not A.attn_exact(qi, k2, vi, False)
    v2 = vi.copy()
    v2[0, 1, 3, 7] = 5
    assert not A.attn_exact(qi, ki, v2, False)
    big = np.zeros((1, 1, 8192, 128), dtype=np.int32)
    assert not A.attn_exact(qi[:, :1, :1], big, big, False)
    assert not A.attn_exact(qi, ki, vi.astype(np.float32), False)
    with pytest.raises(ValueError):
        A.attn_make_inputs("exact", 1, 1, 1, 1, 8192)


def test_random_order_fp32_summation_of_exact_inputs_deviates_by_zero(exact):
    rng = np.random.default_rng(5)
    q, k, v = (A.bf16_to_f32(exact[n]) for n in ("q", "k", "v"))
    ref = A.attn_reference_f32(exact, False)
    for h in range(4):
        s = (q[0, h].astype(np.float64) @ k[0, h // 2].astype(np.float64).T).astype(np.float32)
        p = np.exp2(s - s.max(axis=1, keepdims=True)).astype(np.float32)
        for _ in range(3):
            order = rng.permutation(s.shape[1])
            l = np.add.accumulate(p[:, order], axis=1, dtype=np.float32)[:, -1]
            terms = p[:, order, None] * v[0, h // 2][None, order, :]          # exact products
            acc = np.add.accumulate(terms, axis=1, dtype=np.float32)[:, -1, :]  # sequential fp32 sums
            assert (l.view(np.uint32) == ref["l"][0, h].view(np.uint32)).all()
            assert ((acc / l[:, None]).view(np.uint32) == ref["o32"][0, h].view(np.uint32)).all()


PLAN_MAIN = r"""
#include <cstdio>
#include "ntm/attn_plan.hpp"
namespace at = ntm::attn;
int main() {
  static_assert(at::kLdsBytes == 2 * 2 * 64 * 272, "two stages of K and V");
  struct Shape { long long B, Hq, Hkv, Sq, Sk; int causal; bool ok; long long grid; };
  const Shape shapes[] = {
      {1, 2, 1, 192, 192, 0, true, 4},   {1, 4, 2, 129, 191, 1, true, 8},    {2, 2, 2, 1, 257, 1, true, 4},
      {1, 1, 1, 128, 64, 0, true, 1},    {1, 1, 1, 128, 64, 1, false, 0},    {1, 3, 2, 64, 64, 0, false, 0},
      {1, 1, 1, 1, 65536, 0, true, 1},   {1, 1, 1, 1, 65537, 0, false, 0},   {0, 1, 1, 1, 1, 0, false, 0},
      {4, 32, 8, 4096, 4096, 1, true, 4096}, {1, 1, 1, 1ll << 33, 64, 0, false, 0}};
  int bad = 0;
  for (const Shape& s : shapes) {
    const bool ok = at::shape_ok(s.B, s.Hq, s.Hkv, s.Sq, s.Sk, s.causal);
    if (ok != s.ok || (ok && at::grid(s.B, s.Hq, s.Sq) != s.grid)) ++bad, std::printf("shape %lld %lld\n", s.Sq, s.Sk);
    if (!ok) continue;
    for (long long qt = 0; qt < at::query_tiles(s.Sq) && qt < 64; ++qt) {
      const int n = at::key_steps(qt, s.Sq, (int)s.Sk, s.causal), all = (int)((s.Sk + 63) / 64);
      long long last = (qt + 1) * 128 < s.Sq ? (qt + 1) * 128 : s.Sq;
      // every key the tile's last row sees lies in a walked step, and no walked step is wholly hidden
      const long long seen = at::visible_keys(last - 1, s.Sq, s.Sk, s.causal);
      if (n < 1 || n > all || (long long)n * 64 < seen || (long long)(n - 1) * 64 >= seen) ++bad, std::printf("steps %lld\n", qt);
    }
  }
  if (at::flops(1, 1, 2, 2, 0) != 4.0 * 4 * 128 || at::flops(1, 1, 2, 2, 1) != 4.0 * 3 * 128) ++bad;
  if (at::flops(1, 1, 2, 5, 1) != 4.0 * 9 * 128) ++bad;
  // the generator's inputs pass the predicate, and each broken condition fails it
  at::Inputs in = at::make_exact(1, 4, 2, 129, 191, 7);
  if (!at::attn_exact(in.q.data(), in.k.data(), in.v.data(), 1, 4, 2, 129, 191, 0)) ++bad, std::printf("exact\n");
  if (!at::attn_exact(in.q.data(), in.k.data(), in.v.data(), 1, 4, 2, 129, 191, 1)) ++bad, std::printf("exact causal\n");
  for (size_t j = 0; j < 191; ++j)
    if (in.k[j * 128 + at::kGapDim] == at::kGapK) { in.k[j * 128 + at::kGapDim] = 16; break; }
  if (at::attn_exact(in.q.data(), in.k.data(), in.v.data(), 1, 4, 2, 129, 191, 0)) ++bad, std::printf("gap\n");
  in = at::make_exact(1, 1, 1, 3, 70, 7);
  in.v[5] = 5;
  if (at::attn_exact(in.q.data(), in.k.data(), in.v.data(), 1, 1, 1, 3, 70, 0)) ++bad, std::printf("v\n");
  std::printf("%s\n", at::failure_message(3, "exact causal", "O", 2, 64 * 130 + 3, 0x3f803f80u, 0x3f803f81u, 4, 129, nullptr).c_str());
  // the dump the numpy twin is held to: seed 7, first query row, key rows 0 and 190, value row 1
  in = at::make_exact(1, 4, 2, 129, 191, 7);
  for (int d = 0; d < 128; ++d) std::printf("%d %d %d %d %u\n", in.q[d], in.k[d], in.k[190 * 128 + d], in.v[128 + d], (unsigned)in.qb[d]);
  return bad;
}
"""


def test_plan_header_in_a_sanitized_program_and_the_numpy_twin(exact):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        (Path(d) / "plan.cpp").write_text(PLAN_MAIN)
        subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        f"-I{INCLUDE}", str(Path(d) / "plan.cpp"), "-o", str(Path(d) / "plan")], check=True, timeout=300)
        p = subprocess.run([str(Path(d) / "plan")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert lines[0] == A.attn_failure_message(3, "exact causal", "O", 2, 64 * 130 + 3, 0x3F803F80, 0x3F803F81, 4, 129)
    assert lines[0] == ("gpu3: attn exact causal O: batch 0 head 1 row 1 col 6: expected 0x3f803f80, got 0x3f803f81, "
                        "bad bits 0x00000001; 2 differ")
    rows = np.array([[int(x) for x in ln.split()] for ln in lines[1:129]])
    assert (rows[:, 0] == exact["qi"][0, 0, 0]).all() and (rows[:, 1] == exact["ki"][0, 0, 0]).all()
    assert (rows[:, 2] == exact["ki"][0, 0, 190]).all() and (rows[:, 3] == exact["vi"][0, 0, 1]).all()
    assert (rows[:, 4] == exact["q"][0, 0, 0]).all()
    assert A.ATTN_LDS_BYTES == 2 * 2 * 64 * 272 <= 160 * 1024
    assert A.attn_grid(1, 4, 129) == 8 and A.attn_key_steps(0, 129, 191, True) == 3 and A.attn_key_steps(1, 129, 191, True) == 3
    assert A.attn_flops(1, 1, 2, 5, True) == 4.0 * 9 * 128


def test_attn_check_passes_on_the_cpu_backend():
    r = attn_check("cpu", backend=A.CPU_BACKEND)
    assert r["ok"] and r["failures"] == [] and all(v == 0 for v in r["bad"].values()), r
    assert 0 < r["dense_worst"] < 2.0 ** -7 and r["attn_tflops"] == 0.0 and r["seconds"] > 0


def test_attn_check_corrupt_yields_one_line_of_the_documented_form():
    r = attn_check("cpu", backend=A.CPU_BACKEND, corrupt=True)
    assert not r["ok"] and len(r["failures"]) == 1 and r["bad"]["exact"] == 1, r
    m = re.match(r"gpu0: attn exact O: batch 0 head (\d+) row (\d+) col (\d+): xcd \d+ se \d+ sh \d+ cu \d+: expected "
                 r"(0x[0-9a-f]{8}), got (0x[0-9a-f]{8}), bad bits 0x00080000; 1 differ$", r["failures"][0])
    assert m and len(r["failures"][0]) < 200, r["failures"][0]
    assert int(m.group(4), 16) ^ int(m.group(5), 16) == 0x80000
