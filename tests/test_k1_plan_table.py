"""The K1 dispatch plan (validation/include/ntm/k1_plan.hpp) against the table
tools/k1_plan_table.py recorded before the plan moved into that header
(tests/fixtures/k1_plan_table.json): through the built library, and through a
stand-alone sanitized C++ program that includes nothing but the header. No GPU."""
import json
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
TABLE = json.loads((ROOT / "tests" / "fixtures" / "k1_plan_table.json").read_text())
MODES = ("bf16", "bf16_splitk", "fp8", "fp8_splitk")

# settings of the table's knob section -> (cus, pp, pp_split, margin, min_k, fp8_long, ragged)
SHIPPING = (256, 1, 1, 0.0, -1, 1, 1)
SETTINGS = {
    "cus128": (128, 1, 1, 0.0, -1, 1, 1), "cus80": (80, 1, 1, 0.0, -1, 1, 1),
    "cus32": (32, 1, 1, 0.0, -1, 1, 1), "pp_tiles_off": (256, 0, 1, 0.0, -1, 1, 1),
    "pp_split_off": (256, 1, 0, 0.0, -1, 1, 1), "margin1.1_longk0": (256, 1, 1, 1.1, 0, 1, 1),
    "fp8_long_off": (256, 1, 1, 0.0, -1, 0, 1), "ragged_off": (256, 1, 1, 0.0, -1, 1, 0),
}


def test_table_covers_what_it_should():
    rows = TABLE["rows"]
    assert TABLE["cus"] == 256 and len(rows) >= 600 and len({tuple(r[:3]) for r in rows}) == len(rows)
    assert sum(1 for r in rows if r[3] == 0 and r[0] > 0) >= 24          # infeasible shapes
    assert sum(1 for r in rows if r[5] != 0) >= 100                      # fp8 plans
    assert sum(1 for r in rows if r[4] != 0 and r[4][3] > 1) >= 50       # split-K plans
    assert {r[4][1] for r in rows if r[4] != 0} >= {49, 54, 55}          # every stream-K build
    assert TABLE["settings"] == list(SETTINGS) and len(TABLE["knobs"]) == len(SETTINGS)
    assert all(len(k) == TABLE["knob_rows"] >= 100 for k in TABLE["knobs"])
    for name, k in zip(TABLE["settings"], TABLE["knobs"]):   # each setting changes some plan
        assert k != [r[6 if name == "fp8_long_off" else 4] for r in rows[:TABLE["knob_rows"]]], name
    assert os.path.getsize(ROOT / "tests" / "fixtures" / "k1_plan_table.json") < 100_000


def test_library_plans_equal_the_recorded_table():
    """Every row, all four modes, the stream-K workspace queries and (to 1e-12
    relative: same compiler, same expressions) the two predicted times; then the
    bf16 split-K plan under each CU override and non-shipping knob setting."""
    from nvidia_terraform_modules_amd.ops import _lib

    if not _lib.LIB_PATH.exists():
        pytest.skip("native library not built (python -m nvidia_terraform_modules_amd.ops.build)")
    import importlib.util

    spec = importlib.util.spec_from_file_location("k1_plan_table", ROOT / "tools" / "k1_plan_table.py")
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert _lib.lib().ntm_plan_cus() == 256
    bad = []
    for want in TABLE["rows"]:
        got = tool.row(*want[:3], TABLE["ws_bytes"])
        if got[:8] != want[:8] or (got[8] == 0) != (want[8] == 0):
            bad.append((want, got))
        elif want[8] != 0:
            for g, w in zip(got[8], want[8]):
                assert abs(g - w) <= 1e-12 * abs(w), (want, got)
    assert not bad, bad[:5]
    shapes = [r[:3] for r in TABLE["rows"][:TABLE["knob_rows"]]]
    for (name, on, off, *f), want in zip(tool.SETTINGS, TABLE["knobs"]):
        on()
        try:
            got = [tool._plan(f[0] if f else tool.kernels.k1_splitk_plan, *s) for s in shapes]
        finally:
            off()
        assert got == want, (name, [(s, g, w) for s, g, w in zip(shapes, got, want) if g != w][:5])


PLAN_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "ntm/k1_plan.hpp"
using namespace ntm::k1;
#define REQUIRE(...) \
  do { if (!(__VA_ARGS__)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } } while (0)

static bool same(const K1Plan& a, const K1Plan& b) {
  return a.top_rows == b.top_rows && a.top_variant == b.top_variant &&
         a.rest_variant == b.rest_variant && a.splits == b.splits && a.sk == b.sk &&
         a.unsplit_s == b.unsplit_s && a.sk_s == b.sk_s;
}

int main(int argc, char** argv) {
  REQUIRE(argc == 2);
  std::FILE* f = std::fopen(argv[1], "r");
  REQUIRE(f);
  PlanQuery q{};
  int splitk, fp8, pp, pp_split, fp8_long, ragged;
  while (std::fscanf(f, "%d %d %d %d %d %d %d %d %lf %d %d %d", &q.M, &q.N, &q.K, &q.cus, &splitk,
                     &fp8, &pp, &pp_split, &q.knobs.splitk_margin, &q.knobs.splitk_min_k, &fp8_long,
                     &ragged) == 12) {
    q.splitk = splitk, q.fp8 = fp8, q.knobs.pp = pp, q.knobs.pp_split = pp_split;
    q.knobs.splitk_fp8_long = fp8_long, q.knobs.splitk_ragged = ragged;
    const K1Plan p = plan(q);
    REQUIRE(same(p, plan_search(q)));
    if (!p.feasible()) std::printf("x\n");
    else std::printf("%d %d %d %d\n", p.top_rows, p.top_variant, p.rest_variant, p.splits);
  }
  std::fclose(f);

  // memo eviction: 1,000 distinct queries (4 per slot) asked twice, in opposite orders
  std::vector<PlanQuery> qs;
  for (int i = 0; i < 1000; ++i) {
    PlanQuery e{8 + 8 * ((i * 37) % 1021), 8 + 8 * ((i * 101) % 997), 8 + 8 * i, 256, i % 2 == 0,
                i % 5 == 0, PlanKnobs{}};
    e.knobs.splitk_ragged = i % 3 != 0;
    qs.push_back(e);
  }
  std::vector<K1Plan> first;
  for (const PlanQuery& e : qs) first.push_back(plan(e));
  for (int i = 999; i >= 0; --i) REQUIRE(same(plan(qs[i]), first[i]));
  for (int i = 0; i < 1000; ++i) REQUIRE(same(plan_search(qs[i]), first[i]));
  PlanKnobs k;
  REQUIRE(k == PlanKnobs{} && k.long_k() == 1024 && k.long_margin() == 1.03);
  k.splitk_min_k = 0;
  REQUIRE(!(k == PlanKnobs{}) && k.long_k() == 0);

  // tests/test_k1_plan.py test_stream_k_decomposition_serves, on 256 CUs
  const struct { int m, n, k; bool served; } sk[9] = {
      {4472, 5688, 5832, true}, {4672, 1472, 6696, true}, {1000, 1000, 1000, true},
      {256, 256, 256, true}, {4096, 4096, 4096, false}, {8192, 8192, 8192, false},
      {7472, 1280, 6024, false}, {256, 256, 128, false}, {4096, 4100, 4096, false}};
  for (const auto& c : sk) {
    SkShape s{};
    REQUIRE((shape_ok_sk(c.m, c.n, c.k) && sk_decompose<256, 256, true>(c.m, c.n, c.k, 256, s)) == c.served);
    if (c.served) REQUIRE(s.G == 256 && s.ntiles == ((c.m + 255) / 256) * ((c.n + 255) / 256) &&
                          s.Tp == (c.k + 127) / 128 && (s.S == 0) == (s.ntiles > 256));
  }
  SkShape s{};
  REQUIRE(sk_decompose<256, 256, true>(8192, 8448, 4096, 256, s) && s.S == 0 && s.D == 768);   // 1056 tiles
  REQUIRE(!(sk_decompose<256, 256, false>(4472, 5688, 5832, 256, s)));   // split mode only
  REQUIRE(sk_decompose<192, 256, false>(4152, 1096, 16056, 256, s) && s.S == 2 && s.ntiles == 110);
  REQUIRE(sk_ws_bytes(256) == 4096 + 512 * kPartialBytes && kErrWord == 1023);
  REQUIRE(splitk_kc(7568, 3) == 2560 && splitk_slices(7568, 3) == 3 && splitk_slices(128, 16) == 2);
  REQUIRE(shape_ok6(512, 512, 256) && !shape_ok6(512, 512, 128) && !shape_ok6(500, 512, 256));
  std::printf("ok\n");
  return 0;
}
"""


def _queries():
    """(query line, expected plan) of every fixture row that reaches the search."""
    out = []

    def add(m, n, k, splitk, fp8, setting, want):
        if fp8 and not (m > 0 and n > 0 and k > 0 and n % 8 == 0 and k % 16 == 0):
            assert want == 0            # the C ABI's shape check (N % 8, K % 16), before the plan
            return
        k = k // 2 if fp8 else k        # fp8: K in bf16-sized pairs
        cus, pp, pps, margin, min_k, fp8_long, ragged = setting
        line = f"{m} {n} {k} {cus} {splitk} {fp8} {pp} {pps} {margin!r} {min_k} {fp8_long} {ragged}"
        out.append((line, want if want == 0 or len(want) == 4 else want + [1]))

    for m, n, k, *plans in TABLE["rows"]:
        for mode, want in zip(MODES, plans):
            add(m, n, k, int(mode.endswith("splitk")), int(mode.startswith("fp8")), SHIPPING, want)
    for name, wants in zip(TABLE["settings"], TABLE["knobs"]):
        for (m, n, k, *_), want in zip(TABLE["rows"], wants):
            add(m, n, k, 1, int(name == "fp8_long_off"), SETTINGS[name], want)
    return out


def test_plan_header_alone_under_sanitizers(tmp_path):
    """Stand-alone program with its own main against k1_plan.hpp alone, built with
    -Wall -Werror, AddressSanitizer and UBSan (nothing is loaded into Python):
    the integer plans of every fixture query (the times are the library test's:
    another host compiler may contract them differently), memo eviction, and
    the stream-K decomposition."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe, qfile = tmp_path / "k1_plan_main.cpp", tmp_path / "k1_plan_main", tmp_path / "queries.txt"
    src.write_text(PLAN_MAIN)
    queries = _queries()
    qfile.write_text("".join(line + "\n" for line, _ in queries))
    inc = f"-I{ROOT / 'validation' / 'include'}"
    if cxx:
        static = (["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx)
                  else ["-static-libsan"])
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *static, inc, str(src), "-o", str(exe)]
    elif os.path.exists(hipcc):
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-Xarch_host", "-fsanitize=address",
               "-Xarch_host", "-fsanitize=undefined", "-static-libsan", inc, str(src), "-o", str(exe)]
    else:
        pytest.skip("no C++ compiler")
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr
    p = subprocess.run([str(exe), str(qfile)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and not p.stderr, p.stdout[-2000:] + p.stderr
    lines = p.stdout.split("\n")
    assert lines[len(queries):] == ["ok", ""]
    got = [0 if ln == "x" else [int(v) for v in ln.split()] for ln in lines[:len(queries)]]
    bad = [(q, g, w) for (q, w), g in zip(queries, got) if g != w]
    assert not bad, bad[:5]     # a difference here is a near-tie between compilers: report it
