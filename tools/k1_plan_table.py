#!/usr/bin/env python3
"""Record the K1 dispatch plan of the built library as a table of integers.

Host only (no GPU): every plan comes from the public wrappers of
``ops.kernels``. Run it before a change to the plan's code
(validation/include/ntm/k1_plan.hpp); tests/test_k1_plan_table.py then holds
the changed code to the recorded table, through the library and through a
stand-alone C++ program.

    python tools/k1_plan_table.py [--random 600] [--out tests/fixtures/k1_plan_table.json]

The table (JSON, variants as the integers of ``GEMM_VARIANTS``):
  rows    [M, N, K, bf16, bf16_splitk, fp8, fp8_splitk, served, times]
          a plan is [top_rows, top_variant, rest_variant(, splits)] or 0 where
          the wrapper raises; served = bit 0 / 1 / 2: sk_ws_bytes /
          skh_ws_bytes("pp192x256s") / ("pp256x192s") is ws_bytes, else it is 0;
          times = ntm_k1_plan_times' [unsplit_s, sk_s], 0 without a bf16 plan
  knobs   for the first ``knob_rows`` rows, in ``settings`` order, the
          bf16_splitk plan under a CU override or one non-shipping knob setting
          (fp8_long_off, which bf16 plans do not read: the fp8_splitk plan)
"""
from __future__ import annotations

import argparse
import ctypes
import json
import random
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

from nvidia_terraform_modules_amd.ops import kernels  # noqa: E402
from nvidia_terraform_modules_amd.ops._lib import lib  # noqa: E402

# (name, what to set, how to restore): the CU overrides and each knob's
# non-shipping setting
SETTINGS = [
    ("cus128", lambda: kernels.set_cus_override(128), lambda: kernels.set_cus_override(0)),
    ("cus80", lambda: kernels.set_cus_override(80), lambda: kernels.set_cus_override(0)),
    ("cus32", lambda: kernels.set_cus_override(32), lambda: kernels.set_cus_override(0)),
    ("pp_tiles_off", lambda: kernels.set_plan_pp_tiles(False, split=True),
     lambda: kernels.set_plan_pp_tiles(True)),
    ("pp_split_off", lambda: kernels.set_plan_pp_tiles(True, split=False),
     lambda: kernels.set_plan_pp_tiles(True)),
    ("margin1.1_longk0", lambda: kernels.set_plan_splitk(1.1, 0), lambda: kernels.set_plan_splitk()),
    ("fp8_long_off", lambda: kernels.set_plan_splitk(fp8=False), lambda: kernels.set_plan_splitk(),
     kernels.k1_fp8_splitk_plan),
    ("ragged_off", lambda: kernels.set_plan_splitk_ragged(False),
     lambda: kernels.set_plan_splitk_ragged(True)),
]
KNOB_ROWS = 150


def named_shapes() -> list[tuple[int, int, int]]:
    """Every (M, N, K) tests/test_k1_plan.py names, literal or generated."""
    text = (ROOT / "tests" / "test_k1_plan.py").read_text()
    out = [tuple(int(v) for v in t) for t in re.findall(r"\((\d+),\s*(\d+),\s*(\d+)", text)]
    out += [(256 * i, 256 * j, 512) for i in range(1, 33, 3) for j in range(1, 33, 5)]
    out += [(m, n, k) for m in (64, 333, 1000, 2048) for n in (256, 1004, 4096)
            for k in (1024, 4104, 16384)]
    return out


def random_shapes(count: int) -> list[tuple[int, int, int]]:
    rng = random.Random(2026)
    return [(rng.randrange(1, 9001), rng.randrange(1, 2251) * 4, rng.randrange(1, 2126) * 8)
            for _ in range(count)]


def infeasible_shapes() -> list[tuple[int, int, int]]:
    rng = random.Random(2027)
    out = []
    for i in range(36):
        m, n, k = rng.randrange(1, 9001), rng.randrange(1, 2251) * 4, rng.randrange(1, 2126) * 8
        out.append((m, n, k + rng.randrange(1, 8)) if i % 2 else (m, n + rng.randrange(1, 4), k))
    return out


def _ids(plan: tuple) -> list[int]:
    return [plan[0], kernels.GEMM_VARIANTS[plan[1]], kernels.GEMM_VARIANTS[plan[2]], *plan[3:]]


def _plan(f, m: int, n: int, k: int):
    try:
        return _ids(f(m, n, k))
    except ValueError:
        return 0


def plan_times(m: int, n: int, k: int):
    u, s = ctypes.c_double(), ctypes.c_double()
    if lib().ntm_k1_plan_times(m, n, k, ctypes.byref(u), ctypes.byref(s)) != 0:
        return 0
    return [u.value, s.value]


def row(m: int, n: int, k: int, ws_bytes: int) -> list:
    ws = (kernels.sk_ws_bytes(m, n, k), kernels.skh_ws_bytes("pp192x256s", m, n, k),
          kernels.skh_ws_bytes("pp256x192s", m, n, k))
    assert all(w in (0, ws_bytes) for w in ws), (m, n, k, ws)
    served = sum(1 << i for i, w in enumerate(ws) if w)
    return [m, n, k, _plan(kernels.k1_plan, m, n, k), _plan(kernels.k1_splitk_plan, m, n, k),
            _plan(kernels.k1_fp8_plan, m, n, k), _plan(kernels.k1_fp8_splitk_plan, m, n, k),
            served, plan_times(m, n, k) if m > 0 else 0]


def table(n_random: int) -> dict:
    if lib().ntm_plan_cus() != 256:
        raise SystemExit("the table is recorded for 256 CUs (a machine without a GPU, or SPX mode)")
    ws_bytes = kernels.sk_ws_bytes(4672, 1472, 6696)
    # the knob section takes the first rows: the named shapes (the ones the
    # knobs were tuned on among them) lead
    shapes = list(dict.fromkeys(named_shapes() + random_shapes(n_random) + infeasible_shapes()))
    rows = [row(m, n, k, ws_bytes) for m, n, k in shapes]
    knobs = []
    for _, on, off, *f in SETTINGS:
        on()
        try:
            knobs.append([_plan(f[0] if f else kernels.k1_splitk_plan, *s)
                          for s in shapes[:KNOB_ROWS]])
        finally:
            off()
    return {"cus": 256, "ws_bytes": ws_bytes, "rows": rows, "knob_rows": KNOB_ROWS,
            "settings": [s[0] for s in SETTINGS], "knobs": knobs}


def main(argv: list[str] | None = None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--random", type=int, default=600, help="random shapes (seed 2026)")
    ap.add_argument("--out", default=str(ROOT / "tests" / "fixtures" / "k1_plan_table.json"))
    args = ap.parse_args(argv)
    t = table(args.random)

    def dumps(v) -> str:
        return json.dumps(v, separators=(",", ":"))

    head = dumps({k: v for k, v in t.items() if k not in ("rows", "knobs")})
    text = (head[:-1] + ',\n"rows":[\n' + ",\n".join(dumps(r) for r in t["rows"]) +
            '],\n"knobs":[\n' + ",\n".join(dumps(k) for k in t["knobs"]) + "]}\n")
    Path(args.out).write_text(text)
    print(f"{args.out}: {len(t['rows'])} rows, {len(text)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
