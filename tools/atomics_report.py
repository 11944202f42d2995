#!/usr/bin/env python3
"""K9 atomics check: print the per-op table and the hand-off's XCD pair coverage from a report.

    NTM_ATOMICS_CHECK=1 validation/build/amdgpu-validate --gpus 1 --out report.json
    python tools/atomics_report.py report.json [more.json ...]

Per op: bad slots, Gop/s and GB/s of operand bytes (4 or 8 per operation). The matrix is
writer XCD (row) x reader XCD (column); 1 = a reader on that XCD checked a slab written there.
"""
import json
import sys

WIDE = {"add_u64", "max_u64", "add_f64"}


def main(paths):
    if not paths:
        sys.exit(__doc__)
    for path in paths:
        rep = json.loads(open(path).read().strip().splitlines()[-1])
        for g in rep["gpus"]:
            if "atomics_ops" not in g:
                print(f"{path}: gpu{g['device']}: the atomics check did not run (NTM_ATOMICS_CHECK=1)")
                continue
            print(f"{path}: gpu{g['device']}: {g['atomics_seconds']:.3f} s")
            print(f"  {'op':12s} {'bad':>6s} {'Gop/s':>9s} {'GB/s':>9s}")
            for op in g["atomics_ops"]:
                gops = g[f"atomics_{op}_gops"]
                print(f"  {op:12s} {g[f'atomics_{op}_bad']:6d} {gops:9.2f} {gops * (8 if op in WIDE else 4):9.1f}")
            print(f"  ticket bad {g['atomics_ticket_bad']}; handoff bad words {g['atomics_handoff_bad_words']} "
                  f"(stale {g['atomics_handoff_stale_words']}), {g['atomics_handoff_episodes_per_s']:.3g} episodes/s")
            pairs = g.get("atomics_xcd_pairs", [])
            print(f"  XCD pairs covered {g['atomics_xcd_pairs_covered']} of {len(pairs) ** 2} (writer row, reader column)")
            for w, row in enumerate(pairs):
                print(f"    {w}: " + " ".join(str(v) for v in row))


if __name__ == "__main__":
    main(sys.argv[1:])
