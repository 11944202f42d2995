#!/usr/bin/env python3
"""K14: times ``ntm_pda_fwd`` (the split kernel and the combine) on one GPU at the Job's timed shape
(B 32, Hq 32, Hkv 8, T 1, every length 8192: 1 GiB of K and V together in a shuffled page pool) for
several split counts, in interleaved rounds. Every split count is warmed up for ``--settle``
seconds before its first timed round; a round times ``--iters`` launches between two device
events. The rate is the K and V bytes below ``len_b`` over the time; the yardstick to read it
against is K2's read rate in the Job's report. A record, not a gate: nobody has tuned the kernel
against it. Writes one JSON document (``--out``) and prints the table.

    python tools/pda_rates.py --out profiles/pda/run1/rates.json
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from nvidia_terraform_modules_amd.ops import pda as host  # noqa: E402
from nvidia_terraform_modules_amd.ops._lib import check, lib, stream_handle  # noqa: E402
from nvidia_terraform_modules_amd.ops.attn import ATTN_DEFAULT_SCALE_LOG2  # noqa: E402

B, HQ, HKV, T, LEN = 32, 32, 8, 1, 8192  # the Job's timed shape


def _events_ms(fn, iters: int) -> float:
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _settle(fn, seconds: float) -> None:
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(4):
            fn()
        torch.cuda.synchronize()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--settle", type=float, default=0.5)
    ap.add_argument("--splits", type=int, nargs="*", default=[1, 2, 4, 8])
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("pda_rates: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    L = lib()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    default = L.ntm_pda_default_splits(B, HKV, LEN, cus)
    pt = host.pda_make_page_table([LEN] * B, seed=0x14DA)
    g = torch.Generator(device=dev).manual_seed(LEN)
    shape = (pt["pages"], HKV, host.PDA_PAGE, 128)
    q = (torch.rand((B, HQ, T, 128), device=dev, generator=g) * 2 - 1).bfloat16()
    k_pool = (torch.rand(shape, device=dev, generator=g) * 2 - 1).bfloat16()
    v_pool = (torch.rand(shape, device=dev, generator=g) * 2 - 1).bfloat16()
    bt = torch.from_numpy(pt["table"]).to(dev)
    sl = torch.from_numpy(pt["lens"]).to(dev)
    o = torch.empty_like(q)
    nbytes = host.pda_kv_bytes([LEN] * B, HKV)
    forms = {}
    for S in sorted(set(args.splits + [default])):
        ws = torch.empty((L.ntm_pda_workspace_bytes(B, HKV, S) // 4,), dtype=torch.float32, device=dev)

        def fwd(S=S, ws=ws):
            check(L.ntm_pda_fwd(q.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(), bt.data_ptr(), sl.data_ptr(), o.data_ptr(),
                                None, None, ws.data_ptr(), None, B, HQ, HKV, T, pt["max_pages"], pt["pages"], S,
                                ATTN_DEFAULT_SCALE_LOG2, stream_handle()), "ntm_pda_fwd")
        forms[f"pda_S{S}"] = fwd
    for fn in forms.values():
        _settle(fn, args.settle)
    ms = {name: [] for name in forms}
    for _ in range(args.rounds):
        for name, fn in forms.items():
            ms[name].append(_events_ms(fn, args.iters))
    rows = []
    for name, xs in ms.items():
        rows.append({"form": name, "ms": xs, "gbps": nbytes / (statistics.median(xs) * 1e-3) / 1e9})
        print(f"{name}: {rows[-1]['gbps']:.0f} GB/s (median of {len(xs)} rounds, {statistics.median(xs):.3f} ms)", flush=True)
    doc = {"tool": "pda_rates", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "shape": [B, HQ, HKV, T, LEN],
           "default_splits": default, "kv_bytes": nbytes, "rounds": args.rounds, "iters": args.iters, "settle_s": args.settle,
           "rows": rows}
    text = json.dumps(doc)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
