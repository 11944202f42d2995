#!/usr/bin/env python3
"""K13: times ``ops.gpu.attn.attn_fwd`` against ``torch.nn.functional.scaled_dot_product_attention``
on one GPU, interleaved in rounds on the same tensors, at the Job's timed shape and two others.
Every shape is warmed up for ``--settle`` seconds per implementation before its first timed
round; a round times ``--iters`` launches between two device events (100 launches: 60 to
460 ms a round). A record, not a gate: nobody has tuned the kernel against it. Writes one JSON document (``--out``) and prints the table.

    python tools/attn_rates.py --out profiles/attn/run1/rates.json
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
from nvidia_terraform_modules_amd.ops import attn as host  # noqa: E402
from nvidia_terraform_modules_amd.ops.gpu import attn as gpu  # noqa: E402

# (B, Hq, Hkv, Sq, Sk, causal); the first is the Job's timed shape
SHAPES = [(4, 32, 8, 4096, 4096, True), (4, 32, 8, 2048, 2048, True), (2, 32, 8, 8192, 8192, False)]


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
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--settle", type=float, default=1.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        print("attn_rates: no GPU", file=sys.stderr)
        return 2
    dev = torch.device("cuda", 0)
    rows = []
    for B, Hq, Hkv, Sq, Sk, causal in SHAPES:
        g = torch.Generator(device=dev).manual_seed(Sq)
        q = torch.randn((B, Hq, Sq, 128), device=dev, generator=g).bfloat16()
        k = torch.randn((B, Hkv, Sk, 128), device=dev, generator=g).bfloat16()
        v = torch.randn((B, Hkv, Sk, 128), device=dev, generator=g).bfloat16()
        kr, vr = k.repeat_interleave(Hq // Hkv, 1), v.repeat_interleave(Hq // Hkv, 1)  # outside the timing
        out = torch.empty_like(q)

        def ours():
            gpu.attn_fwd(q, k, v, causal=causal, out=(out, None, None))

        def library():
            return torch.nn.functional.scaled_dot_product_attention(q, kr, vr, is_causal=causal)

        row = {"shape": [B, Hq, Hkv, Sq, Sk], "causal": causal, "flops": host.attn_flops(B, Hq, Sq, Sk, causal)}
        try:
            err = float((library().float() - (ours() or out).float()).abs().max())
            row["max_abs_difference"] = err
            lib_ok = True
        except RuntimeError as e:  # the library has no kernel for this build: recorded, nothing to compare with
            row["library_error"] = str(e)[:200]
            lib_ok = False
        _settle(ours, args.settle)
        if lib_ok:
            _settle(library, args.settle)
        ms = {"ntm": [], "sdpa": []}
        for _ in range(args.rounds):
            ms["ntm"].append(_events_ms(ours, args.iters))
            if lib_ok:
                ms["sdpa"].append(_events_ms(library, args.iters))
        for name, xs in ms.items():
            if xs:
                row[name + "_ms"] = xs
                row[name + "_tflops"] = row["flops"] / (statistics.median(xs) * 1e-3) / 1e12
        row["ratio_ntm_over_sdpa"] = row["ntm_tflops"] / row["sdpa_tflops"] if lib_ok else None
        rows.append(row)
        print(f"{row['shape']} causal={causal}: ntm {row['ntm_tflops']:.1f} TFLOP/s, sdpa "
              f"{row.get('sdpa_tflops', float('nan')):.1f} TFLOP/s, ratio {row['ratio_ntm_over_sdpa']}", flush=True)
    doc = {"tool": "attn_rates", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "rounds": args.rounds,
           "iters": args.iters, "settle_s": args.settle, "rows": rows}
    text = json.dumps(doc)
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
