"""K14: the Job's paged-KV decode attention check with exact answers."""
from __future__ import annotations

import time

import numpy as np
import torch

from ...ops import pda as host
from ...ops.attn import attn_decode_cu
from .._timing import _wall_time
from ._common import device_context, verdict


def pda_check(device: torch.device, corrupt: bool = False,
              exact_shapes: tuple = ((8, 2, 1, (257, 130, 1, 64), 4), (8, 2, 4, (257, 130, 5, 64), 2)),
              dense_shape: tuple = (8, 2, 1, (320, 77, 513), 3), timed_shape: tuple | None = None, iters: int = 3,
              seed: int = 0x14DA) -> dict:
    """K14, the Job's paged-KV decode attention check (``NTM_PDA_CHECK=1``) on ``device``, in the
    Job's sequence; shapes are (Hq, Hkv, T, lens, S). *Exact*: ``ops.pda`` exact problems of
    ``exact_shapes`` (the Job: 24 sequences, 384 workgroups, T 1 and T 4) with a shuffled pool, one
    prefix-shared pair, a NaN poison page and NaN page tails; O, m and l bitwise against K13's
    reference kernel on the gathered keys. *Dense*: uniform bf16 of ``dense_shape``, every element
    within ``pda_tolerance(a)`` of the reference's fp32 O. *Timed*: with ``timed_shape`` (the Job:
    (32, 8, 1, (8192,) * 32, None)) ``iters`` launches. ``corrupt`` flips bit 3 of one O element of
    the first exact run before its compare. Returns ``ok``, ``failures`` (the Job's lines), ``bad``
    per sub-test, ``dense_worst`` (largest err / a), ``xcds`` and ``cus`` seen in the CU tables,
    ``pda_kv_gbps`` and ``seconds``. ``pda_kv_gbps`` is a host clock around ``pda_fwd`` calls, each
    of which reads the lengths and page ids back to check them (a synchronise): it includes those
    round trips, is not comparable with the Job's figure (``tools/pda_rates.py`` times the C entry
    itself) and is never judged. The Job's exact problem shares two prefixes among 24 sequences;
    these hold four sequences, two of them too short to share a page, so one pair."""
    from ...ops.gpu import attn as ga
    from ...ops.gpu import pda as gp

    device = torch.device(device)
    gpu = device.index if device.index is not None else 0
    t_begin = time.perf_counter()
    out = {"bad": {"exact": 0, "dense": 0}, "failures": [], "dense_worst": 0.0, "pda_kv_gbps": 0.0, "xcds": 0, "cus": 0}
    seen = set()

    with device_context(device):
        for n, (Hq, Hkv, T, lens, S) in enumerate(exact_shapes):
            pr = host.pda_make_problem("exact", Hq, Hkv, T, lens, seed=seed + n, shared_pairs=1)
            if not host.pda_exact(pr):
                raise ValueError("pda_check: the exact inputs break attn_exact")
            d = gp.pda_to_device(pr, device)
            args = (d["q"], d["k_pool"], d["v_pool"], d["block_table"], d["seq_lens"])
            sub = f"exact T{T}"
            got_o, got_m, got_l, table = gp.pda_fwd(*args, splits=S, scale_log2=1.0, return_stats=True, table=True)
            ref = gp.pda_reference_gpu(*args, scale_log2=1.0)
            if corrupt and n == 0:
                got_o.view(torch.int16).view(-1)[got_o.numel() // 2 + 5] ^= 1 << 3
            tab = table.cpu().numpy().view(np.uint32)
            seen |= {attn_decode_cu(int(hw), int(xcc)) for hw, xcc in tab}
            for what, e, g in (("O", ref["o"], got_o), ("m", ref["m"], got_m), ("l", ref["l"], got_l)):
                rep = ga.attn_compare(e, g)
                if not rep.ok:
                    out["bad"]["exact"] += rep.count
                    out["failures"].append(host.pda_failure_message(gpu, sub, what, rep.count, rep.first_index, rep.expected,
                                                                    rep.got, Hq, Hkv, T, S, tab))

        Hq, Hkv, T, lens, S = dense_shape
        d = gp.pda_to_device(host.pda_make_problem("dense", Hq, Hkv, T, lens, seed=seed), device)
        args = (d["q"], d["k_pool"], d["v_pool"], d["block_table"], d["seq_lens"])
        got_o = gp.pda_fwd(*args, splits=S)
        ref = gp.pda_reference_gpu(*args)
        err = (got_o.float() - ref["o32"]).abs().double().cpu().numpy().reshape(-1)
        a = ref["a"].double().cpu().numpy().reshape(-1)
        out["dense_worst"] = float((err / np.maximum(a, 1e-30)).max())
        bad = np.flatnonzero(~(err <= host.pda_tolerance(a)))
        if bad.size:
            out["bad"]["dense"] += int(bad.size)
            w = host.pda_locate("O", int(bad[0]) // 2, Hq, Hkv, T, S)
            out["failures"].append(
                f"gpu{gpu}: pda dense O: seq {w['b']} head {w['h']} tok {w['t']} col {int(bad[0]) % 128}: "
                f"error {err[bad[0]]:.3e} above 2^-7 a + 2^-20 = {host.pda_tolerance(a[bad[0]]):.3e}; {bad.size} beyond")

        if timed_shape:
            Hq, Hkv, T, lens, S = timed_shape
            d = gp.pda_to_device(host.pda_make_problem("dense", Hq, Hkv, T, lens, seed=seed), device)
            args = (d["q"], d["k_pool"], d["v_pool"], d["block_table"], d["seq_lens"])
            buf = torch.empty_like(d["q"])
            secs = _wall_time(lambda: gp.pda_fwd(*args, splits=S, out=(buf, None, None)), iters, device)
            out["pda_kv_gbps"] = host.pda_kv_bytes(lens, Hkv) * iters / secs / 1e9
    out["xcds"], out["cus"] = len({s[0] for s in seen}), len(seen)
    return verdict(out, t_begin)
