"""K13: the Job's fused attention check with exact answers."""
from __future__ import annotations

import time

import numpy as np
import torch

from ...ops import attn as host
from .._timing import _wall_time
from ._common import device_context, verdict


def attn_check(device: torch.device, exact_shape: tuple = (1, 4, 2, 129, 191), dense_shape: tuple = (2, 4, 2, 320, 320),
               timed_shape: tuple | None = None, iters: int = 3, backend=None, corrupt: bool = False,
               seed: int = 0x4B3D) -> dict:
    """K13, the Job's fused attention check (``NTM_ATTN_CHECK=1``) on ``device``, in the Job's
    sequence; shapes are (B, Hq, Hkv, Sq, Sk). *Exact*: ``ops.attn`` exact inputs of
    ``exact_shape`` (the Job: enough query tiles for every CU), causal and not, O, m and l
    bitwise against the reference kernel. *Dense*: uniform bf16 of ``dense_shape``, causal and
    not, every element within ``attn_tolerance(a)`` of the reference's fp32 O. *Timed*: with
    ``timed_shape`` (the Job: (4, 32, 8, 4096, 4096)) ``iters`` causal launches. ``corrupt``
    flips bit 3 of one O element of the first exact run before its compare. Returns ``ok``,
    ``failures`` (the Job's lines), ``bad`` per sub-test, ``dense_worst`` (largest err / a),
    ``xcds`` and ``cus`` seen in the CU table, ``attn_tflops`` (host clock around a
    synchronise, never judged) and ``seconds``. ``backend=ops.attn.CPU_BACKEND`` runs the numpy
    emulation of the kernel's arithmetic contract in place of the kernel."""
    device = torch.device(device)
    gpu = device.index if device.index is not None else 0
    if backend is None:
        from ...ops.gpu import attn as backend
    o = backend
    t_begin = time.perf_counter()
    out = {"bad": {"exact": 0, "exact_causal": 0, "dense": 0, "dense_causal": 0}, "failures": [], "dense_worst": 0.0,
           "attn_tflops": 0.0, "xcds": 0, "cus": 0}
    seen = set()

    with device_context(device):
        B, Hq, Hkv, Sq, Sk = exact_shape
        i = host.attn_make_inputs("exact", B, Hq, Hkv, Sq, Sk, seed=seed)
        d = o.attn_to_device(i, device)
        for causal in (False, True):
            if not host.attn_exact(i["qi"], i["ki"], i["vi"], causal):
                raise ValueError("attn_check: the exact inputs break attn_exact")
            sub = "exact causal" if causal else "exact"
            got_o, got_m, got_l, table = o.attn_fwd(d["q"], d["k"], d["v"], causal=causal, scale_log2=1.0,
                                                    return_stats=True, table=True)
            ref = o.attn_reference_gpu(d["q"], d["k"], d["v"], causal=causal, scale_log2=1.0)
            if corrupt and not causal:
                got_o.view(torch.int16).view(-1)[got_o.numel() // 2 + 5] ^= 1 << 3
            tab = table.cpu().numpy().view(np.uint32)
            seen |= {host.attn_decode_cu(int(hw), int(xcc)) for hw, xcc in tab}
            for what, e, g in (("O", ref["o"], got_o), ("m", ref["m"], got_m), ("l", ref["l"], got_l)):
                rep = o.attn_compare(e, g)
                if not rep.ok:
                    out["bad"][sub.replace(" ", "_")] += rep.count
                    out["failures"].append(host.attn_failure_message(gpu, sub, what, rep.count, rep.first_index,
                                                                     rep.expected, rep.got, Hq, Sq, tab))

        B, Hq, Hkv, Sq, Sk = dense_shape
        d = o.attn_to_device(host.attn_make_inputs("dense", B, Hq, Hkv, Sq, Sk, seed=seed), device)
        for causal in (False, True):
            sub = "dense causal" if causal else "dense"
            got_o = o.attn_fwd(d["q"], d["k"], d["v"], causal=causal)
            ref = o.attn_reference_gpu(d["q"], d["k"], d["v"], causal=causal)
            err = (got_o.float() - ref["o32"]).abs().double().cpu().numpy().reshape(-1)
            a = ref["a"].double().cpu().numpy().reshape(-1)
            out["dense_worst"] = max(out["dense_worst"], float((err / np.maximum(a, 1e-30)).max()))
            bad = np.flatnonzero(~(err <= host.attn_tolerance(a)))
            if bad.size:
                out["bad"][sub.replace(" ", "_")] += int(bad.size)
                w = host.attn_locate("O", int(bad[0]) // 2, Hq, Sq)
                out["failures"].append(
                    f"gpu{gpu}: attn {sub} O: batch {w['b']} head {w['h']} row {w['row']} col {int(bad[0]) % 128}: "
                    f"error {err[bad[0]]:.3e} above 2^-7 a + 2^-20 = {host.attn_tolerance(a[bad[0]]):.3e}; {bad.size} beyond")

        if timed_shape:
            B, Hq, Hkv, Sq, Sk = timed_shape
            d = o.attn_to_device(host.attn_make_inputs("dense", B, Hq, Hkv, Sq, Sk, seed=seed), device)
            buf = torch.empty_like(d["q"])
            secs = _wall_time(lambda: o.attn_fwd(d["q"], d["k"], d["v"], causal=True, out=(buf, None, None)), iters, device)
            out["attn_tflops"] = host.attn_flops(B, Hq, Sq, Sk, True) * iters / secs / 1e12
    out["xcds"], out["cus"] = len({s[0] for s in seen}), len(seen)
    return verdict(out, t_begin)
