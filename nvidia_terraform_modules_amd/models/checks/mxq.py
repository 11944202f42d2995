"""K11: the Job's MX quantise / dequantise check."""
from __future__ import annotations

import time

import torch

from .._timing import _wall_time
from ._common import begin, verdict


def mxq_check(device: torch.device, rows: int = 1024, cols: int = 4096, e2e: int = 512, big: int = 0, iters: int = 3,
              corrupt: bool = False, seed: int = 0x4B3B) -> dict:
    """K11, the Job's MX quantise / dequantise check (``NTM_MXQ_CHECK=1``) on ``device``, in the
    Job's sequence: per format of ``ops.MX_FORMATS`` the conversion sweeps (down from fp32 and
    from every finite normal bf16 code through ``mxq_cvt``, up through ``mx_dequantize``) and a
    block quantise of a ``rows`` x ``cols`` fp32 and bf16 matrix, each against the integer
    reference kernel, bitwise through ``mx_compare``; then, for e2m1, e2m3 and e4m3, the
    ``e2e``^3 product of operands quantised on the device against ``mx_reference_gpu`` on the
    host-packed ones; then, with ``big`` > 0 (the Job: 8192), ``iters`` timed fp32 -> e2m1
    quantises of ``big`` x ``big``. ``corrupt`` flips bit 4 of one packed e2m1 byte of the fp32
    block quantise before its compare. Returns ``ok``, ``failures`` (the Job's lines), ``bad``
    per format, ``quantize_gbps`` (host clock around a synchronise: the Job's figure is the one
    to quote) and ``seconds``."""
    o, device, gpu = begin(device)
    t_begin = time.perf_counter()
    out = {"bad": {f: 0 for f in o.MX_FORMATS}, "failures": [], "quantize_gbps": 0.0}

    def words(t):
        flat = t.contiguous().view(torch.uint8).view(-1)
        pad = -flat.numel() % 4
        if pad:
            flat = torch.cat([flat, torch.zeros(pad, dtype=torch.uint8, device=flat.device)])
        return flat.view(torch.int32)

    def judge(fmt, sub, expected, got, row_words, elem_bits):
        rep = o.mx_compare(words(expected), words(got))
        if not rep.ok:
            out["bad"][fmt] += rep.count
            if not any(f.startswith(f"gpu{gpu}: mxq {fmt} {sub}:") for f in out["failures"]):
                out["failures"].append(o.mxq_failure_message(gpu, fmt, sub, rep.count, rep.first_index, rep.expected,
                                                             rep.got, row_words, elem_bits))

    def u8(a):
        return torch.from_numpy(a.copy()).to(device)

    with torch.cuda.device(device):
        for fmt in o.MX_FORMATS:
            bits = o.mx_bits(fmt)
            for kind in ("down", "down_bf16"):
                i = o.mxq_make_inputs(kind, fmt)
                x, s = o.mxq_to_device(i["x"], device, bf16=kind == "down_bf16"), u8(i["scales"][:, None])
                judge(fmt, "down", o.mxq_cvt(x, s, fmt, reference=True), o.mxq_cvt(x, s, fmt), bits, bits)
            i = o.mxq_make_inputs("up", fmt)
            p, s = u8(i["packed"]), u8(i["scales"])
            judge(fmt, "up", o.mx_dequantize_reference_gpu(p, s, fmt), o.mx_dequantize(p, s, fmt), i["kept"].shape[1], 32)
            for bf16 in (False, True):
                x = o.mxq_to_device(o.mxq_make_inputs("block", fmt, rows, cols, seed=seed + gpu, bf16=bf16)["x"], device, bf16)
                p, s = o.mx_quantize(x, fmt)
                if corrupt and fmt == "e2m1" and not bf16:
                    p.view(-1)[(p.numel() // 2 & ~3) + 64] ^= 1 << 4
                pr, sr = o.mx_quantize_reference_gpu(x, fmt)
                judge(fmt, "block", pr, p, cols * bits // 32, bits)
                judge(fmt, "scale", sr, s, max(cols // 128, 1), 8)
        for fmt in ("e2m1", "e2m3", "e4m3"):
            g = o.mxq_make_inputs("grid", fmt, e2e, e2e, N=e2e, seed=seed + gpu, W=max(o.mx_max_spread(fmt, e2e), 0))
            a, sa = o.mx_quantize(o.mxq_to_device(g["xa"], device), fmt)
            b, sb = o.mx_quantize(o.mxq_to_device(g["xb"], device), fmt)
            # no e4m3 product is exact by mx_dense_exact: its answer is mx_gemm on the host-packed operands
            answer = o.mx_gemm if fmt == "e4m3" else o.mx_reference_gpu
            judge(fmt, "e2e", answer(u8(g["a"]), u8(g["b"]), u8(g["sa"]), u8(g["sb"]), fmt),
                  o.mx_gemm(a, b, sa, sb, fmt), e2e, 32)
        if big:
            x = torch.full((big, big), 0.0115, dtype=torch.float32, device=device)
            p, s = o.mx_quantize(x, "e2m1")
            secs = _wall_time(lambda: o.mx_quantize(x, "e2m1", packed=p, scales=s), iters, device)
            out["quantize_gbps"] = (x.numel() * 4 + p.numel() + s.numel()) * iters / secs / 1e9
    return verdict(out, t_begin)
