"""The flagship workload: the post-provision GPU validation Job.

This is what the Kubernetes Job created by ``modules/amd-gpu-stack``
(``kubernetes_job_v1.gpu_validation``) runs on every MI355X it is granted, and
what ``bench.py`` times. It replaces the NVIDIA operator-validator's CUDA
``vectorAdd`` (implicit in /root/reference/eks/main.tf:185-203) with:

* K1 - hand-written bf16 MFMA GEMM (TFLOP/s, fully verified against an
  independent fp32 FMA reference once, then ABFT row-checksummed on every
  checked launch through the fused epilogue - cheap enough to run always),
* K2 - HBM stream bandwidth + capacity check (288 GB class),
* C1 - RCCL all-reduce sweep over xGMI (every element checked),

and fails (non-zero exit / ``passed = False``) on: HIP error, verification
mismatch, TFLOP/s below a floor, HBM below the capacity floor, all-reduce
mismatch. Fault-injection hooks (env ``NTM_FAULT_INJECT``) corrupt one
rank's data to prove the detector fires (failure detection).
"""
from __future__ import annotations

import contextlib
import os
import time
from dataclasses import asdict, dataclass, field

import torch

from ..gpu_ready.phases import PhaseClock
from ..parallel import collectives as coll
from ..parallel.dist import DistEnv, all_reduce_max, all_reduce_sum, barrier

GiB = 1 << 30


@dataclass
class ValidationConfig:
    size: int = 8192                # M = N = K of the K1 GEMM, per GPU
    seed: int = 20250117
    gemm_iters: int = 50            # timed K1 launches for the TFLOP/s figure
    gemm_warmup: int = 5
    check: bool = True              # full-matrix verification vs fp32 reference
    abft_iters: int = 3             # checksum-verified K1 launches (0 = off)
    hbm_bytes: int = 2 * GiB        # K2 copy size (src + dst = 2x this)
    hbm_iters: int = 10
    allreduce_min_bytes: int = 1 << 20
    allreduce_max_bytes: int = 1 << 30
    allreduce_iters: int = 10
    tflops_floor: float = 0.0       # fail below this (0 = report only)
    hbm_floor_GBps: float = 0.0
    min_hbm_capacity_gb: float = 0.0  # 250 on MI355X (288 GB HBM3E per GPU)
    fault_inject: str = field(default_factory=lambda: os.environ.get("NTM_FAULT_INJECT", ""))


class GemmWorkload:
    """Device-resident K1 operands (A: [M,K], B: [N,K], C: [M,N], bf16).

    Operands are generated ON the device by the hash RNG (no host copy), one
    distinct seed per rank so ranks cannot agree by accident.
    """

    def __init__(self, size: int, device: torch.device, seed: int, backend=None):
        from .. import ops  # native; raises if the .so is missing

        self.ops = backend or ops
        self.m = self.n = self.k = size
        if not self.ops.gemm_shape_ok(self.m, self.n, self.k):
            raise ValueError(f"size {size} is not a multiple of 256 (K >= 128)")
        self.device = device
        self.a = torch.empty((self.m, self.k), dtype=torch.bfloat16, device=device)
        self.b = torch.empty((self.n, self.k), dtype=torch.bfloat16, device=device)
        self.c = torch.empty((self.m, self.n), dtype=torch.bfloat16, device=device)
        self.ops.fill_uniform_(self.a, seed=seed * 2 + 1)
        self.ops.fill_uniform_(self.b, seed=seed * 2 + 2)
        self.rowsum = torch.empty(self.m, dtype=torch.float32, device=device)
        # the K1 build step() runs: "default" = the plan; bench.select_k1 may pick
        # another hand-written build that is faster on this box
        self.variant = "default"

    @property
    def flops(self) -> float:
        return 2.0 * self.m * self.n * self.k

    def step(self) -> None:
        if self.variant == "default":
            self.ops.gemm_bf16(self.a, self.b, self.c)
        else:
            self.ops.gemm_bf16(self.a, self.b, self.c, variant=self.variant)

    def step_checked(self) -> None:
        """K1 with the fused ABFT row-checksum epilogue."""
        self.ops.gemm_bf16_rowsum(self.a, self.b, self.c, self.rowsum)

    def abft(self, corrupt: bool = False):
        """Check the last ``step_checked`` output in O(n^2)."""
        if corrupt:
            self.c.view(-1)[4321 % self.c.numel()] += 256.0
        return self.ops.abft_check(self.a, self.b, self.c, self.rowsum)

    def verify(self, corrupt: bool = False):
        if corrupt:
            self.c.view(-1)[12345 % self.c.numel()] += 1.0
        ref = self.ops.ref_gemm_f32(self.a, self.b)
        atol, rtol = self.ops.gemm_tolerance(self.k)
        rep = self.ops.verify_bf16(self.c, ref, atol, rtol)
        del ref
        return rep


def _sync(device: torch.device) -> None:
    if device.type == "cuda":
        torch.cuda.synchronize(device)


def _time_loop(fn, iters: int, device: torch.device) -> float:
    """Seconds per call: events on the current stream (wall clock on CPU)."""
    if device.type != "cuda":
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        return (time.perf_counter() - t0) / iters
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize(device)
    return s.elapsed_time(e) / 1e3 / iters


def hbm_check(device: torch.device, nbytes: int, iters: int, backend=None) -> dict:
    from .. import ops as native

    o = backend or native
    if device.type == "cuda":
        free, total = torch.cuda.mem_get_info(device)
    else:  # rehearsal: host memory stands in, capacity not meaningful
        free, total = 4 * nbytes, 0
    nbytes = min(nbytes, int(free * 0.4)) // 16 * 16
    src = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
    dst = torch.empty_like(src)
    src.uniform_()
    o.stream_copy(src, dst)
    _sync(device)
    copy_ok = bool(torch.equal(src, dst))
    sink = torch.zeros(2048, dtype=torch.float32, device=device)
    t_copy = _time_loop(lambda: o.stream_copy(src, dst), iters, device)
    t_read = _time_loop(lambda: o.stream_read(src, sink), iters, device)
    del src, dst
    return {
        "bytes": nbytes,
        "copy_GBps": 2 * nbytes / t_copy / 1e9,
        "read_GBps": nbytes / t_read / 1e9,
        "copy_ok": copy_ok,
        "capacity_total_gb": total / 1e9,
        "capacity_free_gb": free / 1e9,
    }


def hbm_memtest(device: torch.device, nbytes: int, passes: int = 1, chunk_bytes: int = GiB,
                backend=None) -> dict:
    """K4, the Job's HBM pattern test (``amdgpu-validate --hbm-test-gb``) on ``nbytes``
    of ``device``, in chunks of ``chunk_bytes`` that share one logical address space.

    Per pass: write ADDR to every chunk / verify it and invert in place / verify the
    inverted pattern / write HASH with seed = pass / verify. A chunk is written completely
    before it is read back, so chunks should be far larger than the caches (the Job keeps
    them >= 1 GiB). The first step that finds a bad word ends the test. Memory that
    cannot be allocated shortens the test (``bytes`` < ``requested_bytes``).

    Unlike the Job, which enqueues a whole step and reads one error record per step,
    this model checks per chunk: each ``hbm_pattern_verify`` allocates its own record and
    copies it to the host. ``verify_GBps`` therefore includes one synchronisation per chunk
    and reads low with small chunks; the Job's ``hbm_test_verify_GBps`` is the rate to quote."""
    from .. import ops as native

    o = backend or native
    nbytes, chunk_bytes = nbytes // 16 * 16, max(16, chunk_bytes // 16 * 16)
    t_begin = time.perf_counter()
    chunks, base = [], 0
    while base < nbytes:
        c = min(chunk_bytes, nbytes - base)
        try:
            chunks.append((torch.empty(c // 4, dtype=torch.int32, device=device), base))
        except RuntimeError:           # out of memory: test what could be had
            break
        base += c
    tested = sum(t.numel() * 4 for t, _ in chunks)
    out = {"requested_bytes": nbytes, "bytes": tested, "chunks": len(chunks), "passes": passes,
           "bad_words": 0, "bad_bits": 0, "first_bad_offset": None, "records": [],
           "failed_step": None, "write_GBps": 0.0, "verify_GBps": 0.0}
    secs = {"write": 0.0, "verify": 0.0}
    count = {"write": 0, "verify": 0}

    def step(name: str, kind: str, pattern: int, seed: int, invert: bool) -> bool:
        t0 = time.perf_counter()
        reps = []
        for t, b in chunks:
            if kind == "write":
                o.hbm_pattern_write(t, pattern, seed=seed, invert=invert, base=b)
            else:
                reps.append(o.hbm_pattern_verify(t, pattern, seed=seed, invert=invert, base=b,
                                                 invert_after=kind == "verify_invert"))
        _sync(device)
        if kind in secs:
            secs[kind] += time.perf_counter() - t0
            count[kind] += 1
        bad = [r for r in reps if not r.ok]
        if bad:
            out["bad_words"] = sum(r.bad_words for r in bad)
            for r in bad:
                out["bad_bits"] |= r.bad_bits
            out["first_bad_offset"] = min(r.first_bad_offset for r in bad)
            out["records"] = sorted((x for r in bad for x in r.records),
                                    key=lambda x: x["offset"])[:4]
            out["failed_step"] = name
        return not bad

    for p in range(passes):
        step("addr write", "write", 0, 0, False)
        if not (step("addr verify+invert", "verify_invert", 0, 0, False)
                and step("addr inverted verify", "verify", 0, 0, True)):
            break
        step("hash write", "write", 1, p, False)
        if not step("hash verify", "verify", 1, p, False):
            break
    for k in secs:
        if secs[k] > 0:
            out[f"{k}_GBps"] = tested * count[k] / secs[k] / 1e9
    del chunks
    out["ok"] = tested > 0 and out["bad_words"] == 0
    out["seconds"] = time.perf_counter() - t_begin
    return out


def cu_sweep_check(device: torch.device, iters: int = 16, lds_bytes: int | None = None,
                   seed: int = 0, max_launches: int | None = None, fault_key: int | None = None,
                   fault_subtest=None, backend=None) -> dict:
    """K5, the Job's per-CU compute sweep (``amdgpu-validate --cu-sweep``) on ``device``:
    launches of 4 workgroups per CU, each running ``iters`` rounds of the known-answer
    lds / valu / mfma_bf16 / mfma_fp8 sub-tests, until every CU ran a workgroup or
    ``max_launches`` (8) are spent - a cap, not a retry. Returns the summary of
    ``ops.cu_sweep_summarize`` (``ok``, ``cus``, ``cus_covered``, ``simds_covered``,
    ``launches``, ``bad_cus``, ``message`` ...) plus ``lds_bytes`` and ``seconds``. A CU that
    ran nothing fails the check; SIMD coverage is reported only."""
    import numpy as np

    from .. import ops as native
    from ..ops.kernels import CU_SWEEP_MAX_LAUNCHES

    o = backend or native
    device = torch.device(device)
    cap = CU_SWEEP_MAX_LAUNCHES if max_launches is None else max_launches
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    lds = o.cu_sweep_max_lds_bytes(device) if lds_bytes is None else lds_bytes
    t0 = time.perf_counter()
    recs, launches = [], 0
    for launch in range(cap):
        recs.append(o.cu_sweep(device, iters=iters, lds_bytes=lds, seed=seed + launch,
                               fault_key=fault_key, fault_subtest=fault_subtest))
        launches += 1
        if o.cu_sweep_summarize(np.concatenate(recs), cus, launches)["cus_covered"] >= cus:
            break
    gpu = device.index if device.index is not None else 0
    out = o.cu_sweep_summarize(np.concatenate(recs), cus, launches, gpu=gpu)
    out["lds_bytes"] = lds
    out["iters"] = iters
    out["seconds"] = time.perf_counter() - t0
    return out


def host_link_check(device: torch.device, nbytes: int = 64 << 20, iters: int = 3,
                    backend=None) -> dict:
    """K6, the Job's host-link (PCIe) check (``amdgpu-validate --host-link-mib``) on
    ``device`` with one pinned host buffer and one HBM buffer of ``nbytes``: push the HASH
    pattern (device->host), pull and verify it on the device (host->device), push into one
    half while pulling from the other on two streams, ``copy_`` (hipMemcpyAsync) both ways
    on the same buffers, then the pointer chase over 1024 slots and 4096 hops. Rates are
    medians of ``iters``.

    Unlike the Job, which times each kernel with events and reads the error record once
    per pull, this model synchronises per call, as ``hbm_memtest`` documents for K4: each
    ``host_link_pull`` allocates its own record and copies it to the host, and the timings
    are host clocks around a synchronise. The rates therefore read a little low at small
    ``nbytes``; the Job's ``host_link_*_GBps`` are the rates to quote. With
    ``backend=ops.reference`` (CPU) nothing crosses a link and the rates mean nothing."""
    import numpy as np

    from .. import ops as native
    from ..ops import reference

    o = backend or native
    device = torch.device(device)
    gpu = device.type == "cuda"
    nbytes = max(nbytes // 32 * 32, 1024 * reference.HOST_LINK_SLOT_BYTES)
    half = nbytes // 2
    seed = 0x4B36
    t_begin = time.perf_counter()
    host = torch.empty(nbytes // 4, dtype=torch.int32, pin_memory=gpu)
    dev_buf = torch.empty(nbytes // 4, dtype=torch.int32, device=device)
    out = {"bytes": nbytes, "bad_words": 0, "bad_bits": 0, "first_bad_offset": None, "records": [],
           "failed_step": None, "duplex_GBps": 0.0, "h2d_copy_GBps": 0.0, "d2h_copy_GBps": 0.0,
           "read_latency_us": 0.0, "chase_ok": None}

    def timed(fn) -> float:
        _sync(device)
        t0 = time.perf_counter()
        fn()
        _sync(device)
        return time.perf_counter() - t0

    def bad(rep, step: str) -> bool:
        if rep.ok:
            return False
        out.update(bad_words=rep.bad_words, bad_bits=rep.bad_bits, records=rep.records,
                   first_bad_offset=rep.first_bad_offset, failed_step=step)
        return True

    def rate(n: int, secs: list) -> float:
        return n / float(np.median(secs)) / 1e9

    ctx = torch.cuda.device(device) if gpu else contextlib.nullcontext()
    with ctx:
        out["d2h_GBps"] = rate(nbytes, [timed(lambda: o.host_link_push(host, 1, seed=seed))
                                        for _ in range(iters)])
        secs, reps = [], []
        for _ in range(iters):
            secs.append(timed(lambda: reps.append(o.host_link_pull(host, 1, seed=seed))))
            if bad(reps[-1], "pull"):
                break
        out["h2d_GBps"] = rate(nbytes, secs)
        if out["failed_step"] is None:
            lo, hi = host[: half // 4], host[half // 4:]
            side = torch.cuda.Stream(device) if gpu else None

            def duplex():
                o.host_link_push(lo, 1, seed=seed)
                if side is None:
                    reps.append(o.host_link_pull(hi, 1, seed=seed, base=half))
                else:
                    with torch.cuda.stream(side):
                        reps.append(o.host_link_pull(hi, 1, seed=seed, base=half))

            secs = [timed(duplex) for _ in range(iters)]
            out["duplex_GBps"] = rate(2 * half, secs)
            bad(reps[-1], "duplex pull")
            out["h2d_copy_GBps"] = rate(nbytes, [timed(lambda: dev_buf.copy_(host, non_blocking=True))
                                                 for _ in range(iters)])
            out["d2h_copy_GBps"] = rate(nbytes, [timed(lambda: host.copy_(dev_buf, non_blocking=True))
                                                 for _ in range(iters)])
            table = reference.host_link_chase_table(1024, seed)
            slots = host[: table.size * 2]
            slots.view(torch.int64).copy_(torch.from_numpy(table.view(np.int64).reshape(-1)))
            final, ns = o.host_link_chase(slots, 4096)
            want, _ = reference.host_link_chase(slots, 4096)
            out["chase_ok"] = final == want
            out["read_latency_us"] = ns / 1e3
            if final != want and out["failed_step"] is None:
                out["failed_step"] = "chase"
    del host, dev_buf
    out["ok"] = out["bad_words"] == 0 and out["failed_step"] is None
    out["seconds"] = time.perf_counter() - t_begin
    return out


def mx_check(device: torch.device, size: int = 512, iters: int = 3, backend=None,
             corrupt: bool = False) -> dict:
    """K7, the Job's MX block-scaled matrix check (``amdgpu-validate --mx-check``) on
    ``device``: the decode sweep of all five formats (256 x 128 x 128, all 15 scale windows)
    against the exact integer table, dense e2m3 (``size`` x ``size`` x 512) and dense e2m1
    (``size``^3) with the largest exact scale spread against the reference kernel, every
    element compared bitwise, then ``iters`` timed e2m1 products. ``corrupt`` flips one bit
    of one element of the dense e2m1 result before its compare.

    Unlike the Job, which times with events after a settle, the timing here is a host clock
    around a synchronise: the Job's ``mx_fp4_tflops`` is the rate to quote. With
    ``backend=ops.reference`` (CPU) every product is the integer reference itself and the
    rate means nothing."""
    import numpy as np

    from .. import ops as native
    from ..ops import mx

    o = backend or native
    device = torch.device(device)
    t_begin = time.perf_counter()
    out = {"size": size, "formats": [], "bad_elements": 0, "first": None, "failed_step": None,
           "fp4_tflops": 0.0, "scale_spread": mx.mx_max_spread("e2m1", size)}
    clean = {f: True for f in mx.MX_FORMATS}

    def put(i: dict) -> dict:
        return {k: torch.from_numpy(i[k]).to(device) for k in ("a", "b", "sa", "sb")}

    def judge(rep, fmt: str, mode: str, n_cols: int) -> None:
        if rep.ok:
            return
        out["bad_elements"] += rep.count
        clean[fmt] = False
        if out["first"] is None:
            out["failed_step"] = f"{fmt} {mode}"
            out["first"] = {"format": fmt, "mode": mode, "row": rep.first_index // n_cols,
                            "col": rep.first_index % n_cols, "expected": rep.expected, "got": rep.got}

    ctx = torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()
    with ctx:
        for fmt in mx.MX_FORMATS:
            for window in range(mx.MX_DECODE_WINDOWS):
                i = mx.mx_make_inputs("decode", fmt, 256, 128, 128, seed=window)
                want = torch.from_numpy(mx.mx_matmul_bits(i["a"], i["b"], i["sa"], i["sb"], fmt)
                                        .view(np.int32)).to(device)
                d = put(i)
                judge(o.mx_compare(want, o.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], fmt)), fmt, "decode", 128)
        w6 = mx.mx_max_spread("e2m3", 512)
        d = put(mx.mx_make_inputs("dense", "e2m3", size, size, 512, seed=0x4B37, W=w6))
        judge(o.mx_compare(o.mx_reference_gpu(d["a"], d["b"], d["sa"], d["sb"], "e2m3"),
                           o.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m3")), "e2m3", "dense", size)
        if out["scale_spread"] < 0:
            raise ValueError(f"no exact scale spread for e2m1 at size {size}")
        d = put(mx.mx_make_inputs("dense", "e2m1", size, size, size, seed=0x4B37, W=out["scale_spread"]))
        c = o.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m1")
        if corrupt:
            c.view(torch.int32).view(-1)[c.numel() // 2 + 5] ^= 1 << 3
        judge(o.mx_compare(o.mx_reference_gpu(d["a"], d["b"], d["sa"], d["sb"], "e2m1"), c),
              "e2m1", "dense", size)
        _sync(device)
        t0 = time.perf_counter()
        for _ in range(iters):
            o.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m1", out=c)
        _sync(device)
        out["fp4_tflops"] = 2.0 * size**3 * iters / (time.perf_counter() - t0) / 1e12
    out["formats"] = [f for f in mx.MX_FORMATS if clean[f]]
    out["ok"] = out["bad_elements"] == 0
    out["seconds"] = time.perf_counter() - t_begin
    return out


def mcore_check(device: torch.device, size: int = 512, big: int = 0, iters: int = 3, backend=None,
                corrupt: bool = False, seed: int = 0x4B3A, max_windows: int | None = None) -> dict:
    """K10, the Job's matrix-core check of the formats K1 and K7 never issue
    (``NTM_MCORE_CHECK=1``) on ``device``, in the Job's sequence: per format of
    ``ops.MCORE_FORMATS`` the decode sweep (256 x 128 x 128, every window) and a dense
    ``size``^3 with the widest operands ``mcore_exact`` allows, each against the reference
    kernel, bitwise; then, with ``big`` > 0 (the Job: 4096), a verified dense ``big``^3 for
    f64 and i8 and ``iters`` timed launches of it. ``corrupt`` flips bit 9 of one element of
    the dense f64 result before its compare; ``max_windows`` cuts every format's decode sweep
    short (the Job runs them all). Returns ``ok``, ``failures`` (the Job's lines),
    ``bad`` per format, ``f64_tflops`` / ``i8_tops`` (host clock around a synchronise: the
    Job's figures are the ones to quote) and ``seconds``. With ``backend=ops.reference`` (CPU)
    every product is the numpy reference itself."""
    from .. import ops as native

    o = backend or native
    device = torch.device(device)
    gpu = device.index if device.index is not None else 0
    t_begin = time.perf_counter()
    out = {"size": size, "bad": {f: 0 for f in o.MCORE_FORMATS}, "failures": [], "f64_tflops": 0.0, "i8_tops": 0.0}

    def product(i: dict, mode: str, flip: bool = False):
        d = o.mcore_to_device(i, device)
        fmt = o.MCORE_FORMATS[i["fmt"]]
        c = o.mcore_gemm(d["a"], d["b"], fmt, d["ai"])
        if flip:
            c.view(torch.int32).view(-1)[2 * (c.numel() // 2 + 5)] ^= 1 << 9
        rep = o.mcore_compare(o.mcore_reference_gpu(d["a"], d["b"], fmt, d["ai"]), c)
        if not rep.ok:
            out["bad"][fmt] += rep.count
            if not any(f.startswith(f"gpu{gpu}: mcore: {fmt} {mode}:") for f in out["failures"]):
                out["failures"].append(o.mcore_failure_message(gpu, fmt, mode, rep.count, rep.first_index,
                                                               rep.expected, rep.got, i["N"]))
        return d, c

    ctx = torch.cuda.device(device) if device.type == "cuda" else contextlib.nullcontext()
    with ctx:
        for fmt in o.MCORE_FORMATS:
            for window in range(min(o.mcore_decode_windows(fmt), max_windows or 1 << 30)):
                product(o.mcore_make_inputs("decode", fmt, 256, 128, 128, seed=window), "decode")
            product(o.mcore_make_inputs("dense", fmt, size, size, size, seed=seed), "dense",
                    flip=corrupt and fmt == "f64")
        for fmt, key in (("f64", "f64_tflops"), ("i8", "i8_tops")) if big else ():
            d, c = product(o.mcore_make_inputs("dense", fmt, big, big, big, seed=seed), "dense")
            _sync(device)
            t0 = time.perf_counter()
            for _ in range(iters):
                o.mcore_gemm(d["a"], d["b"], fmt, d["ai"], out=c)
            _sync(device)
            out[key] = 2.0 * big**3 * iters / (time.perf_counter() - t0) / 1e12
    out["ok"] = not out["failures"]
    out["message"] = out["failures"][0] if out["failures"] else ""
    out["seconds"] = time.perf_counter() - t_begin
    return out


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
    from .. import ops as o

    device = torch.device(device)
    gpu = device.index if device.index is not None else 0
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
            _sync(device)
            t0 = time.perf_counter()
            for _ in range(iters):
                o.mx_quantize(x, "e2m1", packed=p, scales=s)
            _sync(device)
            out["quantize_gbps"] = (x.numel() * 4 + p.numel() + s.numel()) * iters / (time.perf_counter() - t0) / 1e9
    out["ok"] = not out["failures"]
    out["message"] = out["failures"][0] if out["failures"] else ""
    out["seconds"] = time.perf_counter() - t_begin
    return out


def wave_check(device: torch.device, corrupt: str | None = None, seed: int = 0x4B3C, grid_per_cu: int = 2,
               max_launches: int = 8) -> dict:
    """K12, the Job's wave data-path and special-function check (``NTM_WAVE_CHECK=1``) on
    ``device``, in the Job's sequence: per family (lane, ldstr, valu) the reference kernel makes
    the expected table, then ``grid_per_cu`` workgroups per CU run the family against it, launch
    after launch until every CU ran it (``max_launches`` is a cap, not a retry); sfu: one digest
    per instruction and workgroup held to the majority's, then the distance of every result from
    the host's brackets. A workgroup whose digest is off is named by its CU, and a second, small
    launch (one workgroup on that CU, one on another) names the first input whose words differ.
    ``corrupt="lane"`` flips bit 10 of one result word of workgroup 0 before its compare;
    ``corrupt="sfu"`` makes every workgroup on one CU flip bit 10 of one v_exp_f32 word. Returns the Job's fields: ``wave_lane_bad``, ``wave_ldstr_bad``,
    ``wave_valu_bad``, ``wave_sfu_inconsistent``, ``wave_sfu_max_distance``,
    ``wave_sfu_beyond_bound``, ``wave_cus_covered``, ``wave_seconds``, and ``ok``, ``failures``."""
    import numpy as np

    from .. import ops as o
    from ..ops import wave as w

    if corrupt not in (None, "lane", "sfu"):
        raise ValueError("corrupt must be None, 'lane' or 'sfu'")
    device = torch.device(device)
    gpu = device.index if device.index is not None else 0
    t_begin = time.perf_counter()
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    grid = grid_per_cu * cus
    seed = (seed + gpu) & 0xFFFFFFFF
    out = {"failures": [], "wave_lane_bad": 0, "wave_ldstr_bad": 0, "wave_valu_bad": 0, "wave_sfu_inconsistent": 0,
           "wave_sfu_max_distance": {}, "wave_sfu_beyond_bound": 0}
    covered = []

    def where(r, t):
        h = int(r["hw_id"])
        return (int(r["xcc_id"]) & 15, (h >> 13) & 7, (h >> 12) & 1, (h >> 8) & 15, int(r["simd"][(t // 64) & 3]) & 3)

    def sweep(family, inputs, layout, expected, on_bad, fault=None, fault_key=None):
        seen, recs_all = set(), []
        for launch in range(max_launches):
            recs = o.wave_sweep(family, inputs, layout, expected, grid,
                                fault_wg=fault_key if fault_key is not None else 0 if fault is not None and launch == 0 else None,
                                fault_index=fault or 0)
            recs_all.append(recs)
            for r in recs:
                if r["magic"] != 0x4B31324B:
                    out["failures"].append(f"gpu{gpu}: wave {family}: a workgroup wrote no record")
                    continue
                seen.add((int(r["xcc_id"]) & 15, int(r["hw_id"]) & 0xFF00))
                if r["bad"]:
                    out[f"wave_{family}_bad"] += int(r["bad"])
                    if not any(f.startswith(f"gpu{gpu}: wave {family}") for f in out["failures"]):
                        out["failures"].append(on_bad(r, (~int(r["first"])) & 0xFFFFFFFF))
            if len(seen) >= cus:
                break
        covered.append(len(seen))
        return np.concatenate(recs_all)

    lanes = np.arange(256)
    with torch.cuda.device(device):
        # lane
        x = w.wave_hash32(seed, 0, lanes // 64, 0, lanes % 64)
        y = w.wave_hash32(seed, 1, lanes // 64, 0, lanes % 64)
        din = o.wave_to_device(np.concatenate([x, y]), device)
        ops_list = w.wave_lane_ops()
        exp = torch.cat([o.wave_lane_reference_gpu(i, None, din[:256], din[256:]) for i in range(len(ops_list))])
        fault = (8 + 15 + 2) * 256 + 2 * 64 + 19 if corrupt == "lane" else None      # row_shr:3 bound_ctrl:0, wave 2 lane 19
        sweep("lane", din, None, exp,
              lambda r, i: w.wave_failure_message(gpu, "lane", w.wave_lane_op_name(ops_list[i // 256]), where(r, i % 256), "lane",
                                                  i % 64, int(r["expected"]), int(r["got"])), fault)
        # ldstr
        imgs, exps = [], []
        for f, bits in enumerate(w.WAVE_TR_BITS):
            img = np.zeros(16384, np.uint8)
            st = w.wave_sweep_stride(bits)
            img[:64 * st] = w.wave_make_image(bits, 64, st, (seed + f) & 0xFFFFFFFF)
            imgs.append(img)
            exps.append(o.wave_tr_read_reference_gpu(bits, torch.from_numpy(img[:64 * st].copy()).to(device), st))
        base = np.cumsum([0] + [e.numel() for e in exps])

        def ldstr_line(r, i):
            f = int(np.searchsorted(base, i, side="right")) - 1
            bits = w.WAVE_TR_BITS[f]
            return w.wave_failure_message(gpu, "ldstr", f"tr_b{bits} stride {w.wave_sweep_stride(bits)}", where(r, i % 256),
                                          "element", i - int(base[f]), int(r["expected"]), int(r["got"]))
        sweep("ldstr", o.wave_to_device(np.concatenate(imgs).view(np.uint32), device), None, torch.cat(exps), ldstr_line)
        # valu
        cv = w.wave_cvt_inputs(seed, 1024)
        t3 = np.arange(768)
        abc = w.wave_hash32(seed, 2 + t3 // 256, (t3 // 64) & 3, 0, t3 % 64)
        din = o.wave_to_device(np.concatenate([abc, cv, cv[::-1]]), device)
        n = len(cv)
        exp = torch.cat([o.wave_valu("bitop3", din[:256], din[256:512], din[512:768], reference=True).reshape(-1),
                         o.wave_valu("cvt_pk_bf16", din[768:768 + n], din[768 + n:], reference=True)])
        sweep("valu", din, [n], exp,
              lambda r, i: w.wave_failure_message(gpu, "valu", f"bitop3:0x{i // 256:02x}" if i < 65536 else "cvt_pk_bf16_f32",
                                                  where(r, i % 256), "element", i % 256 if i < 65536 else i - 65536,
                                                  int(r["expected"]), int(r["got"])))
        # sfu
        lists = [w.wave_sfu_inputs(op)[0] for op in range(7)]
        d_all = o.wave_to_device(np.concatenate(lists), device)
        counts = [len(v) for v in lists]
        fault_key, fault_index = None, 1000
        if corrupt == "sfu":     # the CU workgroup 0 of a first launch ran on
            fault_key = o.wave_cu_key(o.wave_sweep("sfu", d_all, counts, None, grid)[0])
        recs = sweep("sfu", d_all, counts, None, None, fault=fault_index if fault_key is not None else None, fault_key=fault_key)
        recs = recs[recs["magic"] == 0x4B31324B]
        for op, name in enumerate(w.WAVE_SFU_OPS):
            vals, counts = np.unique(recs["digest"][:, op], return_counts=True)
            want = vals[np.argmax(counts)]
            off = recs[recs["digest"][:, op] != want]
            out["wave_sfu_inconsistent"] += len(off)
            if len(off) and not any(" sfu " in f for f in out["failures"]):
                wh, key = where(off[0], 0), o.wave_cu_key(off[0])
                line = (f"gpu{gpu}: wave sfu {name}: xcd {wh[0]} se {wh[1]} sh {wh[2]} cu {wh[3]}: digest "
                        f"{int(off[0]['digest'][op]):#x} differs from {int(want):#x} of the other workgroups (not seen again in "
                        "a second launch)")
                dx = o.wave_to_device(lists[op], device)
                there = o.wave_sfu_locate(op, dx, key, True, grid, max_launches, fault_key, fault_index)
                there = there and (there[0].cpu().numpy().view(np.uint32), there[1])
                other = o.wave_sfu_locate(op, dx, key, False, grid, max_launches, fault_key, fault_index)
                if there and other:
                    good = other[0].cpu().numpy().view(np.uint32)
                    diff = np.flatnonzero(good != there[0])
                    if len(diff):
                        i = int(diff[0])
                        wh = where(there[1], i % 256)
                        line = (f"gpu{gpu}: wave sfu {name}: xcd {wh[0]} se {wh[1]} sh {wh[2]} cu {wh[3]} simd {wh[4]} element {i} "
                                f"input 0x{int(lists[op][i]):08x}: expected 0x{int(good[i]):08x}, got 0x{int(there[0][i]):08x}, "
                                f"bad bits 0x{int(good[i]) ^ int(there[0][i]):08x}")[:199]
                out["failures"].append(line)
            dx = o.wave_to_device(lists[op], device)
            d = o.wave_sfu_distance(op, dx, o.wave_sfu(op, dx), w.WAVE_SFU_BOUND[name])
            out["wave_sfu_max_distance"][name] = {"d": d["max_d"], "judged": w.WAVE_SFU_BOUND[name] is not None,
                                                  "input": f"0x{int(lists[op][d['max_index']]) if d['max_d'] else 0:08x}"}
            if w.WAVE_SFU_BOUND[name] is not None and d["beyond"]:
                out["wave_sfu_beyond_bound"] += d["beyond"]
                out["failures"].append(f"gpu{gpu}: wave sfu {name}: {d['beyond']} result(s) beyond {w.WAVE_SFU_BOUND[name]} "
                                       f"step(s) of the bracket, first input 0x{int(lists[op][d['first_beyond']]):08x}")
    out["wave_cus_covered"] = min(covered)
    if out["wave_cus_covered"] < cus:
        out["failures"].append(f"gpu{gpu}: wave coverage: {cus - out['wave_cus_covered']} of {cus} CUs did not run every "
                               f"family after {max_launches} launches")
    out["ok"] = not out["failures"]
    out["message"] = out["failures"][0] if out["failures"] else ""
    out["wave_seconds"] = time.perf_counter() - t_begin
    return out


def xcd_sweep_check(device: torch.device, hbm_mib: int = 256, ratio: float = 0.0, seed: int = 0x4B38,
                    slow_xcd: int | None = None, slow_factor: int = 4, corrupt_xcd: int | None = None,
                    levels=("l2", "mall", "hbm", "mfma"), backend=None) -> dict:
    """K8, the Job's per-XCD sweep (``amdgpu-validate --xcd-sweep``) on ``device``: a buffer of
    ``xcds x hbm_mib`` MiB filled with K4's hash pattern; per level (``l2`` 1 MiB, ``mall``
    16 MiB, ``hbm`` ``hbm_mib`` per XCD) every XCD reads and verifies its own slice alone (one
    launch per XCD) and together (one launch); ``mfma`` is the clock probe under matrix load.
    Each cell runs once to warm up and to size its passes for spans of at least 100 us, then
    for the record. Returns ``ok``, ``failures``, ``seconds``, ``xcds`` and ``cells``: the
    summaries of ``ops.xcd_sweep_summarize`` keyed ``"<level>/<mode>"``, each with ``passes``.
    The ratio applies to the cells ``ops.xcd_sweep_gated`` names; the others are reported.
    ``corrupt_xcd`` flips one bit of that XCD's ``hbm`` slice before the ``hbm`` level."""
    import numpy as np

    from .. import ops as native

    o = backend or native
    device = torch.device(device)
    gpu = device.index if device.index is not None else 0
    xcds = o.xcd_sweep_xcds(device)
    t0 = time.perf_counter()
    buf = torch.empty(xcds * hbm_mib << 20, dtype=torch.uint8, device=device)
    o.hbm_pattern_write(buf, "hash", seed)
    slow = dict(slow_xcd=slow_xcd, slow_factor=slow_factor if slow_xcd is not None else 1)
    cells, failures = {}, []

    def run(level, mode, passes, r):
        masks = [1 << x for x in range(xcds)] if mode == "alone" else [(1 << xcds) - 1]
        if level == "mfma":
            recs = [o.xcd_sweep_mfma(device, batches=passes, xcd_mask=m, **slow) for m in masks]
            expected = 0
        else:
            mib = min({"l2": 1, "mall": 16}.get(level, hbm_mib), hbm_mib)
            part = buf[: xcds * mib << 20]
            recs = [o.xcd_sweep_read(part, "hash", seed, m, passes, **slow) for m in masks]
            expected = passes * (mib << 20) // (64 * 1024)
        out = o.xcd_sweep_summarize(np.concatenate(recs), level, mode, xcds, ratio=r, gpu=gpu,
                                    expected_tiles=expected)
        out["passes"] = passes
        return out

    for level in levels:
        if level == "hbm" and corrupt_xcd is not None:
            off = (corrupt_xcd * hbm_mib << 20) + (hbm_mib << 19) + 40
            buf[off] ^= 2
        for mode in ("alone", "together"):
            if level == "mfma" and mode == "alone":
                continue
            passes = {"l2": 64, "mall": 4, "hbm": 1, "mfma": 16}[level]
            def timed(c):       # the XCDs that timed something; one that ran nothing fails on its own
                return [p["span_ticks"] for p in c["per_xcd"] if p["span_ticks"]]

            cell = run(level, mode, passes, 0.0)
            for _ in range(2):
                spans = timed(cell)
                if spans and min(spans) < 10000:
                    passes = min(-(-passes * 2 * 10000 // min(spans)), 65536 if level == "mfma" else 1 << 20)
                cell = run(level, mode, passes, ratio if o.xcd_sweep_gated(level, mode) else 0.0)
                if not timed(cell) or min(timed(cell)) >= 10000:
                    break
            cells[f"{level}/{mode}"] = cell
            failures += cell["failures"]
    torch.cuda.synchronize(device)
    return {"ok": not failures, "failures": failures, "message": failures[0] if failures else "",
            "xcds": xcds, "hbm_mib": hbm_mib, "ratio": ratio, "cells": cells,
            "seconds": time.perf_counter() - t0}


def atomics_check(device: torch.device, slots: int = 4096, wg_per_cu: int = 2, iters: int = 4,
                  heads: int = 8, episodes: int | None = None, episode_size: int = 8, rounds: int = 3,
                  seed: int = 0x4B39, ops=None, corrupt_atomic: bool = False, stale_handoff: bool = False,
                  ticket_inject: int | None = None, backend=None) -> dict:
    """K9, the Job's atomics and cross-XCD hand-off check (``NTM_ATOMICS_CHECK=1``) on
    ``device``: every op of ``ops.ATOMIC_OPS`` on a table of ``slots`` words from
    ``wg_per_cu`` workgroups per CU, compared bitwise with the reference kernel's table; the
    ticket draw on ``heads`` counters; ``rounds`` rounds of the hand-off on ``episodes``
    episodes (default: one workgroup per CU) of ``episode_size`` workgroups. Float operands
    take the largest size the exactness bound allows, up to 255. Returns ``ok``,
    ``failures``, ``message``, ``rmw`` (per op), ``tickets``, ``handoff`` and ``seconds``.
    ``corrupt_atomic`` flips one bit of the fp32 table, ``stale_handoff`` makes one writer of
    the last round leave a line stale, ``ticket_inject`` is ``ops.atomics_tickets``' inject."""
    from .. import ops as native

    o = backend or native
    device = torch.device(device)
    gpu = device.index if device.index is not None else 0
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    xcds = max(1, o.xcd_sweep_xcds(device))
    grid = cus * wg_per_cu
    adds = grid * 256 * iters // slots
    t0 = time.perf_counter()
    failures, rmw = [], {}
    for op in ops or o.ATOMIC_OPS:
        max_abs = 1
        while max_abs < 255 and o.atomics_exact(op, adds, 2 * max_abs + 1):
            max_abs = 2 * max_abs + 1
        got = o.atomics_rmw(op, slots, grid, iters, seed, max_abs, device)
        if corrupt_atomic and op == "add_f32":
            got[slots // 2] ^= 1 << 9
        rmw[op] = o.atomics_summarize("rmw", gpu, op=op, got=got,
                                      expected=o.atomics_rmw_reference(op, slots, grid, iters, seed, max_abs, device))
        rmw[op]["max_abs"] = max_abs
        failures += rmw[op]["failures"]
    tk = o.atomics_tickets(heads, grid, iters, device, inject=ticket_inject)
    tickets = o.atomics_summarize("tickets", gpu, **{k: tk[k] for k in ("counters", "claim", "grid", "iters")})
    failures += tickets["failures"]
    episodes = episodes or cus // episode_size
    inject = (rounds, (episodes // 2) * episode_size + 1) if stale_handoff else None
    recs = o.atomics_handoff(episodes, episode_size, rounds, seed, device, inject=inject)
    handoff = o.atomics_summarize("handoff", gpu, records=recs, episodes=episodes, episode_size=episode_size,
                                  xcds=xcds, launches=rounds)
    failures += handoff["failures"]
    return {"ok": not failures, "failures": failures, "message": failures[0] if failures else "",
            "rmw": rmw, "tickets": tickets, "handoff": handoff, "xcds": xcds,
            "seconds": time.perf_counter() - t0}


@dataclass
class ValidationReport:
    rank: int
    world_size: int
    device_name: str
    gemm: dict
    hbm: dict
    allreduce: list
    phases: dict
    failures: list

    @property
    def passed(self) -> bool:
        return not self.failures

    def as_dict(self) -> dict:
        d = asdict(self)
        d["passed"] = self.passed
        return d


def run_validation(env: DistEnv, cfg: ValidationConfig, clock: PhaseClock | None = None,
                   with_hbm: bool = True, with_allreduce: bool = True,
                   backend=None) -> ValidationReport:
    """Run the whole validation Job on this rank's GPU; collective across ranks.

    ``backend`` defaults to the native gfx950 ops; ``ops.reference`` (CPU)
    is for rehearsing the multi-rank logic in tests only."""
    clock = clock or PhaseClock()
    dev = env.device
    if dev.type == "cuda":
        torch.cuda.init()
    _ = torch.empty(1, device=dev)
    clock.mark("hip_init")
    failures: list[str] = []
    fi = cfg.fault_inject

    wl = GemmWorkload(cfg.size, dev, cfg.seed + env.rank, backend=backend)
    _sync(dev)
    clock.mark("buffers_ready")
    wl.step()
    _sync(dev)
    clock.mark("first_kernel")

    gemm: dict = {"m": wl.m, "n": wl.n, "k": wl.k}
    if cfg.check:
        corrupt = fi == "corrupt_gemm" and env.rank == env.world_size - 1
        rep = wl.verify(corrupt=corrupt)
        gemm["verify"] = rep.as_dict()
        if not rep.ok:
            failures.append(f"gemm verification: {rep.bad} elements out of tolerance")
    for _ in range(cfg.gemm_warmup):
        wl.step()
    barrier(env)
    sec = _time_loop(wl.step, cfg.gemm_iters, dev)
    gemm["ms"] = sec * 1e3
    gemm["tflops"] = wl.flops / sec / 1e12
    if cfg.tflops_floor and gemm["tflops"] < cfg.tflops_floor:
        failures.append(f"gemm {gemm['tflops']:.1f} TFLOP/s below floor {cfg.tflops_floor}")
    if cfg.abft_iters:
        sec_chk = _time_loop(wl.step_checked, cfg.abft_iters, dev)
        corrupt = fi == "corrupt_abft" and env.rank == env.world_size - 1
        rep = wl.abft(corrupt=corrupt)
        gemm["abft"] = rep.as_dict()
        gemm["abft_tflops"] = wl.flops / sec_chk / 1e12
        if not rep.ok:
            failures.append(f"gemm ABFT checksum: {rep.bad_acc} accumulator / "
                            f"{rep.bad_store} stored rows inconsistent")
    clock.mark("gemm_verified")
    del wl

    hbm: dict = {}
    if with_hbm:
        hbm = hbm_check(dev, cfg.hbm_bytes, cfg.hbm_iters, backend=backend)
        if not hbm["copy_ok"]:
            failures.append("hbm copy mismatch")
        if cfg.hbm_floor_GBps and hbm["copy_GBps"] < cfg.hbm_floor_GBps:
            failures.append(f"hbm {hbm['copy_GBps']:.0f} GB/s below floor {cfg.hbm_floor_GBps}")
        if cfg.min_hbm_capacity_gb and hbm["capacity_total_gb"] < cfg.min_hbm_capacity_gb:
            failures.append(f"hbm capacity {hbm['capacity_total_gb']:.0f} GB below "
                            f"{cfg.min_hbm_capacity_gb} GB")
    clock.mark("hbm_checked")

    ar: list = []
    if with_allreduce and env.world_size > 1:
        sizes = coll.sweep_sizes(cfg.allreduce_min_bytes, cfg.allreduce_max_bytes, factor=4)
        impl = None
        if fi == "corrupt_allreduce" and env.rank == 0:
            import torch.distributed as tdist

            def impl(t):  # noqa: E306 - fault injection: rank 0 adds garbage
                t.view(-1)[0] += 3
                tdist.all_reduce(t)
        res = coll.all_reduce_sweep(env, sizes, dtype="bf16", iters=cfg.allreduce_iters,
                                    warmup=2, impl=impl)
        ar = [r.as_dict() for r in res]
        errs = all_reduce_sum(env, float(sum(r.errors for r in res)))
        if errs:
            failures.append(f"all-reduce mismatch: {int(errs)} wrong elements (sum over ranks)")
    clock.mark("collectives_checked")

    # every rank must agree on pass/fail
    nfail = all_reduce_max(env, float(len(failures)))
    if nfail and not failures:
        failures.append("another rank failed validation")
    clock.mark("done")
    return ValidationReport(
        rank=env.rank, world_size=env.world_size,
        device_name=torch.cuda.get_device_name(dev) if dev.type == "cuda" else "cpu",
        gemm=gemm, hbm=hbm, allreduce=ar,
        phases=clock.as_dict(), failures=failures)
