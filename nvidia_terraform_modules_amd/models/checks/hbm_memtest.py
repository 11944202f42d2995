"""K4: the Job's HBM pattern test as a Python model."""
from __future__ import annotations

import time

import torch

from ... import ops as native
from .._timing import _sync


def hbm_memtest(device: torch.device, nbytes: int, passes: int = 1, chunk_bytes: int = 1 << 30,
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
