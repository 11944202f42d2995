"""PyTorch reference implementations of the ``ops`` API (K1/K2/K3).

Used ONLY by ``bench.py --rehearsal`` and CPU tests to rehearse the
multi-process orchestration (torch.distributed.run launch, barriers, max over
ranks, the JSON contract) on machines without an MI355X. Never selected
implicitly: the real entry points in ``ops`` load the gfx950 library or raise
``NativeLibraryMissing`` - there is no silent fallback.

Semantics match the native kernels: ``gemm_bf16`` = bf16(fp32 a @ b.T),
``fill_uniform_`` is a deterministic U[-1, 1) fill (a different generator than
the device hash RNG: rehearsal numbers are not comparable to device ones).
"""
from __future__ import annotations

import numpy as np
import torch

from .kernels import (AbftReport, HbmPatternReport, VerifyReport, gemm_shape_ok,  # noqa: F401
                      gemm_tolerance, hbm_pattern_check_args, hbm_pattern_id)


def fill_uniform_(t: torch.Tensor, seed: int, scale: float = 1.0) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(seed & 0x7FFFFFFFFFFFFFFF)
    v = torch.rand(t.shape, generator=g, dtype=torch.float32) * 2 - 1
    t.copy_((v * scale).to(t.dtype))
    return t


def gemm_bf16(a, b, out=None, variant="default"):
    r = (a.float() @ b.float().T).to(torch.bfloat16)
    if out is None:
        return r
    out.copy_(r)
    return out


def gemm_bf16_rowsum(a, b, out=None, rowsum=None):
    acc = a.float() @ b.float().T
    out = gemm_bf16(a, b, out)
    if rowsum is None:
        rowsum = torch.empty(a.shape[0], dtype=torch.float32, device=a.device)
    rowsum.copy_(acc.sum(1))
    return out, rowsum


def ref_gemm_f32(a, b):
    return a.float() @ b.float().T


def verify_bf16(c, ref, atol, rtol) -> VerifyReport:
    err = (c.float() - ref).abs()
    bad = int((~(err <= atol + rtol * ref.abs())).sum())
    rel = float((err.double().pow(2).sum() / ref.double().pow(2).sum()).sqrt())
    return VerifyReport(n=c.numel(), bad=bad, max_abs_err=float(err.max()), rel_rms_err=rel)


def abft_check(a, b, c, rowsum) -> AbftReport:
    r = a.double() @ b.double().sum(0)
    cd = c.double()
    norm = cd.norm(dim=1)
    e_acc = (rowsum.double() - r).abs()
    e_st = (cd.sum(1) - rowsum.double()).abs()
    return AbftReport(
        rows=a.shape[0],
        bad_acc=int((~(e_acc <= 1e-3 + 2**-14 * norm)).sum()),
        bad_store=int((~(e_st <= 1e-3 + 2**-6 * norm)).sum()),
        max_rel_acc=float((e_acc / norm.clamp_min(1e-30)).max()),
        max_rel_store=float((e_st / norm.clamp_min(1e-30)).max()))


def stream_copy(src, dst, config="tuned") -> None:
    dst.view(-1)[: src.numel()].copy_(src.view(-1))


def stream_read(src, sink, config="tuned") -> None:
    s = float(src.float().sum())
    if s != s:
        sink[0] = s


# K4 on the CPU, written from the pattern's definition (validation/README.md), with
# w = (base + byte offset) / 4 the 64-bit global index of a 32-bit word:
#   ADDR: each 8-byte word = (w / 2) ^ seed;  HASH: each 32-bit word = x ^ hi(w) * 0x9E3779B9
#   with x = lo(w) + (uint32)seed; x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15.
def hbm_pattern_words(nbytes: int, pattern, seed: int = 0, invert: bool = False,
                      base: int = 0) -> np.ndarray:
    """The pattern of logical bytes ``base .. base + nbytes`` as little-endian uint32 words."""
    pat = hbm_pattern_id(pattern)
    seed &= 2**64 - 1
    if pat == 0:
        q = np.arange(nbytes // 8, dtype=np.uint64) + np.uint64(base // 8)
        words = (q ^ np.uint64(seed)).view(np.uint32)
    else:
        w = np.arange(nbytes // 4, dtype=np.uint64) + np.uint64(base // 4)
        x = (w + np.uint64(seed & 0xFFFFFFFF)).astype(np.uint32)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        words = x ^ ((w >> np.uint64(32)).astype(np.uint32) * np.uint32(0x9E3779B9))
    return ~words if invert else words


def _bytes_of(t: torch.Tensor) -> np.ndarray:
    if t.is_cuda:
        raise ValueError("ops.reference works on CPU tensors")
    return t.view(-1).view(torch.uint8).numpy()


def hbm_pattern_write(t: torch.Tensor, pattern, seed: int = 0, invert: bool = False,
                      base: int = 0) -> torch.Tensor:
    nbytes = hbm_pattern_check_args(t, base)
    _bytes_of(t)[:] = hbm_pattern_words(nbytes, pattern, seed, invert, base).view(np.uint8)
    return t


def hbm_pattern_verify(t: torch.Tensor, pattern, seed: int = 0, invert: bool = False,
                       base: int = 0, invert_after: bool = False) -> HbmPatternReport:
    nbytes = hbm_pattern_check_args(t, base)
    exp = hbm_pattern_words(nbytes, pattern, seed, invert, base)
    mem = _bytes_of(t)
    e64, g64 = exp.view(np.uint64), mem.view(np.uint64).copy()
    if invert_after:
        mem[:] = (~exp).view(np.uint8)
    diff = e64 ^ g64
    idx = np.flatnonzero(diff)
    recs = [{"offset": base + 8 * int(i), "expected": int(e64[i]), "got": int(g64[i])}
            for i in idx[:4]]
    return HbmPatternReport(
        bad_words=int(idx.size),
        bad_bits=int(np.bitwise_or.reduce(diff[idx])) if idx.size else 0,
        first_bad_offset=base + 8 * int(idx[0]) if idx.size else None, records=recs)
