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

from . import mcore as _mcore
from . import mx as _mx
from .gpu.hbm_pattern import HbmPatternReport, hbm_pattern_check_args, hbm_pattern_id
from .gpu.mcore import McoreCompareReport, mcore_check_args
from .gpu.mcore import mcore_to_device as _mcore_to_device
from .gpu.mx import MxCompareReport, mx_check_args
from .kernels import AbftReport, VerifyReport, gemm_shape_ok, gemm_tolerance  # noqa: F401
from .mcore import (MCORE_FORMATS, mcore_compress, mcore_decode_windows, mcore_exact,  # noqa: F401
                    mcore_expand, mcore_failure_message, mcore_make_inputs, mcore_matmul_bits,
                    mcore_max_abits)
from .mx import mx_dense_exact, mx_make_inputs, mx_matmul_bits, mx_pack, mx_unpack  # noqa: F401


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


# K6 on the CPU: the host-link kernels write and check K4's pattern, so push / pull are
# hbm_pattern_write / hbm_pattern_verify on a plain CPU tensor (nothing crosses a link;
# blocks only shapes the launch), and the chase is a numpy walk.
HOST_LINK_SLOT_BYTES = 64


def host_link_push(host: torch.Tensor, pattern, seed: int = 0, invert: bool = False,
                   base: int = 0, blocks=None) -> torch.Tensor:
    return hbm_pattern_write(host, pattern, seed=seed, invert=invert, base=base)


def host_link_pull(host: torch.Tensor, pattern, seed: int = 0, invert: bool = False,
                   base: int = 0, dst: torch.Tensor | None = None, blocks=None) -> HbmPatternReport:
    rep = hbm_pattern_verify(host, pattern, seed=seed, invert=invert, base=base)
    if dst is not None:
        _bytes_of(dst)[:] = _bytes_of(host)
    return rep


def _splitmix64(state: int) -> tuple[int, int]:
    m = 2**64 - 1
    state = (state + 0x9E3779B97F4A7C15) & m
    z = state
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return state, z ^ (z >> 31)


def host_link_chase_next(nslots: int, seed: int = 0) -> np.ndarray:
    """next[i] of the chase: Sattolo's algorithm on splitmix64(seed), one cycle of length
    ``nslots`` (the same permutation as host_link_plan.hpp chase_permutation)."""
    nxt = list(range(nslots))
    s = seed & (2**64 - 1)
    for i in range(nslots - 1, 0, -1):
        s, z = _splitmix64(s)
        j = z % i
        nxt[i], nxt[j] = nxt[j], nxt[i]
    return np.asarray(nxt, dtype=np.uint64)


def host_link_chase_table(nslots: int, seed: int = 0) -> np.ndarray:
    """The chase laid out as the kernel reads it: uint64 [nslots, 8], one 64-byte slot per
    hop, word 0 = the next slot's index."""
    table = np.zeros((nslots, HOST_LINK_SLOT_BYTES // 8), dtype=np.uint64)
    table[:, 0] = host_link_chase_next(nslots, seed)
    return table


def host_link_chase(host: torch.Tensor, hops: int, start: int = 0) -> tuple[int, float]:
    """The walk on the host: (final slot index, 0.0 - no link, no latency)."""
    nxt = _bytes_of(host).view(np.uint64).reshape(-1, HOST_LINK_SLOT_BYTES // 8)[:, 0]
    if not 0 <= start < len(nxt) or hops < 1:
        raise ValueError("host_link_chase needs 0 <= start < slots and hops >= 1")
    i = start
    for _ in range(hops):
        i = int(nxt[i])
    return i, 0.0


# K5 on the CPU: the expected tables of the per-CU compute sweep, written from the
# definitions in validation/include/ntm/cu_sweep_plan.hpp with numpy integer arithmetic
# (uint32 / uint64 wrap-around, int64 sums). One round = 7680 32-bit words:
#   hash u32[256] | mad u64[256] | f32 bits[256] | f64 bits[256] |
#   bf16 16x16 f32 bits [4][16][16] | bf16 32x32 [4][32][32] | fp8 16x16 [4][16][16]
CU_SWEEP_ROUND_WORDS = 7680


def _h32(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.uint32)
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def _u32(v: int) -> np.ndarray:
    return np.array([v & 0xFFFFFFFF], dtype=np.uint32)


def cu_sweep_round_seed(seed: int, rnd: int) -> int:
    return int(_h32(_u32(seed + 0x9E3779B9 * (rnd + 1)))[0])


def cu_sweep_lds_words(seed: int, rnd: int, nwords: int) -> np.ndarray:
    """The words the lds sub-test writes in round ``rnd`` (then their complement)."""
    return _h32(np.arange(nwords, dtype=np.uint32) + np.uint32(cu_sweep_round_seed(seed, rnd)))


def cu_sweep_operands(rs: int, kind: int, n: int, k: int, fp8: bool) -> np.ndarray:
    """[4 waves][n][k] integer operands: row i of A (even kind) or column i of B (odd kind)."""
    w, i, kk = np.meshgrid(np.arange(4, dtype=np.uint32), np.arange(n, dtype=np.uint32),
                           np.arange(k, dtype=np.uint32), indexing="ij")
    idx = ((((np.uint32(kind * 4) + w) * np.uint32(32) + i) << np.uint32(8)) | kk) + np.uint32(rs)
    h = _h32(idx) >> np.uint32(8)
    return ((h & np.uint32(7)).astype(np.int64) - 4 if fp8
            else (h & np.uint32(15)).astype(np.int64) - 8)


def _fma_chain(rs: int, chain: int, steps: int, segments: int) -> np.ndarray:
    t = np.arange(256, dtype=np.uint32)
    coeff = lambda i: _h32(_u32(rs) + _u32((chain * 64 + i + 1) << 12) + t)  # noqa: E731
    big = (7, 5) if chain else (3, 2)
    total = np.zeros(256, dtype=np.int64)
    for s in range(segments):
        c0 = coeff(s * steps)
        acc = ((c0 >> np.uint32(16)) & np.uint32(0xFF)).astype(np.int64) - 128
        for i in range(steps):
            c = coeff(s * steps + i)
            mul = np.where(c & np.uint32(1), big[0], big[1]) * np.where(c & np.uint32(2), -1, 1)
            acc = acc * mul + (((c >> np.uint32(8)) & np.uint32(0xFF)).astype(np.int64) - 128)
            assert np.abs(acc).max() < (2**53 if chain else 2**24)
        total += acc
    return total


def cu_sweep_expected(iters: int, seed: int, lds_bytes: int) -> dict:
    """Expected values of ``ops.cu_sweep(iters=, seed=, lds_bytes=)``: ``table`` (uint32, the
    device table, iters * 7680 words), its sections per round (``hash``, ``mad``, ``f32``, ``f64``,
    ``bf16_16``, ``bf16_32``, ``fp8``), the integer operands (``*_a`` [iters][4][n][K], ``*_b``
    [iters][4][n][K] by column), ``peak``: the largest sum of |a * b| of any element, which
    bounds every partial sum whatever the order, and ``lds``: [iters][lds_bytes / 4] fill words."""
    if not 1 <= iters <= 1024 or lds_bytes < 16 or lds_bytes % 16:
        raise ValueError("cu_sweep_expected needs 1 <= iters <= 1024 and lds_bytes % 16 == 0")
    seed &= 0xFFFFFFFF
    t = np.arange(256, dtype=np.uint32)
    out = {k: [] for k in ("hash", "mad", "f32", "f64", "bf16_16", "bf16_32", "fp8", "lds",
                           "bf16_16_a", "bf16_16_b", "bf16_32_a", "bf16_32_b", "fp8_a", "fp8_b")}
    rows, peak = [], 0
    for r in range(iters):
        rs = cu_sweep_round_seed(seed, r)
        x = t * np.uint32(0x9E3779B9) + np.uint32(rs)
        for i in range(16):
            x = _h32(x + np.uint32(i))
        a = _h32(np.uint32(rs) + np.uint32(2) * t + np.uint32(1))
        b = _h32(np.uint32(rs) ^ (t * np.uint32(0x85EBCA6B)))
        acc = a.astype(np.uint64)
        for i in range(16):
            acc = a.astype(np.uint64) * b.astype(np.uint64) + acc
            a = acc.astype(np.uint32) + np.uint32(i)
            b = (acc >> np.uint64(32)).astype(np.uint32) | np.uint32(1)
        f32 = _fma_chain(rs, 0, 8, 4).astype(np.float32).view(np.uint32)
        f64 = _fma_chain(rs, 1, 16, 1).astype(np.float64).view(np.uint64)
        prods = {}
        for name, kind, n, k, fp8 in (("bf16_16", 0, 16, 128, False), ("bf16_32", 2, 32, 128, False),
                                      ("fp8", 4, 16, 256, True)):
            oa = cu_sweep_operands(rs, kind, n, k, fp8)
            ob = cu_sweep_operands(rs, kind + 1, n, k, fp8)
            d = np.einsum("wik,wjk->wij", oa, ob)
            peak = max(peak, int(np.einsum("wik,wjk->wij", np.abs(oa), np.abs(ob)).max()))
            prods[name] = d.astype(np.float32).view(np.uint32)
            out[name + "_a"].append(oa)
            out[name + "_b"].append(ob)
        row = np.concatenate([x, acc.view(np.uint32), f32, f64.view(np.uint32),
                              prods["bf16_16"].ravel(), prods["bf16_32"].ravel(), prods["fp8"].ravel()])
        assert row.size == CU_SWEEP_ROUND_WORDS
        rows.append(row.astype(np.uint32))
        for k, v in (("hash", x), ("mad", acc), ("f32", f32), ("f64", f64), ("bf16_16", prods["bf16_16"]),
                     ("bf16_32", prods["bf16_32"]), ("fp8", prods["fp8"]),
                     ("lds", cu_sweep_lds_words(seed, r, lds_bytes // 4))):
            out[k].append(v)
    res = {k: np.stack(v) for k, v in out.items()}
    res["table"] = np.concatenate(rows)
    res["peak"] = peak
    return res


# K7 on the CPU: the MX check's products come from the exact integer reference in ops/mx.py
# (table decode, integer dot); tensors are CPU uint8 / fp32, nothing runs on a matrix core.
def mx_gemm(a, b, sa, sb, fmt, out: torch.Tensor | None = None) -> torch.Tensor:
    mx_check_args(a, b, sa, sb, fmt, out, need_cuda=False)
    bits = _mx.mx_matmul_bits(a.numpy(), b.numpy(), sa.numpy(), sb.numpy(), fmt)
    c = torch.from_numpy(bits.view(np.float32).copy())
    if out is None:
        return c
    out.copy_(c)
    return out


mx_reference_gpu = mx_gemm


def _compare(expected: torch.Tensor, got: torch.Tensor, word, what: str) -> MxCompareReport:   # = McoreCompareReport
    e = _bytes_of(expected).view(word)
    g = _bytes_of(got).view(word)
    if e.size != g.size:
        raise ValueError(f"{what} needs two tensors of one size")
    idx = np.flatnonzero(e != g)
    if not idx.size:
        return MxCompareReport(0, None, None, None)
    return MxCompareReport(int(idx.size), int(idx[0]), int(e[idx[0]]), int(g[idx[0]]))


def mx_compare(expected: torch.Tensor, got: torch.Tensor) -> MxCompareReport:
    return _compare(expected, got, np.uint32, "mx_compare")


# K10 on the CPU: every product is the exact numpy reference (ops/mcore.py)
def mcore_to_device(inputs: dict, device) -> dict:
    return _mcore_to_device(inputs, "cpu")


def mcore_gemm(a, b, fmt, ai=None, out: torch.Tensor | None = None) -> torch.Tensor:
    mcore_check_args(a, b, fmt, ai, out, need_cuda=False)
    f = _mcore.mcore_format(fmt)

    def arr(t):
        return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()
    bits = _mcore.mcore_matmul_bits(arr(a), arr(b), fmt, None if ai is None else ai.numpy())
    acc = np.int32 if f["integer"] else np.float64 if f["acc_bytes"] == 8 else np.float32
    c = torch.from_numpy(bits.view(acc).copy())
    if out is None:
        return c
    out.copy_(c)
    return out


mcore_reference_gpu = mcore_gemm


def mcore_compare(expected: torch.Tensor, got: torch.Tensor) -> McoreCompareReport:
    return _compare(expected, got, np.uint64 if expected.element_size() == 8 else np.uint32, "mcore_compare")
