"""K13 host side in numpy, no GPU: the twin of validation/include/ntm/attn_plan.hpp (shapes, the
exact-input predicate and generator, the tolerance, the failure line), a float64 attention, an
emulation of the arithmetic contract of ``ntm_attn_fwd`` and a CPU backend for
``models.checks.attn.attn_check``. The device side is ops/gpu/attn.py.

Q is [B, Hq, Sq, 128], K and V [B, Hkv, Sk, 128]; tensors cross this module as uint16 arrays of
bf16 bits. ``causal`` is bottom-right aligned: key j is visible to query i iff j <= i + Sk - Sq."""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

ATTN_HEAD_DIM = 128
ATTN_QTILE = 128
ATTN_KEY_STEP = 64
ATTN_MAX_SK = 65536
ATTN_EXACT_R = 10
ATTN_EXACT_GAP = 200
ATTN_EXACT_MAX_V = 4
ATTN_EXACT_MAX_SK = 4096
ATTN_EXACT_MAX_OPERAND = 256
ATTN_LDS_BYTES = 2 * 2 * ATTN_KEY_STEP * (ATTN_HEAD_DIM * 2 + 16)
ATTN_DEFAULT_SCALE_LOG2 = float(np.float32(np.float32(1.4426950408889634) / np.float32(11.313708498984761)))
_GAP_DIM, _GAP_Q, _GAP_K, _BIT_DIMS = 5, 10, 21, 10
_STREAM_Q, _STREAM_K, _STREAM_V, _STREAM_NEAR, _STREAM_W = 1, 2, 3, 4, 5
_M32 = np.uint64(0xFFFFFFFF)


def attn_shape_ok(B: int, Hq: int, Hkv: int, Sq: int, Sk: int, causal: bool) -> bool:
    if min(B, Hq, Hkv, Sq, Sk) < 1 or Sk > ATTN_MAX_SK or Hq % Hkv or (causal and Sk < Sq):
        return False
    tiles = -(-Sq // ATTN_QTILE)
    return B <= 1 << 20 and Hq <= 1 << 16 and Sq <= 1 << 32 and B * Hq <= (1 << 31) // tiles


def attn_grid(B: int, Hq: int, Sq: int) -> int:
    return B * Hq * -(-Sq // ATTN_QTILE)


def attn_key_steps(qt: int, Sq: int, Sk: int, causal: bool) -> int:
    every = -(-Sk // ATTN_KEY_STEP)
    if not causal:
        return every
    last = min((qt + 1) * ATTN_QTILE, Sq)
    return min((last - 1 + Sk - Sq) // ATTN_KEY_STEP + 1, every)


def attn_flops(B: int, Hq: int, Sq: int, Sk: int, causal: bool) -> float:
    pairs = Sq * ((Sk - Sq + 1) + Sk) / 2.0 if causal else float(Sq) * Sk
    return 4.0 * B * Hq * pairs * ATTN_HEAD_DIM


def _visible(Sq: int, Sk: int, causal: bool) -> np.ndarray:
    """[Sq, Sk] bool: key j visible to query i."""
    if not causal:
        return np.ones((Sq, Sk), dtype=bool)
    return np.arange(Sk)[None, :] <= np.arange(Sq)[:, None] + (Sk - Sq)


# ---- bf16 bits
def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """Round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16)


def _bf16_round(x: np.ndarray) -> np.ndarray:
    return bf16_to_f32(f32_to_bf16_bits(x))


# ---- the generator of exact inputs (attn_plan.hpp: exact_q / exact_k / exact_v)
def _h32(x):
    x = np.asarray(x, dtype=np.uint64) & _M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & _M32
    x ^= x >> np.uint64(16)
    return x


def _attn_hash(seed: int, stream: int, idx) -> np.ndarray:
    key = _h32(np.uint64((seed ^ (stream * 0x9E3779B9)) & 0xFFFFFFFF))
    return _h32((key + (np.asarray(idx, dtype=np.uint64) & _M32)) & _M32)


def _small7(h):
    return ((h >> np.uint64(8)) % np.uint64(7)).astype(np.int32) - 3


def _exact_ints(B, Hq, Hkv, Sq, Sk, seed):
    D = ATTN_HEAD_DIM
    d = np.arange(D, dtype=np.uint64)
    bit = (d >= 3) & ((d - 3) % 12 == 0) & ((d - 3) // 12 < _BIT_DIMS)
    qrows, krows = B * Hq * Sq, B * Hkv * Sk
    hq = _attn_hash(seed, _STREAM_Q, np.arange(qrows, dtype=np.uint64)[:, None] * np.uint64(D) + d[None, :])
    q = np.where(bit[None, :], ((hq >> np.uint64(8)) & np.uint64(1)).astype(np.int32), _small7(hq))
    q[:, _GAP_DIM] = _GAP_Q
    kidx = np.arange(krows, dtype=np.uint64)
    hk = _attn_hash(seed, _STREAM_K, kidx[:, None] * np.uint64(D) + d[None, :])
    hw = _attn_hash(seed, _STREAM_W, (kidx // np.uint64(Sk))[:, None] * np.uint64(D) + d[None, :])
    k = np.where(bit[None, :], ((hk >> np.uint64(8)) & np.uint64(1)).astype(np.int32), _small7(hw))
    near = (_attn_hash(seed, _STREAM_NEAR, kidx) >> np.uint64(8)) % np.uint64(4) == 0
    k[:, _GAP_DIM] = np.where(near, _GAP_K, 0)
    hv = _attn_hash(seed, _STREAM_V, kidx[:, None] * np.uint64(D) + d[None, :])
    v = ((hv >> np.uint64(8)) % np.uint64(9)).astype(np.int32) - 4
    return (q.astype(np.int32).reshape(B, Hq, Sq, D), k.astype(np.int32).reshape(B, Hkv, Sk, D),
            v.reshape(B, Hkv, Sk, D))


def attn_make_inputs(kind: str, B: int, Hq: int, Hkv: int, Sq: int, Sk: int, seed: int = 0) -> dict:
    """``"exact"``: integer Q, K, V that ``attn_exact`` accepts for both causal settings, to run
    with ``scale_log2`` 1.0 (keys ``qi`` / ``ki`` / ``vi`` hold the integers); ``"dense"``: uniform
    bf16 in [-1, 1), default scale. ``q`` / ``k`` / ``v`` are uint16 bf16 bits."""
    if not attn_shape_ok(B, Hq, Hkv, Sq, Sk, False):
        raise ValueError("attention needs B, Hq, Hkv, Sq >= 1, 1 <= Sk <= 65536 and Hq a multiple of Hkv")
    out = {"kind": kind, "B": B, "Hq": Hq, "Hkv": Hkv, "Sq": Sq, "Sk": Sk}
    if kind == "exact":
        if Sk > ATTN_EXACT_MAX_SK:
            raise ValueError("exact inputs need Sk <= 4096")
        qi, ki, vi = _exact_ints(B, Hq, Hkv, Sq, Sk, seed & 0xFFFFFFFF)
        out.update(qi=qi, ki=ki, vi=vi, scale_log2=1.0,
                   **{n: f32_to_bf16_bits(x.astype(np.float32)).reshape(x.shape) for n, x in (("q", qi), ("k", ki), ("v", vi))})
    elif kind == "dense":
        rng = np.random.default_rng(seed)
        for n, shape in (("q", (B, Hq, Sq)), ("k", (B, Hkv, Sk)), ("v", (B, Hkv, Sk))):
            x = rng.uniform(-1.0, 1.0, shape + (ATTN_HEAD_DIM,)).astype(np.float32)
            out[n] = f32_to_bf16_bits(x).reshape(x.shape)
        out["scale_log2"] = ATTN_DEFAULT_SCALE_LOG2
    else:
        raise ValueError('kind must be "exact" or "dense"')
    return out


def attn_exact(qi: np.ndarray, ki: np.ndarray, vi: np.ndarray, causal: bool) -> bool:
    """The exact-input predicate (attn_plan.hpp ``attn_exact``), integer arithmetic only: with
    ``scale_log2`` 1.0 every visible score of a row is within R = 10 of the row maximum or at
    least 200 below it, the far ones within R of each other; |v| <= 4; Sk <= 4096."""
    qi, ki, vi = (np.asarray(x) for x in (qi, ki, vi))
    if qi.ndim != 4 or ki.ndim != 4 or ki.shape != vi.shape or not all(np.issubdtype(x.dtype, np.integer) for x in (qi, ki, vi)):
        return False
    B, Hq, Sq, D = qi.shape
    Hkv, Sk = ki.shape[1], ki.shape[2]
    if D != ATTN_HEAD_DIM or ki.shape[0] != B or ki.shape[3] != D or not attn_shape_ok(B, Hq, Hkv, Sq, Sk, causal):
        return False
    if Sk > ATTN_EXACT_MAX_SK or np.abs(vi).max() > ATTN_EXACT_MAX_V:
        return False
    if max(np.abs(qi).max(), np.abs(ki).max()) > ATTN_EXACT_MAX_OPERAND:
        return False
    vis = _visible(Sq, Sk, causal)
    big = np.int64(1) << np.int64(40)
    for b in range(B):
        for h in range(Hq):
            s = qi[b, h].astype(np.int64) @ ki[b, h // (Hq // Hkv)].astype(np.int64).T
            if np.abs(s).max() >= 1 << 24:
                return False
            top = np.where(vis, s, -big).max(axis=1, keepdims=True)
            below = top - s
            far = vis & (below > ATTN_EXACT_R)
            if (far & (below < ATTN_EXACT_GAP)).any():
                return False
            spread = np.where(far, s, -big).max(axis=1) - np.where(far, s, big).min(axis=1)
            if (spread[far.any(axis=1)] > ATTN_EXACT_R).any():
                return False
    return True


# ---- arithmetic
def _exp2(x: np.ndarray) -> np.ndarray:
    """fp32 2^x; integer-valued x (and -inf) through ldexp, so powers of two are exact."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        whole = (x == np.trunc(x)) | np.isneginf(x)
        n = np.clip(np.where(whole, x, 0), -200, 127).astype(np.int32)
        return np.where(whole, np.ldexp(np.float32(1), n), np.exp2(np.where(whole, 0, x))).astype(np.float32)


def attn_reference(inputs: dict, causal: bool, scale_log2: float | None = None) -> dict:
    """Attention in float64 on the bf16 values: ``o`` [B, Hq, Sq, 128], ``a`` = sum p |v| / l,
    ``m`` (row maximum of the raw scores) and ``l`` (row sum of p = 2^(scale_log2 (s - m)))."""
    B, Hq, Hkv, Sq, Sk = (inputs[n] for n in ("B", "Hq", "Hkv", "Sq", "Sk"))
    scale = float(inputs["scale_log2"] if scale_log2 is None else scale_log2)
    q, k, v = (bf16_to_f32(inputs[n]).astype(np.float64) for n in ("q", "k", "v"))
    vis = _visible(Sq, Sk, causal)
    o, a = np.empty((B, Hq, Sq, ATTN_HEAD_DIM)), np.empty((B, Hq, Sq, ATTN_HEAD_DIM))
    m, l = np.empty((B, Hq, Sq)), np.empty((B, Hq, Sq))
    for b in range(B):
        for h in range(Hq):
            g = h // (Hq // Hkv)
            s = np.where(vis, q[b, h] @ k[b, g].T, -np.inf)
            m[b, h] = s.max(axis=1)
            p = np.exp2(scale * (s - m[b, h][:, None]))
            l[b, h] = p.sum(axis=1)
            o[b, h] = p @ v[b, g] / l[b, h][:, None]
            a[b, h] = p @ np.abs(v[b, g]) / l[b, h][:, None]
    return {"o": o, "a": a, "m": m, "l": l}


def attn_emulate(inputs: dict, causal: bool, scale_log2: float | None = None) -> dict:
    """The arithmetic contract of ``ntm_attn_fwd`` in numpy fp32, key steps of 64: online softmax
    in the log2 domain, l from the unrounded p, p rounded to bf16 before P V, one fp32 division,
    a nearest-even pack. ``o`` is uint16 bf16 bits, ``m`` / ``l`` fp32. (fp32 sums inside a step
    run in numpy's order, not the MFMA's: equal on exact inputs, within rounding otherwise.)"""
    B, Hq, Hkv, Sq, Sk = (inputs[n] for n in ("B", "Hq", "Hkv", "Sq", "Sk"))
    scale = np.float32(inputs["scale_log2"] if scale_log2 is None else scale_log2)
    q, k, v = (bf16_to_f32(inputs[n]) for n in ("q", "k", "v"))
    vis = _visible(Sq, Sk, causal)
    o = np.empty((B, Hq, Sq, ATTN_HEAD_DIM), dtype=np.uint16)
    m, l = np.empty((B, Hq, Sq), dtype=np.float32), np.empty((B, Hq, Sq), dtype=np.float32)
    for b in range(B):
        for h in range(Hq):
            g = h // (Hq // Hkv)
            s = np.where(vis, (q[b, h].astype(np.float64) @ k[b, g].astype(np.float64).T).astype(np.float32),
                         np.float32(-np.inf))
            m_run = np.full((Sq, 1), -np.inf, dtype=np.float32)
            l_run = np.zeros((Sq, 1), dtype=np.float32)
            acc = np.zeros((Sq, ATTN_HEAD_DIM), dtype=np.float32)
            for j in range(0, Sk, ATTN_KEY_STEP):
                t = s[:, j:j + ATTN_KEY_STEP]
                m_new = np.maximum(m_run, t.max(axis=1, keepdims=True))
                with np.errstate(invalid="ignore"):
                    alpha = _exp2(scale * (m_run - m_new))
                    p = _exp2(scale * (t - m_new))
                l_run = l_run * alpha + p.sum(axis=1, keepdims=True, dtype=np.float32)
                acc = acc * alpha + (_bf16_round(p) @ v[b, g, j:j + ATTN_KEY_STEP]).astype(np.float32)
                m_run = m_new
            o[b, h] = f32_to_bf16_bits(acc / l_run)
            m[b, h], l[b, h] = m_run[:, 0], l_run[:, 0]
    return {"o": o, "m": m, "l": l}


def attn_reference_f32(inputs: dict, causal: bool, scale_log2: float | None = None) -> dict:
    """``ntm_attn_reference`` in numpy: two passes, p and the division in fp32; the sums run in
    float64 and are rounded once, which equals the kernel's fp32 index-order sums on exact
    inputs. ``o`` uint16 bf16 bits, ``o32`` the fp32 quotient, ``a``, ``m``, ``l`` fp32."""
    B, Hq, Hkv, Sq, Sk = (inputs[n] for n in ("B", "Hq", "Hkv", "Sq", "Sk"))
    scale = np.float32(inputs["scale_log2"] if scale_log2 is None else scale_log2)
    q, k, v = (bf16_to_f32(inputs[n]).astype(np.float64) for n in ("q", "k", "v"))
    vis = _visible(Sq, Sk, causal)
    shape = (B, Hq, Sq, ATTN_HEAD_DIM)
    out = {"o": np.empty(shape, np.uint16), "o32": np.empty(shape, np.float32), "a": np.empty(shape, np.float32),
           "m": np.empty(shape[:3], np.float32), "l": np.empty(shape[:3], np.float32)}
    for b in range(B):
        for h in range(Hq):
            g = h // (Hq // Hkv)
            s = np.where(vis, (q[b, h] @ k[b, g].T).astype(np.float32), np.float32(-np.inf))
            top = s.max(axis=1, keepdims=True)
            p = _exp2(scale * (s - top))
            l = p.astype(np.float64).sum(axis=1, keepdims=True).astype(np.float32)
            acc = (_bf16_round(p).astype(np.float64) @ v[b, g]).astype(np.float32)
            ab = (p.astype(np.float64) @ np.abs(v[b, g])).astype(np.float32)
            out["o32"][b, h] = acc / l
            out["o"][b, h] = f32_to_bf16_bits(out["o32"][b, h])
            out["a"][b, h] = ab / l
            out["m"][b, h], out["l"][b, h] = top[:, 0], l[:, 0]
    return out


def attn_tolerance(a):
    """The dense sub-test's bound on |O - reference fp32 O| per element: 2^-7 a + 2^-20, with
    a = sum p |v| / l (derivation: profiles/attn/README.md)."""
    return 2.0 ** -7 * np.asarray(a, dtype=np.float64) + 2.0 ** -20


# ---- failure lines (attn_plan.hpp failure_message)
def attn_decode_cu(hw_id: int, xcc_id: int) -> tuple[int, int, int, int]:
    """(xcd, se, sh, cu) of the raw HW_ID / XCC_ID words of the CU table."""
    return xcc_id & 0xF, (hw_id >> 13) & 0x7, (hw_id >> 12) & 0x1, (hw_id >> 8) & 0xF


def attn_locate(what: str, word: int, Hq: int, Sq: int) -> dict:
    """Where 4-byte word ``word`` of O (two bf16 elements), m or l lies, and its workgroup."""
    is_o = what == "O"
    flat = word * 2 // ATTN_HEAD_DIM if is_o else word
    row, h, b = flat % Sq, flat // Sq % Hq, flat // Sq // Hq
    return {"b": b, "h": h, "row": row, "col": word * 2 % ATTN_HEAD_DIM if is_o else None,
            "wg": (b * Hq + h) * -(-Sq // ATTN_QTILE) + row // ATTN_QTILE}


def attn_failure_message(gpu: int, sub: str, what: str, count: int, word: int, expected: int, got: int, Hq: int,
                         Sq: int, table=None) -> str:
    """"gpu0: attn exact causal O: batch 0 head 1 row 5 col 6: xcd 2 se 1 sh 0 cu 3: expected
    0x3f803f80, got 0x3f803f81, bad bits 0x00000001; 1 differ" (``table``: the CU table, or None)."""
    w = attn_locate(what, word, Hq, Sq)
    where = f"batch {w['b']} head {w['h']} row {w['row']}" + ("" if w["col"] is None else f" col {w['col']}")
    if table is not None:
        t = np.asarray(table).reshape(-1, 2)
        xcd, se, sh, cu = attn_decode_cu(int(t[w["wg"], 0]), int(t[w["wg"], 1]))
        where += f": xcd {xcd} se {se} sh {sh} cu {cu}"
    return (f"gpu{gpu}: attn {sub} {what}: {where}: expected 0x{expected & 0xFFFFFFFF:08x}, got 0x{got & 0xFFFFFFFF:08x}, "
            f"bad bits 0x{(expected ^ got) & 0xFFFFFFFF:08x}; {count} differ")


# ---- the CPU backend of models.checks.attn.attn_check: the names of ops.gpu.attn on torch CPU
# tensors, ``attn_fwd`` being the emulation above and the CU table all zeros.
def _cpu_backend():
    import torch

    from .gpu._common import CompareReport

    def to_bits(t):
        return t.contiguous().view(torch.int16).numpy().view(np.uint16)

    def as_inputs(q, k, v):
        return {"B": q.shape[0], "Hq": q.shape[1], "Hkv": k.shape[1], "Sq": q.shape[2], "Sk": k.shape[2],
                "q": to_bits(q), "k": to_bits(k), "v": to_bits(v)}

    def bf16_tensor(bits):
        return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16).copy()).view(torch.bfloat16)

    def attn_to_device(inputs, device=None):
        return {n: bf16_tensor(inputs[n]) for n in ("q", "k", "v")}

    def attn_fwd(q, k, v, causal=False, softmax_scale=None, scale_log2=None, return_stats=False, table=False, out=None):
        scale = _scale_log2(softmax_scale, scale_log2)
        r = attn_emulate(as_inputs(q, k, v), causal, scale)
        o = bf16_tensor(r["o"])
        if not (return_stats or table):
            return o
        out = [o]
        if return_stats:
            out += [torch.from_numpy(r["m"]), torch.from_numpy(r["l"])]
        if table:
            out.append(torch.zeros((attn_grid(q.shape[0], q.shape[1], q.shape[2]), 2), dtype=torch.int32))
        return tuple(out)

    def attn_reference_gpu(q, k, v, causal=False, softmax_scale=None, scale_log2=None):
        r = attn_reference_f32(as_inputs(q, k, v), causal, _scale_log2(softmax_scale, scale_log2))
        return {"o": bf16_tensor(r["o"]), **{n: torch.from_numpy(r[n]) for n in ("o32", "a", "m", "l")}}

    def attn_compare(expected, got):
        e = expected.contiguous().view(torch.int32).numpy().view(np.uint32).reshape(-1)
        g = got.contiguous().view(torch.int32).numpy().view(np.uint32).reshape(-1)
        bad = np.flatnonzero(e != g)
        if not bad.size:
            return CompareReport(0, None, None, None)
        return CompareReport(int(bad.size), int(bad[0]), int(e[bad[0]]), int(g[bad[0]]))

    return SimpleNamespace(attn_to_device=attn_to_device, attn_fwd=attn_fwd, attn_reference_gpu=attn_reference_gpu,
                           attn_compare=attn_compare)


def _scale_log2(softmax_scale, scale_log2) -> float:
    """The kernel's ``scale_log2`` argument: given, or log2(e) * softmax_scale, default log2(e) / sqrt(128)."""
    if scale_log2 is not None and softmax_scale is not None:
        raise ValueError("give softmax_scale or scale_log2, not both")
    if scale_log2 is None:
        scale_log2 = ATTN_DEFAULT_SCALE_LOG2 if softmax_scale is None else math.log2(math.e) * float(softmax_scale)
    if not scale_log2 > 0:
        raise ValueError("the softmax scale must be positive")
    return float(scale_log2)


class _LazyBackend:
    """``ops.attn.CPU_BACKEND``: built on first use, so importing this module needs no torch."""
    _ns = None

    def __getattr__(self, name):
        if _LazyBackend._ns is None:
            _LazyBackend._ns = _cpu_backend()
        return getattr(_LazyBackend._ns, name)


CPU_BACKEND = _LazyBackend()
