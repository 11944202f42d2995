"""K14 host side in numpy, no GPU: the twin of validation/include/ntm/pda_plan.hpp (shapes, the
split plan, the page-table generator, scatter and gather, exact inputs per sequence, the failure
line) and a float32 twin of the split arithmetic and its merge (``pda_emulate``). The device side
is ops/gpu/pda.py; the exact-input machinery is ops/attn.py's.

Q is [B, Hq, T, 128] with T = 1 .. 4 new tokens, the K and V pools [pages, Hkv, 16, 128],
``block_table`` [B, max_pages] int32, ``seq_lens`` [B] int32; tensors cross this module as uint16
arrays of bf16 bits. Row (g, t) of sequence b sees key j iff j <= len_b - T + t."""
from __future__ import annotations

import numpy as np

from . import attn as A

PDA_HEAD_DIM = A.ATTN_HEAD_DIM
PDA_PAGE = 16
PDA_KEY_STEP = 64
PDA_ROWS = 32
PDA_MAX_T = 4
PDA_WAVES = 4
PDA_MAX_LEN = 65536
PDA_MAX_SPLITS = 64
PDA_MIN_STEPS_PER_SPLIT = 4
PDA_LDS_BYTES = PDA_WAVES * PDA_KEY_STEP * (PDA_HEAD_DIM * 2 + 16) + 8 * 64 * 16  # the V stages and Q^T
PDA_PARTIAL_FLOATS = PDA_ROWS * PDA_HEAD_DIM + 2 * PDA_ROWS
PDA_NAN_BITS = 0x7FC0
_STREAM_PERM = 6
_M32 = np.uint64(0xFFFFFFFF)


def pda_shape_ok(B: int, Hq: int, Hkv: int, T: int, max_pages: int, pages: int, S: int) -> bool:
    if min(B, Hq, Hkv, T, max_pages, pages, S) < 1 or T > PDA_MAX_T or S > PDA_MAX_SPLITS:
        return False
    if Hq % Hkv or Hq // Hkv * T > PDA_ROWS or max_pages > PDA_MAX_LEN // PDA_PAGE:
        return False
    return B <= 1 << 20 and Hq <= 1 << 10 and pages <= 1 << 24 and B * Hkv * S < 1 << 31


def pda_grid(B: int, Hkv: int, S: int) -> int:
    return B * Hkv * S


def pda_workspace_bytes(B: int, Hkv: int, S: int) -> int:
    return 0 if min(B, Hkv, S) < 1 else pda_grid(B, Hkv, S) * PDA_PARTIAL_FLOATS * 4


def pda_table_bytes(B: int, Hkv: int, S: int) -> int:
    return 0 if min(B, Hkv, S) < 1 else pda_grid(B, Hkv, S) * 2 * 4


def pda_key_steps(length: int) -> int:
    return -(-length // PDA_KEY_STEP)


def pda_split_range(length: int, s: int, S: int) -> tuple[int, int]:
    """Key steps [begin, end) of split ``s`` of ``S``; empty when begin >= end."""
    steps = pda_key_steps(length)
    per = -(-steps // S)
    return min(s * per, steps), min((s + 1) * per, steps)


def pda_wave_steps(length: int, s: int, S: int, w: int) -> range:
    begin, end = pda_split_range(length, s, S)
    return range(begin + w, end, PDA_WAVES)


def pda_splits(B: int, Hkv: int, max_len: int, cus: int) -> int:
    """The default S: the smallest with B * Hkv * S >= 2 * cus, capped so that every split of the
    longest sequence keeps at least 4 key steps, within 1 .. 64."""
    if min(B, Hkv, max_len, cus) < 1:
        return 1
    want = -(-2 * cus // (B * Hkv))
    cap = pda_key_steps(max_len) // PDA_MIN_STEPS_PER_SPLIT
    return max(1, min(want, cap, PDA_MAX_SPLITS))


def pda_kv_bytes(lens, Hkv: int) -> float:
    return float(np.sum(np.asarray(lens, dtype=np.float64))) * Hkv * PDA_HEAD_DIM * 2.0 * 2.0


# ---- the page-table generator (pda_plan.hpp make_page_table)
def pda_pages_of(length: int) -> int:
    return -(-length // PDA_PAGE)


def pda_make_page_table(lens, seed: int = 0, shared_pairs: int = 0) -> dict:
    """One pool page per logical page of every sequence plus one poison page, handed out through a
    seeded permutation; sequence 2 i + 1 of the first ``shared_pairs`` pairs points its first
    min(len_2i // 16, len_2i+1 // 16) // 2 logical pages at those of sequence 2 i; every entry
    past a sequence's last page names the poison page. ``table`` is [B, max_pages] int32."""
    lens = [int(n) for n in lens]
    total = sum(pda_pages_of(n) for n in lens)
    max_pages = max(pda_pages_of(n) for n in lens)
    pages = total + 1
    perm = list(range(pages))
    if pages > 1:
        draws = A._attn_hash(seed & 0xFFFFFFFF, _STREAM_PERM, np.arange(pages, dtype=np.uint64))
        for i in range(pages - 1, 0, -1):
            j = int(draws[i]) % (i + 1)
            perm[i], perm[j] = perm[j], perm[i]
    poison = perm[total]
    table = np.full((len(lens), max_pages), poison, dtype=np.int32)
    nxt = 0
    for b, n in enumerate(lens):
        k = pda_pages_of(n)
        table[b, :k] = perm[nxt:nxt + k]
        nxt += k
    for i in range(shared_pairs):
        a, b = 2 * i, 2 * i + 1
        if b >= len(lens):
            break
        share = min(lens[a] // PDA_PAGE, lens[b] // PDA_PAGE) // 2
        table[b, :share] = table[a, :share]
    return {"B": len(lens), "max_pages": max_pages, "pages": pages, "poison": poison,
            "lens": np.asarray(lens, dtype=np.int32), "table": table}


def pda_scatter_to_pages(pt: dict, b: int, src: np.ndarray, pool: np.ndarray) -> None:
    """``src`` [Hkv, len_b, 128] of sequence b into ``pool`` [pages, Hkv, 16, 128], in place."""
    n = int(pt["lens"][b])
    j = np.arange(n)
    pool[pt["table"][b, j // PDA_PAGE], :, j % PDA_PAGE, :] = np.asarray(src)[:, :n].transpose(1, 0, 2)


def pda_gather_from_pages(pt: dict, b: int, pool: np.ndarray) -> np.ndarray:
    """[Hkv, len_b, 128]: the keys of sequence b as its block table names them."""
    j = np.arange(int(pt["lens"][b]))
    return np.ascontiguousarray(pool[pt["table"][b, j // PDA_PAGE], :, j % PDA_PAGE, :].transpose(1, 0, 2))


# ---- inputs
def pda_exact_sequence(seed: int, b: int, Hq: int, Hkv: int, T: int, length: int) -> tuple:
    """pda_plan.hpp ``exact_sequence``: integer q [Hq, T, 128], k and v [Hkv, len, 128]. The
    dimensions all keys of a head share depend on the key/value head alone, so keys of two
    sequences may meet in one softmax (prefix sharing) and ``attn_exact`` still holds."""
    D = PDA_HEAD_DIM
    seed &= 0xFFFFFFFF
    d = np.arange(D, dtype=np.uint64)
    bit = (d >= 3) & ((d - 3) % 12 == 0) & ((d - 3) // 12 < A._BIT_DIMS)
    qrow = np.uint64(b * 4096) + np.arange(Hq * T, dtype=np.uint64)
    hq = A._attn_hash(seed, A._STREAM_Q, (qrow[:, None] * np.uint64(D) + d[None, :]) & _M32)
    q = np.where(bit[None, :], ((hq >> np.uint64(8)) & np.uint64(1)).astype(np.int32), A._small7(hq))
    q[:, A._GAP_DIM] = A._GAP_Q
    h = np.repeat(np.arange(Hkv, dtype=np.uint64), length)
    j = np.tile(np.arange(length, dtype=np.uint64), Hkv)
    krow = ((np.uint64(b * Hkv) + h) * np.uint64(PDA_MAX_LEN) + j) & _M32
    kidx = (krow[:, None] * np.uint64(D) + d[None, :]) & _M32
    hk = A._attn_hash(seed, A._STREAM_K, kidx)
    hw = A._attn_hash(seed, A._STREAM_W, h[:, None] * np.uint64(D) + d[None, :])
    k = np.where(bit[None, :], ((hk >> np.uint64(8)) & np.uint64(1)).astype(np.int32), A._small7(hw))
    near = (A._attn_hash(seed, A._STREAM_NEAR, krow) >> np.uint64(8)) % np.uint64(4) == 0
    k[:, A._GAP_DIM] = np.where(near, A._GAP_K, 0)
    v = ((A._attn_hash(seed, A._STREAM_V, kidx) >> np.uint64(8)) % np.uint64(9)).astype(np.int32) - 4
    return (q.astype(np.int32).reshape(Hq, T, D), k.astype(np.int32).reshape(Hkv, length, D),
            v.reshape(Hkv, length, D))


def _bits_of_ints(x: np.ndarray) -> np.ndarray:
    return A.f32_to_bf16_bits(x.astype(np.float32)).reshape(x.shape)


def pda_make_problem(kind: str, Hq: int, Hkv: int, T: int, lens, seed: int = 0, shared_pairs: int = 0) -> dict:
    """A whole paged problem. ``"exact"``: integer inputs per sequence (``scale_log2`` 1.0);
    ``"dense"``: uniform bf16 in [-1, 1), the default scale. The pools start as bf16 NaN (0x7FC0)
    everywhere, so the poison page, every unused page and every page tail past ``len_b`` are NaN.
    Returns ``q`` [B, Hq, T, 128], ``k_pool`` / ``v_pool`` [pages, Hkv, 16, 128] (uint16 bits),
    ``block_table``, ``seq_lens``, ``pt`` (the page table) and ``seqs``: per sequence the attention
    inputs of ops.attn (B 1, Sq T, Sk len_b) GATHERED back from the pools, which is what the
    kernel reads where pages are shared; exact ones carry ``qi`` / ``ki`` / ``vi``."""
    lens = [int(n) for n in lens]
    if not lens or min(lens) < T or max(lens) > PDA_MAX_LEN or (kind == "exact" and max(lens) > A.ATTN_EXACT_MAX_SK):
        raise ValueError("pda: needs T <= len <= 65536 (exact inputs: 4096) for every sequence")
    if kind not in ("exact", "dense"):
        raise ValueError('kind must be "exact" or "dense"')
    pt = pda_make_page_table(lens, seed, shared_pairs)
    if not pda_shape_ok(len(lens), Hq, Hkv, T, pt["max_pages"], pt["pages"], 1):
        raise ValueError("pda: needs 1 <= T <= 4, Hq a multiple of Hkv and Hq / Hkv * T <= 32")
    D, B = PDA_HEAD_DIM, len(lens)
    shape = (pt["pages"], Hkv, PDA_PAGE, D)
    q = np.empty((B, Hq, T, D), dtype=np.uint16)
    k_pool, v_pool = np.full(shape, PDA_NAN_BITS, dtype=np.uint16), np.full(shape, PDA_NAN_BITS, dtype=np.uint16)
    ki_pool = vi_pool = None
    qi = []
    if kind == "exact":
        ki_pool, vi_pool = np.zeros(shape, dtype=np.int32), np.zeros(shape, dtype=np.int32)
    rng = np.random.default_rng(seed)
    for b, n in enumerate(lens):
        if kind == "exact":
            qb, kb, vb = pda_exact_sequence(seed, b, Hq, Hkv, T, n)
            qi.append(qb)
            q[b] = _bits_of_ints(qb)
            pda_scatter_to_pages(pt, b, kb, ki_pool)
            pda_scatter_to_pages(pt, b, vb, vi_pool)
            pda_scatter_to_pages(pt, b, _bits_of_ints(kb), k_pool)
            pda_scatter_to_pages(pt, b, _bits_of_ints(vb), v_pool)
        else:
            q[b] = A.f32_to_bf16_bits(rng.uniform(-1.0, 1.0, (Hq, T, D)).astype(np.float32)).reshape(Hq, T, D)
            for pool in (k_pool, v_pool):
                x = rng.uniform(-1.0, 1.0, (Hkv, n, D)).astype(np.float32)
                pda_scatter_to_pages(pt, b, A.f32_to_bf16_bits(x).reshape(x.shape), pool)
    seqs = []
    for b, n in enumerate(lens):
        s = {"B": 1, "Hq": Hq, "Hkv": Hkv, "Sq": T, "Sk": n, "q": q[b][None],
             "k": pda_gather_from_pages(pt, b, k_pool)[None], "v": pda_gather_from_pages(pt, b, v_pool)[None],
             "scale_log2": 1.0 if kind == "exact" else A.ATTN_DEFAULT_SCALE_LOG2}
        if kind == "exact":
            s.update(qi=qi[b][None], ki=pda_gather_from_pages(pt, b, ki_pool)[None],
                     vi=pda_gather_from_pages(pt, b, vi_pool)[None])
        seqs.append(s)
    return {"kind": kind, "B": B, "Hq": Hq, "Hkv": Hkv, "T": T, "q": q, "k_pool": k_pool, "v_pool": v_pool,
            "block_table": pt["table"], "seq_lens": pt["lens"], "pt": pt, "seqs": seqs,
            "scale_log2": 1.0 if kind == "exact" else A.ATTN_DEFAULT_SCALE_LOG2}


def pda_exact(problem: dict) -> bool:
    """``attn_exact`` (causal) on the gathered integers of every sequence."""
    return all(A.attn_exact(s["qi"], s["ki"], s["vi"], True) for s in problem["seqs"])


# ---- arithmetic: the float32 twin of pda_split_kernel and pda_combine_kernel
def _merge(parts: list, scale: np.float32) -> tuple:
    """The merge of the contract, in list order: m = max m_p; alpha_p = exp2(scale (m_p - m)),
    0 where m_p = -inf; l and acc by one fp32 multiply and one fp32 add per partial."""
    m = parts[0][0]
    for p in parts[1:]:
        m = np.maximum(m, p[0])
    l = np.zeros_like(m)
    acc = np.zeros_like(parts[0][2])
    for mp, lp, ap in parts:
        empty = np.isneginf(mp)
        with np.errstate(invalid="ignore"):
            alpha = np.where(empty, np.float32(0), A._exp2(scale * (np.where(empty, np.float32(0), mp) - np.where(empty, np.float32(0), m))))
        alpha = alpha.astype(np.float32)
        l = (l + (alpha * lp).astype(np.float32)).astype(np.float32)
        acc = (acc + (alpha * ap).astype(np.float32)).astype(np.float32)
    return m, l, acc


def _partial(s: np.ndarray, v: np.ndarray, steps, scale: np.float32) -> tuple:
    """One wave's partial over its key steps: ``s`` [rows, len] masked scores (-inf where hidden)."""
    rows = s.shape[0]
    m_run = np.full((rows, 1), -np.inf, dtype=np.float32)
    l_run = np.zeros((rows, 1), dtype=np.float32)
    acc = np.zeros((rows, PDA_HEAD_DIM), dtype=np.float32)
    for step in steps:
        j = step * PDA_KEY_STEP
        t = s[:, j:j + PDA_KEY_STEP]
        m_new = np.maximum(m_run, t.max(axis=1, keepdims=True))
        m_sub = np.where(np.isneginf(m_new), np.float32(0), m_new)
        alpha = A._exp2(scale * (m_run - m_sub))
        p = A._exp2(scale * (t - m_sub))
        l_run = (l_run * alpha + p.sum(axis=1, keepdims=True, dtype=np.float32)).astype(np.float32)
        acc = (acc * alpha + (A._bf16_round(p) @ v[j:j + PDA_KEY_STEP]).astype(np.float32)).astype(np.float32)
        m_run = m_new
    return m_run, l_run, acc


def pda_emulate(problem: dict, S: int, scale_log2: float | None = None) -> dict:
    """The arithmetic contract of ``ntm_pda_fwd`` in numpy fp32: per (sequence, key/value head)
    the partial of every wave of every split over the steps the plan gives it, the waves merged
    in wave order, then the splits in split order, one fp32 division, a nearest-even pack.
    ``o`` [B, Hq, T, 128] uint16 bf16 bits, ``m`` / ``l`` [B, Hq, T] fp32. (fp32 sums inside a
    step run in numpy's order, not the MFMA's: equal on exact inputs.)"""
    B, Hq, Hkv, T = (problem[n] for n in ("B", "Hq", "Hkv", "T"))
    scale = np.float32(problem["scale_log2"] if scale_log2 is None else scale_log2)
    G = Hq // Hkv
    o = np.empty((B, Hq, T, PDA_HEAD_DIM), dtype=np.uint16)
    m, l = np.empty((B, Hq, T), dtype=np.float32), np.empty((B, Hq, T), dtype=np.float32)
    for b, seq in enumerate(problem["seqs"]):
        n = seq["Sk"]
        q, k, v = (A.bf16_to_f32(seq[x][0]) for x in ("q", "k", "v"))
        vis = np.tile(A._visible(T, n, True), (G, 1))  # row g T + t
        for h in range(Hkv):
            qr = q[h * G:(h + 1) * G].reshape(G * T, PDA_HEAD_DIM)
            s = np.where(vis, (qr.astype(np.float64) @ k[h].astype(np.float64).T).astype(np.float32), np.float32(-np.inf))
            splits = [_merge([_partial(s, v[h], pda_wave_steps(n, sp, S, w), scale) for w in range(PDA_WAVES)], scale)
                      for sp in range(S)]
            mm, ll, acc = _merge(splits, scale)
            with np.errstate(invalid="ignore", divide="ignore"):
                o[b, h * G:(h + 1) * G] = A.f32_to_bf16_bits(acc / ll).reshape(G, T, PDA_HEAD_DIM)
            m[b, h * G:(h + 1) * G], l[b, h * G:(h + 1) * G] = mm.reshape(G, T), ll.reshape(G, T)
    return {"o": o, "m": m, "l": l}


def pda_reference_f32(problem: dict, scale_log2: float | None = None) -> dict:
    """``ops.attn.attn_reference_f32`` (causal) on the gathered keys of every sequence, stacked:
    ``o`` bits, ``o32``, ``a`` [B, Hq, T, 128], ``m``, ``l`` [B, Hq, T]."""
    per = [A.attn_reference_f32(s, True, scale_log2) for s in problem["seqs"]]
    return {n: np.concatenate([r[n] for r in per], axis=0) for n in ("o", "o32", "a", "m", "l")}


pda_tolerance = A.attn_tolerance  # the merge's S + 4 extra fp32 roundings fit it: profiles/pda/README.md


# ---- failure lines (pda_plan.hpp failure_message)
def pda_locate(what: str, word: int, Hq: int, Hkv: int, T: int, S: int) -> dict:
    """Where 4-byte word ``word`` of O (two bf16 elements), m or l lies, and its row's split 0."""
    is_o = what == "O"
    flat = word * 2 // PDA_HEAD_DIM if is_o else word
    t, h, b = flat % T, flat // T % Hq, flat // T // Hq
    return {"b": b, "h": h, "t": t, "col": word * 2 % PDA_HEAD_DIM if is_o else None,
            "wg": (b * Hkv + h // (Hq // Hkv)) * S}


def pda_failure_message(gpu: int, sub: str, what: str, count: int, word: int, expected: int, got: int, Hq: int,
                        Hkv: int, T: int, S: int, table=None) -> str:
    """"gpu0: pda exact T4 O: seq 23 head 31 tok 3 col 126: cu 7.3.1.15 0.0.0.2 (xcd.se.sh.cu):
    expected 0x3f803f80, got 0x3f803f81, bad bits 0x00000001; 1 differ": the CUs of the first 4
    split workgroups that fed the row (``table``: the CU table, or None)."""
    w = pda_locate(what, word, Hq, Hkv, T, S)
    where = f"seq {w['b']} head {w['h']} tok {w['t']}" + ("" if w["col"] is None else f" col {w['col']}")
    if table is not None:
        t = np.asarray(table).reshape(-1, 2)
        cus = [A.attn_decode_cu(int(t[w["wg"] + i, 0]), int(t[w["wg"] + i, 1])) for i in range(min(S, 4))]
        where += ": cu " + " ".join(".".join(map(str, c)) for c in cus) + " (xcd.se.sh.cu)"
    return (f"gpu{gpu}: pda {sub} {what}: {where}: expected 0x{expected & 0xFFFFFFFF:08x}, got 0x{got & 0xFFFFFFFF:08x}, "
            f"bad bits 0x{(expected ^ got) & 0xFFFFFFFF:08x}; {count} differ")
