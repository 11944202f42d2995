"""K14: paged-KV decode attention on the device (validation/include/ntm/pda.hpp, pda_plan.hpp). The
host side (the split plan, page tables, exact inputs, the float32 twin, messages) is numpy:
ops/pda.py. The reference and the compare are K13's (ops/gpu/attn.py)."""
from __future__ import annotations

import torch

from .._lib import check, lib, stream_handle
from ..attn import _scale_log2
from ..pda import PDA_HEAD_DIM, PDA_MAX_LEN, PDA_MAX_T, PDA_PAGE, PDA_ROWS
from ._common import bits_to_tensor
from .attn import attn_reference_gpu


def _pda_shapes(q, k_pool, v_pool, block_table, seq_lens) -> tuple[int, int, int, int, int, int]:
    for name, t in (("q", q), ("k_pool", k_pool), ("v_pool", v_pool)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16 or t.dim() != 4 or not t.is_cuda:
            raise ValueError(f"pda: {name} must be a 4-D bf16 GPU tensor (q [B, Hq, T, 128], pools [pages, Hkv, 16, 128])")
        if t.shape[3] != PDA_HEAD_DIM:
            raise ValueError(f"pda: the head dimension must be 128, {name} has {t.shape[3]}")
        if not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"pda: {name} must be contiguous and 16-byte aligned")
    B, Hq, T, _ = q.shape
    pages, Hkv = k_pool.shape[0], k_pool.shape[1]
    if k_pool.shape != v_pool.shape or k_pool.shape[2] != PDA_PAGE or k_pool.device != q.device or v_pool.device != q.device:
        raise ValueError("pda: the K and V pools must be [pages, Hkv, 16, 128] on q's device")
    for name, t, shape in (("block_table", block_table, None), ("seq_lens", seq_lens, (B,))):
        if (not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or not t.is_contiguous() or t.device != q.device
                or (shape is not None and tuple(t.shape) != shape)):
            raise ValueError(f"pda: {name} must be a contiguous int32 tensor on q's device (block_table [B, max_pages], seq_lens [B])")
    if block_table.dim() != 2 or block_table.shape[0] != B or block_table.shape[1] < 1:
        raise ValueError("pda: block_table must be [B, max_pages]")
    max_pages = block_table.shape[1]
    if not 1 <= T <= PDA_MAX_T or Hkv < 1 or Hq % Hkv or Hq // Hkv * T > PDA_ROWS:
        raise ValueError("pda: needs 1 <= T <= 4, Hq a multiple of Hkv and G * T = Hq / Hkv * T <= 32")
    return B, Hq, Hkv, T, max_pages, pages


def pda_fwd(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor, seq_lens: torch.Tensor,
            splits: int | None = None, softmax_scale: float | None = None, scale_log2: float | None = None,
            return_stats: bool = False, table: bool = False, out=None):
    """K14: decode attention over a paged KV cache -> O [B, Hq, T, 128] bf16. q [B, Hq, T, 128] holds
    the T = 1 .. 4 new tokens of every sequence, the pools [pages, Hkv, 16, 128] the cached keys and
    values in 16-token pages, ``block_table`` [B, max_pages] int32 the physical page of every logical
    page (entries past a sequence's last page must still be valid page ids) and ``seq_lens`` [B]
    int32 the lengths, T <= len <= min(65536, 16 max_pages), the new tokens included. Token t of
    a sequence sees key j iff j <= len - T + t. ``splits`` cuts every sequence's keys over that
    many workgroups per key/value head (default: ``ntm_pda_default_splits`` for this device);
    the result does not depend on it on exact inputs. ``softmax_scale`` / ``scale_log2`` as in
    ``attn_fwd``. ``return_stats`` adds m and l [B, Hq, T] fp32; ``table`` adds the int32 CU table
    [B * Hkv * splits, 2] (raw HW_ID, XCC_ID). ``out``: (O, m, l) or (O, m, l, workspace) to write
    into (m and l may be None unless ``return_stats``; the workspace a 16-byte aligned fp32 tensor
    of ``ntm_pda_workspace_bytes``). The lengths and page ids are read back once to check them
    (a synchronise). The arithmetic contract is in pda_plan.hpp. Stream-ordered: two launches."""
    B, Hq, Hkv, T, max_pages, pages = _pda_shapes(q, k_pool, v_pool, block_table, seq_lens)
    scale = _scale_log2(softmax_scale, scale_log2)
    lens = seq_lens.cpu()
    if int(lens.min()) < T or int(lens.max()) > min(PDA_MAX_LEN, PDA_PAGE * max_pages):
        raise ValueError("pda: every sequence needs T <= len <= min(65536, 16 * max_pages)")
    if int(block_table.min()) < 0 or int(block_table.max()) >= pages:
        raise ValueError("pda: every block-table entry must be a page id in [0, pages)")
    L = lib()
    if splits is None:
        cus = torch.cuda.get_device_properties(q.device).multi_processor_count
        splits = L.ntm_pda_default_splits(B, Hkv, int(lens.max()), cus)
    splits = int(splits)
    if not L.ntm_pda_shape_ok(B, Hq, Hkv, T, max_pages, pages, splits):
        raise ValueError("pda: needs 1 <= splits <= 64, max_pages <= 4096 and a grid below 2^31")
    ws_floats = L.ntm_pda_workspace_bytes(B, Hkv, splits) // 4
    o = m = l = ws = None
    if out is not None:
        o, m, l = out[:3]
        ws = out[3] if len(out) > 3 else None
        if return_stats and (m is None or l is None):
            raise ValueError("pda: return_stats with out needs m and l in out")
    else:
        o = torch.empty_like(q)
        m = torch.empty((B, Hq, T), dtype=torch.float32, device=q.device) if return_stats else None
        l = torch.empty((B, Hq, T), dtype=torch.float32, device=q.device) if return_stats else None
    if ws is None:
        ws = torch.empty((ws_floats,), dtype=torch.float32, device=q.device)
    if (not isinstance(o, torch.Tensor) or o.dtype != torch.bfloat16 or o.shape not in (q.shape, (q.numel(),))
            or not o.is_contiguous() or o.data_ptr() % 16 or o.device != q.device):
        raise ValueError("pda: O must be contiguous bf16 of q's shape (or flat, q's size), 16-byte aligned, on q's device")
    for s in (m, l):
        if s is not None and (not isinstance(s, torch.Tensor) or s.dtype != torch.float32
                              or s.shape not in ((B, Hq, T), (B * Hq * T,)) or not s.is_contiguous()
                              or s.data_ptr() % 4 or s.device != q.device):
            raise ValueError("pda: m and l must be contiguous fp32 [B, Hq, T] (or flat), 4-byte aligned, on q's device")
    if (not isinstance(ws, torch.Tensor) or ws.dtype != torch.float32 or ws.numel() != ws_floats or not ws.is_contiguous()
            or ws.data_ptr() % 16 or ws.device != q.device):
        raise ValueError(f"pda: the workspace must be a contiguous fp32 tensor of {ws_floats} elements, 16-byte aligned, on q's device")
    tab = None
    if table:
        tab = torch.zeros((L.ntm_pda_table_bytes(B, Hkv, splits) // 8, 2), dtype=torch.int32, device=q.device)
    with torch.cuda.device(q.device):
        rc = L.ntm_pda_fwd(q.data_ptr(), k_pool.data_ptr(), v_pool.data_ptr(), block_table.data_ptr(), seq_lens.data_ptr(),
                           o.data_ptr(), m.data_ptr() if m is not None else None, l.data_ptr() if l is not None else None,
                           ws.data_ptr(), tab.data_ptr() if tab is not None else None, B, Hq, Hkv, T, max_pages, pages,
                           splits, scale, stream_handle())
    check(rc, "ntm_pda_fwd")
    if not (return_stats or table):
        return o
    return (o,) + ((m, l) if return_stats else ()) + ((tab,) if table else ())


def pda_gather(pool: torch.Tensor, block_table: torch.Tensor, seq_lens: torch.Tensor, b: int) -> torch.Tensor:
    """The keys (or values) of sequence ``b`` as its block table names them: [1, Hkv, len_b, 128],
    contiguous - K13's layout, for ``attn_reference_gpu``."""
    n = int(seq_lens[b])
    ids = block_table[b, :-(-n // PDA_PAGE)].long()
    rows = pool[ids].permute(1, 0, 2, 3).reshape(pool.shape[1], -1, pool.shape[3])
    return rows[:, :n].contiguous().unsqueeze(0)


def pda_reference_gpu(q: torch.Tensor, k_pool: torch.Tensor, v_pool: torch.Tensor, block_table: torch.Tensor,
                      seq_lens: torch.Tensor, softmax_scale: float | None = None, scale_log2: float | None = None) -> dict:
    """K14's oracle: per sequence the gathered keys through K13's reference kernel (no matrix, no
    cross-lane instruction), causal with Sq = T and Sk = len_b, stacked: ``o`` bf16, ``o32``, ``a``
    [B, Hq, T, 128], ``m``, ``l`` [B, Hq, T]."""
    _pda_shapes(q, k_pool, v_pool, block_table, seq_lens)
    per = [attn_reference_gpu(q[b:b + 1].contiguous(), pda_gather(k_pool, block_table, seq_lens, b),
                              pda_gather(v_pool, block_table, seq_lens, b), causal=True, softmax_scale=softmax_scale,
                              scale_log2=scale_log2) for b in range(q.shape[0])]
    return {n: torch.cat([r[n] for r in per], dim=0) for n in ("o", "o32", "a", "m", "l")}


def pda_to_device(problem: dict, device) -> dict:
    """``ops.pda.pda_make_problem``'s arrays as GPU tensors: q and the pools bf16, the table and the
    lengths int32."""
    d = {n: bits_to_tensor(problem[n], device, torch.bfloat16) for n in ("q", "k_pool", "v_pool")}
    d["block_table"] = torch.from_numpy(problem["block_table"].copy()).to(device)
    d["seq_lens"] = torch.from_numpy(problem["seq_lens"].copy()).to(device)
    return d
