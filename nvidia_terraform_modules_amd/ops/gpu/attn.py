"""K13: fused attention forward on the device (validation/include/ntm/attn.hpp, attn_plan.hpp). The
host side (exact inputs, float64 reference, tolerance, messages) is numpy: ops/attn.py."""
from __future__ import annotations

import torch

from .._lib import check, lib, stream_handle
from ..attn import ATTN_HEAD_DIM, _scale_log2
from ._common import CompareReport, _bitwise_compare, bits_to_tensor


def _attn_shapes(q, k, v, causal: bool) -> tuple[int, int, int, int, int]:
    for name, t in (("q", q), ("k", k), ("v", v)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.bfloat16 or t.dim() != 4 or not t.is_cuda:
            raise ValueError(f"attention: {name} must be a 4-D bf16 GPU tensor [B, H, S, 128]")
        if t.shape[3] != ATTN_HEAD_DIM:
            raise ValueError(f"attention: the head dimension must be 128, {name} has {t.shape[3]}")
        if not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"attention: {name} must be contiguous and 16-byte aligned")
    B, Hq, Sq, _ = q.shape
    Hkv, Sk = k.shape[1], k.shape[2]
    if k.shape != v.shape or k.shape[0] != B or k.device != q.device or v.device != q.device:
        raise ValueError("attention: k and v must be [B, Hkv, Sk, 128] on q's device")
    if causal and Sk < Sq:
        raise ValueError("attention: causal needs Sk >= Sq (bottom-right aligned: no row may be fully masked)")
    if not lib().ntm_attn_shape_ok(B, Hq, Hkv, Sq, Sk, int(bool(causal))):
        raise ValueError("attention: needs B, Hq, Hkv, Sq >= 1, 1 <= Sk <= 65536 and Hq a multiple of Hkv")
    return B, Hq, Hkv, Sq, Sk


def attn_fwd(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False, softmax_scale: float | None = None,
             scale_log2: float | None = None, return_stats: bool = False, table: bool = False, out=None):
    """K13: flash-attention forward, ``softmax(softmax_scale q k^T) v`` -> O [B, Hq, Sq, 128] bf16.
    q [B, Hq, Sq, 128], k and v [B, Hkv, Sk, 128], contiguous bf16; query head h reads key/value
    head h // (Hq // Hkv). ``causal`` is bottom-right aligned (key j visible to query i iff
    j <= i + Sk - Sq) and needs Sk >= Sq. ``softmax_scale`` defaults to 1 / sqrt(128);
    ``scale_log2`` gives the kernel's log2-domain factor directly instead (exact inputs: 1.0).
    ``return_stats`` adds m (row maximum of the raw scores) and l (row sum of p) [B, Hq, Sq] fp32;
    ``table`` adds the int32 CU table [workgroups, 2] (raw HW_ID, XCC_ID). ``out``: (O, m, l) to
    write into, of the shapes above or flat (m and l may be None unless ``return_stats``). The
    arithmetic contract is in attn_plan.hpp. Stream-ordered."""
    B, Hq, Hkv, Sq, Sk = _attn_shapes(q, k, v, causal)
    scale = _scale_log2(softmax_scale, scale_log2)
    if out is not None:
        o, m, l = out
        if return_stats and (m is None or l is None):
            raise ValueError("attention: return_stats with out needs m and l in out")
    else:
        o = torch.empty_like(q)
        m = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device) if return_stats else None
        l = torch.empty((B, Hq, Sq), dtype=torch.float32, device=q.device) if return_stats else None
    if (not isinstance(o, torch.Tensor) or o.dtype != torch.bfloat16 or o.shape not in (q.shape, (q.numel(),))
            or not o.is_contiguous() or o.data_ptr() % 16 or o.device != q.device):
        raise ValueError("attention: O must be contiguous bf16 of q's shape (or flat, q's size), 16-byte aligned, on q's device")
    for s in (m, l):
        if s is not None and (not isinstance(s, torch.Tensor) or s.dtype != torch.float32
                              or s.shape not in ((B, Hq, Sq), (B * Hq * Sq,)) or not s.is_contiguous()
                              or s.data_ptr() % 4 or s.device != q.device):
            raise ValueError("attention: m and l must be contiguous fp32 [B, Hq, Sq] (or flat), 4-byte aligned, on q's device")
    tab = None
    if table:
        tab = torch.zeros((lib().ntm_attn_table_bytes(B, Hq, Sq) // 8, 2), dtype=torch.int32, device=q.device)
    with torch.cuda.device(q.device):
        rc = lib().ntm_attn_fwd(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), m.data_ptr() if m is not None else None,
                                l.data_ptr() if l is not None else None, tab.data_ptr() if tab is not None else None,
                                B, Hq, Hkv, Sq, Sk, int(bool(causal)), scale, stream_handle())
    check(rc, "ntm_attn_fwd")
    if not (return_stats or table):
        return o
    return (o,) + ((m, l) if return_stats else ()) + ((tab,) if table else ())


def attn_reference_gpu(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, causal: bool = False,
                       softmax_scale: float | None = None, scale_log2: float | None = None) -> dict:
    """K13: the reference kernel (no matrix, no cross-lane instruction; two-pass softmax, fp32
    loops in index order) -> ``o`` bf16, ``o32`` the fp32 quotient before the pack, ``a`` =
    sum p |v| / l per element, ``m``, ``l``."""
    B, Hq, Hkv, Sq, Sk = _attn_shapes(q, k, v, causal)
    scale = _scale_log2(softmax_scale, scale_log2)
    f32 = dict(dtype=torch.float32, device=q.device)
    r = {"o": torch.empty_like(q), "o32": torch.empty(q.shape, **f32), "a": torch.empty(q.shape, **f32),
         "m": torch.empty((B, Hq, Sq), **f32), "l": torch.empty((B, Hq, Sq), **f32)}
    with torch.cuda.device(q.device):
        rc = lib().ntm_attn_reference(q.data_ptr(), k.data_ptr(), v.data_ptr(), r["o"].data_ptr(), r["o32"].data_ptr(),
                                      r["a"].data_ptr(), r["m"].data_ptr(), r["l"].data_ptr(), B, Hq, Hkv, Sq, Sk,
                                      int(bool(causal)), scale, stream_handle())
    check(rc, "ntm_attn_reference")
    return r


def attn_compare(expected: torch.Tensor, got: torch.Tensor) -> CompareReport:
    """K13: the bitwise compare of two results in 4-byte words (two bf16 elements of O, or one
    fp32 of m / l): count, first word index, and the words there."""
    if (expected.dtype != got.dtype or expected.shape != got.shape or not expected.is_contiguous() or not got.is_contiguous()
            or expected.device != got.device or not got.is_cuda or (got.numel() * got.element_size()) % 4):
        raise ValueError("attn_compare needs two contiguous GPU tensors of one dtype and shape, a multiple of 4 bytes")
    L = lib()
    e, g = expected.view(torch.int32).view(-1), got.view(torch.int32).view(-1)
    return _bitwise_compare((L.ntm_attn_mismatch_bytes, L.ntm_attn_compare), e, g, 4, "ntm_attn_compare")


def attn_to_device(inputs: dict, device) -> dict:
    """The ``q`` / ``k`` / ``v`` bf16 bits of ``ops.attn.attn_make_inputs`` as bf16 GPU tensors."""
    return {n: bits_to_tensor(inputs[n], device, torch.bfloat16) for n in ("q", "k", "v")}
