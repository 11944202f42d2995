"""K7: MX block-scaled matrix check (validation/include/ntm/mx_gemm.hpp, mx_plan.hpp). The host side
(formats, packing, generators, bound, exact reference) is numpy: ops/mx.py."""
from __future__ import annotations

import torch

from .._lib import check, lib, stream_handle
from ..mx import MX_BLOCK, mx_bits, mx_format_id, mx_shape_ok
from ._common import CompareReport, _bitwise_compare

MxCompareReport = CompareReport


def mx_check_args(a, b, sa, sb, fmt, out=None, need_cuda: bool = True) -> tuple[int, int, int, int]:
    """(format code, M, N, K) of one MX product; ValueError unless a / b / sa / sb are
    contiguous uint8 matrices (on one GPU when ``need_cuda``) whose shapes agree, with M, N
    and K multiples of 128, and ``out`` (if given) a contiguous fp32 [M, N] beside them."""
    f = mx_format_id(fmt)
    bits = mx_bits(f)
    for name, t in (("a", a), ("b", b), ("sa", sa), ("sb", sb)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"MX check: {name} must be a contiguous 2-D uint8 tensor")
        if need_cuda and not t.is_cuda:
            raise ValueError("MX check needs GPU tensors")
        if t.device != a.device:
            raise ValueError("MX check: all tensors must be on one device")
    M, N = a.shape[0], b.shape[0]
    K = a.shape[1] * 8 // bits
    if (a.shape[1] * 8) % bits or b.shape[1] != a.shape[1] or not mx_shape_ok(M, N, K):
        raise ValueError("MX check needs a [M, K*bits/8], b [N, K*bits/8] with M, N, K multiples of 128")
    if tuple(sa.shape) != (M, K // MX_BLOCK) or tuple(sb.shape) != (N, K // MX_BLOCK):
        raise ValueError("MX check needs sa [M, K/32] and sb [N, K/32]")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != torch.float32
                            or tuple(out.shape) != (M, N) or not out.is_contiguous()
                            or out.device != a.device):
        raise ValueError("MX check: out must be a contiguous fp32 [M, N] tensor on the operands' device")
    return f, M, N, K


def _mx_product(entry: str, a, b, sa, sb, fmt, out):
    f, M, N, K = mx_check_args(a, b, sa, sb, fmt, out)
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=a.device)
    with torch.cuda.device(a.device):
        rc = getattr(lib(), entry)(f, a.data_ptr(), b.data_ptr(), sa.data_ptr(), sb.data_ptr(),
                                   out.data_ptr(), M, N, K, stream_handle())
    check(rc, entry)
    return out


def mx_gemm(a: torch.Tensor, b: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, fmt,
            out: torch.Tensor | None = None) -> torch.Tensor:
    """K7: C [M, N] fp32 = A @ B.T on the block-scaled f8f6f4 matrix instruction. ``a`` / ``b``:
    packed uint8 rows of format ``fmt`` (``mx_pack``), ``sa`` / ``sb``: E8M0 scale bytes
    [rows, K/32]. M, N and K must be multiples of 128. Stream-ordered."""
    return _mx_product("ntm_mx_gemm", a, b, sa, sb, fmt, out)


def mx_reference_gpu(a: torch.Tensor, b: torch.Tensor, sa: torch.Tensor, sb: torch.Tensor, fmt,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """K7: the same product without the matrix cores (integer decode, ldexpf, an fp32 FMA
    chain in k order); exact under ``mx_dense_exact``. Stream-ordered."""
    return _mx_product("ntm_mx_reference", a, b, sa, sb, fmt, out)


def mx_compare(expected: torch.Tensor, got: torch.Tensor) -> MxCompareReport:
    """K7: bitwise compare of two GPU tensors of 32-bit elements on the device
    (synchronises)."""
    for t in (expected, got):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("mx_compare needs GPU tensors")
        if t.element_size() != 4 or not t.is_contiguous():
            raise ValueError("mx_compare needs contiguous tensors of 32-bit elements")
    if expected.numel() != got.numel() or expected.device != got.device:
        raise ValueError("mx_compare needs two tensors of one size on one device")
    return _bitwise_compare((lib().ntm_mx_mismatch_bytes, lib().ntm_mx_compare), expected, got, 4, "ntm_mx_compare")
