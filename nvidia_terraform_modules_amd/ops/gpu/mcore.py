"""K10: fp64 / fp32 / fp16 / int8 / 2:4-sparse matrix-core check (validation/include/ntm/mcore.hpp,
mcore_plan.hpp). The host side (format table, packers, generators, bound, exact reference) is numpy:
ops/mcore.py."""
from __future__ import annotations

import numpy as np
import torch

from .._lib import check, lib, stream_handle
from ..mcore import MCORE_FORMATS, mcore_format, mcore_format_id, mcore_shape_ok
from ._common import CompareReport, _bitwise_compare, bits_to_tensor

McoreCompareReport = CompareReport

_MCORE_TORCH = {"f64": (torch.float64,), "f32": (torch.float32,), "f16": (torch.float16,), "i8": (torch.int8,),
                "sp_bf16": (torch.bfloat16, torch.int16), "sp_i8": (torch.int8,)}
_MCORE_ACC = {"f64": torch.float64, "f32": torch.float32, "f16": torch.float32, "i8": torch.int32,
              "sp_bf16": torch.float32, "sp_i8": torch.int32}


def mcore_to_device(inputs: dict, device) -> dict:
    """``mcore_make_inputs``' numpy arrays as GPU tensors (bf16 bit patterns become bfloat16)."""
    def t(x):
        if x is None:
            return None
        if x.dtype == np.uint16:
            return bits_to_tensor(x, device, torch.bfloat16)
        return torch.from_numpy(x.copy()).to(device)
    return {**inputs, "a": t(inputs["a"]), "ai": t(inputs["ai"]), "b": t(inputs["b"])}


def mcore_check_args(a, b, fmt, ai=None, out=None, need_cuda: bool = True) -> tuple[int, int, int, int]:
    """(format code, M, N, K) of one matrix-core product; ValueError unless a / b (/ ai) are
    contiguous matrices of the format's element type (on one GPU when ``need_cuda``) whose
    shapes agree, with M, N and K multiples of 128, and ``out`` (if given) a contiguous [M, N]
    tensor of the accumulator's type beside them."""
    f = mcore_format(fmt)
    name = f["name"]
    tensors = [("a", a, _MCORE_TORCH[name]), ("b", b, _MCORE_TORCH[name])]
    if f["sparse"]:
        tensors.append(("ai", ai, (torch.uint8,)))
    for label, t, dtypes in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype not in dtypes or t.dim() != 2 or not t.is_contiguous():
            raise ValueError(f"matrix-core check: {label} must be a contiguous 2-D tensor of {dtypes[0]}")
        if need_cuda and not t.is_cuda:
            raise ValueError("matrix-core check needs GPU tensors")
        if t.device != a.device:
            raise ValueError("matrix-core check: all tensors must be on one device")
    M, N, K = a.shape[0], b.shape[0], b.shape[1]
    if a.shape[1] != (K // 2 if f["sparse"] else K) or not mcore_shape_ok(M, N, K):
        raise ValueError("matrix-core check needs a [M, K] (sparse: [M, K/2]) and b [N, K] with M, N, K multiples of 128")
    if f["sparse"] and tuple(ai.shape) != (M, K // 4):
        raise ValueError("matrix-core check needs ai [M, K/4]")
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != _MCORE_ACC[name]
                            or tuple(out.shape) != (M, N) or not out.is_contiguous() or out.device != a.device):
        raise ValueError(f"matrix-core check: out must be a contiguous {_MCORE_ACC[name]} [M, N] tensor on the operands' device")
    return mcore_format_id(fmt), M, N, K


def _mcore_product(entry: str, a, b, fmt, ai, out):
    f, M, N, K = mcore_check_args(a, b, fmt, ai, out)
    if out is None:
        out = torch.empty((M, N), dtype=_MCORE_ACC[MCORE_FORMATS[f]], device=a.device)
    with torch.cuda.device(a.device):
        rc = getattr(lib(), entry)(f, a.data_ptr(), ai.data_ptr() if ai is not None else None, b.data_ptr(),
                                   out.data_ptr(), M, N, K, stream_handle())
    check(rc, entry)
    return out


def mcore_gemm(a: torch.Tensor, b: torch.Tensor, fmt, ai: torch.Tensor | None = None,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """K10: C [M, N] = A @ B.T on the format's matrix instruction (``MCORE_FORMATS``): fp64,
    fp32, fp16 or int8 MFMA, or a 2:4-sparse SMFMAC with ``a`` = Ac [M, K/2] and ``ai`` [M, K/4].
    M, N and K must be multiples of 128. Stream-ordered."""
    return _mcore_product("ntm_mcore_gemm", a, b, fmt, ai, out)


def mcore_reference_gpu(a: torch.Tensor, b: torch.Tensor, fmt, ai: torch.Tensor | None = None,
                        out: torch.Tensor | None = None) -> torch.Tensor:
    """K10: the same product with no matrix instruction (one thread per element, an fma or
    integer multiply-add loop in k order); exact under ``mcore_exact``. Stream-ordered."""
    return _mcore_product("ntm_mcore_reference", a, b, fmt, ai, out)


def mcore_compare(expected: torch.Tensor, got: torch.Tensor) -> McoreCompareReport:
    """K10: bitwise compare of two GPU tensors of 4- or 8-byte elements on the device
    (synchronises)."""
    for t in (expected, got):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("mcore_compare needs GPU tensors")
        if t.element_size() not in (4, 8) or not t.is_contiguous():
            raise ValueError("mcore_compare needs contiguous tensors of 4- or 8-byte elements")
    if expected.numel() != got.numel() or expected.device != got.device or expected.element_size() != got.element_size():
        raise ValueError("mcore_compare needs two tensors of one size and word width on one device")
    return _bitwise_compare((lib().ntm_mcore_mismatch_bytes, lib().ntm_mcore_compare), expected, got, 8, "ntm_mcore_compare")
