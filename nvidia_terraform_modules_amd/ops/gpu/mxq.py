"""K11: MX quantise / dequantise on the device (validation/include/ntm/mxq.hpp, mxq_plan.hpp). The host
side (rules, generators) is numpy: ops/mxq.py."""
from __future__ import annotations

import numpy as np
import torch

from .._lib import check, lib, stream_handle
from ..mx import MX_BLOCK, mx_bits, mx_format_id
from ..mxq import MXQ_ROUNDING
from ._common import bits_to_tensor

_MXQ_DTYPE = {torch.float32: 0, torch.bfloat16: 1}


def _mxq_rounding(rounding, seed) -> tuple[int, int]:
    if rounding not in MXQ_ROUNDING:
        raise ValueError(f"rounding must be one of {MXQ_ROUNDING}")
    if rounding == "stochastic" and seed is None:
        raise ValueError("stochastic rounding needs a seed")
    return MXQ_ROUNDING.index(rounding), int(seed or 0) & (2**64 - 1)


def _mxq_source(x) -> tuple[int, int, int]:
    """(R, K, ldx) of a 2-D fp32 / bf16 GPU tensor whose rows are contiguous."""
    if not isinstance(x, torch.Tensor) or x.dtype not in _MXQ_DTYPE or x.dim() != 2 or not x.is_cuda:
        raise ValueError("MX quantise needs a 2-D fp32 or bf16 GPU tensor")
    if x.shape[1] and x.stride(1) != 1:
        raise ValueError("MX quantise needs rows of contiguous elements")
    return x.shape[0], x.shape[1], x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])


def _mxq_down(entry: str, x, fmt, scales, packed, rounding="rne", seed=None):
    f = mx_format_id(fmt)
    R, K, ldx = _mxq_source(x)
    given = entry.endswith("cvt")
    KB = K // MX_BLOCK
    if given:
        if (not isinstance(scales, torch.Tensor) or scales.dtype != torch.uint8 or tuple(scales.shape) != (R, KB)
                or not scales.is_contiguous() or scales.device != x.device):
            raise ValueError("mxq_cvt needs contiguous uint8 scales [R, K/32] on the source's device")
    elif scales is None:
        scales = torch.empty((R, max(KB, 0)), dtype=torch.uint8, device=x.device)
    if packed is None:
        packed = torch.empty((R, K * mx_bits(f) // 8), dtype=torch.uint8, device=x.device)
    args = [f, _MXQ_DTYPE[x.dtype], x.data_ptr()]
    args += [scales.data_ptr(), packed.data_ptr()] if given else [packed.data_ptr(), scales.data_ptr()]
    args += [R, K, ldx]
    if "reference" not in entry:
        args += list(_mxq_rounding(rounding, seed))
    elif rounding != "rne":
        raise ValueError("the reference kernels round to nearest even only")
    with torch.cuda.device(x.device):
        rc = getattr(lib(), entry)(*args, stream_handle())
    check(rc, entry)
    return packed, scales


def mx_quantize(x: torch.Tensor, fmt, rounding: str = "rne", seed: int | None = None, packed=None, scales=None):
    """K11: quantise ``x`` [R, K] (fp32 or bf16, K a multiple of 32, row stride >= K) to MX format
    ``fmt`` on the device with the scaled-conversion instructions -> (packed uint8 [R, K*bits/8],
    scales uint8 [R, K/32]) laid out as ``mx_gemm`` takes them. OCP MX v1.0: scale byte =
    clamp(floor(log2(amax)) - emax_elem + 127, 1, 254), 127 for a zero block; elements round to
    nearest even and saturate. ``rounding="stochastic"`` (e2m1, e4m3) needs ``seed``: the random
    word of element i is ``hash32(seed, 11, i)``. Not judged: Inf / NaN inputs saturate, fp32
    denormals are whatever the instruction makes of them. Stream-ordered."""
    return _mxq_down("ntm_mxq_quantize", x, fmt, scales, packed, rounding, seed)


def mx_quantize_reference_gpu(x: torch.Tensor, fmt, packed=None, scales=None):
    """K11: ``mx_quantize`` by integer bit arithmetic only (no conversion instruction)."""
    return _mxq_down("ntm_mxq_reference_quantize", x, fmt, scales, packed)


def mxq_cvt(x: torch.Tensor, scales: torch.Tensor, fmt, rounding: str = "rne", seed: int | None = None,
            reference: bool = False, packed=None) -> torch.Tensor:
    """K11: the element-level form: convert ``x`` [R, K] with the given scale bytes [R, K/32]
    (1 .. 254) -> packed codes. ``reference=True`` runs the integer kernel."""
    return _mxq_down("ntm_mxq_reference_cvt" if reference else "ntm_mxq_cvt", x, fmt, scales, packed, rounding, seed)[0]


def _mxq_up(entry: str, packed, scales, fmt, dtype, out):
    f = mx_format_id(fmt)
    bits = mx_bits(f)
    for name, t in (("packed", packed), ("scales", scales)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 2 or not t.is_contiguous() or not t.is_cuda:
            raise ValueError(f"MX dequantise: {name} must be a contiguous 2-D uint8 GPU tensor")
    if dtype not in _MXQ_DTYPE:
        raise ValueError("MX dequantise: dtype must be torch.float32 or torch.bfloat16")
    R, K = packed.shape[0], packed.shape[1] * 8 // bits
    if (packed.shape[1] * 8) % bits or tuple(scales.shape) != (R, K // MX_BLOCK) or scales.device != packed.device:
        raise ValueError("MX dequantise needs packed [R, K*bits/8] and scales [R, K/32] on one device")
    if out is None:
        out = torch.empty((R, K), dtype=dtype, device=packed.device)
    elif out.dtype != dtype or out.dim() != 2 or tuple(out.shape) != (R, K) or out.stride(1) != 1 or out.device != packed.device:
        raise ValueError("MX dequantise: out must be [R, K] of the asked dtype with contiguous rows")
    ldx = out.stride(0) if R > 1 else max(out.stride(0), K)
    with torch.cuda.device(packed.device):
        rc = getattr(lib(), entry)(f, _MXQ_DTYPE[dtype], packed.data_ptr(), scales.data_ptr(), out.data_ptr(), R, K, ldx,
                                   stream_handle())
    check(rc, entry)
    return out


def mx_dequantize(packed: torch.Tensor, scales: torch.Tensor, fmt, dtype=torch.float32, out=None) -> torch.Tensor:
    """K11: the inverse of ``mx_quantize`` on the device: code value * 2^(byte - 127) as fp32, or
    that rounded to nearest even as bf16. Not judged: results outside the normal fp32 range and
    the NaN / Inf codes of e4m3 / e5m2 come out as the instruction makes them. Stream-ordered."""
    return _mxq_up("ntm_mxq_dequantize", packed, scales, fmt, dtype, out)


def mx_dequantize_reference_gpu(packed: torch.Tensor, scales: torch.Tensor, fmt, dtype=torch.float32, out=None):
    """K11: ``mx_dequantize`` by integer bit arithmetic only."""
    return _mxq_up("ntm_mxq_reference_dequantize", packed, scales, fmt, dtype, out)


def mxq_to_device(bits, device, bf16: bool = False) -> torch.Tensor:
    """fp32 bit patterns (numpy uint32, any strides kept as a dense copy) -> an fp32 GPU tensor,
    or with ``bf16`` their upper halves as a bf16 tensor."""
    b = np.ascontiguousarray(bits, dtype=np.uint32)
    if bf16:
        return bits_to_tensor((b >> np.uint32(16)).astype(np.uint16), device, torch.bfloat16)
    return bits_to_tensor(b, device, torch.float32)
