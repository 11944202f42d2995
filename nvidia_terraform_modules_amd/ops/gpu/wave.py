"""K12: wave data paths and the special-function unit (validation/include/ntm/wave_paths.hpp,
wave_paths_plan.hpp). The host side (op list, maps, generators, brackets) is numpy: ops/wave.py."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from .._lib import check, lib, stream_handle
from .. import wave as _wave
from ._common import bits_to_tensor


def _wave_words(t, name, device=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.element_size() != 4 or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous GPU tensor of 32-bit elements")
    if device is not None and t.device != device:
        raise ValueError(f"{name} must be on {device}")
    return t


def wave_to_device(words, device) -> torch.Tensor:
    """numpy uint32 words -> an int32 GPU tensor of the same bits."""
    return bits_to_tensor(np.asarray(words, dtype=np.uint32), device)


def _wave_lane(reference, op, ctrl, x, old):
    if isinstance(op, str):
        op = _wave.wave_lane_op_index(op if ctrl is None else f"{op} {ctrl}")
    op = int(op)
    x, old = _wave_words(x, "x"), _wave_words(old, "old", x.device)
    if x.numel() != old.numel():
        raise ValueError("x and old must have one size")
    out = torch.zeros_like(x, dtype=torch.int32)
    with torch.cuda.device(x.device):
        rc = lib().ntm_wave_lane(int(reference), op, 1, x.data_ptr(), old.data_ptr(), out.data_ptr(), x.numel(), stream_handle())
    check(rc, "ntm_wave_lane")
    return out


def wave_lane(op, ctrl, x: torch.Tensor, old: torch.Tensor) -> torch.Tensor:
    """K12: one op of the ``lane`` family on the words ``x`` (and ``old``: the DPP old value, the
    second register of a swap), a multiple of 256 words, each 64 one wave. ``op`` is an index
    into ``wave_lane_ops()`` or the op's name (``"row_shr:3"`` with ``ctrl="bound_ctrl:0"``, or
    the whole name with ``ctrl=None``). A bad op or size raises and launches nothing."""
    return _wave_lane(False, op, ctrl, x, old)


def wave_lane_reference_gpu(op, ctrl, x: torch.Tensor, old: torch.Tensor) -> torch.Tensor:
    """K12: ``wave_lane`` through LDS by the plan's lane map, with no cross-lane instruction."""
    return _wave_lane(True, op, ctrl, x, old)


def _wave_tr(reference, bits, image, stride):
    if not isinstance(image, torch.Tensor) or image.dtype != torch.uint8 or not image.is_cuda or not image.is_contiguous():
        raise ValueError("the image must be a contiguous uint8 GPU tensor")
    stride = int(stride)
    rows = image.numel() // stride if stride > 0 else 0
    n = lib().ntm_wave_tr_out_words(int(bits), rows, stride) if stride > 0 and rows * stride == image.numel() else 0
    if n == 0:
        raise ValueError("bad transposed-read shape (rows a multiple of the block's, stride a multiple of 8 - 16 for "
                         "6-bit - and at least 32, image within 16 KiB)")
    out = torch.zeros(n, dtype=torch.int32, device=image.device)
    with torch.cuda.device(image.device):
        rc = lib().ntm_wave_tr_read(int(reference), int(bits), image.data_ptr(), rows, stride, out.data_ptr(), stream_handle())
    check(rc, "ntm_wave_tr_read")
    return out


def wave_tr_read(bits: int, image: torch.Tensor, stride: int) -> torch.Tensor:
    """K12: one workgroup reads ``image`` (uint8, rows x ``stride`` bytes, 16-byte aligned) through
    the ``bits``-wide transposed LDS read -> int32 words in the layout of
    ``wave_expected_tr_read``. A misaligned image or a bad stride raises and launches nothing."""
    return _wave_tr(False, bits, image, stride)


def wave_tr_read_reference_gpu(bits: int, image: torch.Tensor, stride: int) -> torch.Tensor:
    """K12: ``wave_tr_read`` with byte reads and shifts by the plan's map."""
    return _wave_tr(True, bits, image, stride)


def _sfu_id(op) -> int:
    if isinstance(op, str):
        if op not in _wave.WAVE_SFU_OPS:
            raise ValueError(f"op must be one of {_wave.WAVE_SFU_OPS}")
        return _wave.WAVE_SFU_OPS.index(op)
    return int(op)


def wave_sfu(op, x: torch.Tensor) -> torch.Tensor:
    """K12: the raw result words of one fp32 transcendental instruction on the words ``x``."""
    x = _wave_words(x, "x")
    y = torch.zeros_like(x, dtype=torch.int32)
    with torch.cuda.device(x.device):
        rc = lib().ntm_wave_sfu(_sfu_id(op), x.data_ptr(), y.data_ptr(), x.numel(), stream_handle())
    check(rc, "ntm_wave_sfu")
    return y


def wave_sfu_distance(op, x: torch.Tensor, y: torch.Tensor, bound: int | None = None) -> dict:
    """K12: the ordered-integer distance of the results ``y`` of ``op`` on ``x`` from the host's
    brackets (``ops.wave_sfu_brackets``), computed on the device in integers: ``max_d``,
    ``max_index``, and with a ``bound`` the count ``beyond`` it and ``first_beyond``."""
    x, y = _wave_words(x, "x"), _wave_words(y, "y", x.device)
    lo, hi = _wave.wave_sfu_brackets(_sfu_id(op), x.cpu().numpy().view(np.uint32))
    dlo, dhi = wave_to_device(lo, x.device), wave_to_device(hi, x.device)
    res = torch.tensor([0, -1, 0, -1], dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib().ntm_wave_sfu_distance(y.data_ptr(), dlo.data_ptr(), dhi.data_ptr(), x.numel(),
                                         0xFFFFFFFF if bound is None else int(bound), res.data_ptr(), stream_handle())
    check(rc, "ntm_wave_sfu_distance")
    r = res.cpu().numpy().view(np.uint32)
    return {"max_d": int(r[0]), "max_index": None if r[0] == 0 else int(r[1]), "beyond": int(r[2]),
            "first_beyond": None if r[2] == 0 else int(r[3])}


def wave_valu(op: str, a: torch.Tensor, b: torch.Tensor, c: torch.Tensor | None = None, reference: bool = False) -> torch.Tensor:
    """K12: ``op="bitop3"``: v_bitop3_b32 of a, b, c under all 256 truth tables -> [256, n];
    ``op="cvt_pk_bf16"``: v_cvt_pk_bf16_f32 of the fp32 words a (low half) and b (high half) -> [n].
    ``reference=True`` evaluates the table bit by bit / rounds in integers."""
    if op not in ("bitop3", "cvt_pk_bf16"):
        raise ValueError("op must be 'bitop3' or 'cvt_pk_bf16'")
    a, b = _wave_words(a, "a"), _wave_words(b, "b", a.device)
    if op == "bitop3":
        c = _wave_words(c, "c", a.device)
    n = a.numel()
    if b.numel() != n or (op == "bitop3" and c.numel() != n):
        raise ValueError("the operands must have one size")
    out = torch.zeros((256, n) if op == "bitop3" else (n,), dtype=torch.int32, device=a.device)
    with torch.cuda.device(a.device):
        rc = lib().ntm_wave_valu(int(reference), 0 if op == "bitop3" else 1, a.data_ptr(), b.data_ptr(),
                                 c.data_ptr() if op == "bitop3" else None, out.data_ptr(), n, stream_handle())
    check(rc, "ntm_wave_valu")
    return out


def wave_sweep(family: str, inputs: torch.Tensor, layout, expected: torch.Tensor | None, grid: int,
               fault_wg: int | None = None, fault_index: int = 0):
    """K12: the per-CU form of one family: ``grid`` workgroups each run it against ``expected``
    and leave one record -> a numpy structured array (``hw_id``, ``xcc_id``, ``simd``, ``magic``,
    ``wg``, ``bad``, ``first`` (complement of the smallest bad index, 0 = none), ``expected``,
    ``got``, ``digest`` [7]). Layout of ``inputs``: wave_paths.hpp. For ``"sfu"`` ``fault_wg`` is the
    key of a CU (``wave_cu_key``) whose workgroups flip bit 10 of word ``fault_index`` of v_exp_f32."""
    fam = _wave.WAVE_FAMILIES.index(family)
    inputs = _wave_words(inputs, "inputs")
    nb = lib().ntm_wave_record_bytes()
    rec = torch.zeros(int(grid) * nb // 8, dtype=torch.int64, device=inputs.device)
    lay = (ctypes.c_uint * max(len(layout or ()), 1))(*(layout or (0,)))
    with torch.cuda.device(inputs.device):
        rc = lib().ntm_wave_sweep(fam, inputs.data_ptr(), inputs.numel(), ctypes.cast(lay, ctypes.c_void_p) if layout else None,
                                  expected.data_ptr() if expected is not None else None, rec.data_ptr(), int(grid),
                                  0xFFFFFFFF if fault_wg is None else int(fault_wg), int(fault_index), stream_handle())
    check(rc, "ntm_wave_sweep")
    dt = _wave_record_dtype()
    assert dt.itemsize == nb
    return rec.cpu().numpy().view(dt)


def wave_sfu_digest(device, grid: int):
    """K12: every workgroup of ``grid`` runs the whole input list of the seven transcendentals;
    -> (records, digests uint64 [grid, 7])."""
    lists = [_wave.wave_sfu_inputs(op)[0] for op in range(7)]
    recs = wave_sweep("sfu", wave_to_device(np.concatenate(lists), device), [len(v) for v in lists], None, grid)
    return recs, recs["digest"]


def wave_sfu_locate(op, x: torch.Tensor, cu_key: int, on_key: bool, grid: int, max_launches: int = 8,
                    fault_key: int | None = None, fault_index: int = 0):
    """K12: the second, small launch behind an inconsistent digest. Of ``grid`` workgroups the first
    that runs on the CU ``cu_key`` (``on_key``; else on any other CU) stores the result words of
    instruction ``op`` on ``x`` -> (words int32 tensor, its record) or ``None`` when no workgroup
    landed there within ``max_launches`` launches (a cap, not a retry)."""
    x = _wave_words(x, "x")
    nb = lib().ntm_wave_record_bytes()
    y = torch.zeros_like(x, dtype=torch.int32)
    for _ in range(max_launches):
        side = torch.zeros(8 + nb // 8, dtype=torch.int64, device=x.device)
        with torch.cuda.device(x.device):
            rc = lib().ntm_wave_sfu_locate(_sfu_id(op), x.data_ptr(), x.numel(), int(cu_key), int(bool(on_key)), side.data_ptr(),
                                           y.data_ptr(), side.data_ptr() + 64, int(grid),
                                           0xFFFFFFFF if fault_key is None else int(fault_key), int(fault_index), stream_handle())
        check(rc, "ntm_wave_sfu_locate")
        raw = side.cpu().numpy()
        if raw[0] & 0xFFFFFFFF:
            return y, raw[8:].view(_wave_record_dtype())[0]
    return None


def _wave_record_dtype():
    return np.dtype([("hw_id", "<u4"), ("xcc_id", "<u4"), ("simd", "u1", 4), ("magic", "<u4"), ("wg", "<u4"), ("bad", "<u4"),
                     ("first", "<u4"), ("expected", "<u4"), ("got", "<u4"), ("pad", "<u4"), ("digest", "<u8", 7)])


def wave_cu_key(rec) -> int:
    """(xcc, se, sh, cu) of a record packed as the header's ``cu_key``."""
    h, x = int(rec["hw_id"]), int(rec["xcc_id"])
    return ((x & 15) << 8) | (((h >> 13) & 7) << 5) | (((h >> 12) & 1) << 4) | ((h >> 8) & 15)
