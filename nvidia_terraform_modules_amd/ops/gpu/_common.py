"""What the per-check device wrappers share: the reader of device result records, the bitwise
compare behind K7 and K10, and the numpy-bits-to-tensor step of the ``*_to_device`` helpers."""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np
import torch

from .._lib import check, stream_handle


def unpack_record(raw, fmt: str) -> tuple:
    """The leading fields of a device result record by the ``struct`` format ``fmt`` of its C struct
    (little-endian, padding spelt ``x``); ``raw``: its bytes, or the tensor that holds it (synchronises)."""
    if isinstance(raw, torch.Tensor):
        raw = raw.cpu().numpy().tobytes()
    return struct.unpack_from("<" + fmt, raw)


@dataclass
class CompareReport:
    count: int                 # result words that differ (K7: 32-bit words)
    first_index: int | None    # smallest flat index of one
    expected: int | None       # the words at first_index
    got: int | None

    @property
    def ok(self) -> bool:
        return self.count == 0

    def as_dict(self) -> dict:
        return {"count": self.count, "first_index": self.first_index, "expected": self.expected,
                "got": self.got, "ok": self.ok}


def compare_report(raw, word_bytes: int) -> CompareReport:
    """Decodes a mismatch record: ``ntm::mx::Mismatch`` (mx_plan.hpp; ``word_bytes`` 4: count and
    first_index, then expected / got as 4-byte words at 16 and 20) or ``ntm::mcore::Mismatch``
    (mcore_plan.hpp; 8: expected / got as 8-byte fields at 16 and 24)."""
    count, first, expected, got = unpack_record(raw, "QQII" if word_bytes == 4 else "QQQQ")
    return CompareReport(count, first, expected, got) if count else CompareReport(0, None, None, None)


def _bitwise_compare(entry, expected: torch.Tensor, got: torch.Tensor, word_bytes: int, what: str) -> CompareReport:
    """A check's C compare on two tensors the caller checked. ``entry``: its (mismatch_bytes, compare)
    pair, ``what``: the compare's name in an error; K10's (8-byte record words) also takes the element size."""
    record_bytes, compare = entry
    res = torch.zeros(record_bytes() // 8, dtype=torch.int64, device=got.device)
    res[1] = -1                                     # first_index: all ones
    width = () if word_bytes == 4 else (expected.element_size(),)
    with torch.cuda.device(got.device):
        rc = compare(expected.data_ptr(), got.data_ptr(), expected.numel(), *width, res.data_ptr(), stream_handle())
    check(rc, what)
    return compare_report(res, word_bytes)


def bits_to_tensor(bits, device, view: torch.dtype | None = None) -> torch.Tensor:
    """numpy uint16 / uint32 bit patterns -> a tensor of the same bits on ``device`` (a dense copy):
    int16 / int32, or viewed as ``view`` (bf16 / fp32)."""
    b = np.ascontiguousarray(bits)
    t = torch.from_numpy(b.view(np.int16 if b.dtype == np.uint16 else np.int32).copy()).to(device)
    return t if view is None else t.view(view)
