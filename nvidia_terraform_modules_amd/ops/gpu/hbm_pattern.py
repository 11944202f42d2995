"""K4: HBM pattern fill and on-device compare (validation/include/ntm/hbm_pattern.hpp)."""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .._lib import check, lib, stream_handle
from ._common import unpack_record

# Pattern ids of the C ABI.
HBM_PATTERN_ADDR = 0
HBM_PATTERN_HASH = 1
HBM_PATTERNS = {"addr": HBM_PATTERN_ADDR, "hash": HBM_PATTERN_HASH}


def hbm_pattern_id(pattern: int | str) -> int:
    p = HBM_PATTERNS.get(pattern.lower()) if isinstance(pattern, str) else pattern
    if p not in (HBM_PATTERN_ADDR, HBM_PATTERN_HASH):
        raise ValueError(f"unknown HBM pattern {pattern!r} (addr = 0, hash = 1)")
    return p


def hbm_pattern_check_args(t: torch.Tensor, base: int) -> int:
    """Bytes of ``t``; raises unless it is contiguous and size and base are 16-byte multiples."""
    nbytes = t.numel() * t.element_size()
    if not t.is_contiguous() or nbytes % 16 or base % 16 or base < 0 or base + nbytes > 2**64:
        raise ValueError("HBM pattern needs a contiguous tensor, bytes % 16 == 0 and base % 16 == 0")
    return nbytes


@dataclass
class HbmPatternReport:
    bad_words: int                 # 8-byte words that differ from the pattern
    bad_bits: int                  # OR of expected ^ got over them (64 bit)
    first_bad_offset: int | None   # smallest base + byte offset of one
    records: list                  # up to 4 of {"offset", "expected", "got"}

    @property
    def ok(self) -> bool:
        return self.bad_words == 0

    def as_dict(self) -> dict:
        return {"bad_words": self.bad_words, "bad_bits": self.bad_bits,
                "first_bad_offset": self.first_bad_offset, "records": self.records, "ok": self.ok}


def hbm_pattern_write(t: torch.Tensor, pattern: int | str, seed: int = 0, invert: bool = False,
                      base: int = 0) -> torch.Tensor:
    """K4: fill ``t``'s bytes with the ADDR (0) or HASH (1) pattern of the logical
    byte range ``base .. base + nbytes`` (formulas: validation/README.md)."""
    nbytes = hbm_pattern_check_args(t, base)
    if not t.is_cuda:
        raise ValueError("hbm_pattern_write needs a GPU tensor")
    rc = lib().ntm_hbm_pattern_write(t.data_ptr(), nbytes, base, hbm_pattern_id(pattern),
                                     seed & (2**64 - 1), int(bool(invert)), stream_handle())
    check(rc, "ntm_hbm_pattern_write")
    return t


def hbm_pattern_verify(t: torch.Tensor, pattern: int | str, seed: int = 0, invert: bool = False,
                       base: int = 0, invert_after: bool = False) -> HbmPatternReport:
    """K4: compare ``t``'s bytes with the pattern on the device (synchronises).
    ``invert_after`` also leaves the complement of the expected pattern in ``t``."""
    nbytes = hbm_pattern_check_args(t, base)
    if not t.is_cuda:
        raise ValueError("hbm_pattern_verify needs a GPU tensor")
    res = new_pattern_result(t.device)
    rc = lib().ntm_hbm_pattern_verify(t.data_ptr(), nbytes, base, hbm_pattern_id(pattern),
                                      seed & (2**64 - 1), int(bool(invert)),
                                      int(bool(invert_after)), res.data_ptr(), stream_handle())
    check(rc, "ntm_hbm_pattern_verify")
    return read_pattern_result(res)


def new_pattern_result(device) -> torch.Tensor:
    """An initialised ntm::hbm::PatternResult (128 bytes) in device memory."""
    res = torch.zeros(lib().ntm_hbm_pattern_result_bytes() // 8, dtype=torch.int64, device=device)
    res[2] = -1                                     # first_bad_offset: all ones
    return res


def read_pattern_result(res: torch.Tensor) -> HbmPatternReport:
    """Copies the record to the host (synchronises) and decodes it (``res``: the tensor, or its
    bytes): ntm::hbm::PatternResult, hbm_test_plan.hpp."""
    bad, bits, first, nrec, *words = unpack_record(res, "QQQI4x12Q")
    recs = [dict(zip(("offset", "expected", "got"), words[3 * i:3 * i + 3])) for i in range(min(nrec, 4))]
    return HbmPatternReport(bad_words=bad, bad_bits=bits, first_bad_offset=first if bad else None,
                            records=sorted(recs, key=lambda r: r["offset"]))
