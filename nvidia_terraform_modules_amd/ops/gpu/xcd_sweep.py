"""K8: per-XCD sweep (validation/include/ntm/xcd_sweep.hpp, xcd_sweep_plan.hpp)."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import torch

from .._lib import check, lib, stream_handle
from .hbm_pattern import hbm_pattern_id

XCD_SWEEP_MAGIC = 0x4B385843
XCD_SWEEP_LEVELS = ("l2", "mall", "hbm", "mfma")
XCD_SWEEP_MODES = ("alone", "together")
XCD_SWEEP_TILE_BYTES = 64 * 1024
XCD_SWEEP_CUS_PER_XCD = 32
XCD_SWEEP_MFMA_PER_BATCH = 512     # per wave; a workgroup is 4 waves


def xcd_sweep_record_dtype():
    """numpy dtype of the 64-byte per-workgroup record (ntm::xcs::Record)."""
    dt = np.dtype([("magic", "<u4"), ("hw_id", "<u4"), ("xcc_id", "<u4"), ("wg", "<u4"),
                   ("tiles", "<u4"), ("bad_words", "<u4"), ("rt_ticks", "<u4"), ("cycles", "<u4"),
                   ("rt_start", "<u8"), ("first_off", "<u8"), ("expected", "<u8"), ("got", "<u8")])
    assert dt.itemsize == 64
    return dt


def xcd_sweep_gated(level: int | str, mode: int | str) -> bool:
    """Whether the Job's rate rule judges this cell (mall / together and hbm / together are
    reported only: profiles/xcd_sweep/README.md)."""
    lv = XCD_SWEEP_LEVELS.index(level) if level in XCD_SWEEP_LEVELS else level
    md = XCD_SWEEP_MODES.index(mode) if mode in XCD_SWEEP_MODES else mode
    return bool(lib().ntm_xcd_sweep_gated(lv, md))


def xcd_sweep_xcds(device=None) -> int:
    """XCDs the sweep expects on ``device``: its CU count / 32."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.cuda.get_device_properties(dev).multi_processor_count // XCD_SWEEP_CUS_PER_XCD


def _xcd_sweep_slow(slow_xcd, slow_factor):
    if slow_xcd is None:
        return -1, 1
    if not 0 <= int(slow_xcd) < 16 or not 1 <= int(slow_factor) <= 64:
        raise ValueError("slow_xcd must be in 0 .. 15 and slow_factor in 1 .. 64")
    return int(slow_xcd), int(slow_factor)


def _xcd_sweep_records(rec: torch.Tensor):
    raw = rec.cpu().numpy()            # synchronises
    return raw.view(xcd_sweep_record_dtype()).copy()


def xcd_sweep_read(buf: torch.Tensor, pattern: int | str, seed: int, xcd_mask: int, passes: int,
                   wg_per_cu: int = 2, slow_xcd: int | None = None, slow_factor: int = 1):
    """K8: one launch of the verified per-XCD read; returns the workgroups' records (a numpy
    structured array, ``xcd_sweep_record_dtype``). ``buf`` is ``xcds`` equal slices (a
    multiple of 64 KiB each) that ``hbm_pattern_write(buf, pattern, seed)`` filled; slice x
    is read by the workgroups that find themselves on XCD x, ``passes`` times over, when bit
    x of ``xcd_mask`` is set. ``slow_xcd`` / ``slow_factor``: fault injection, the workgroups
    on that XCD sleep until each tile took ``slow_factor`` times its own duration."""
    if not buf.is_cuda or not buf.is_contiguous():
        raise ValueError("xcd_sweep_read needs a contiguous GPU tensor")
    xcds = xcd_sweep_xcds(buf.device)
    nbytes = buf.numel() * buf.element_size()
    if xcds < 1 or nbytes % xcds or (nbytes // xcds) % XCD_SWEEP_TILE_BYTES or nbytes == 0:
        raise ValueError(f"the buffer must be {xcds} slices, each a multiple of 64 KiB; got {nbytes} bytes")
    slice_bytes = nbytes // xcds
    if passes < 1 or passes * (slice_bytes // XCD_SWEEP_TILE_BYTES) >= 2**31 or wg_per_cu < 1:
        raise ValueError("xcd_sweep_read needs passes >= 1, passes * tiles < 2^31 and wg_per_cu >= 1")
    sx, sf = _xcd_sweep_slow(slow_xcd, slow_factor)
    grid = xcds * XCD_SWEEP_CUS_PER_XCD * int(wg_per_cu)
    with torch.cuda.device(buf.device):
        heads = torch.empty(lib().ntm_xcd_sweep_heads_bytes() // 4, dtype=torch.int32, device=buf.device)
        rec = torch.zeros(grid * 16, dtype=torch.int32, device=buf.device)
        rc = lib().ntm_xcd_sweep_read_launch(buf.data_ptr(), slice_bytes, xcds, int(xcd_mask) & 0xFFFFFFFF,
                                             int(passes), hbm_pattern_id(pattern), seed & (2**64 - 1), grid,
                                             sx, sf, heads.data_ptr(), rec.data_ptr(), stream_handle())
        check(rc, "ntm_xcd_sweep_read_launch")
        return _xcd_sweep_records(rec)


def xcd_sweep_mfma(device=None, batches: int = 64, seed: int = 7, xcd_mask: int | None = None,
                   wg_per_cu: int = 1, slow_xcd: int | None = None, slow_factor: int = 1):
    """K8: one launch of the per-XCD clock probe under matrix load: one 4-wave workgroup per
    CU (``wg_per_cu``), each wave running ``batches`` x 512 back-to-back bf16 MFMAs between
    two stamp pairs. Returns the records; ``tiles`` is the workgroup's MFMA count."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("xcd_sweep_mfma needs a GPU device")
    xcds = xcd_sweep_xcds(dev)
    if xcds < 1 or not 1 <= batches <= 65536 or wg_per_cu < 1:
        raise ValueError("xcd_sweep_mfma needs 1 <= batches <= 65536 and wg_per_cu >= 1")
    sx, sf = _xcd_sweep_slow(slow_xcd, slow_factor)
    mask = (1 << xcds) - 1 if xcd_mask is None else int(xcd_mask) & 0xFFFFFFFF
    grid = xcds * XCD_SWEEP_CUS_PER_XCD * int(wg_per_cu)
    with torch.cuda.device(dev):
        sink = torch.zeros(1, dtype=torch.float32, device=dev)
        rec = torch.zeros(grid * 16, dtype=torch.int32, device=dev)
        rc = lib().ntm_xcd_sweep_mfma_launch(grid, int(batches), seed & 0xFFFFFFFF, xcds, mask, sx, sf,
                                             rec.data_ptr(), sink.data_ptr(), stream_handle())
        check(rc, "ntm_xcd_sweep_mfma_launch")
        return _xcd_sweep_records(rec)


def xcd_sweep_summarize(records, level: int | str, mode: int | str, xcds: int, ratio: float = 0.0,
                        gpu: int = 0, expected_tiles: int = 0, xcd_mask: int | None = None) -> dict:
    """Aggregate records (one launch, or launches with disjoint masks concatenated) per XCD:
    workgroups, CUs, tiles, bytes, span over the XCD's own stamps, rate, clock; conservation
    against ``expected_tiles`` (passes x tiles per slice; 0 = not checked); the rule
    ``rate < ratio x median`` when ``ratio > 0`` and at least 3 XCDs are judged; ``ok``,
    ``failures`` and the Job's one-line ``message``. No GPU needed."""
    lv = XCD_SWEEP_LEVELS.index(level) if level in XCD_SWEEP_LEVELS else level
    md = XCD_SWEEP_MODES.index(mode) if mode in XCD_SWEEP_MODES else mode
    if lv not in range(4) or md not in range(2):
        raise ValueError(f"level is one of {XCD_SWEEP_LEVELS}, mode one of {XCD_SWEEP_MODES}")
    if not 1 <= xcds <= 16:
        raise ValueError("xcds must be in 1 .. 16")
    mask = (1 << xcds) - 1 if xcd_mask is None else int(xcd_mask) & 0xFFFFFFFF
    recs = np.ascontiguousarray(records, dtype=xcd_sweep_record_dtype())
    buf = recs.tobytes()
    args = (buf, len(recs), lv, md, xcds, mask, int(expected_tiles), float(ratio), gpu)
    n = lib().ntm_xcd_sweep_summarize(*args, None, 0)
    out = ctypes.create_string_buffer(n + 1)
    lib().ntm_xcd_sweep_summarize(*args, out, n + 1)
    return json.loads(out.value.decode())
