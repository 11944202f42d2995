"""K6: host-link (PCIe) check (validation/include/ntm/host_link.hpp, host_link_plan.hpp)."""
from __future__ import annotations

import torch

from .._lib import check, lib, stream_handle
from .hbm_pattern import hbm_pattern_id, new_pattern_result, read_pattern_result

HOST_LINK_SLOT_BYTES = 64      # one chase slot: the next index (8 bytes) + padding
HOST_LINK_MAX_BLOCKS = 65536
HOST_LINK_UNROLLS = (1, 2, 4, 8)


def host_link_check_args(host: torch.Tensor, pattern, base: int, blocks, multiple: int = 16) -> int:
    """Bytes of ``host``; ValueError unless the pattern is known, size and base are
    ``multiple``-byte multiples and ``host`` is a contiguous pinned CPU tensor."""
    if pattern is not None:
        hbm_pattern_id(pattern)
    if not isinstance(host, torch.Tensor):
        raise ValueError("host link needs a pinned CPU tensor")
    nbytes = host.numel() * host.element_size()
    if nbytes % multiple or base % 16 or base < 0 or base + nbytes > 2**64:
        raise ValueError(f"host link needs bytes % {multiple} == 0 and base % 16 == 0")
    if blocks is not None and not 1 <= int(blocks) <= HOST_LINK_MAX_BLOCKS:
        raise ValueError(f"blocks must be in 1 .. {HOST_LINK_MAX_BLOCKS}")
    if host.is_cuda or not host.is_contiguous() or not host.is_pinned():
        raise ValueError("host link needs a contiguous pinned CPU tensor (is_pinned())")
    return nbytes


def host_link_default_blocks(pull: bool = False) -> int:
    """Blocks of the persistent push (``pull``: pull) kernel when ``blocks`` is None."""
    return lib().ntm_host_link_default_blocks(int(bool(pull)))


def host_link_tile_bytes(pull: bool = False) -> int:
    """Bytes a block moves per loop trip in the default push (``pull``: pull) build."""
    return lib().ntm_host_link_tile_bytes(int(bool(pull)))


def _host_link_knobs(config):
    if config is None:
        return None
    unroll, nt = config
    if unroll not in HOST_LINK_UNROLLS:
        raise ValueError(f"unroll must be one of {HOST_LINK_UNROLLS}")
    return int(unroll), int(bool(nt))


def host_link_push(host: torch.Tensor, pattern: int | str, seed: int = 0, invert: bool = False,
                   base: int = 0, blocks: int | None = None, config=None) -> torch.Tensor:
    """K6, device->host: the current GPU writes the ADDR (0) or HASH (1) pattern of the
    logical byte range ``base .. base + nbytes`` into the pinned CPU tensor ``host``
    (stream-ordered: synchronise before reading it on the host). ``config`` =
    (unroll, nontemporal) selects a sweep build instead of the measured default."""
    nbytes = host_link_check_args(host, pattern, base, blocks)
    knobs = _host_link_knobs(config)
    args = (host.data_ptr(), nbytes, base, hbm_pattern_id(pattern), seed & (2**64 - 1),
            int(bool(invert)), int(blocks or 0))
    if knobs is None:
        rc = lib().ntm_host_link_push(*args, stream_handle())
    else:
        rc = lib().ntm_host_link_push_ex(*args, *knobs, stream_handle())
    check(rc, "ntm_host_link_push")
    return host


def host_link_pull(host: torch.Tensor, pattern: int | str, seed: int = 0, invert: bool = False,
                   base: int = 0, dst: torch.Tensor | None = None, blocks: int | None = None,
                   config=None, result: torch.Tensor | None = None):
    """K6, host->device: the current GPU reads the pinned CPU tensor ``host`` and compares
    it with the pattern on the device (synchronises; returns the report). ``dst`` (a GPU
    tensor of the same size) also receives the bytes read. With ``result`` (from an earlier
    call's ``new_pattern_result``) the call only enqueues and returns None."""
    nbytes = host_link_check_args(host, pattern, base, blocks)
    knobs = _host_link_knobs(config)
    if dst is not None and (not dst.is_cuda or not dst.is_contiguous()
                            or dst.numel() * dst.element_size() != nbytes):
        raise ValueError("dst must be a contiguous GPU tensor of host's size")
    res = new_pattern_result(dst.device if dst is not None else "cuda") if result is None else result
    args = (host.data_ptr(), nbytes, base, hbm_pattern_id(pattern), seed & (2**64 - 1),
            int(bool(invert)), dst.data_ptr() if dst is not None else None, int(blocks or 0))
    if knobs is None:
        rc = lib().ntm_host_link_pull(*args, res.data_ptr(), stream_handle())
    else:
        rc = lib().ntm_host_link_pull_ex(*args, *knobs, res.data_ptr(), stream_handle())
    check(rc, "ntm_host_link_pull")
    return read_pattern_result(res) if result is None else None


def host_link_chase(host: torch.Tensor, hops: int, start: int = 0) -> tuple[int, float]:
    """K6, read round trip: one lane follows the chain in the pinned CPU tensor ``host``
    (64-byte slots, the first 8 bytes of slot i = the index of the next slot;
    ``reference.host_link_chase_table``) for ``hops`` dependent loads from slot ``start``.
    Returns (final slot index, nanoseconds per hop); synchronises. An index that is no
    slot ends the walk early and raises."""
    nbytes = host_link_check_args(host, None, 0, None, multiple=HOST_LINK_SLOT_BYTES)
    nslots = nbytes // HOST_LINK_SLOT_BYTES
    if nslots < 1 or not 0 <= start < nslots or not 1 <= hops < 2**32:
        raise ValueError("host_link_chase needs >= 1 slot, 0 <= start < slots and 1 <= hops < 2^32")
    dev = torch.cuda.current_device()
    khz = lib().ntm_host_link_clock_khz(dev)
    if khz <= 0:
        raise RuntimeError("cannot read the device's wall clock rate")
    out = torch.zeros(3, dtype=torch.int64, device=torch.device("cuda", dev))
    rc = lib().ntm_host_link_chase(host.data_ptr(), nslots, start, hops, out.data_ptr(), stream_handle())
    check(rc, "ntm_host_link_chase")
    final, ticks, done = (int(v) for v in out.cpu())
    if done != hops:
        raise RuntimeError(f"host_link_chase read {final}, not a slot index, after {done} hops")
    return final, ticks / khz * 1e6 / hops
