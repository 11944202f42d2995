"""K9: atomics and cross-XCD hand-off check (validation/include/ntm/atomics.hpp, atomics_plan.hpp)."""
from __future__ import annotations

import ctypes
import json

import numpy as np
import torch

from .._lib import check, lib, stream_handle

ATOMIC_OPS = ("add_u32", "add_u64", "and_u32", "or_u32", "xor_u32", "min_i32", "max_i32", "max_u64",
              "cas_u32", "add_f32", "add_f64", "add_bf16x2", "add_f16x2")
ATOMICS_MAGIC = 0x4B394154
ATOMICS_SLAB_WORDS = 256           # 16-byte words of a 4 KiB slab
ATOMICS_SENTINEL = 0xFFFFFFFF
_ATOMICS_OFF = 0xFFFFFFFF          # no injection


def _atomic_op(op) -> int:
    if op in ATOMIC_OPS:
        return ATOMIC_OPS.index(op)
    if isinstance(op, int) and 0 <= op < len(ATOMIC_OPS):
        return op
    raise ValueError(f"op is one of {ATOMIC_OPS}")


def _atomics_device(device):
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError("the atomics check needs a GPU device")
    return dev


def atomics_exact(op, adds_per_slot: int, max_abs: int) -> bool:
    """Whether ``adds_per_slot`` adds of integers up to ``max_abs`` in size are exact in any
    order for ``op``: adds x max_abs < 2^24 (fp32), < 2^53 (fp64), <= 255 (bf16), <= 2047
    (fp16); a packed slot is two cells that take every second add. Integer ops: always."""
    if adds_per_slot < 0 or max_abs < 0 or adds_per_slot >= 2**64 or max_abs >= 2**64:
        return False
    return bool(lib().ntm_atomics_exact(_atomic_op(op), int(adds_per_slot), int(max_abs)))


def atomics_record_dtype():
    """numpy dtype of the 96-byte per-workgroup hand-off record (ntm::atm::Record)."""
    names = ("magic", "hw_id", "xcc_id", "wg", "episode", "episodes_read", "words_checked", "bad_words",
             "stale_words", "writer_mask", "warm_bad", "first_class", "writer_hw", "writer_xcc", "writer_wg",
             "first_off")
    dt = np.dtype([(n, "<u4") for n in names] + [("expected", "<u8"), ("got", "<u8"), ("ticket", "<u4"),
                                                ("sleeps", "<u4"), ("pad0", "<u4"), ("pad1", "<u4")])
    assert dt.itemsize == 96
    return dt


def _atomics_rmw(fn, what, op, slots, grid, iters, seed, max_abs, device):
    o, dev = _atomic_op(op), _atomics_device(device)
    if not lib().ntm_atomics_rmw_shape_ok(o, int(slots), int(grid), int(iters), int(max_abs)):
        raise ValueError(f"{what}: {ATOMIC_OPS[o]} refuses slots={slots}, grid={grid}, iters={iters}, "
                         f"max_abs={max_abs} (grid x 256 x iters must be a multiple of slots and below 2^32; "
                         "float adds must stay exact: atomics_exact)")
    wide = lib().ntm_atomics_slot_bytes(o) == 8
    with torch.cuda.device(dev):
        table = torch.empty(int(slots), dtype=torch.int64 if wide else torch.int32, device=dev)
        check(fn(o, table.data_ptr(), int(slots), int(grid), int(iters), seed & (2**64 - 1), int(max_abs),
                 stream_handle()), what)
        return table.cpu().numpy().view(np.uint64 if wide else np.uint32).copy()


def atomics_rmw(op, slots: int, grid: int, iters: int, seed: int = 0x4B39, max_abs: int = 1, device=None):
    """K9: ``grid`` x 256 threads x ``iters`` non-returning agent-scope atomics of kind ``op``;
    operation ``k = gid * iters + it`` hits slot ``k % slots``. Returns the table (numpy uint32,
    or uint64 for the 8-byte ops; ``cas_u32``: claim word low, success count high)."""
    return _atomics_rmw(lib().ntm_atomics_rmw_launch, "ntm_atomics_rmw_launch", op, slots, grid, iters, seed,
                        max_abs, device)


def atomics_rmw_reference(op, slots: int, grid: int, iters: int, seed: int = 0x4B39, max_abs: int = 1,
                          device=None):
    """The table ``atomics_rmw`` must produce, from a GPU kernel that uses no atomic: one
    thread per slot folds its operations in order."""
    return _atomics_rmw(lib().ntm_atomics_rmw_reference_launch, "ntm_atomics_rmw_reference_launch", op, slots,
                        grid, iters, seed, max_abs, device)


def atomics_rmw_expected(op, slots: int, total: int, seed: int = 0x4B39, max_abs: int = 1):
    """The same table computed on the host. No GPU needed."""
    o = _atomic_op(op)
    out = np.zeros(int(slots), dtype=np.uint64 if lib().ntm_atomics_slot_bytes(o) == 8 else np.uint32)
    if lib().ntm_atomics_expected(o, int(slots), int(total), seed & (2**64 - 1), int(max_abs), out.ctypes.data):
        raise ValueError("atomics_rmw_expected: refused arguments")
    return out


def atomics_tickets(heads: int, grid: int, iters: int, device=None, inject: int | None = None) -> dict:
    """K9: every thread draws ``iters`` tickets with a returning fetch-add, head
    ``(gid + it) % heads``, and stores its gid into ``claim[head][ticket]``. Returns
    ``counters`` (one per head, as the device holds them: 32 words apart), ``claim``
    (heads x tickets per head) and the shape. ``inject``: that thread writes its first
    ticket one entry too high (fault injection)."""
    dev = _atomics_device(device)
    nbytes = lib().ntm_atomics_ticket_claim_bytes(int(heads), int(grid), int(iters))
    if not nbytes:
        raise ValueError("atomics_tickets needs 1 <= heads <= 1024 dividing grid x 256, and iters >= 1")
    with torch.cuda.device(dev):
        counters = torch.empty(lib().ntm_atomics_counter_bytes(int(heads)) // 4, dtype=torch.int32, device=dev)
        claim = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        check(lib().ntm_atomics_ticket_launch(counters.data_ptr(), claim.data_ptr(), int(heads), int(grid),
                                              int(iters), _ATOMICS_OFF if inject is None else int(inject),
                                              stream_handle()), "ntm_atomics_ticket_launch")
        return {"counters": counters.cpu().numpy().view(np.uint32).copy(),
                "claim": claim.cpu().numpy().view(np.uint32).reshape(int(heads), -1).copy(),
                "heads": int(heads), "grid": int(grid), "iters": int(iters)}


def atomics_handoff(episodes: int, episode_size: int, rounds: int = 1, seed: int = 0x4B39, device=None,
                    inject: tuple[int, int] | None = None):
    """K9: ``rounds`` launches of the cross-XCD hand-off on ``episodes`` episodes of
    ``episode_size`` workgroups; round r finds the slabs holding round r - 1. Returns the
    records of all rounds, concatenated (``atomics_record_dtype``). ``inject = (round, wg)``:
    in that round (1-based) that workgroup leaves one 64-byte line of its slab at last
    round's pattern (fault injection: a lost write-back)."""
    dev = _atomics_device(device)
    nbytes = lib().ntm_atomics_handoff_slab_bytes(int(episodes), int(episode_size))
    if not nbytes or rounds < 1:
        raise ValueError("atomics_handoff needs episodes >= 1, 2 <= episode_size <= 64 and rounds >= 1")
    grid = int(episodes) * int(episode_size)
    with torch.cuda.device(dev):
        slabs = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
        counters = torch.empty(lib().ntm_atomics_counter_bytes(int(episodes)) // 4, dtype=torch.int32, device=dev)
        check(lib().ntm_atomics_handoff_init(slabs.data_ptr(), int(episodes), int(episode_size),
                                             seed & (2**64 - 1), 0, stream_handle()), "ntm_atomics_handoff_init")
        out = []
        for r in range(1, int(rounds) + 1):
            rec = torch.zeros(grid * 24, dtype=torch.int32, device=dev)
            wg = int(inject[1]) if inject is not None and int(inject[0]) == r else _ATOMICS_OFF
            check(lib().ntm_atomics_handoff_launch(slabs.data_ptr(), counters.data_ptr(), rec.data_ptr(),
                                                   int(episodes), int(episode_size), seed & (2**64 - 1), r, wg,
                                                   stream_handle()), "ntm_atomics_handoff_launch")
            out.append(rec.cpu().numpy().view(atomics_record_dtype()).copy())
        return np.concatenate(out)


def atomics_summarize(kind: str, gpu: int = 0, **kw) -> dict:
    """The Job's verdict on one sub-test, no GPU needed: ``ok``, the counts, ``failures`` and
    the one-line ``message``.

    ``"rmw"``: ``op``, ``got``, ``expected`` (tables) - names op, slot, expected, got, bad bits.
    ``"tickets"``: ``counters``, ``claim``, ``grid``, ``iters`` (``atomics_tickets``' result) -
    names head and ticket as missing, duplicate or invalid, and a counter that is short.
    ``"handoff"``: ``records``, ``episodes``, ``episode_size``, ``xcds``, ``launches`` - names
    reader and writer of a stale or corrupt word; one reader per episode and launch, all words
    checked, and at least one cross-XCD pair on a device with more than one XCD."""
    L = lib()
    if kind == "rmw":
        o = _atomic_op(kw["op"])
        dt = np.uint64 if L.ntm_atomics_slot_bytes(o) == 8 else np.uint32
        got, exp = np.ascontiguousarray(kw["got"], dtype=dt), np.ascontiguousarray(kw["expected"], dtype=dt)
        if got.shape != exp.shape:
            raise ValueError("got and expected differ in shape")
        call = lambda out, cap: L.ntm_atomics_summarize_rmw(o, got.ctypes.data, exp.ctypes.data, got.size, gpu, out, cap)
    elif kind == "tickets":
        counters = np.ascontiguousarray(kw["counters"], dtype=np.uint32)
        claim = np.ascontiguousarray(kw["claim"], dtype=np.uint32)
        heads = claim.shape[0]
        if claim.nbytes != L.ntm_atomics_ticket_claim_bytes(heads, kw["grid"], kw["iters"]) or \
                counters.nbytes < L.ntm_atomics_counter_bytes(heads):
            raise ValueError("counters / claim do not fit heads, grid and iters")
        call = lambda out, cap: L.ntm_atomics_summarize_tickets(counters.ctypes.data, claim.ctypes.data, heads,
                                                                kw["grid"], kw["iters"], gpu, out, cap)
    elif kind == "handoff":
        recs = np.ascontiguousarray(kw["records"], dtype=atomics_record_dtype())
        buf = recs.tobytes()
        call = lambda out, cap: L.ntm_atomics_summarize_handoff(buf, len(recs), kw["episodes"], kw["episode_size"],
                                                                kw["xcds"], kw.get("launches", 1), gpu, out, cap)
    else:
        raise ValueError('kind is "rmw", "tickets" or "handoff"')
    n = call(None, 0)
    if not n:
        raise ValueError(f"atomics_summarize({kind!r}): refused arguments")
    out = ctypes.create_string_buffer(n + 1)
    call(out, n + 1)
    return json.loads(out.value.decode())
