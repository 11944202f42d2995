"""K9: the Job's atomics and cross-XCD hand-off check."""
from __future__ import annotations

import time

import torch

from ._common import begin


def atomics_check(device: torch.device, slots: int = 4096, wg_per_cu: int = 2, iters: int = 4,
                  heads: int = 8, episodes: int | None = None, episode_size: int = 8, rounds: int = 3,
                  seed: int = 0x4B39, ops=None, corrupt_atomic: bool = False, stale_handoff: bool = False,
                  ticket_inject: int | None = None, backend=None) -> dict:
    """K9, the Job's atomics and cross-XCD hand-off check (``NTM_ATOMICS_CHECK=1``) on
    ``device``: every op of ``ops.ATOMIC_OPS`` on a table of ``slots`` words from
    ``wg_per_cu`` workgroups per CU, compared bitwise with the reference kernel's table; the
    ticket draw on ``heads`` counters; ``rounds`` rounds of the hand-off on ``episodes``
    episodes (default: one workgroup per CU) of ``episode_size`` workgroups. Float operands
    take the largest size the exactness bound allows, up to 255. Returns ``ok``,
    ``failures``, ``message``, ``rmw`` (per op), ``tickets``, ``handoff`` and ``seconds``.
    ``corrupt_atomic`` flips one bit of the fp32 table, ``stale_handoff`` makes one writer of
    the last round leave a line stale, ``ticket_inject`` is ``ops.atomics_tickets``' inject."""
    o, device, gpu = begin(device, backend)
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    xcds = max(1, o.xcd_sweep_xcds(device))
    grid = cus * wg_per_cu
    adds = grid * 256 * iters // slots
    t0 = time.perf_counter()
    failures, rmw = [], {}
    for op in ops or o.ATOMIC_OPS:
        max_abs = 1
        while max_abs < 255 and o.atomics_exact(op, adds, 2 * max_abs + 1):
            max_abs = 2 * max_abs + 1
        got = o.atomics_rmw(op, slots, grid, iters, seed, max_abs, device)
        if corrupt_atomic and op == "add_f32":
            got[slots // 2] ^= 1 << 9
        rmw[op] = o.atomics_summarize("rmw", gpu, op=op, got=got,
                                      expected=o.atomics_rmw_reference(op, slots, grid, iters, seed, max_abs, device))
        rmw[op]["max_abs"] = max_abs
        failures += rmw[op]["failures"]
    tk = o.atomics_tickets(heads, grid, iters, device, inject=ticket_inject)
    tickets = o.atomics_summarize("tickets", gpu, **{k: tk[k] for k in ("counters", "claim", "grid", "iters")})
    failures += tickets["failures"]
    episodes = episodes or cus // episode_size
    inject = (rounds, (episodes // 2) * episode_size + 1) if stale_handoff else None
    recs = o.atomics_handoff(episodes, episode_size, rounds, seed, device, inject=inject)
    handoff = o.atomics_summarize("handoff", gpu, records=recs, episodes=episodes, episode_size=episode_size,
                                  xcds=xcds, launches=rounds)
    failures += handoff["failures"]
    return {"ok": not failures, "failures": failures, "message": failures[0] if failures else "",
            "rmw": rmw, "tickets": tickets, "handoff": handoff, "xcds": xcds,
            "seconds": time.perf_counter() - t0}
