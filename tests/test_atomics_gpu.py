"""K9 on the GPU: every kind of global atomic against the reference kernel's and the host's
table (bitwise), the ticket draw, and the cross-XCD hand-off with its conservation law, its
XCD coverage and the stale-line injection.

Shapes: 16 workgroups x 256 threads is the smallest grid that round-robin dispatch spreads
over all 8 XCDs twice; slots = 64 puts 256 operations from every XCD on each slot. The
float ops run again at the largest adds-per-slot their bound allows (fp32 / fp64: the
largest operand instead, since the bound is on the product)."""
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAGIC = 0x4B394154
SEED = 0x5EED
SLOTS, GRID, ITERS = 64, 16, 4
ADDS = GRID * 256 * ITERS // SLOTS        # 256 per slot, 128 per cell of a packed slot
# the largest operand at which 256 adds stay exact: < 2^24, < 2^53, <= 255 per cell, <= 2047 per cell
MAX_ABS = {"add_f32": 65535, "add_f64": 2**45 - 1, "add_bf16x2": 1, "add_f16x2": 15}
# (slots, grid, iters, max_abs) with the most adds per slot the bound allows
AT_THE_BOUND = {
    "add_f32": (1, 16, 4, 1023),           # 16384 adds on ONE slot x 1023 = 2^24 - 16384
    "add_f64": (1, 16, 4, 2**39 - 1),      # 16384 x (2^39 - 1) < 2^53
    "add_bf16x2": (256, 255, 2, 1),        # 510 adds per slot = 255 per cell
    "add_f16x2": (128, 2047, 1, 1),        # 4094 adds per slot = 2047 per cell
}


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nvidia_terraform_modules_amd import ops as o
    return o


@pytest.fixture(scope="module")
def xcds(ops):
    return max(1, ops.xcd_sweep_xcds("cuda:0"))


def _check(ops, op, slots, grid, iters, max_abs):
    got = ops.atomics_rmw(op, slots, grid, iters, SEED, max_abs, "cuda:0")
    ref = ops.atomics_rmw_reference(op, slots, grid, iters, SEED, max_abs, "cuda:0")
    host = ops.atomics_rmw_expected(op, slots, grid * 256 * iters, SEED, max_abs)
    assert (ref == host).all(), f"{op}: the reference kernel and the host table differ"
    s = ops.atomics_summarize("rmw", 0, op=op, got=got, expected=ref)
    assert s["ok"] and s["bad_slots"] == 0, s["failures"]
    assert got.tobytes() == ref.tobytes() == host.tobytes()
    return got


def test_every_op_matches_reference_and_host(ops):
    for op in ops.ATOMIC_OPS:
        got = _check(ops, op, SLOTS, GRID, ITERS, MAX_ABS.get(op, 1))
        if op == "cas_u32":                    # one winner per slot, a contender of that slot
            assert (got >> np.uint64(32) == 1).all() and ((got & np.uint64(0xFFFFFFFF)) == np.arange(1, SLOTS + 1)).all()
        else:
            assert len(set(got.tolist())) > 1, op      # the table is not trivially constant


@pytest.mark.parametrize("op", sorted(AT_THE_BOUND))
def test_float_adds_at_the_bound(ops, op):
    slots, grid, iters, max_abs = AT_THE_BOUND[op]
    adds = grid * 256 * iters // slots
    assert ops.atomics_exact(op, adds, max_abs)
    assert not ops.atomics_exact(op, adds + 1, max_abs + (op in ("add_f32", "add_f64")))
    _check(ops, op, slots, grid, iters, max_abs)


def test_shapes_outside_the_bound_are_refused(ops):
    with pytest.raises(ValueError):
        ops.atomics_rmw("add_f32", SLOTS, GRID, ITERS, SEED, 65536, "cuda:0")
    with pytest.raises(ValueError):
        ops.atomics_rmw("add_bf16x2", SLOTS, GRID, ITERS, SEED, 2, "cuda:0")
    with pytest.raises(ValueError):
        ops.atomics_rmw("add_u32", 60, GRID, ITERS, SEED, 1, "cuda:0")       # 16384 is no multiple of 60
    with pytest.raises(ValueError):
        ops.atomics_rmw("nand_u32", SLOTS, GRID, ITERS, SEED, 1, "cuda:0")


def test_tickets_are_handed_out_exactly_once(ops):
    t = ops.atomics_tickets(2, 16, 4, "cuda:0")
    assert t["claim"].shape == (2, 8192) and (t["counters"][::32][:2] == 8192).all()
    assert (t["claim"] != 0xFFFFFFFF).all()
    assert (np.bincount(t["claim"].ravel(), minlength=16 * 256) == 4).all()
    s = ops.atomics_summarize("tickets", 0, **{k: t[k] for k in ("counters", "claim", "grid", "iters")})
    assert s["ok"] and s["bad"] == 0, s["failures"]


def test_injected_ticket_is_named(ops):
    gid = 1234 + 1                                  # its first draw is from head (gid + 0) % 2 = 1
    t = ops.atomics_tickets(2, 16, 4, "cuda:0", inject=gid)
    s = ops.atomics_summarize("tickets", 0, **{k: t[k] for k in ("counters", "claim", "grid", "iters")})
    print(s["failures"])
    assert not s["ok"] and s["missing"] == 1 and s["short_counters"] == 0
    m = re.match(r"gpu0: atomics: ticket: head 1 ticket (\d+) missing: nobody wrote the entry$", s["message"])
    assert m, s["message"]
    assert t["claim"][1, int(m.group(1))] == 0xFFFFFFFF


@pytest.mark.parametrize("e", [8, 16])
@pytest.mark.parametrize("episodes", [4, 32])
def test_handoff_arrives_fresh(ops, xcds, e, episodes):
    rec = ops.atomics_handoff(episodes, e, rounds=3, seed=SEED, device="cuda:0")
    n = episodes * e
    assert len(rec) == 3 * n and (rec["magic"] == MAGIC).all()
    assert (rec["wg"] == np.tile(np.arange(n), 3)).all() and (rec["episode"] == rec["wg"] // e).all()
    readers = rec[rec["episodes_read"] == 1]
    print(f"E={e} episodes={episodes}: reader tickets ok, writer masks {sorted(set(readers['writer_mask'].tolist()))[:4]}, "
          f"sleeps {np.bincount(rec['sleeps'], minlength=8).tolist()}")
    assert not rec["bad_words"].any() and not rec["warm_bad"].any()
    # conservation: one reader per episode and round, every word of the episode checked
    for r in range(3):
        part = rec[r * n:(r + 1) * n]
        rd = part[part["episodes_read"] == 1]
        assert sorted(rd["episode"].tolist()) == list(range(episodes))
        assert (rd["ticket"] == e - 1).all() and (rd["words_checked"] == e * 256).all()
        for ep in range(episodes):               # every ticket of an episode drawn once
            assert sorted(part["ticket"][part["episode"] == ep].tolist()) == list(range(e))
    s = ops.atomics_summarize("handoff", 0, records=rec, episodes=episodes, episode_size=e, xcds=xcds, launches=3)
    print("pairs covered", s["xcd_pairs_covered"], "cross", s["cross_xcd_pairs"])
    assert s["ok"] and s["words_checked"] == 3 * episodes * e * 256 and s["bad_words"] == 0, s["failures"]
    if xcds == 8:
        assert all(bin(int(m)).count("1") > 1 for m in readers["writer_mask"]), readers["writer_mask"]
        assert s["cross_xcd_pairs"] > 0


def test_stale_line_is_classed_stale_and_pinned_to_its_writer(ops, xcds):
    e, episodes, wg = 8, 4, 2 * 8 + 3
    rec = ops.atomics_handoff(episodes, e, rounds=3, seed=SEED, device="cuda:0", inject=(3, wg))
    s = ops.atomics_summarize("handoff", 0, records=rec, episodes=episodes, episode_size=e, xcds=xcds, launches=3)
    print(s["failures"])
    assert not s["ok"] and s["bad_words"] == 4 and s["stale_words"] == 4 and len(s["failures"]) == 1
    assert not rec[: 2 * episodes * e]["bad_words"].any()           # rounds 1 and 2 are clean
    bad = rec[rec["bad_words"] > 0]
    assert len(bad) == 1 and bad[0]["episode"] == 2 and bad[0]["writer_wg"] == wg and bad[0]["first_class"] == 1
    assert bad[0]["first_off"] == 3 * 4096 + 16 * 16                # slab 3 of the episode, 16-byte word 16
    writer = rec[2 * episodes * e + wg]
    assert (bad[0]["writer_hw"], bad[0]["writer_xcc"]) == (writer["hw_id"], writer["xcc_id"])
    assert re.match(r"gpu0: atomics: handoff: stale word: reader xcd \d+ se \d+ cu \d+, writer xcd \d+ cu \d+ "
                    rf"\(workgroup {wg}\), episode 2, offset 0x3100, expected 0x[0-9a-f]+, got 0x[0-9a-f]+; "
                    r"4 bad, 4 stale$", s["message"]), s["message"]


def test_check_model_passes_and_sees_the_injections(ops):
    from nvidia_terraform_modules_amd.models import atomics_check
    out = atomics_check(torch.device("cuda:0"))
    print({op: r["max_abs"] for op, r in out["rmw"].items()}, out["handoff"]["xcd_pairs_covered"], out["seconds"])
    assert out["ok"] and set(out["rmw"]) == set(ops.ATOMIC_OPS), out["failures"]
    bad = atomics_check(torch.device("cuda:0"), ops=("add_f32",), corrupt_atomic=True, stale_handoff=True)
    assert not bad["ok"] and bad["rmw"]["add_f32"]["bad_slots"] == 1 and bad["handoff"]["stale_words"] == 4
