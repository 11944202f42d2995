"""K8 on the GPU: ``ops.xcd_sweep_read`` / ``ops.xcd_sweep_mfma`` - every XCD reads and
verifies its own slice through its own work queue. Coverage and the conservation law
(tiles pulled per XCD = passes x tiles per slice) together and alone, a slice with fewer
tiles than workgroups, a flipped bit pinned to its XCD and offset, and the slow-XCD
injection that the rate rule must name while the XCD's clock stays normal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MAGIC = 0x4B385843
SEED = 0x5EED
TILE = 64 * 1024
MIB = 1 << 20


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from nvidia_terraform_modules_amd import ops as o
    return o


@pytest.fixture(scope="module")
def xcds(ops):
    n = ops.xcd_sweep_xcds("cuda:0")
    assert n >= 1 and n == torch.cuda.get_device_properties(0).multi_processor_count // 32
    return n


@pytest.fixture(scope="module")
def filled(ops, xcds):
    """xcds x 32 MiB of the hash pattern: shared; the smaller cases read its head (the pattern
    depends on the position alone). The corruption test copies the part it changes."""
    buf = torch.empty(xcds * 32 * MIB, dtype=torch.uint8, device="cuda:0")
    ops.hbm_pattern_write(buf, "hash", SEED)
    torch.cuda.synchronize()
    return buf


def per_xcd_tiles(rec, xcds):
    x = rec["xcc_id"] & 0xF
    return [int(rec["tiles"][x == i].sum()) for i in range(xcds)]


def cus_of(rec, i):
    r = rec[(rec["xcc_id"] & 0xF) == i]
    return len(set(zip((r["hw_id"] >> 13) & 7, (r["hw_id"] >> 12) & 1, (r["hw_id"] >> 8) & 0xF)))


def test_together_covers_every_xcd_and_conserves_tiles(ops, xcds, filled):
    rec = ops.xcd_sweep_read(filled[: xcds * 4 * MIB], "hash", SEED, (1 << xcds) - 1, passes=2)
    assert len(rec) == xcds * 32 * 2
    assert (rec["magic"] == MAGIC).all() and (rec["wg"] == np.arange(len(rec))).all()
    assert ((rec["xcc_id"] & 0xF) < xcds).all()
    assert [cus_of(rec, i) for i in range(xcds)] == [32] * xcds
    assert per_xcd_tiles(rec, xcds) == [2 * 64] * xcds
    assert not rec["bad_words"].any()
    s = ops.xcd_sweep_summarize(rec, "l2", "together", xcds, expected_tiles=2 * 64)
    print({k: s[k] for k in ("rates", "clocks_ghz", "min_over_median")})
    assert s["ok"] and s["message"] == "" and s["bad"] == [] and s["slow"] == []
    assert all(p["cus"] == 32 and p["tiles"] == 128 and p["bytes"] == 128 * TILE for p in s["per_xcd"])
    assert all(0.5 < c < 3.0 for c in s["clocks_ghz"]), s["clocks_ghz"]


def test_fewer_tiles_than_workgroups(ops, xcds, filled):
    rec = ops.xcd_sweep_read(filled[: xcds * 3 * TILE], "hash", SEED, (1 << xcds) - 1, passes=1)
    assert (rec["magic"] == MAGIC).all() and not rec["bad_words"].any()
    assert per_xcd_tiles(rec, xcds) == [3] * xcds
    idle = int((rec["tiles"] == 0).sum())
    print(f"{idle} of {len(rec)} workgroups pulled nothing")
    assert idle >= len(rec) - 3 * xcds
    assert ops.xcd_sweep_summarize(rec, "l2", "together", xcds, expected_tiles=3)["ok"]


def test_alone_only_the_masked_xcd_pulls(ops, xcds, filled):
    for x in (0, xcds - 1):                      # XCD 0, then XCD 7 on a whole MI355X
        rec = ops.xcd_sweep_read(filled[: xcds * 4 * MIB], "hash", SEED, 1 << x, passes=2)
        assert (rec["magic"] == MAGIC).all() and not rec["bad_words"].any()
        want = [0] * xcds
        want[x] = 2 * 64
        assert per_xcd_tiles(rec, xcds) == want
        assert not rec["tiles"][(rec["xcc_id"] & 0xF) != x].any()
        s = ops.xcd_sweep_summarize(rec, "l2", "alone", xcds, expected_tiles=128, xcd_mask=1 << x)
        assert s["ok"] and s["per_xcd"][x]["tiles"] == 128, s["failures"]


def test_flipped_bit_is_pinned_to_its_xcd_and_offset(ops, xcds, filled):
    if xcds < 4:
        pytest.skip("needs XCD 3")
    buf = filled[: xcds * 4 * MIB].clone()
    off = 2 * MIB + 5 * TILE + 4104 + 3          # byte 3 of an 8-byte word of slice 3
    buf[3 * 4 * MIB + off] ^= 0x10
    rec = ops.xcd_sweep_read(buf, "hash", SEED, (1 << xcds) - 1, passes=1)
    s = ops.xcd_sweep_summarize(rec, "mall", "together", xcds, expected_tiles=64, gpu=0)
    assert not s["ok"] and s["bad"] == [3], s["failures"]
    first = s["per_xcd"][3]["first"]
    assert int(first["offset"], 16) == off - 3
    flipped = int(first["expected"], 16) ^ int(first["got"], 16)
    assert flipped == 0x10 << 24 and int(first["bad_bits"], 16) == flipped
    assert s["per_xcd"][3]["bad_words"] == 1
    assert all(p["bad_words"] == 0 and p["first"] is None for p in s["per_xcd"] if p["xcd"] != 3)
    assert s["message"].startswith("gpu0: XCD sweep: xcd 3 read wrong data at mall/together: slice offset "
                                   f"{off - 3:#x}, expected ") and len(s["message"]) < 200
    assert per_xcd_tiles(rec, xcds) == [64] * xcds


def test_slow_xcd_is_named_at_a_normal_clock(ops, xcds, filled):
    if xcds < 6:
        pytest.skip("needs XCD 5")
    full = (1 << xcds) - 1
    tiles = 32 * MIB // TILE
    ops.xcd_sweep_read(filled, "hash", SEED, full, passes=1)                      # warm-up
    clean = ops.xcd_sweep_summarize(ops.xcd_sweep_read(filled, "hash", SEED, full, passes=1),
                                    "hbm", "together", xcds, expected_tiles=tiles)
    rec = ops.xcd_sweep_read(filled, "hash", SEED, full, passes=1, slow_xcd=5, slow_factor=4)
    s = ops.xcd_sweep_summarize(rec, "hbm", "together", xcds, ratio=0.5, expected_tiles=tiles)
    print("clean", clean["rates"], clean["clocks_ghz"])
    print("slow ", s["rates"], s["clocks_ghz"], s["min_over_median"])
    assert per_xcd_tiles(rec, xcds) == [tiles] * xcds and not rec["bad_words"].any()
    rates = s["rates"]
    assert rates[5] == min(rates) and rates[5] < 0.5 * s["median_rate"]
    assert s["slow"] == [5] and not s["ok"] and len(s["failures"]) == 1
    assert s["message"].startswith("gpu0: XCD sweep: xcd 5 slow at hbm/together: ") and len(s["message"]) < 200
    # slow at a normal clock, not throttled: XCD 5 is no slower than the slowest XCD of the clean
    # launch. The high side is not asserted: an XCD that sleeps three quarters of the time draws
    # less power and clocks above the clean spread (printed here; profiles/xcd_sweep/README.md).
    lo, hi = min(clean["clocks_ghz"]), max(clean["clocks_ghz"])
    print(f"clock of xcd 5 {s['clocks_ghz'][5]:.3f} GHz, clean spread {lo:.3f} - {hi:.3f}")
    assert s["clocks_ghz"][5] >= lo, (s["clocks_ghz"], clean["clocks_ghz"])
    # alone: XCD 5 against XCD 2
    alone = np.concatenate([ops.xcd_sweep_read(filled, "hash", SEED, 1 << x, passes=1, slow_xcd=5, slow_factor=4)
                            for x in (5, 2)])
    a = ops.xcd_sweep_summarize(alone, "hbm", "alone", xcds, expected_tiles=tiles, xcd_mask=(1 << 5) | (1 << 2))
    print("alone", a["rates"][5], a["rates"][2])
    assert a["ok"] and a["rule_ran"] is False
    assert a["rates"][5] < 0.5 * a["rates"][2]


def test_mfma_probe_covers_every_cu_and_names_the_slow_xcd(ops, xcds):
    rec = ops.xcd_sweep_mfma("cuda:0", batches=32)
    assert len(rec) == xcds * 32 and (rec["magic"] == MAGIC).all()
    assert (rec["tiles"] == 32 * 512 * 4).all()
    s = ops.xcd_sweep_summarize(rec, "mfma", "together", xcds, ratio=0.5)
    print(s["rates"], s["clocks_ghz"])
    assert all(p["cus"] == 32 and p["workgroups"] == 32 for p in s["per_xcd"])
    clocks = rec["cycles"] / rec["rt_ticks"] * 0.1
    assert ((clocks > 0.5) & (clocks < 3.0)).all(), (clocks.min(), clocks.max())
    assert s["ok"] and s["unit"] == "GMFMA/s", s["failures"]
    if xcds < 6:
        return
    slow = ops.xcd_sweep_summarize(ops.xcd_sweep_mfma("cuda:0", batches=32, slow_xcd=5, slow_factor=4),
                                   "mfma", "together", xcds, ratio=0.5)
    print(slow["rates"], slow["clocks_ghz"], slow["min_over_median"])
    assert slow["slow"] == [5] and slow["message"].startswith("gpu0: XCD sweep: xcd 5 slow at mfma/together: ")


def test_check_model_runs_the_stage(ops, xcds):
    from nvidia_terraform_modules_amd.models import xcd_sweep_check
    out = xcd_sweep_check(torch.device("cuda:0"), hbm_mib=16, levels=("l2", "mfma"))
    print({k: (c["passes"], c["min_over_median"]) for k, c in out["cells"].items()})
    assert out["ok"] and set(out["cells"]) == {"l2/alone", "l2/together", "mfma/together"}, out["failures"]
    for c in out["cells"].values():
        assert min(p["span_ticks"] for p in c["per_xcd"]) >= 10000


def test_argument_refusals(ops, xcds, filled):
    with pytest.raises(ValueError):
        ops.xcd_sweep_read(filled[: xcds * TILE + 16], "hash", SEED, 1, passes=1)   # no whole tiles
    with pytest.raises(ValueError):
        ops.xcd_sweep_read(filled[: xcds * TILE], "hash", SEED, 1, passes=0)
    with pytest.raises(ValueError):
        ops.xcd_sweep_read(filled[: xcds * TILE], "hash", SEED, 1, passes=1, slow_xcd=16, slow_factor=4)
    with pytest.raises(ValueError):
        ops.xcd_sweep_mfma("cuda:0", batches=0)
