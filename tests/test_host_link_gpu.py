"""K6, the host-link (PCIe) check, on the GPU: the push / pull / chase kernels of
``validation/include/ntm/host_link.hpp`` through ``ops.host_link_*`` on pinned host
memory, bitwise against ``ops.reference.hbm_pattern_words`` on the host, the C ABI's
argument checks and ``models.host_link_check``. No rate is asserted beyond > 0."""
import ctypes
from functools import lru_cache

import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import models, ops
from nvidia_terraform_modules_amd.ops import reference
from nvidia_terraform_modules_amd.ops._lib import lib

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0xA5
SEED = 0x1234_5678_9ABC_DEF1
CARRY_BASE = 2**34 - 2048          # the 32-bit word index crosses 2^32 at byte 2048
HIP_ERROR_INVALID_VALUE = 1


def _sizes(pull=False):
    """16 B; 4080 B; 4096 B; one tile of the shipped U minus 16 B; blocks x tile + 48 B
    (whole tiles for every block of the default grid, then a 3-vector tail); 1 MiB + 16 B."""
    tile, blocks = ops.host_link_tile_bytes(pull), ops.host_link_default_blocks(pull)
    return [16, 4080, 4096, tile - 16, blocks * tile + 48, (1 << 20) + 16]


def _pinned(nbytes):
    """(whole, view): a pinned uint8 tensor of sentinel bytes and its middle, 64 guard
    bytes on each side."""
    whole = torch.full((nbytes + 2 * GUARD,), SENTINEL, dtype=torch.uint8).pin_memory()
    return whole, whole[GUARD:GUARD + nbytes]


@lru_cache(maxsize=None)
def _want(nbytes, pattern, seed, invert, base):
    w = reference.hbm_pattern_words(nbytes, pattern, seed, invert, base).view(np.uint8)
    w.setflags(write=False)
    return w


def _check_push(nbytes, pattern, seed=SEED, invert=False, base=0, blocks=None):
    whole, host = _pinned(nbytes)
    ops.host_link_push(host, pattern, seed=seed, invert=invert, base=base, blocks=blocks)
    torch.cuda.synchronize()
    got = whole.numpy()
    assert np.array_equal(got[GUARD:GUARD + nbytes], _want(nbytes, pattern, seed, invert, base))
    assert (got[:GUARD] == SENTINEL).all() and (got[GUARD + nbytes:] == SENTINEL).all()


@pytest.mark.parametrize("pattern", [0, 1], ids=["addr", "hash"])
def test_push_writes_the_pattern_and_nothing_else(pattern):
    for n in _sizes():
        _check_push(n, pattern)


@pytest.mark.parametrize("base", [0, CARRY_BASE], ids=["base0", "base_carry"])
@pytest.mark.parametrize("invert", [False, True])
@pytest.mark.parametrize("pattern", [0, 1], ids=["addr", "hash"])
def test_push_patterns_invert_and_base(pattern, invert, base):
    _check_push(4096 + 48, pattern, invert=invert, base=base)
    if base:
        assert ((base + 2044) // 4 >> 32, (base + 2048) // 4 >> 32) == (0, 1)


def test_push_with_one_block_and_with_more_blocks_than_tiles():
    tile = ops.host_link_tile_bytes()
    n = 5 * tile + 4080
    _check_push(n, 1, blocks=1)
    _check_push(n, 1, blocks=64)               # 5 tiles: 59 blocks only share the tail
    _check_push(48, 0, blocks=64)              # no whole tile at all
    _check_push(n, 0, blocks=3)


@pytest.mark.parametrize("pattern", [0, 1], ids=["addr", "hash"])
def test_pull_of_a_host_filled_buffer_is_clean_and_dst_gets_the_bytes(pattern):
    for n in _sizes(pull=True):
        whole, host = _pinned(n)
        host.numpy()[:] = _want(n, pattern, SEED, False, CARRY_BASE)
        rep = ops.host_link_pull(host, pattern, seed=SEED, base=CARRY_BASE)
        assert rep.ok and rep.bad_words == 0 and rep.first_bad_offset is None and rep.records == []
        dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        rep = ops.host_link_pull(host, pattern, seed=SEED, base=CARRY_BASE, dst=dst)
        assert rep.ok
        assert np.array_equal(dst.cpu().numpy(), host.numpy())
        # a wrong seed is a mismatch of every word, and the host buffer is only read
        if n <= 4096:
            assert ops.host_link_pull(host, pattern, seed=SEED + 1, base=CARRY_BASE).bad_words == n // 8
        assert np.array_equal(host.numpy(), _want(n, pattern, SEED, False, CARRY_BASE))


def test_pull_with_one_block_and_with_more_blocks_than_tiles():
    n = 5 * ops.host_link_tile_bytes(pull=True) + 4080
    whole, host = _pinned(n)
    host.numpy()[:] = _want(n, 1, 3, True, 0)
    for blocks in (1, 3, 64):
        dst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        assert ops.host_link_pull(host, 1, seed=3, invert=True, dst=dst, blocks=blocks).ok
        assert np.array_equal(dst.cpu().numpy(), host.numpy())


def test_pull_sees_three_words_the_host_changed_after_a_push():
    tile = ops.host_link_tile_bytes(pull=True)
    n, base = 2 * tile + 48, 1 << 20
    whole, host = _pinned(n)
    ops.host_link_push(host, "hash", seed=5, base=base, blocks=2)
    torch.cuda.synchronize()
    assert ops.host_link_pull(host, "hash", seed=5, base=base, blocks=2).ok
    words = host.numpy().view(np.uint64)
    exp = _want(n, 1, 5, False, base).view(np.uint64)
    flips = {5 * 8: 1 << 3, tile + 1000 * 8: 1 << 45, 2 * tile + 40: (1 << 63) | 1}  # first tile, body, tail
    for off, bits in flips.items():
        words[off // 8] ^= np.uint64(bits)
    rep = ops.host_link_pull(host, "hash", seed=5, base=base, blocks=2)
    assert not rep.ok and rep.bad_words == 3 and rep.first_bad_offset == base + 40
    assert rep.bad_bits == (1 << 3) | (1 << 45) | (1 << 63) | 1
    assert rep.records == [{"offset": base + off, "expected": int(exp[off // 8]),
                            "got": int(exp[off // 8]) ^ bits} for off, bits in sorted(flips.items())]
    for off, bits in flips.items():              # ... and a host repair is seen as well
        words[off // 8] ^= np.uint64(bits)
    assert ops.host_link_pull(host, "hash", seed=5, base=base, blocks=2).ok


def test_chase_ends_where_the_host_walk_ends():
    table = reference.host_link_chase_table(1024, seed=11)
    host = torch.from_numpy(table.view(np.int64).reshape(-1).copy()).pin_memory()
    want, _ = reference.host_link_chase(host, 4096)
    final, ns_per_hop = ops.host_link_chase(host, 4096)
    print(f"chase: {ns_per_hop:.0f} ns per hop")
    assert final == want and ns_per_hop > 0
    assert ops.host_link_chase(host, 1024)[0] == 0              # once round the cycle
    assert ops.host_link_chase(host, 1, start=7)[0] == int(table[7, 0])
    host[8 * 3] = 5000                                          # slot 3 points outside the table
    with pytest.raises(RuntimeError, match="not a slot index"):
        ops.host_link_chase(host, 8, start=3)


def test_c_abi_refuses_unmapped_memory_and_bad_sizes():
    L = lib()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    plain = np.zeros(1 << 14, dtype=np.uint8)                   # pageable: not mapped
    p = plain.ctypes.data + (-plain.ctypes.data) % 64
    whole, host = _pinned(4096)
    res = ops.gpu.hbm_pattern.new_pattern_result("cuda")
    out = torch.zeros(3, dtype=torch.int64, device="cuda")
    bad = HIP_ERROR_INVALID_VALUE
    assert L.ntm_host_link_push(p, 4096, 0, 1, 0, 0, 0, s) == bad
    assert L.ntm_host_link_pull(p, 4096, 0, 1, 0, 0, None, 0, res.data_ptr(), s) == bad
    assert L.ntm_host_link_chase(p, 64, 0, 16, out.data_ptr(), s) == bad
    h = host.data_ptr()
    for size, base, pattern in ((24, 0, 1), (4096, 8, 1), (4096, 0, 2), (4096, 0, -1)):
        assert L.ntm_host_link_push(h, size, base, pattern, 0, 0, 0, s) == bad
        assert L.ntm_host_link_pull(h, size, base, pattern, 0, 0, None, 0, res.data_ptr(), s) == bad
    assert L.ntm_host_link_push(h + 8, 4096 - 16, 0, 1, 0, 0, 0, s) == bad      # misaligned pointer
    assert L.ntm_host_link_push_ex(h, 4096, 0, 1, 0, 0, 0, 3, 1, s) == bad       # no such unroll
    assert L.ntm_host_link_pull(h, 4096, 0, 1, 0, 0, None, 0, None, s) == bad    # no record
    assert L.ntm_host_link_chase(h, 64, 64, 16, out.data_ptr(), s) == bad        # start is no slot
    assert L.ntm_host_link_chase(h, 64, 0, 0, out.data_ptr(), s) == bad          # no hops
    torch.cuda.synchronize()
    assert (whole.numpy() == SENTINEL).all()                    # nothing was launched
    assert L.ntm_host_link_push(h, 4096, 0, 1, 0, 0, 0, s) == 0
    assert L.ntm_host_link_push(h, 0, 0, 1, 0, 0, 0, s) == 0   # nothing to do is no error
    torch.cuda.synchronize()
    assert np.array_equal(host.numpy(), _want(4096, 1, 0, False, 0))
    assert L.ntm_host_link_default_blocks(0) >= 1 and L.ntm_host_link_default_blocks(1) >= 1


def test_ops_refuse_gpu_tensors_and_mismatched_dst():
    whole, host = _pinned(4096)
    with pytest.raises(ValueError, match="pinned"):
        ops.host_link_push(torch.zeros(1024, dtype=torch.int32, device="cuda"), 0)
    with pytest.raises(ValueError, match="dst"):
        ops.host_link_pull(host, 0, dst=torch.zeros(4080, dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError, match="dst"):
        ops.host_link_pull(host, 0, dst=torch.zeros(4096, dtype=torch.uint8))


def test_model_runs_the_jobs_sequence():
    rep = models.host_link_check(torch.device("cuda", 0), 8 << 20)
    print({k: v for k, v in rep.items() if k != "records"})
    assert rep["ok"] and rep["bad_words"] == 0 and rep["chase_ok"]
    assert rep["h2d_GBps"] > 0 and rep["d2h_GBps"] > 0
    assert rep["h2d_copy_GBps"] > 0 and rep["d2h_copy_GBps"] > 0 and rep["duplex_GBps"] > 0
    assert rep["read_latency_us"] > 0
