"""K4, the HBM pattern test kernels, on an MI355X: the native write against the
CPU reference bit for bit, the verify kernels' error record, the in-place
inversion, 64-bit offsets on one buffer beyond 4 GiB, argument checks and the
Job's sequence through ``models.validation_job.hbm_memtest``."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

MiB, GiB = 1 << 20, 1 << 30
BASE_CARRY = 2**35 - 4096   # 4096 bytes in, the 8-byte index and the 32-bit word index both carry
# one float4 / less than one tile (4 KiB write, 8 KiB verify) / whole tiles + a tail / ...
SIZES = [16, 4080, 8192 + 16, MiB + 48, 64 * MiB]
SENTINEL = 4096


@pytest.fixture(scope="module")
def ops():
    from nvidia_terraform_modules_amd import ops

    return ops


@functools.lru_cache(maxsize=None)
def _ref_words(nbytes, pattern, seed, base):
    """The reference pattern as CPU int32: computed once per case, shared, never written."""
    from nvidia_terraform_modules_amd.ops import reference

    t = torch.empty(nbytes // 4, dtype=torch.int32)
    reference.hbm_pattern_write(t, pattern, seed=seed, base=base)
    return t


def ref_words(nbytes, pattern, seed, invert, base):
    r = _ref_words(nbytes, pattern, seed, base)
    return ~r if invert else r


def _buf(nbytes):
    """nbytes of device memory followed by a 4 KiB sentinel of 0xA5."""
    raw = torch.full((nbytes + SENTINEL,), 0xA5, dtype=torch.uint8, device="cuda")
    return raw, raw[:nbytes].view(torch.int32)


@pytest.mark.parametrize("base", [0, BASE_CARRY], ids=["base0", "base_carry"])
@pytest.mark.parametrize("invert", [False, True], ids=["plain", "inverted"])
@pytest.mark.parametrize("pattern", [0, 1], ids=["addr", "hash"])
@pytest.mark.parametrize("nbytes", SIZES)
def test_write_matches_reference_bit_for_bit(ops, nbytes, pattern, invert, base):
    seed = 0x0123_4567_89AB_CDEF
    raw, t = _buf(nbytes)
    ops.hbm_pattern_write(t, pattern, seed=seed, invert=invert, base=base)
    torch.cuda.synchronize()
    assert torch.equal(t.cpu(), ref_words(nbytes, pattern, seed, invert, base))
    assert bool((raw[nbytes:] == 0xA5).all()), "wrote past the end of the buffer"
    rep = ops.hbm_pattern_verify(t, pattern, seed=seed, invert=invert, base=base)
    assert rep.ok and rep.bad_words == 0 and rep.first_bad_offset is None and rep.records == []
    assert torch.equal(t.cpu(), ref_words(nbytes, pattern, seed, invert, base))   # verify stores nothing


@pytest.mark.parametrize("base", [0, BASE_CARRY], ids=["base0", "base_carry"])
@pytest.mark.parametrize("pattern", [0, 1], ids=["addr", "hash"])
@pytest.mark.parametrize("nbytes", [8192 + 16, MiB + 48])
def test_verify_finds_one_flipped_bit(ops, nbytes, pattern, base):
    seed = 77
    _, t = _buf(nbytes)
    n = nbytes // 4
    for word in (0, (n // 2) | 1, n - 1):              # first / a middle (upper half) / last int32
        ops.hbm_pattern_write(t, pattern, seed=seed, base=base)
        t[word] ^= 1 << 13
        rep = ops.hbm_pattern_verify(t, pattern, seed=seed, base=base)
        assert not rep.ok and rep.bad_words == 1, (word, rep)
        assert rep.first_bad_offset == base + word // 2 * 8, (word, rep)
        assert rep.bad_bits == (1 << 13) << (32 * (word % 2)), (word, rep)
        exp = ref_words(nbytes, pattern, seed, False, base).view(torch.int64)[word // 2].item()
        assert rep.records == [{"offset": base + word // 2 * 8, "expected": exp & (2**64 - 1),
                                "got": (exp & (2**64 - 1)) ^ rep.bad_bits}]


def test_verify_counts_many_bad_words_and_keeps_four_records(ops):
    nbytes = MiB + 48
    _, t = _buf(nbytes)
    ops.hbm_pattern_write(t, "hash", seed=1)
    bad = torch.arange(10, nbytes // 4, 20011, device="cuda")      # even int32 indices and odd ones
    t[bad] ^= 0x101
    rep = ops.hbm_pattern_verify(t, "hash", seed=1)
    assert rep.bad_words == bad.numel() and rep.first_bad_offset == 10 // 2 * 8
    assert rep.bad_bits == 0x101 | (0x101 << 32)
    assert len(rep.records) == 4
    offs = {int(b) // 2 * 8 for b in bad.cpu()}
    assert all(r["offset"] in offs and r["expected"] ^ r["got"] in (0x101, 0x101 << 32)
               for r in rep.records)


@pytest.mark.parametrize("pattern", [0, 1], ids=["addr", "hash"])
@pytest.mark.parametrize("nbytes", [4080, 8192 + 16, MiB + 48])
def test_verify_invert_leaves_the_inverted_reference(ops, nbytes, pattern):
    seed, base = 5, BASE_CARRY
    raw, t = _buf(nbytes)
    ops.hbm_pattern_write(t, pattern, seed=seed, base=base)
    rep = ops.hbm_pattern_verify(t, pattern, seed=seed, base=base, invert_after=True)
    assert rep.ok
    assert torch.equal(t.cpu(), ref_words(nbytes, pattern, seed, True, base))
    assert bool((raw[nbytes:] == 0xA5).all())
    assert ops.hbm_pattern_verify(t, pattern, seed=seed, invert=True, base=base).ok
    assert not ops.hbm_pattern_verify(t, pattern, seed=seed, base=base).ok


def test_one_buffer_beyond_4_gib(ops):
    """A 32-bit byte offset would wrap at 4 GiB: device write + device verify must be
    clean, three 1 MiB windows must match the reference, and a bit flipped at 4 GiB +
    4096 must be found at that offset."""
    from nvidia_terraform_modules_amd.ops import reference

    if torch.cuda.mem_get_info()[0] < 12 * GiB:
        pytest.skip("needs 12 GiB of free HBM")
    nbytes = 4 * GiB + 8192
    t = torch.empty(nbytes // 4, dtype=torch.int32, device="cuda")
    for pattern in (0, 1):
        ops.hbm_pattern_write(t, pattern, seed=9)
        assert ops.hbm_pattern_verify(t, pattern, seed=9).ok
        # first / straddling the 4 GiB mark (only 8 KiB lie beyond it) / last
        for off in (0, 4 * GiB + 4096 - MiB, nbytes - MiB):
            want = torch.empty(MiB // 4, dtype=torch.int32)
            reference.hbm_pattern_write(want, pattern, seed=9, base=off)
            got = t[off // 4: (off + MiB) // 4].cpu()
            assert got.numel() == want.numel() and torch.equal(got, want), (pattern, off)
    t[(4 * GiB + 4096) // 4] ^= 1 << 13
    rep = ops.hbm_pattern_verify(t, 1, seed=9)
    assert rep.bad_words == 1 and rep.first_bad_offset == 4 * GiB + 4096 and rep.bad_bits == 1 << 13
    del t


def test_argument_checks(ops):
    t = torch.zeros(64, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.hbm_pattern_write(t[:6], 0)                # 24 bytes
    with pytest.raises(ValueError):
        ops.hbm_pattern_verify(t[:6], 0)
    with pytest.raises(ValueError):
        ops.hbm_pattern_write(t, 0, base=8)
    with pytest.raises(ValueError):
        ops.hbm_pattern_verify(t, 0, base=24)
    with pytest.raises(ValueError):
        ops.hbm_pattern_write(t, 2)
    # the C ABI itself refuses them too (hipErrorInvalidValue = 1)
    from nvidia_terraform_modules_amd.ops import _lib

    lib = _lib.lib()
    res = torch.zeros(16, dtype=torch.int64, device="cuda")
    assert lib.ntm_hbm_pattern_result_bytes() == 128
    assert lib.ntm_hbm_pattern_write(t.data_ptr(), 24, 0, 0, 0, 0, _lib.stream_handle()) == 1
    assert lib.ntm_hbm_pattern_write(t.data_ptr(), 32, 8, 0, 0, 0, _lib.stream_handle()) == 1
    assert lib.ntm_hbm_pattern_verify(t.data_ptr(), 24, 0, 0, 0, 0, 0, res.data_ptr(),
                                      _lib.stream_handle()) == 1
    assert lib.ntm_hbm_pattern_verify(t.data_ptr(), 32, 8, 0, 0, 0, 0, res.data_ptr(),
                                      _lib.stream_handle()) == 1
    torch.cuda.synchronize()
    assert not t.any()


def test_memtest_runs_the_jobs_sequence(ops):
    from nvidia_terraform_modules_amd.models.validation_job import hbm_memtest

    rep = hbm_memtest(torch.device("cuda"), 256 * MiB, chunk_bytes=64 * MiB)
    assert rep["ok"] and rep["bad_words"] == 0, rep
    assert rep["chunks"] == 4 and rep["bytes"] == 256 * MiB
    assert rep["write_GBps"] > 0 and rep["verify_GBps"] > 0
