"""K10 on the GPU: the fp64 / fp32 / fp16 / int8 MFMA and 2:4-sparse bf16 / int8 SMFMAC GEMMs,
bitwise against the exact numpy table (``ops.mcore_matmul_bits``) - the decode sweep, dense at
one tile and one K-step, dense at several tiles and K-steps with guard words round C - plus the
reference kernel, the compare, the argument checks and ``models.mcore_check``."""
import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import models, ops
from nvidia_terraform_modules_amd.ops._lib import lib, stream_handle

pytestmark = pytest.mark.gpu

FORMATS = ops.MCORE_FORMATS
HIP_ERROR_INVALID_VALUE = 1
# shapes and seeds of the dense cases; tests/test_mcore_cpu.py holds the seeds to "no result is zero"
ONE_TILE = (128, 128, 128, 0x4B3A)
MANY_TILES = (256, 384, 512, 0x4B3B)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _bits(t: torch.Tensor) -> np.ndarray:
    raw = t.cpu().contiguous().view(torch.uint8).numpy().reshape(-1)
    return raw.view(np.uint64 if t.element_size() == 8 else np.uint32).reshape(t.shape)


def _where(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.argwhere(got != want)
    if not len(bad):
        return ""
    r, c = bad[0]
    return f"{len(bad)} differ, first at row {r} col {c}: expected {int(want[r, c]):#x}, got {int(got[r, c]):#x}"


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_sweep_is_bitwise_exact(dev, fmt):
    M, N, K = 256, 128, 128
    for window in range(ops.mcore_decode_windows(fmt)):
        i = ops.mcore_make_inputs("decode", fmt, M, N, K, seed=window)
        d = ops.mcore_to_device(i, dev)
        got = _bits(ops.mcore_gemm(d["a"], d["b"], fmt, d["ai"]))
        want = ops.mcore_matmul_bits(i["a"], i["b"], fmt, i["ai"])
        assert not _where(got, want), (fmt, window, _where(got, want))


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_one_tile_one_k_step(dev, fmt):
    M, N, K, seed = ONE_TILE
    i = ops.mcore_make_inputs("dense", fmt, M, N, K, seed=seed)
    d = ops.mcore_to_device(i, dev)
    want = ops.mcore_matmul_bits(i["a"], i["b"], fmt, i["ai"])
    got = _bits(ops.mcore_gemm(d["a"], d["b"], fmt, d["ai"]))
    assert not _where(got, want), (fmt, _where(got, want))


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_many_tiles_with_guards(dev, fmt):
    """GEMM kernel, reference kernel and table agree; the words either side of C are intact."""
    M, N, K, seed = MANY_TILES
    i = ops.mcore_make_inputs("dense", fmt, M, N, K, seed=seed)
    d = ops.mcore_to_device(i, dev)
    want = ops.mcore_matmul_bits(i["a"], i["b"], fmt, i["ai"])
    acc = torch.float64 if fmt == "f64" else torch.int32 if "i8" in fmt else torch.float32
    guard = 4096
    for op in (ops.mcore_gemm, ops.mcore_reference_gpu):
        buf = torch.full((guard + M * N + guard,), -7, dtype=torch.int64 if fmt == "f64" else torch.int32, device=dev)
        c = buf[guard:guard + M * N].view(acc).view(M, N)
        assert op(d["a"], d["b"], fmt, d["ai"], out=c) is c
        got = _bits(c)
        assert not _where(got, want), (fmt, op.__name__, _where(got, want))
        assert bool((buf[:guard] == -7).all()) and bool((buf[guard + M * N:] == -7).all()), (fmt, op.__name__)
    assert ops.mcore_compare(ops.mcore_reference_gpu(d["a"], d["b"], fmt, d["ai"]),
                             ops.mcore_gemm(d["a"], d["b"], fmt, d["ai"])).ok


@pytest.mark.parametrize("acc", [torch.float32, torch.float64])
def test_compare_reports_a_planted_bit(dev, acc):
    M, N = 256, 384
    g = torch.Generator(device="cpu").manual_seed(3)
    e = torch.randn(M, N, generator=g, dtype=acc).to(dev)
    c = e.clone()
    assert ops.mcore_compare(e, c).ok
    row, col, bit = 201, 77, 9
    word = torch.int64 if acc == torch.float64 else torch.int32
    c.view(word)[row, col] ^= 1 << bit
    rep = ops.mcore_compare(e, c)
    assert rep.count == 1 and rep.first_index == row * N + col and rep.expected ^ rep.got == 1 << bit
    assert rep.expected == int(_bits(e)[row, col])
    c.view(word)[3, 5] ^= 1 << 40 if acc == torch.float64 else 1 << 30
    rep = ops.mcore_compare(e, c)
    assert rep.count == 2 and rep.first_index == 3 * N + 5
    msg = ops.mcore_failure_message(0, "f64" if acc == torch.float64 else "f32", "dense", rep.count, rep.first_index,
                                    rep.expected, rep.got, N)
    assert msg.startswith("gpu0: mcore: f") and "row 3 col 5" in msg and msg.endswith("; 2 differ")


@pytest.mark.parametrize("fmt", FORMATS)
def test_bad_format_or_shape_is_refused_and_c_untouched(dev, fmt):
    i = ops.mcore_make_inputs("dense", fmt, 128, 128, 128, seed=1)
    d = ops.mcore_to_device(i, dev)
    f = FORMATS.index(fmt)
    c = torch.full((128, 128), -7, dtype=torch.int64, device=dev)   # room for either word width
    ai = d["ai"].data_ptr() if d["ai"] is not None else None
    s = stream_handle()
    for entry in (lib().ntm_mcore_gemm, lib().ntm_mcore_reference):
        bad = [entry(6, d["a"].data_ptr(), ai, d["b"].data_ptr(), c.data_ptr(), 128, 128, 128, s),
               entry(-1, d["a"].data_ptr(), ai, d["b"].data_ptr(), c.data_ptr(), 128, 128, 128, s),
               entry(f, d["a"].data_ptr(), ai, d["b"].data_ptr(), c.data_ptr(), 64, 128, 128, s),
               entry(f, d["a"].data_ptr(), ai, d["b"].data_ptr(), c.data_ptr(), 128, 128, 96, s),
               entry(f, d["a"].data_ptr(), ai, d["b"].data_ptr(), c.data_ptr(), 128, 0, 128, s),
               entry(f, None, ai, d["b"].data_ptr(), c.data_ptr(), 128, 128, 128, s),
               entry(f, d["a"].data_ptr(), ai, d["b"].data_ptr(), None, 128, 128, 128, s)]
        if ai is not None:
            bad.append(entry(f, d["a"].data_ptr(), None, d["b"].data_ptr(), c.data_ptr(), 128, 128, 128, s))
        assert bad == [HIP_ERROR_INVALID_VALUE] * len(bad)
    assert lib().ntm_mcore_compare(c.data_ptr(), c.data_ptr(), 16, 2, c.data_ptr(), s) == HIP_ERROR_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((c == -7).all())
    with pytest.raises(ValueError, match="multiples of 128"):
        ops.mcore_gemm(d["a"][:64].contiguous(), d["b"], fmt, None if d["ai"] is None else d["ai"][:64].contiguous())


def test_models_mcore_check_clean_and_corrupt(dev):
    r = models.mcore_check(dev, size=256)
    assert r["ok"] and not r["failures"] and not any(r["bad"].values()), r["failures"]
    r = models.mcore_check(dev, size=256, corrupt=True, max_windows=2)
    assert len(r["failures"]) == 1 and r["bad"]["f64"] == 1 and sum(r["bad"].values()) == 1, r["failures"]
    assert r["failures"][0].startswith("gpu0: mcore: f64 dense: row 128 col 5: expected 0x")
    assert r["failures"][0].endswith(", bad bits 0x200; 1 differ")
