"""K11 on the GPU: ``ops.mx_quantize`` / ``mx_dequantize`` / ``mxq_cvt`` (the gfx950
scaled-conversion instructions) and the integer reference kernels, bitwise against the numpy
mirror ``ops.mxq`` - the conversion sweeps, block quantise with sentinels, the round trip, the
end-to-end product through ``mx_gemm``, stochastic rounding's two properties, the argument
checks and ``models.mxq_check``."""
import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import models, ops
from nvidia_terraform_modules_amd.ops import mxq
from nvidia_terraform_modules_amd.ops._lib import lib, stream_handle

pytestmark = pytest.mark.gpu

FORMATS = ops.MX_FORMATS
HIP_ERROR_INVALID_VALUE = 1
SENTINEL = 0xA5
# R, K, ldx: one block; 9 blocks (a masked tail, not a wave's worth); several waves; several
# workgroups with strided rows; rows that are not 16-byte aligned (the narrow loads)
BLOCK_CASES = ((1, 32, 32), (3, 96, 96), (128, 128, 128), (257, 4096, 4096 + 64), (5, 64, 66))
E2E_CASES = ((128, 128, 128, 0x4B3B), (256, 384, 512, 0x4B3C))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


def _np(t: torch.Tensor) -> np.ndarray:
    return t.cpu().contiguous().view(torch.uint8).numpy()


def _first(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.argwhere(got != want)
    if not len(bad):
        return ""
    i = tuple(bad[0])
    return f"{len(bad)} differ, first at {i}: expected {int(want[i]):#x}, got {int(got[i]):#x}"


def _u8(a: np.ndarray, dev) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(dev)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("kind", ("down", "down_bf16"))
def test_conversion_sweep_down(dev, fmt, kind):
    i = ops.mxq_make_inputs(kind, fmt)
    want, _ = ops.mxq_quantize_bits(i["x"], fmt, i["scales"][:, None])
    x = ops.mxq_to_device(i["x"], dev, bf16=kind == "down_bf16")
    s = _u8(i["scales"][:, None], dev)
    assert not _first(_np(ops.mxq_cvt(x, s, fmt)), want)
    assert not _first(_np(ops.mxq_cvt(x, s, fmt, reference=True)), want)


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16))
def test_conversion_sweep_up(dev, fmt, dtype):
    i = ops.mxq_make_inputs("up", fmt)
    want = ops.mxq_dequantize_bits(i["packed"], i["scales"], fmt, "bfloat16" if dtype == torch.bfloat16 else "float32")
    p, s = _u8(i["packed"], dev), _u8(i["scales"], dev)
    view = np.uint16 if dtype == torch.bfloat16 else np.uint32
    for fn in (ops.mx_dequantize, ops.mx_dequantize_reference_gpu):
        got = _np(fn(p, s, fmt, dtype)).view(view)
        assert not _first(got, want), fn.__name__


def _guarded(n: int, dev):
    """A uint8 buffer of n bytes with 64 sentinel bytes before and after, and its middle."""
    buf = torch.full((n + 128,), SENTINEL, dtype=torch.uint8, device=dev)
    return buf, buf[64:64 + n]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("bf16", (False, True), ids=("f32", "bf16"))
@pytest.mark.parametrize("R,K,ldx", BLOCK_CASES)
def test_block_quantize(dev, fmt, bf16, R, K, ldx):
    xb = ops.mxq_make_inputs("block", fmt, R, K, ldx, seed=0x4B3B + R, bf16=bf16)["x"]
    want_p, want_s = ops.mxq_quantize_bits(xb[:, :K], fmt)
    x = ops.mxq_to_device(xb, dev, bf16=bf16)[:, :K]
    for fn in (ops.mx_quantize, ops.mx_quantize_reference_gpu):
        pbuf, p = _guarded(want_p.size, dev)
        sbuf, s = _guarded(want_s.size, dev)
        fn(x, fmt, packed=p.view(want_p.shape), scales=s.view(want_s.shape))
        assert not _first(_np(p).reshape(want_p.shape), want_p), fn.__name__
        assert not _first(_np(s).reshape(want_s.shape), want_s), fn.__name__ + " scales"
        for buf in (pbuf, sbuf):
            raw = _np(buf)
            assert (raw[:64] == SENTINEL).all() and (raw[-64:] == SENTINEL).all(), fn.__name__ + " wrote outside"


@pytest.mark.parametrize("fmt", FORMATS)
def test_round_trip_on_the_grid(dev, fmt):
    g = ops.mxq_make_inputs("grid", fmt, 128, 256, N=128, seed=0x4B3B, W=1)
    p, s = _u8(g["a"], dev), _u8(g["sa"], dev)
    for dtype in (torch.float32, torch.bfloat16):
        q, qs = ops.mx_quantize(ops.mx_dequantize(p, s, fmt, dtype), fmt)
        assert not _first(_np(q), g["a"]) and not _first(_np(qs), g["sa"]), dtype


@pytest.mark.parametrize("fmt", ("e2m1", "e2m3", "e4m3"))
@pytest.mark.parametrize("M,N,K,seed", E2E_CASES)
def test_end_to_end_through_mx_gemm(dev, fmt, M, N, K, seed):
    W = max(ops.mx_max_spread(fmt, K), 0)     # e4m3: no spread is exact by the bound (test_mxq_cpu.py); 0 is used
    g = ops.mxq_make_inputs("grid", fmt, M, K, N=N, seed=seed, W=W)
    a, sa = ops.mx_quantize(ops.mxq_to_device(g["xa"], dev), fmt)
    b, sb = ops.mx_quantize(ops.mxq_to_device(g["xb"], dev), fmt)
    got = ops.mx_gemm(a, b, sa, sb, fmt)
    host = (_u8(g["a"], dev), _u8(g["b"], dev), _u8(g["sa"], dev), _u8(g["sb"], dev))
    want = ops.mx_reference_gpu(*host, fmt)
    if fmt == "e4m3":
        # No e4m3 product is exact by mx_dense_exact (test_mxq_cpu.py), so the reference kernel's
        # fp32 sums round differently from the matrix core's: measured at 128^3 and spread 0,
        # 16377 of 16384 words differ in their low bits (first: 0xae243056 against 0xae2430df).
        # The operands must be the host's bit for bit, and the product that of the host's operands.
        print(f"e4m3 against mx_reference_gpu: {_first(_np(got).view(np.uint32), _np(want).view(np.uint32))}")
        assert torch.equal(a, host[0]) and torch.equal(b, host[1]) and torch.equal(sa, host[2]) and torch.equal(sb, host[3])
        want = ops.mx_gemm(*host, fmt)
    assert not _first(_np(got).view(np.uint32), _np(want).view(np.uint32))
    assert np.count_nonzero(_np(want).view(np.uint32)) > M * N // 2


@pytest.mark.parametrize("fmt", ("e2m1", "e4m3"))
def test_stochastic_rounding_stays_between_the_neighbours(dev, fmt):
    R, K = 64, 256
    xb = ops.mxq_make_inputs("block", fmt, R, K, seed=7)["x"]
    x = ops.mxq_to_device(xb, dev)
    p, s = ops.mx_quantize(x, fmt, rounding="stochastic", seed=1234)
    s = _np(s)
    assert not _first(s, ops.mxq_scale_bytes(xb, fmt))
    table = mxq.mxq_value_table(fmt)
    mags = np.abs(table[:ops.MXQ_MAX_CODE[fmt] + 1])
    got = table[ops.mx_unpack(_np(p), fmt)]
    with np.errstate(over="ignore"):
        v = np.ldexp(xb.view(np.float32).astype(np.float64), 127 - np.repeat(s, 32, axis=1).astype(np.int64))
    v = np.clip(v, -mags[-1], mags[-1])
    lo = mags[np.clip(np.searchsorted(mags, np.abs(v), side="right") - 1, 0, None)]
    hi = mags[np.clip(np.searchsorted(mags, np.abs(v), side="left"), None, mags.size - 1)]
    ok = (np.abs(got) == lo) | (np.abs(got) == hi)
    sign_ok = (got == 0) | (np.signbit(got) == np.signbit(v))
    print(f"{fmt}: rounded up {np.count_nonzero((np.abs(got) == hi) & (hi != lo))} of {np.count_nonzero(hi != lo)} inexact inputs")
    assert ok.all() and sign_ok.all()
    again, _ = ops.mx_quantize(x, fmt, rounding="stochastic", seed=1234)
    assert torch.equal(again, p), "a seed must reproduce its run"


@pytest.mark.parametrize("fmt", ("e2m1", "e4m3"))
def test_stochastic_rounding_keeps_exact_inputs(dev, fmt):
    g = ops.mxq_make_inputs("grid", fmt, 128, 128, N=128, seed=0x4B3B, W=1)
    x = ops.mxq_to_device(g["xa"], dev)
    want_p, want_s = _u8(g["a"], dev), _u8(g["sa"], dev)
    for seed in range(256):
        p, s = ops.mx_quantize(x, fmt, rounding="stochastic", seed=seed)
        assert torch.equal(p, want_p) and torch.equal(s, want_s), seed


def test_argument_checks_launch_nothing(dev):
    x = torch.zeros((4, 128), dtype=torch.float32, device=dev)
    p = torch.full((4 * 128,), SENTINEL, dtype=torch.uint8, device=dev)
    s = torch.full((64,), SENTINEL, dtype=torch.uint8, device=dev)
    y = torch.full((4, 128), 7.0, dtype=torch.float32, device=dev)
    L = lib()
    st = stream_handle()
    bad = ((4, 4, 48, 48), (5, 4, 64, 64), (-1, 4, 64, 64), (4, 4, 64, 32), (4, 0, 64, 64))   # fmt, R, K, ldx
    for fmt, R, K, ldx in bad:
        assert L.ntm_mxq_quantize(fmt, 0, x.data_ptr(), p.data_ptr(), s.data_ptr(), R, K, ldx, 0, 0, st) == HIP_ERROR_INVALID_VALUE
        assert L.ntm_mxq_cvt(fmt, 0, x.data_ptr(), s.data_ptr(), p.data_ptr(), R, K, ldx, 0, 0, st) == HIP_ERROR_INVALID_VALUE
        assert L.ntm_mxq_reference_quantize(fmt, 0, x.data_ptr(), p.data_ptr(), s.data_ptr(), R, K, ldx, st) == HIP_ERROR_INVALID_VALUE
        assert L.ntm_mxq_reference_cvt(fmt, 0, x.data_ptr(), s.data_ptr(), p.data_ptr(), R, K, ldx, st) == HIP_ERROR_INVALID_VALUE
        assert L.ntm_mxq_dequantize(fmt, 0, p.data_ptr(), s.data_ptr(), y.data_ptr(), R, K, ldx, st) == HIP_ERROR_INVALID_VALUE
        assert L.ntm_mxq_reference_dequantize(fmt, 0, p.data_ptr(), s.data_ptr(), y.data_ptr(), R, K, ldx, st) == HIP_ERROR_INVALID_VALUE
    # a bad dtype, a bad rounding mode, stochastic rounding for a 6-bit format
    assert L.ntm_mxq_quantize(4, 2, x.data_ptr(), p.data_ptr(), s.data_ptr(), 4, 64, 64, 0, 0, st) == HIP_ERROR_INVALID_VALUE
    assert L.ntm_mxq_quantize(4, 0, x.data_ptr(), p.data_ptr(), s.data_ptr(), 4, 64, 64, 2, 0, st) == HIP_ERROR_INVALID_VALUE
    assert L.ntm_mxq_quantize(2, 0, x.data_ptr(), p.data_ptr(), s.data_ptr(), 4, 64, 64, 1, 0, st) == HIP_ERROR_INVALID_VALUE
    torch.cuda.synchronize()
    assert (p == SENTINEL).all() and (s == SENTINEL).all() and (y == 7.0).all()
    assert L.ntm_mxq_shape_ok(1, 32, 32) == 1 and L.ntm_mxq_shape_ok(1, 48, 48) == 0 and L.ntm_mxq_shape_ok(1, 64, 32) == 0


def test_models_mxq_check_passes(dev):
    rep = models.mxq_check(dev, rows=64, cols=256, e2e=128)
    print({k: v for k, v in rep.items() if k != "failures"})
    assert rep["ok"] and not rep["failures"], rep["failures"]
    assert all(v == 0 for v in rep["bad"].values())
    bad = models.mxq_check(dev, rows=64, cols=256, e2e=128, corrupt=True)
    assert not bad["ok"] and len(bad["failures"]) == 1 and bad["bad"]["e2m1"] == 1
    assert bad["failures"][0].startswith("gpu0: mxq e2m1 block: 1 bad word(s), first at row ")
