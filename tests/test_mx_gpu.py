"""K7, the MX block-scaled matrix check, on the GPU: ``mx_gemm_kernel`` (the scaled f8f6f4
matrix instruction with real E8M0 scales), ``mx_ref_kernel`` and ``mx_compare_kernel`` of
``validation/include/ntm/mx_gemm.hpp`` through ``ops.mx_*``. Every expected value is the
exact integer table of ``ops.mx_matmul_bits`` (numpy) and every compare is bitwise: the
inputs satisfy ``ops.mx_dense_exact``, under which every order of fp32 accumulation is
exact, so no tolerance is involved.

Measured on an MI355X (profiles/mx/README.md): dense e2m1 at K = 512 is bitwise exact at
the generator's cap W = 3 (no element differs), so W was not lowered."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import models, ops
from nvidia_terraform_modules_amd.ops._lib import lib, lib_experimental, stream_handle

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 64, 0xA5A5A5A5
HIP_ERROR_INVALID_VALUE = 1
SEED_FP4 = 0x4B58      # no dense result of the shapes below is an exact zero with these seeds
SEED_FP6 = 0x4B37


@lru_cache(maxsize=None)
def _case(kind, fmt, M, N, K, seed, W):
    """(inputs on the host, their GPU copies, the exact result bits): built once per case."""
    i = ops.mx_make_inputs(kind, fmt, M, N, K, seed=seed, W=W)
    want = ops.mx_matmul_bits(i["a"], i["b"], i["sa"], i["sb"], fmt)
    want.setflags(write=False)
    dev = {k: torch.from_numpy(i[k]).cuda() for k in ("a", "b", "sa", "sb")}
    return i, dev, want


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


def _first_diff(got, want):
    idx = np.flatnonzero(got.ravel() != want.ravel())
    if not idx.size:
        return "equal"
    r, c = divmod(int(idx[0]), want.shape[1])
    return (f"{idx.size} differ, first at row {r} col {c}: expected 0x{int(want[r, c]):08x}, "
            f"got 0x{int(got[r, c]):08x}")


@pytest.mark.parametrize("fmt", ops.MX_FORMATS)
def test_decode_sweep_matches_the_integer_table(fmt):
    """One non-zero per row of A at a k that moves with the row, every finite code, all 15
    windows of A scale bytes 0 .. 254: pins the operand and scale lane maps and the element
    decoders with no assumption about the hardware's internal sum."""
    for window in range(15):
        _, d, want = _case("decode", fmt, 256, 128, 128, window, 0)
        got = _bits(ops.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], fmt))
        assert np.array_equal(got, want), f"{fmt} window {window}: {_first_diff(got, want)}"


def test_dense_e2m1_one_tile_one_k_step():
    _, d, want = _case("dense", "e2m1", 128, 128, 128, SEED_FP4, 3)
    got = _bits(ops.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m1"))
    assert np.array_equal(got, want), _first_diff(got, want)


def test_dense_e2m1_several_tiles_against_table_and_reference_kernel():
    M, N, K = 256, 384, 512
    assert ops.mx_dense_exact("e2m1", K, 3)
    _, d, want = _case("dense", "e2m1", M, N, K, SEED_FP4, 3)
    whole = torch.from_numpy(np.full(M * N + 2 * GUARD, SENTINEL, dtype=np.uint32).view(np.float32)).cuda()
    out = whole[GUARD:GUARD + M * N].view(M, N)
    assert ops.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m1", out=out) is out
    ref = ops.mx_reference_gpu(d["a"], d["b"], d["sa"], d["sb"], "e2m1")
    torch.cuda.synchronize()
    got, raw = _bits(out), _bits(whole)
    print("dense e2m1 256x384x512 W=3 vs table:", _first_diff(got, want))
    print("reference kernel vs table:", _first_diff(_bits(ref), want))
    assert np.array_equal(_bits(ref), want), _first_diff(_bits(ref), want)
    assert np.array_equal(got, want), _first_diff(got, want)
    assert (raw[:GUARD] == SENTINEL).all() and (raw[GUARD + M * N:] == SENTINEL).all()
    assert ops.mx_compare(ref, out).ok


def test_dense_e2m3_with_spread_1():
    assert ops.mx_dense_exact("e2m3", 512, 1) and not ops.mx_dense_exact("e2m3", 512, 2)
    _, d, want = _case("dense", "e2m3", 128, 256, 512, SEED_FP6, 1)
    got = _bits(ops.mx_gemm(d["a"], d["b"], d["sa"], d["sb"], "e2m3"))
    assert np.array_equal(got, want), _first_diff(got, want)
    ref = _bits(ops.mx_reference_gpu(d["a"], d["b"], d["sa"], d["sb"], "e2m3"))
    assert np.array_equal(ref, want), _first_diff(ref, want)


def test_one_scale_byte_changes_exactly_its_row():
    M, N, K = 256, 384, 512
    _, d, want = _case("dense", "e2m1", M, N, K, SEED_FP4, 3)
    sa = d["sa"].clone()
    row, kb = 133, 9
    sa[row, kb] += 1
    got = _bits(ops.mx_gemm(d["a"], d["b"], sa, d["sb"], "e2m1"))
    bad_rows = np.unique(np.nonzero(got != want)[0])
    assert bad_rows.tolist() == [row], bad_rows
    assert (got[row] != want[row]).sum() >= 1


@pytest.mark.parametrize("shape", [(64, 128, 128), (128, 128, 96)])
def test_c_abi_refuses_shapes_that_are_no_multiple_of_128(shape):
    M, N, K = shape
    a = torch.zeros((M, K // 2), dtype=torch.uint8, device="cuda")
    b = torch.zeros((N, K // 2), dtype=torch.uint8, device="cuda")
    sa = torch.full((M, K // 32), 127, dtype=torch.uint8, device="cuda")
    sb = torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda")
    c = torch.full((M, N), 7.0, device="cuda")
    assert lib().ntm_mx_shape_ok(M, N, K) == 0 and lib().ntm_mx_shape_ok(128, 256, 384) == 1
    for entry in (lib().ntm_mx_gemm, lib().ntm_mx_reference):
        rc = entry(4, a.data_ptr(), b.data_ptr(), sa.data_ptr(), sb.data_ptr(), c.data_ptr(), M, N, K,
                   stream_handle())
        assert rc == HIP_ERROR_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((c == 7.0).all())                  # nothing was launched
    with pytest.raises(ValueError, match="multiples of 128"):
        ops.mx_gemm(a, b, sa, sb, "e2m1")


def test_compare_names_the_one_word_that_differs():
    x = torch.arange(100_000, dtype=torch.int32, device="cuda")
    y = x.clone()
    assert ops.mx_compare(x, y).ok
    y[77_777] ^= 1 << 20
    rep = ops.mx_compare(x, y)
    assert (rep.count, rep.first_index, rep.expected, rep.got) == (1, 77_777, 77_777, 77_777 ^ (1 << 20))
    y[5] = -1
    rep = ops.mx_compare(x, y)
    assert (rep.count, rep.first_index, rep.expected, rep.got) == (2, 5, 5, 0xFFFFFFFF)


@pytest.mark.parametrize("fmt", ops.MX_FORMATS)
def test_one_instruction_probe_confirms_the_lane_map(fmt):
    """One scaled MFMA on caller-built register images (libntm_experimental.so): lane l's
    scale byte is that of row l & 15, k-block g = l >> 4; the 6- and 4-bit formats keep that
    block's 32 values in lane l, the 8-bit ones k 16g .. 16g+15 and 64+16g .. 64+16g+15."""
    f = ops.MX_FORMATS.index(fmt)
    i = ops.mx_make_inputs("decode", fmt, 128, 128, 128, seed=7)
    a, b, sa, sb = (i[k][:16] for k in ("a", "b", "sa", "sb"))
    want = ops.mx_matmul_bits(a, b, sa, sb, fmt)
    frag = a.shape[1] // 4                           # bytes of a lane's 32 values
    lanes = np.arange(64)

    def stage(m):
        img = np.zeros((64, 32), dtype=np.uint8)
        if frag == 32:
            rows, g = m[lanes & 15], (lanes >> 4)[:, None]
            k = np.concatenate([16 * g + np.arange(16), 64 + 16 * g + np.arange(16)], axis=1)
            img[:] = np.take_along_axis(rows, k, axis=1)
        else:
            img[:, :frag] = m.reshape(16, 4, frag)[lanes & 15, lanes >> 4]
        return torch.from_numpy(img).cuda()

    def scales(sc):
        return torch.from_numpy(sc[lanes & 15, lanes >> 4].astype(np.int32)).cuda()

    d = torch.empty((64, 4), dtype=torch.float32, device="cuda")
    args = (stage(a), stage(b), scales(sa), scales(sb))
    rc = lib_experimental().ntm_mx_mfma_probe(f, *(t.data_ptr() for t in args), d.data_ptr(), stream_handle())
    assert rc == 0
    torch.cuda.synchronize()
    dc = _bits(d)
    got = np.empty((16, 16), dtype=np.uint32)
    for lane in range(64):
        got[4 * (lane >> 4):4 * (lane >> 4) + 4, lane & 15] = dc[lane]
    assert np.array_equal(got, want), _first_diff(got, want)


def test_model_runs_the_sequence_on_the_gpu():
    rep = models.mx_check(torch.device("cuda"), size=256, iters=2)
    print(rep)
    assert rep["ok"] and rep["bad_elements"] == 0 and rep["formats"] == list(ops.MX_FORMATS)
    assert rep["scale_spread"] == 3 and rep["fp4_tflops"] > 0
