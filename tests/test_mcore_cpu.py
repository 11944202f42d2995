"""K10, the matrix-core check of the formats K1 and K7 never issue, without a GPU: the
exactness bound's worked numbers, the 2:4 packers, the generators (deterministic, no dense
result zero at the GPU tests' shapes and seeds, the decode sweep's coverage), the numpy
reference against exact fractions, ``models.mcore_check`` on the CPU backend, the ops'
argument checks, the module's switch, and ``mcore_plan.hpp`` against numpy through a
stand-alone sanitized program."""
import os
import shutil
import subprocess
import zlib
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import models, ops
from nvidia_terraform_modules_amd.ops import mcore, reference

ROOT = Path(__file__).resolve().parents[1]
STACK_DIR = ROOT / "modules" / "amd-gpu-stack"
BIN = ROOT / "validation" / "build" / "amdgpu-validate"
FORMATS = ("f64", "f32", "f16", "i8", "sp_bf16", "sp_i8")
FLOATS = ("f64", "f32", "f16", "sp_bf16")
# the GPU tests' dense cases (tests/test_mcore_gpu.py): shape and seed. The seeds are chosen
# so that no dense result is zero (test_dense_results_are_normal_and_not_zero holds them to it).
GPU_DENSE = ((128, 128, 128, 0x4B3A), (256, 384, 512, 0x4B3B))


def test_format_table():
    assert ops.MCORE_FORMATS == FORMATS
    rows = [ops.mcore_format(f) for f in FORMATS]
    assert [r["elem_bytes"] for r in rows] == [8, 4, 2, 1, 2, 1]
    assert [r["acc_bytes"] for r in rows] == [8, 4, 4, 4, 4, 4]
    assert [r["acc_bits"] for r in rows] == [53, 24, 24, 31, 24, 31]
    assert [r["sparse"] for r in rows] == [False, False, False, False, True, True]
    assert [r["cap_abits"] for r in rows] == [21, 7, 7, 8, 7, 8]
    with pytest.raises(ValueError, match="unknown matrix-core format"):
        ops.mcore_format("bf16")


def test_exactness_bound_worked_numbers():
    # f64: K = 512 at 21 bits is 2^9 * (2^21 - 1)^2 < 2^51 < 2^53
    assert 512 * (2**21 - 1) ** 2 < 2**51 and ops.mcore_exact("f64", 512, 21)
    assert not ops.mcore_exact("f64", 4096, 21) and ops.mcore_exact("f64", 4096, 20)
    assert ops.mcore_max_abits("f64", 512) == 21 and ops.mcore_max_abits("f64", 4096) == 20
    # f32 / f16: K = 512 at 7 bits is 8,258,048 < 2^24
    assert 512 * 127**2 == 8_258_048 < 2**24
    for fmt in ("f32", "f16"):
        assert ops.mcore_exact(fmt, 512, 7) and ops.mcore_max_abits(fmt, 512) == 7
        # K = 4096: 5 bits are exact (3,936,256). So are 6 under the bound as it is defined,
        # K * (2^abits - 1)^2 = 16,257,024 < 16,777,216, and 7 are not (66,064,384).
        assert ops.mcore_exact(fmt, 4096, 5) and 4096 * 31**2 == 3_936_256
        assert ops.mcore_exact(fmt, 4096, 6) and 4096 * 63**2 == 16_257_024 < 2**24
        assert not ops.mcore_exact(fmt, 4096, 7) and ops.mcore_max_abits(fmt, 4096) == 6
    # int8, full range -128 .. 127: any K below 131072
    assert ops.mcore_exact("i8", 131072 - 128, 8) and not ops.mcore_exact("i8", 131072, 8)
    assert ops.mcore_max_abits("i8", 4096) == 8 and ops.mcore_max_abits("sp_i8", 4096) == 8
    # a sparse A has K / 2 products per dot product
    assert ops.mcore_exact("sp_bf16", 1024, 7) and not ops.mcore_exact("sp_bf16", 4096, 7)
    assert ops.mcore_exact("sp_i8", 131072, 8) and not ops.mcore_exact("sp_i8", 262144, 8)
    # outside the element format
    assert not ops.mcore_exact("f64", 128, 22) and not ops.mcore_exact("f16", 128, 8)
    assert not ops.mcore_exact("f32", 128, 0) and not ops.mcore_exact("f32", 0, 3)


def test_compress_expand_round_trip_and_rejection():
    rng = np.random.default_rng(5)
    dense = np.zeros((8, 64), dtype=np.int64)
    for r in range(8):
        for g in range(16):
            keep = rng.choice(4, size=rng.integers(0, 3), replace=False)
            dense[r, 4 * g + keep] = rng.integers(1, 100, size=keep.size)
    ac, ai = ops.mcore_compress(dense)
    assert ac.shape == (8, 32) and ai.shape == (8, 16) and ai.dtype == np.uint8
    assert np.all((ai & 3) < ((ai >> 2) & 3)) and np.all(ai < 16)
    assert np.array_equal(ops.mcore_expand(ac, ai), dense)
    # kept values stay in k order
    one = np.array([[0, 7, 0, 9, 3, 0, 0, 0]])
    ac, ai = ops.mcore_compress(one)
    assert ac.tolist() == [[7, 9, 3, 0]] and ai.tolist() == [[1 | 3 << 2, 0 | 1 << 2]]
    with pytest.raises(ValueError, match="more than two non-zeros"):
        ops.mcore_compress(np.array([[1, 2, 3, 0]]))
    with pytest.raises(ValueError, match="p0 < p1"):
        ops.mcore_expand(np.array([[1, 2]]), np.array([[2 | 1 << 2]], dtype=np.uint8))


@pytest.mark.parametrize("fmt", FORMATS)
def test_generators_are_deterministic(fmt):
    for kind, seed in (("dense", 9), ("decode", 3)):
        x = ops.mcore_make_inputs(kind, fmt, 256, 128, 128, seed=seed)
        y = ops.mcore_make_inputs(kind, fmt, 256, 128, 128, seed=seed)
        z = ops.mcore_make_inputs(kind, fmt, 256, 128, 128, seed=seed + 1)
        assert x["a"].tobytes() == y["a"].tobytes() and x["b"].tobytes() == y["b"].tobytes()
        if kind == "dense" or ops.mcore_decode_windows(fmt) > 1:   # i8's single window holds all 256 codes
            assert x["a"].tobytes() != z["a"].tobytes()
        assert (x["ai"] is None) == (not ops.mcore_format(fmt)["sparse"])
        if x["ai"] is not None:
            assert x["ai"].tobytes() == y["ai"].tobytes() and x["ai"].shape == (256, 32)
            assert x["a"].shape == (256, 64)


@pytest.mark.parametrize("fmt", FORMATS)
def test_dense_results_are_normal_and_not_zero(fmt):
    f = ops.mcore_format(fmt)
    for M, N, K, seed in GPU_DENSE:
        i = ops.mcore_make_inputs("dense", fmt, M, N, K, seed=seed)
        abits = ops.mcore_max_abits(fmt, K)
        assert ops.mcore_exact(fmt, K, abits)
        va, vb = mcore.mcore_values(i["a"], fmt), mcore.mcore_values(i["b"], fmt)
        if f["integer"]:
            assert int(np.abs(va).max()) == 128 and int(va.max()) == 127
        else:  # an integer of abits bits times one power of two per row
            m = np.abs(va).max(axis=1, keepdims=True)
            scaled = va / 2.0 ** np.floor(np.log2(m) - (abits - 1))
            assert np.array_equal(scaled, np.round(scaled)) and np.abs(scaled).max() < 2**abits
            assert np.all(np.isfinite(va)) and np.all(np.isfinite(vb))
        bits = ops.mcore_matmul_bits(i["a"], i["b"], fmt, i["ai"])
        if f["integer"]:
            assert np.count_nonzero(bits) == bits.size
        elif f["acc_bytes"] == 8:
            v = bits.view(np.float64)
            assert np.all(np.abs(v) >= np.finfo(np.float64).tiny) and np.all(np.isfinite(v))
        else:
            v = bits.view(np.float32)
            assert np.all(np.abs(v) >= np.finfo(np.float32).tiny) and np.all(np.isfinite(v))


def test_decode_sweep_visits_every_code_pair_and_slot():
    M, N, K = 256, 128, 128
    assert [ops.mcore_decode_windows(f) for f in FORMATS] == [4, 4, 241, 1, 12, 12]
    # f16: every normal code and both zeros, nothing else
    codes = set()
    for w in range(ops.mcore_decode_windows("f16")):
        a = ops.mcore_make_inputs("decode", "f16", M, N, K, seed=w)["a"].view(np.uint16)
        nz = a[np.arange(M), mcore.mcore_decode_position(np.arange(M), K)]
        codes |= set(int(c) for c in nz)
        assert np.count_nonzero(a) <= M            # one entry per row (a zero code leaves none)
    normal = {s << 15 | e << 10 | m for s in (0, 1) for e in range(1, 31) for m in range(1024)}
    assert codes == normal | {0x0000, 0x8000}
    # int8, dense and sparse: all 256 codes
    for fmt in ("i8", "sp_i8"):
        seen = set()
        for w in range(ops.mcore_decode_windows(fmt)):
            i = ops.mcore_make_inputs("decode", fmt, M, N, K, seed=w)
            a = i["a"] if i["ai"] is None else ops.mcore_expand(i["a"], i["ai"])
            assert np.all(np.count_nonzero(a, axis=1) <= 1)
            seen |= set(int(v) for v in a.view(np.uint8)[a != 0]) | ({0} if np.any(np.count_nonzero(a, axis=1) == 0) else set())
        assert seen == set(range(256))
    # sparse: all six pairs, the non-zero in either kept slot, for every row over the sweep
    for fmt in ("sp_bf16", "sp_i8"):
        per_row = [set() for _ in range(M)]
        for w in range(ops.mcore_decode_windows(fmt)):
            i = ops.mcore_make_inputs("decode", fmt, M, N, K, seed=w)
            pos = mcore.mcore_decode_position(np.arange(M), K)
            for r in range(M):
                byte = int(i["ai"][r, pos[r] // 4])
                slot = (r + w) % 12 // 6
                pair = (byte & 3, byte >> 2 & 3)
                assert pair in ops.mcore.MCORE_PAIRS
                others = np.delete(i["a"][r], 2 * (pos[r] // 4) + slot)
                assert not others.any()
                per_row[r].add((pair, slot))
            assert len({int(b) for b in i["ai"][0]}) == 6     # a row's groups step through the pairs
        assert all(len(s) == 12 for s in per_row)
    # f32 / f64: the lowest fraction bit is set (all 24 / 53 significant bits in use), no subnormal
    a32 = ops.mcore_make_inputs("decode", "f32", M, N, K, seed=1)["a"]
    nz = a32.view(np.uint32)[a32 != 0]
    assert nz.size == M and np.all(nz & 1) and np.all((nz >> 23 & 0xFF) > 0) and len(set(nz >> 23 & 0xFF)) > 20
    a64 = ops.mcore_make_inputs("decode", "f64", M, N, K, seed=1)["a"]
    nz = a64.view(np.uint64)[a64 != 0]
    assert nz.size == M and np.all(nz & np.uint64(1)) and len(set(int(x) >> 32 & 0xFFFFF for x in nz)) > 200


def _fraction(x) -> Fraction:
    return Fraction(float(x)) if isinstance(x, (float, np.floating)) else Fraction(int(x))


@pytest.mark.parametrize("fmt", FORMATS)
def test_matmul_bits_equals_a_fraction_dot(fmt):
    f = ops.mcore_format(fmt)
    for kind, seed in (("dense", 11), ("decode", 2)):
        i = ops.mcore_make_inputs(kind, fmt, 128, 128, 128, seed=seed)
        bits = ops.mcore_matmul_bits(i["a"], i["b"], fmt, i["ai"])
        assert bits.shape == (128, 128) and bits.dtype == (np.uint64 if fmt == "f64" else np.uint32)
        va, vb = mcore.mcore_values(i["a"], fmt), mcore.mcore_values(i["b"], fmt)
        if f["sparse"]:
            va = ops.mcore_expand(va, i["ai"])
        for r, c in ((0, 0), (5, 77), (127, 127), (64, 3)):
            exact = sum(_fraction(x) * _fraction(y) for x, y in zip(va[r], vb[c]))
            if f["integer"]:
                got = Fraction(int(bits[r, c:c + 1].view(np.int32)[0]))
            elif f["acc_bytes"] == 8:
                got = Fraction(float(bits[r, c:c + 1].view(np.float64)[0]))
            else:
                got = Fraction(float(bits[r, c:c + 1].view(np.float32)[0]))
            assert got == exact, (fmt, kind, r, c)


def test_models_mcore_check_runs_on_the_cpu_backend():
    r = models.mcore_check("cpu", size=128, backend=reference)
    assert r["ok"] and r["failures"] == [] and set(r["bad"]) == set(FORMATS) and not any(r["bad"].values())
    r = models.mcore_check("cpu", size=128, backend=reference, corrupt=True)
    assert not r["ok"] and len(r["failures"]) == 1 and r["bad"]["f64"] == 1
    assert r["failures"][0].startswith("gpu0: mcore: f64 dense: row 64 col 5: expected 0x")
    assert r["failures"][0].endswith(", bad bits 0x200; 1 differ")


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    i = reference.mcore_to_device(ops.mcore_make_inputs("dense", "sp_i8", 128, 128, 128), "cpu")
    with pytest.raises(ValueError, match="needs GPU tensors"):
        ops.mcore_gemm(i["a"], i["b"], "sp_i8", i["ai"])
    with pytest.raises(ValueError, match="needs GPU tensors"):
        ops.mcore_reference_gpu(i["a"], i["b"], "sp_i8", i["ai"])
    with pytest.raises(ValueError, match="needs GPU tensors"):
        ops.mcore_compare(torch.zeros(4), torch.zeros(4))
    check = ops.gpu.mcore.mcore_check_args
    assert check(i["a"], i["b"], "sp_i8", i["ai"], need_cuda=False) == (5, 128, 128, 128)
    with pytest.raises(ValueError, match="ai"):
        check(i["a"], i["b"], "sp_i8", None, need_cuda=False)
    with pytest.raises(ValueError, match=r"ai \[M, K/4\]"):
        check(i["a"], i["b"], "sp_i8", i["ai"][:, :16].contiguous(), need_cuda=False)
    with pytest.raises(ValueError, match="multiples of 128"):
        check(i["a"][:, :32].contiguous(), i["b"][:, :64].contiguous(), "sp_i8", i["ai"][:, :16].contiguous(),
              need_cuda=False)
    with pytest.raises(ValueError, match="contiguous 2-D tensor"):
        check(i["a"].float(), i["b"], "sp_i8", i["ai"], need_cuda=False)
    with pytest.raises(ValueError, match="out must be"):
        check(i["a"], i["b"], "sp_i8", i["ai"], torch.zeros(128, 128), need_cuda=False)
    d = torch.zeros(128, 128, dtype=torch.float64)
    with pytest.raises(ValueError, match="multiples of 128"):
        check(d[:64].contiguous(), d, "f64", need_cuda=False)
    with pytest.raises(ValueError, match="unknown matrix-core format"):
        check(d, d, "fp64", need_cuda=False)
    with pytest.raises(ValueError, match="multiples of 128"):
        ops.mcore_make_inputs("dense", "f64", 64, 128, 128)
    with pytest.raises(ValueError, match="unknown matrix-core input kind"):
        ops.mcore_make_inputs("sparse", "f64", 128, 128, 128)
    with pytest.raises(ValueError, match="abits must be"):
        ops.mcore_make_inputs("dense", "f16", 128, 128, 128, abits=8)


# ------------------------------------------------------------ the module
def _stack_local(name, **overrides):
    from nvidia_terraform_modules_amd.tfcheck.config import load_module
    from nvidia_terraform_modules_amd.tfcheck.evaluate import Evaluator, Scope, convert

    mod = load_module(STACK_DIR)
    ev = Evaluator()
    variables = {}
    for vn, v in mod.variables.items():
        if vn in overrides:
            variables[vn] = overrides[vn]
        elif not v.required:
            variables[vn] = convert(ev.eval(v.block.body.attr("default"), Scope({}, {})), v.type_expr)
    scope = Scope(variables, {n: e for n, (e, _, _) in mod.locals.items()}, str(mod.path))
    return ev.eval(mod.locals[name][0], scope)


def test_module_sets_the_variable_only_when_asked():
    off, on = _stack_local("validation_env"), _stack_local("validation_env", validation_mcore_check=True)
    assert "NTM_MCORE_CHECK" not in off and on["NTM_MCORE_CHECK"] == "1"
    assert {k: v for k, v in on.items() if k != "NTM_MCORE_CHECK"} == off
    args = _stack_local("validation_args")
    assert _stack_local("validation_args", validation_mcore_check=True) == args
    assert not [a for a in args if "mcore" in a]
    text = (STACK_DIR / "variables.tf").read_text()
    block = text.split('variable "validation_mcore_check"')[1].split("\n}")[0]
    assert "bool" in block and "false" in block and "profiles/mcore/README.md" in block


def test_injection_without_the_switch_is_refused():
    if not BIN.exists():
        pytest.skip("amdgpu-validate not built (python -m nvidia_terraform_modules_amd.ops.build)")
    e = {k: v for k, v in os.environ.items() if k not in ("NTM_FAULT_INJECT", "NTM_MCORE_CHECK")}
    p = subprocess.run([str(BIN), "--gpus", "1", "--fault-inject", "corrupt_mcore"], capture_output=True,
                       text=True, timeout=60, env=e)
    assert p.returncode == 2 and "fault-inject corrupt_mcore needs NTM_MCORE_CHECK=1" in p.stderr
    assert p.stdout == ""


# ------------------------------------------------- the plan header, sanitized
PLAN_MAIN = r"""
#include "ntm/mcore_plan.hpp"
using namespace ntm::mc;
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
static uint32_t crc32(const uint8_t* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}
static void emit(const Inputs& in) {
  std::vector<uint64_t> c;
  host_reference(in, c);
  std::vector<uint8_t> cb;
  const int wb = kFormatTable[in.fmt].acc_bytes;
  for (uint64_t w : c)
    for (int i = 0; i < wb; ++i) cb.push_back((uint8_t)(w >> (8 * i)));
  std::printf("case %s %zu %08x %zu %08x %zu %08x %08x\n", format_name(in.fmt), in.a.size(),
              crc32(in.a.data(), in.a.size()), in.ai.size(), crc32(in.ai.data(), in.ai.size()), in.b.size(),
              crc32(in.b.data(), in.b.size()), crc32(cb.data(), cb.size()));
}
int main() {
  for (int f = 0; f < kFormats; ++f) {
    const Format& t = kFormatTable[f];
    std::printf("fmt %s %d %d %d %d %d %d %d %d %d %d\n", t.name, t.elem_bytes, t.acc_bytes, t.acc_bits, (int)t.sparse,
                (int)t.integer, t.cap_abits, mcore_max_abits(f, 128), mcore_max_abits(f, 512), mcore_max_abits(f, 4096),
                decode_windows(f));
  }
  // the bound's worked numbers
  REQUIRE(mcore_exact(kF64, 512, 21) && !mcore_exact(kF64, 4096, 21) && mcore_exact(kF64, 4096, 20));
  REQUIRE(mcore_exact(kF32, 512, 7) && mcore_exact(kF16, 512, 7) && mcore_exact(kF16, 4096, 5) && !mcore_exact(kF32, 4096, 7));
  REQUIRE(mcore_exact(kI8, 131072 - 128, 8) && !mcore_exact(kI8, 131072, 8) && !mcore_exact(kF64, 128, 22));
  REQUIRE(shape_ok(128, 256, 384) && !shape_ok(64, 128, 128) && !shape_ok(128, 128, 96) && !shape_ok(0, 128, 128));
  // 2:4 packing: a round trip, kept values in k order, a group of three refused
  {
    const int32_t dense[12] = {0, 7, 0, 9, 3, 0, 0, 0, 0, 0, 0, -4};
    int32_t ac[6], back[12];
    uint8_t ai[3];
    REQUIRE(compress_2of4(dense, 12, ac, ai));
    REQUIRE(ac[0] == 7 && ac[1] == 9 && ac[2] == 3 && ac[3] == 0 && ac[4] == 0 && ac[5] == -4);
    REQUIRE(ai[0] == (1 | 3 << 2) && ai[1] == (0 | 1 << 2) && ai[2] == (0 | 3 << 2));
    expand_2of4(ac, ai, 12, back);
    for (int k = 0; k < 12; ++k) REQUIRE(back[k] == dense[k]);
    const int32_t three[4] = {1, 2, 3, 0};
    REQUIRE(!compress_2of4(three, 4, ac, ai));
  }
  // the generators and the host reference: checksums of bytes and result bits for numpy to match
  for (int f = 0; f < kFormats; ++f) {
    emit(make_dense(f, 128, 128, 128, 0x4B3A, mcore_max_abits(f, 128)));
    emit(make_dense(f, 128, 256, 256, 7, 3));
    emit(make_decode(f, 256, 128, 128, 0));
    emit(make_decode(f, 256, 128, 256, decode_windows(f) - 1));
  }
  Mismatch m;
  mismatch_init(m);
  REQUIRE(m.count == 0 && m.first_index == ~0ull);
  m.count = 1, m.first_index = 5 * 384 + 7, m.expected = 0x42c95523035c06c0ull, m.got = 0x42c95523035c04c0ull;
  std::printf("%s\n", failure_message(3, kF64, "dense", m, 384).c_str());
  m.count = 12, m.first_index = 9, m.expected = 0x41200000, m.got = 0xc1200000u;
  std::printf("%s\n", failure_message(0, kSpI8, "decode", m, 128).c_str());
  return 0;
}
"""


def test_plan_header_matches_numpy_under_sanitizers(tmp_path):
    """Stand-alone program with its own main against mcore_plan.hpp, built with AddressSanitizer
    and UBSan (host code only; nothing is loaded into Python): its format table, generator
    bytes and reference bits must be numpy's."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "mcore_main.cpp", tmp_path / "mcore_main"
    src.write_text(PLAN_MAIN)
    inc = [f"-I{ROOT / 'validation' / 'include'}"]
    if cxx:
        static = (["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx)
                  else ["-static-libsan"])
        cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
               "-fno-sanitize-recover=all", *static, *inc, str(src), "-o", str(exe)]
    elif os.path.exists(hipcc):
        cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
               "-fsanitize=undefined", "-static-libsan", *inc, str(src), "-o", str(exe)]
    else:
        pytest.skip("no C++ compiler")
    subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=300)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr
    lines = p.stdout.strip().splitlines()
    for f, fmt in enumerate(FORMATS):
        t = ops.mcore_format(fmt)
        want = [fmt, t["elem_bytes"], t["acc_bytes"], t["acc_bits"], int(t["sparse"]), int(t["integer"]),
                t["cap_abits"], ops.mcore_max_abits(fmt, 128), ops.mcore_max_abits(fmt, 512),
                ops.mcore_max_abits(fmt, 4096), ops.mcore_decode_windows(fmt)]
        assert lines[f].split()[1:] == [str(w) for w in want]
    at = len(FORMATS)
    for fmt in FORMATS:
        cases = [("dense", 128, 128, 128, 0x4B3A, None), ("dense", 128, 256, 256, 7, 3),
                 ("decode", 256, 128, 128, 0, None), ("decode", 256, 128, 256, ops.mcore_decode_windows(fmt) - 1, None)]
        for kind, M, N, K, seed, abits in cases:
            i = ops.mcore_make_inputs(kind, fmt, M, N, K, seed=seed, abits=abits)
            ai = b"" if i["ai"] is None else i["ai"].tobytes()
            bits = ops.mcore_matmul_bits(i["a"], i["b"], fmt, i["ai"])
            want = ["case", fmt, str(i["a"].nbytes), f"{zlib.crc32(i['a'].tobytes()):08x}", str(len(ai)),
                    f"{zlib.crc32(ai):08x}", str(i["b"].nbytes), f"{zlib.crc32(i['b'].tobytes()):08x}",
                    f"{zlib.crc32(bits.tobytes()):08x}"]
            assert lines[at].split() == want, (kind, fmt, M, N, K, seed)
            at += 1
    assert lines[at] == ops.mcore_failure_message(3, "f64", "dense", 1, 5 * 384 + 7, 0x42c95523035c06c0,
                                                  0x42c95523035c04c0, 384)
    assert lines[at] == ("gpu3: mcore: f64 dense: row 5 col 7: expected 0x42c95523035c06c0, "
                         "got 0x42c95523035c04c0, bad bits 0x200; 1 differ")
    assert lines[at + 1] == ops.mcore_failure_message(0, "sp_i8", "decode", 12, 9, 0x41200000, 0xc1200000, 128)
