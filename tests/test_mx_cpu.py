"""K7, the MX block-scaled matrix check, without a GPU: the numpy host side (``ops.mx``:
formats, packers, generators, the exactness bound, the exact integer reference), the
argument checks of ``ops.mx_*``, ``validation/include/ntm/mx_plan.hpp`` against numpy
through a stand-alone sanitized C++ program, and the module's ``validation_mx_check``."""
import os
import shutil
import subprocess
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import ops
from nvidia_terraform_modules_amd.models import validation_job as vj
from nvidia_terraform_modules_amd.ops import mx, reference

ROOT = Path(__file__).resolve().parents[1]
STACK_DIR = ROOT / "modules" / "amd-gpu-stack"
FORMATS = ("e4m3", "e5m2", "e2m3", "e3m2", "e2m1")
SEED_FP4, SEED_FP6 = 0x4B58, 0x4B37      # the seeds of tests/test_mx_gpu.py

# ---- every finite code's value, written by hand from the OCP MX definitions: the
# non-negative half of each format; a set sign bit negates.
E2M1 = [0, 0.5, 1, 1.5, 2, 3, 4, 6]
E2M3 = [m / 8 for m in range(8)] + [1 + m / 8 for m in range(8)] + [2 + m / 4 for m in range(8)] + \
       [4 + m / 2 for m in range(8)]
E3M2 = [m / 16 for m in range(4)] + [(1 + m / 4) * 2.0**e for e in range(-2, 5) for m in range(4)]
E4M3 = [m / 512 for m in range(8)] + [(1 + m / 8) * 2.0**e for e in range(-6, 9) for m in range(8)]
E5M2 = [m / 65536 for m in range(4)] + [(1 + m / 4) * 2.0**e for e in range(-14, 16) for m in range(4)]
HAND = {"e2m1": E2M1, "e2m3": E2M3, "e3m2": E3M2, "e4m3": E4M3[:-1], "e5m2": E5M2}
NONFINITE = {"e4m3": {0x7F, 0xFF}, "e5m2": {0x7C, 0x7D, 0x7E, 0x7F, 0xFC, 0xFD, 0xFE, 0xFF},
             "e2m3": set(), "e3m2": set(), "e2m1": set()}


def test_format_codes_are_the_instructions():
    assert ops.MX_FORMATS == FORMATS and [mx.mx_format_id(f) for f in FORMATS] == [0, 1, 2, 3, 4]
    assert [mx.mx_bits(f) for f in FORMATS] == [8, 8, 6, 6, 4]
    with pytest.raises(ValueError, match="unknown MX format"):
        mx.mx_format_id("e3m4")
    with pytest.raises(ValueError, match="unknown MX format"):
        mx.mx_format_id(5)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_finite_code_decodes_to_the_hand_written_value(fmt):
    bits = mx.mx_bits(fmt)
    half = 2 ** (bits - 1)
    assert set(mx.mx_nonfinite_codes(fmt)) == NONFINITE[fmt]
    assert len(HAND[fmt]) == half - len(NONFINITE[fmt]) // 2
    table = mx.mx_quanta_table(fmt)
    unit = Fraction(2) ** mx._quantum_exp(fmt)
    for code in range(2 ** bits):
        if code in NONFINITE[fmt]:
            continue
        want = Fraction(HAND[fmt][code % half]) * (-1 if code >= half else 1)
        assert mx.mx_code_value(fmt, code) == want, hex(code)
        assert int(table[code]) * unit == want, hex(code)
    assert max(HAND[fmt]) == {"e2m1": 6, "e2m3": 7.5, "e3m2": 28, "e4m3": 448, "e5m2": 57344}[fmt]
    # 1.5, the decode sweep's B value, in every format
    assert mx.mx_code_value(fmt, mx._LAYOUT[fmt][4]) == Fraction(3, 2)


@pytest.mark.parametrize("fmt", FORMATS)
def test_pack_unpack_round_trip(fmt):
    bits = mx.mx_bits(fmt)
    rng = np.random.default_rng(bits)
    codes = rng.integers(0, 2 ** bits, size=(5, 96), dtype=np.uint8)
    codes[0, :2 ** min(bits, 6)] = np.arange(2 ** min(bits, 6))
    packed = ops.mx_pack(codes, fmt)
    assert packed.dtype == np.uint8 and packed.shape == (5, 96 * bits // 8)
    assert np.array_equal(ops.mx_unpack(packed, fmt), codes)
    if bits < 8:
        with pytest.raises(ValueError, match="out of range"):
            ops.mx_pack(np.full((1, 32), 2 ** bits, dtype=np.uint8), fmt)


def test_fp4_packs_low_nibble_first_and_fp6_straddles_bytes():
    assert ops.mx_pack(np.array([[0x1, 0xF, 0x7, 0x0] * 2], dtype=np.uint8), "e2m1").tolist() == \
        [[0xF1, 0x07, 0xF1, 0x07]]
    # 32 six-bit codes -> 24 bytes, one little-endian bit string: code k occupies bits 6k .. 6k+5
    codes = np.array([[(5 * k + 33) % 64 for k in range(32)]], dtype=np.uint8)
    packed = ops.mx_pack(codes, "e2m3")
    assert packed.shape == (1, 24)
    whole = int.from_bytes(packed[0].tobytes(), "little")
    assert [(whole >> (6 * k)) & 63 for k in range(32)] == codes[0].tolist()
    # codes 1, 2, 5, 6, ... cross a byte boundary: bits 6 .. 11 lie in bytes 0 and 1
    assert ops.mx_pack(np.array([[0, 0b111111, 0, 0]], dtype=np.uint8), "e3m2").tolist() == [[0xC0, 0x0F, 0x00]]
    assert np.array_equal(ops.mx_unpack(packed, "e2m3"), codes)


def _nearest_fp32(x: Fraction) -> Fraction:
    """x rounded to the nearest normal fp32, ties to even, in exact arithmetic."""
    if x == 0:
        return x
    e = abs(x).numerator.bit_length() - abs(x).denominator.bit_length()
    if Fraction(2) ** e > abs(x):
        e -= 1
    q = abs(x) / Fraction(2) ** (e - 23)                 # 2^23 <= q < 2^24
    n, rem = q.numerator // q.denominator, q - q.numerator // q.denominator
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n & 1):
        n += 1
    return (n if x > 0 else -n) * Fraction(2) ** (e - 23)


def test_numpy_reference_equals_a_fractions_dot():
    for fmt, W in (("e2m1", 3), ("e2m3", 1), ("e4m3", 2)):
        i = ops.mx_make_inputs("dense", fmt, 128, 128, 128, seed=11, W=W)
        a, b, sa, sb = i["a"][:16, :32 * mx.mx_bits(fmt) // 8], i["b"][:16, :32 * mx.mx_bits(fmt) // 8], \
            i["sa"][:16, :1], i["sb"][:16, :1]
        got = ops.mx_matmul_bits(a, b, sa, sb, fmt).view(np.float32)
        ca, cb = ops.mx_unpack(a, fmt), ops.mx_unpack(b, fmt)
        for r in range(16):
            for c in range(16):
                dot = sum(mx.mx_code_value(fmt, int(ca[r, k])) * mx.mx_code_value(fmt, int(cb[c, k]))
                          for k in range(32))
                dot *= Fraction(2) ** (int(sa[r, 0]) + int(sb[c, 0]) - 254)
                assert Fraction(float(got[r, c])) == _nearest_fp32(dot), (fmt, r, c)
                assert fmt == "e4m3" or _nearest_fp32(dot) == dot      # exact under the bound


def test_dense_exact_reproduces_the_worked_numbers():
    assert mx.mx_worst_sum("e2m1", 512, 3) == 4_718_592 and ops.mx_dense_exact("e2m1", 512, 3)
    assert mx.mx_worst_sum("e2m1", 4096, 2) == 9_437_184 and ops.mx_dense_exact("e2m1", 4096, 2)
    assert mx.mx_worst_sum("e2m3", 512, 1) == 7_372_800 and ops.mx_dense_exact("e2m3", 512, 1)
    assert not ops.mx_dense_exact("e2m1", 8192, 3) and not ops.mx_dense_exact("e2m1", 4096, 3)
    assert not ops.mx_dense_exact("e2m3", 512, 2)
    # the full code sets of the other three formats cannot meet the bound at any K
    for fmt in ("e3m2", "e4m3", "e5m2"):
        assert not ops.mx_dense_exact(fmt, 128, 0)
    assert [ops.mx_max_spread("e2m1", k) for k in (512, 4096, 8192)] == [3, 2, 1]
    assert ops.mx_max_spread("e2m3", 512) == 1 and ops.mx_max_spread("e4m3", 128) == -1


@pytest.mark.parametrize("fmt", FORMATS)
def test_generators_are_deterministic_and_never_emit_non_finite_codes(fmt):
    for kind, kw in (("dense", {"seed": 5, "W": 3}), ("decode", {"seed": 14})):
        i = ops.mx_make_inputs(kind, fmt, 256, 128, 128, **kw)
        j = ops.mx_make_inputs(kind, fmt, 256, 128, 128, **kw)
        bits = mx.mx_bits(fmt)
        assert i["a"].shape == (256, 128 * bits // 8) and i["b"].shape == (128, 128 * bits // 8)
        assert i["sa"].shape == (256, 4) and i["sb"].shape == (128, 4)
        for k in ("a", "b", "sa", "sb"):
            assert i[k].dtype == np.uint8 and np.array_equal(i[k], j[k])
        for k in ("a", "b"):
            assert not set(np.unique(ops.mx_unpack(i[k], fmt)).tolist()) & NONFINITE[fmt]
        assert i["sa"].max() < 255 and i["sb"].max() < 255
    d = ops.mx_make_inputs("dense", fmt, 256, 128, 128, seed=5, W=3)
    other = ops.mx_make_inputs("dense", fmt, 256, 128, 128, seed=6, W=3)
    assert not np.array_equal(d["a"], other["a"])
    finite = set(range(2 ** mx.mx_bits(fmt))) - NONFINITE[fmt]
    assert set(np.unique(ops.mx_unpack(d["a"], fmt)).tolist()) == finite      # every code is used
    assert set(np.unique(ops.mx_unpack(d["b"], fmt)).tolist()) == finite
    assert not np.array_equal(d["a"][:128], d["b"])                            # A and B differ
    delta = d["sa"].astype(int) - d["sa"].min(axis=1, keepdims=True)
    assert delta.max() == 3 and 95 <= d["sa"].min() and d["sa"].max() <= 162
    assert np.ptp(d["sa"].min(axis=1)) > 40                                    # bases vary widely


@pytest.mark.parametrize("fmt", FORMATS)
def test_decode_sweep_visits_every_code_every_position_and_every_scale_byte(fmt):
    bits = mx.mx_bits(fmt)
    positions, codes_seen, bytes_seen = set(), set(), set()
    for window in range(15):
        i = ops.mx_make_inputs("decode", fmt, 256, 128, 128, seed=window)
        codes = ops.mx_unpack(i["a"], fmt)
        nz = codes != 0
        assert (nz.sum(axis=1) <= 1).all()                   # one non-zero term per dot product
        rows, ks = np.nonzero(nz)
        assert np.array_equal(ks, mx.mx_decode_position(rows, 128))
        positions |= set(mx.mx_decode_position(np.arange(256), 128).tolist())
        codes_seen |= set(codes[np.arange(256), mx.mx_decode_position(np.arange(256), 128)].tolist())
        bytes_seen |= set(np.unique(i["sa"]).tolist())
        assert (ops.mx_unpack(i["b"], fmt) == mx._LAYOUT[fmt][4]).all()
        combined = i["sa"].astype(int)[:, None, :] + i["sb"].astype(int)[None, :, :] - 254
        assert combined.min() >= -8 and combined.max() <= 8
    assert positions == set(range(128))
    assert codes_seen == set(range(2 ** bits)) - NONFINITE[fmt]
    assert bytes_seen == set(range(255))
    # the register slots: every byte of a lane's 32 values is hit
    assert {p % 32 for p in positions} == set(range(32))


@pytest.mark.parametrize("fmt,shape,seed,W", [("e2m1", (128, 128, 128), SEED_FP4, 3),
                                              ("e2m1", (256, 384, 512), SEED_FP4, 3),
                                              ("e2m3", (128, 256, 512), SEED_FP6, 1)])
def test_dense_results_at_the_test_shapes_are_normal_fp32(fmt, shape, seed, W):
    """The bases keep every result between 2^-100 and 2^100. A sum of signed products can
    cancel to an exact zero (still exact, still compared bitwise); the seeds of the GPU
    tests are chosen so that none does at these shapes."""
    i = ops.mx_make_inputs("dense", fmt, *shape, seed=seed, W=W)
    c = np.abs(ops.mx_matmul_bits(i["a"], i["b"], i["sa"], i["sb"], fmt).view(np.float32))
    assert np.isfinite(c).all() and c.min() >= 2.0**-100 and c.max() <= 2.0**100


def test_model_runs_the_sequence_on_the_cpu_backend():
    rep = vj.mx_check(torch.device("cpu"), size=128, iters=1, backend=reference)
    assert rep["ok"] and rep["bad_elements"] == 0 and rep["formats"] == list(FORMATS)
    assert rep["scale_spread"] == 3
    bad = vj.mx_check(torch.device("cpu"), size=128, iters=1, backend=reference, corrupt=True)
    assert not bad["ok"] and bad["bad_elements"] == 1 and "e2m1" not in bad["formats"]
    f = bad["first"]
    assert (f["format"], f["mode"], f["row"], f["col"]) == ("e2m1", "dense", 64, 5)
    assert f["expected"] ^ f["got"] == 1 << 3


# ------------------------------------------------------- the argument checks
def test_ops_refuse_cpu_tensors_and_bad_shapes():
    i = ops.mx_make_inputs("dense", "e2m1", 128, 128, 128, seed=1, W=0)
    t = {k: torch.from_numpy(i[k]) for k in ("a", "b", "sa", "sb")}
    for fn in (ops.mx_gemm, ops.mx_reference_gpu):
        with pytest.raises(ValueError, match="needs GPU tensors"):
            fn(t["a"], t["b"], t["sa"], t["sb"], "e2m1")
    with pytest.raises(ValueError, match="needs GPU tensors"):
        ops.mx_compare(torch.zeros(4), torch.zeros(4))
    check = lambda *a, **k: ops.gpu.mx.mx_check_args(*a, need_cuda=False, **k)  # noqa: E731
    assert check(t["a"], t["b"], t["sa"], t["sb"], "e2m1") == (4, 128, 128, 128)
    with pytest.raises(ValueError, match="multiples of 128"):
        check(t["a"][:64], t["b"], t["sa"][:64], t["sb"], "e2m1")
    with pytest.raises(ValueError, match="multiples of 128"):       # K = 96
        check(t["a"][:, :48].contiguous(), t["b"][:, :48].contiguous(), t["sa"][:, :3].contiguous(),
              t["sb"][:, :3].contiguous(), "e2m1")
    with pytest.raises(ValueError, match=r"sa \[M, K/32\]"):
        check(t["a"], t["b"], t["sa"][:, :3].contiguous(), t["sb"], "e2m1")
    with pytest.raises(ValueError, match="contiguous 2-D uint8"):
        check(t["a"].to(torch.int32), t["b"], t["sa"], t["sb"], "e2m1")
    with pytest.raises(ValueError, match="out must be"):
        check(t["a"], t["b"], t["sa"], t["sb"], "e2m1", torch.zeros(128, 64))
    with pytest.raises(ValueError, match="unknown MX format"):
        check(t["a"], t["b"], t["sa"], t["sb"], "fp4")
    with pytest.raises(ValueError, match="multiples of 128"):
        ops.mx_make_inputs("dense", "e2m1", 64, 128, 128)
    with pytest.raises(ValueError, match="unknown MX input kind"):
        ops.mx_make_inputs("sparse", "e2m1", 128, 128, 128)
    assert ops.mx_shape_ok(128, 256, 384) and not ops.mx_shape_ok(128, 128, 96)


# ------------------------------------------------- the plan header, sanitized
PLAN_MAIN = r"""
#include "ntm/mx_plan.hpp"
using namespace ntm::mx;
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
static void dump(const char* name, const std::vector<uint8_t>& v) {
  std::printf("%s", name);
  for (uint8_t b : v) std::printf(" %02x", b);
  std::printf("\n");
}
static void emit(const Inputs& in) {
  dump("a", in.a); dump("b", in.b); dump("sa", in.sa); dump("sb", in.sb);
  std::vector<uint32_t> c;
  REQUIRE(host_reference(in, c));
  std::printf("c");
  for (uint32_t w : c) std::printf(" %08x", w);
  std::printf("\n");
}
int main() {
  // the table: names, widths, the codes that are not finite, 1.5
  for (int f = 0; f < kFormats; ++f) {
    std::printf("fmt %s %d %lld", format_name(f), format_bits(f), (long long)max_quanta(f));
    for (int c = 0; c < format_codes(f); ++c) {
      if (is_nonfinite(f, c)) { std::printf(" x"); continue; }
      std::printf(" %lld", (long long)quanta(f, c));
    }
    std::printf("\n");
    const Decoded d = decode(f, kFormatTable[f].one_point_five);
    REQUIRE(d.mant * std::ldexp(1.0, d.exp2) == 1.5);
  }
  // the bound
  REQUIRE(dense_worst_sum(kFmtE2M1, 512, 3) == 4718592 && dense_exact(kFmtE2M1, 512, 3));
  REQUIRE(dense_worst_sum(kFmtE2M1, 4096, 2) == 9437184 && dense_exact(kFmtE2M1, 4096, 2));
  REQUIRE(dense_worst_sum(kFmtE2M3, 512, 1) == 7372800 && dense_exact(kFmtE2M3, 512, 1));
  REQUIRE(!dense_exact(kFmtE2M1, 8192, 3) && !dense_exact(kFmtE2M3, 512, 2));
  REQUIRE(!dense_exact(kFmtE3M2, 128, 0) && !dense_exact(kFmtE4M3, 128, 0) && !dense_exact(kFmtE5M2, 128, 0));
  REQUIRE(dense_max_spread(kFmtE2M1, 4096) == 2 && dense_max_spread(kFmtE2M1, 512) == 3);
  REQUIRE(dense_max_spread(kFmtE5M2, 128) == -1);
  REQUIRE(shape_ok(128, 256, 384) && !shape_ok(64, 128, 128) && !shape_ok(128, 128, 96) && !shape_ok(0, 128, 128));
  // pack / unpack, an FP6 row whose codes straddle bytes
  for (int f = 0; f < kFormats; ++f) {
    std::vector<uint8_t> codes(64), row(row_bytes(f, 64) + 1, 0xEE);
    for (int k = 0; k < 64; ++k) codes[k] = (uint8_t)((k * 7 + 3) & (format_codes(f) - 1));
    pack_row(f, codes.data(), 64, row.data());
    REQUIRE(row.back() == 0xEE);
    for (int k = 0; k < 64; ++k) REQUIRE(unpack_code(f, row.data(), k) == codes[k]);
  }
  // the generators and the host reference: bytes and result bits for numpy to match
  emit(make_dense(kFmtE2M1, 128, 128, 128, 0x4B58, 3));
  emit(make_dense(kFmtE2M3, 128, 128, 256, 7, 1));
  emit(make_dense(kFmtE4M3, 128, 128, 128, 9, 2));
  for (int f = 0; f < kFormats; ++f) emit(make_decode(f, 256, 128, 128, 3 * f + 2));
  // the messages
  Mismatch m;
  mismatch_init(m);
  REQUIRE(m.count == 0 && m.first_index == ~0ull);
  m.count = 1, m.first_index = 5 * 384 + 7, m.expected = 0x41200000, m.got = 0x41200001;
  std::printf("%s\n", failure_message(3, kFmtE2M1, "dense", m, 384).c_str());
  m.count = ~0ull, m.first_index = 16383ull * 16384 + 16383, m.expected = m.got = 0xffffffffu;
  std::printf("%s\n", failure_message(15, kFmtE4M3, "decode", m, 16384).c_str());
  return 0;
}
"""


def test_plan_header_matches_numpy_under_sanitizers(tmp_path):
    """Stand-alone program with its own main against mx_plan.hpp, built with AddressSanitizer
    and UBSan (host code only; nothing is loaded into Python): its format table, generator
    bytes and reference bits must be numpy's."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "mx_main.cpp", tmp_path / "mx_main"
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
        name, bits, qmax, *codes = lines[f].split()[1:]
        table = mx.mx_quanta_table(fmt)
        assert (name, int(bits), int(qmax)) == (fmt, mx.mx_bits(fmt), int(table.max()))
        assert {c for c, v in enumerate(codes) if v == "x"} == NONFINITE[fmt]
        assert [int(v) for c, v in enumerate(codes) if v != "x"] == \
            [int(table[c]) for c in range(len(codes)) if c not in NONFINITE[fmt]]
    cases = [("dense", "e2m1", 128, 128, 128, 0x4B58, 3), ("dense", "e2m3", 128, 128, 256, 7, 1),
             ("dense", "e4m3", 128, 128, 128, 9, 2)] + \
            [("decode", fmt, 256, 128, 128, 3 * f + 2, 0) for f, fmt in enumerate(FORMATS)]
    at = len(FORMATS)
    for kind, fmt, M, N, K, seed, W in cases:
        i = ops.mx_make_inputs(kind, fmt, M, N, K, seed=seed, W=W)
        for key in ("a", "b", "sa", "sb"):
            tag, *hexes = lines[at].split()
            assert tag == key
            assert bytes.fromhex("".join(hexes)) == i[key].tobytes(), (kind, fmt, key)
            at += 1
        tag, *words = lines[at].split()
        at += 1
        want = ops.mx_matmul_bits(i["a"], i["b"], i["sa"], i["sb"], fmt)
        assert tag == "c" and np.array_equal(np.array([int(w, 16) for w in words], dtype=np.uint32),
                                             want.ravel()), (kind, fmt)
    one, widest = lines[at:]
    assert one == "gpu3: mx e2m1 dense: 1 bad element(s), first at row 5 col 7: expected 0x41200000, got 0x41200001"
    assert widest == ("gpu15: mx e4m3 decode: 18446744073709551615 bad element(s), first at row 16383 col "
                      "16383: expected 0xffffffff, got 0xffffffff")
    assert len(one) < 200 and len(widest) < 200


# ------------------------------------------------------------ the module
def _stack_local(name, **overrides):
    """local.<name> of modules/amd-gpu-stack with variable defaults + overrides."""
    from nvidia_terraform_modules_amd.tfcheck.config import load_module
    from nvidia_terraform_modules_amd.tfcheck.evaluate import Evaluator, Scope, convert

    mod = load_module(STACK_DIR)
    ev = Evaluator()
    variables = {}
    for vn, v in mod.variables.items():
        if vn in overrides:
            variables[vn] = overrides[vn]
        elif not v.required:
            variables[vn] = convert(ev.eval(v.block.body.attr("default"), Scope({}, {})),
                                    v.type_expr)
    scope = Scope(variables, {n: e for n, (e, _, _) in mod.locals.items()}, str(mod.path))
    return ev.eval(mod.locals[name][0], scope)


# local.validation_args at the variables' defaults before validation_mx_check existed (the
# list pinned in tests/test_host_link_cpu.py)
PARENT_DEFAULT_ARGS = [
    "--gpus", "8", "--size", "8192", "--tflops-floor", "1000", "--min-hbm-gb", "250",
    "--allreduce-max-mib", "1024", "--json", "--fp8-tflops-floor", "2000",
    "--xgmi-tune", "--require-host-prep", "--termination-log", "/dev/termination-log"]


def test_job_args_carry_the_mx_check_only_when_asked():
    args = _stack_local("validation_args")
    assert not [a for a in args if "mx" in a] and args == PARENT_DEFAULT_ARGS
    assert _stack_local("validation_args", validation_mx_check=False) == PARENT_DEFAULT_ARGS
    on = _stack_local("validation_args", validation_mx_check=True)
    i = on.index("--mx-check")
    assert i < on.index("--termination-log")
    assert [a for j, a in enumerate(on) if j != i] == PARENT_DEFAULT_ARGS
    desc = (STACK_DIR / "variables.tf").read_text().split('variable "validation_mx_check"')[1]
    assert "profiles/mx/README.md" in desc.split("}")[0]
