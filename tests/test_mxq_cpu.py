"""K11 without a GPU: the numpy mirror ``ops.mxq`` against two independent implementations
(torch's float8 casts and a brute-force nearest-value search), against ``mxq_plan.hpp`` through
a sanitized stand-alone program, the conditions of the conversion sweeps, generator (d) and the
edges of the scale rule."""
import os
import shutil
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import ops
from nvidia_terraform_modules_amd.ops import mxq

ROOT = Path(__file__).resolve().parents[1]
FORMATS = ops.MX_FORMATS


def _f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def _bits(v):
    return np.asarray(v, dtype=np.float32).view(np.uint32)


def _brute_force(fmt, xbits, byte):
    """Nearest value of the format's decoded table to x * 2^(127 - byte), ties to the even code,
    saturating; exact rational comparison through float64 (every value here is exact in it)."""
    table = mxq.mxq_value_table(fmt)
    finite = [c for c in range(len(table) // 2) if c <= ops.MXQ_MAX_CODE[fmt]]
    out = []
    for xb, b in zip(xbits.ravel(), np.broadcast_to(byte, xbits.shape).ravel()):
        v = abs(float(np.ldexp(np.float64(_f32(xb)), 127 - int(b))))
        best = min(finite, key=lambda c: (abs(table[c] - v), c & 1))
        out.append(best | ((int(xb) >> 31) << (mxq.mx_bits(fmt) - 1)))
    return np.asarray(out, dtype=np.uint8).reshape(xbits.shape)


# ------------------------------------------------------------ the mirror against two oracles
@pytest.mark.parametrize("fmt", FORMATS)
def test_mirror_equals_a_brute_force_search(fmt):
    x, s = mxq.mxq_down_sweep(fmt)
    pick = np.arange(0, x.shape[0], max(1, x.shape[0] // 40))          # every point at some scale bytes
    x, s = x[pick], s[pick]
    got = ops.mxq_quantize_codes(x, s[:, None], fmt)
    assert np.array_equal(got, _brute_force(fmt, x, s[:, None]))
    xb, sb = mxq.mxq_down_bf16(fmt)
    pick = np.arange(0, xb.shape[0], 97)
    assert np.array_equal(ops.mxq_quantize_codes(xb[pick], sb[pick, None], fmt), _brute_force(fmt, xb[pick], sb[pick, None]))


@pytest.mark.parametrize("fmt,dtype", (("e4m3", "float8_e4m3fn"), ("e5m2", "float8_e5m2")))
def test_mirror_equals_torch_float8_in_range(fmt, dtype):
    if not hasattr(torch, dtype):
        pytest.skip(f"torch has no {dtype}")
    pts = mxq.mxq_down_points(fmt)
    mags = np.abs(mxq.mxq_value_table(fmt))
    top = mags[ops.MXQ_MAX_CODE[fmt]]
    step = top - mags[ops.MXQ_MAX_CODE[fmt] - 1]
    pts = pts[np.abs(_f32(pts).astype(np.float64)) < top + step / 2]      # in range: what rounds to a finite value
    try:
        want = torch.from_numpy(_f32(pts).copy()).to(getattr(torch, dtype)).view(torch.uint8).numpy()
    except (RuntimeError, TypeError) as e:                                 # no CPU cast here: the brute force covers it
        pytest.skip(f"{dtype} does not cast on the CPU: {e}")
    got = ops.mxq_quantize_codes(pts, 127, fmt)
    assert np.array_equal(got, want)


# ------------------------------------------------------------ the scale rule at its edges
@pytest.mark.parametrize("fmt", FORMATS)
def test_scale_rule_edges(fmt):
    emax = ops.MXQ_EMAX[fmt]

    def byte(amax_bits):
        blk = np.zeros((1, 32), np.uint32)
        blk[0, 5] = amax_bits | 0x80000000                              # the sign must not matter
        return int(ops.mxq_scale_bytes(blk, fmt)[0, 0])
    assert byte(_bits(1.0)) == 127 - emax                               # a power of two
    assert byte(_bits(1.0) - 1) == 126 - emax                           # just below one
    assert byte(_bits(2.0 ** emax)) == 127 and byte(_bits(2.0 ** (emax + 1)) - 1) == 127
    assert byte(1 << 23) == 1 and byte(_bits(2.0 ** (emax - 126))) == 1 and byte(_bits(2.0 ** (emax - 125))) == 2
    assert byte(0x7F7FFFFF) == 254 - emax <= 254                        # the upper clamp is never reached by a finite fp32
    assert int(ops.mxq_scale_bytes(np.zeros((1, 32), np.uint32), fmt)[0, 0]) == 127
    assert int(ops.mxq_scale_bytes(np.full((1, 32), 0x80000000, np.uint32), fmt)[0, 0]) == 127
    # amax / scale reaches the top binade and saturates above the largest finite value
    top = np.zeros((1, 32), np.uint32)
    top[0, 0] = _bits(2.0 ** (emax + 1)) - 1
    p, s = ops.mxq_quantize_bits(top, fmt)
    assert int(ops.mx_unpack(p, fmt)[0, 0]) == ops.MXQ_MAX_CODE[fmt] and int(s[0, 0]) == 127


# ------------------------------------------------------------ the conditions of the sweeps
@pytest.mark.parametrize("fmt", FORMATS)
def test_bf16_sweep_judges_every_finite_normal_code(fmt):
    x, s = mxq.mxq_down_bf16(fmt)
    assert not (x & 0xFFFF).any() and s.min() >= 1 and s.max() <= 254
    codes = (x >> 16).astype(np.uint16)
    seen = np.unique(codes)
    e = (seen >> 7) & 0xFF
    assert seen.size == 65026 and set(seen[e == 0]) == {0x0000, 0x8000}   # +-0, no denormal
    assert not (e == 255).any()
    assert set(range(65536)) - set(seen.tolist()) == {c for c in range(65536)
                                                      if ((c >> 7) & 0xFF) == 255 or (((c >> 7) & 0xFF) == 0 and c & 0x7F)}
    # the scaled value is a normal fp32 operand: exponent field of x - byte + 127 in 1 .. 254
    scaled = ((x >> 23) & 0xFF).astype(np.int64) - s[:, None] + 127
    assert ((scaled >= 1) & (scaled <= 254))[(x & 0x7FFFFFFF) != 0].all()


@pytest.mark.parametrize("fmt", FORMATS)
def test_down_sweep_covers_every_boundary_with_normal_operands(fmt):
    pts = mxq.mxq_down_points(fmt)
    n_pairs = ops.MXQ_MAX_CODE[fmt]
    assert pts.size == 2 * (5 * n_pairs + 5)
    codes = ops.mxq_quantize_codes(pts, 127, fmt) & (2 ** (mxq.mx_bits(fmt) - 1) - 1)
    per = codes[:5 * n_pairs].reshape(n_pairs, 5)
    lo = np.arange(n_pairs)
    assert np.array_equal(per[:, 0], lo) and np.array_equal(per[:, 1], lo) and np.array_equal(per[:, 3], lo + 1)
    assert np.array_equal(per[:, 2], lo + (lo & 1)) and np.array_equal(per[:, 4], lo + 1)    # the tie goes to the even code
    assert (codes[5 * n_pairs:5 * n_pairs + 5] == ops.MXQ_MAX_CODE[fmt]).all()               # saturation
    x, s = mxq.mxq_down_sweep(fmt)
    e = (x >> 23) & 0xFF
    assert ((e >= 1) & (e <= 254))[(x & 0x7FFFFFFF) != 0].all() and len(set(s.tolist())) >= 20


@pytest.mark.parametrize("fmt", FORMATS)
def test_up_sweep_keeps_at_least_250_bytes_per_finite_code(fmt):
    packed, scales, kept = mxq.mxq_up_sweep(fmt)
    n = 2 ** mxq.mx_bits(fmt)
    bad = set(mxq.mx_nonfinite_codes(fmt))
    per_code = kept[:, :n].sum(axis=0)
    finite = [c for c in range(n) if c not in bad]
    assert all(per_code[c] == 0 for c in bad) and not kept[:, n:].any()
    # exact: a code whose value has exponent q loses max(0, -q) bytes at the bottom (result below 2^-126)
    # and max(0, q) at the top (2^128 and above) - |q| in all; zero keeps all 254
    _, _, mb, bias, _ = mxq._LAYOUT[fmt]
    table = np.abs(mxq.mxq_value_table(fmt))
    for c in finite:
        q = 0 if table[c] == 0 else int(np.floor(np.log2(table[c])))
        assert per_code[c] == 254 - abs(q), (fmt, c)
    worst = max(ops.MXQ_EMAX[fmt], bias - 1 + mb)
    assert min(per_code[c] for c in finite) == 254 - worst
    if worst <= 4:
        assert min(per_code[c] for c in finite) >= 250
    y = ops.mxq_dequantize_bits(packed, scales, fmt)
    e = (y >> 23) & 0xFF
    assert ((e >= 1) & (e <= 254) | ((y & 0x7FFFFFFF) == 0)).all()      # every compared word is zero or normal


# ------------------------------------------------------------ generator (d)
@pytest.mark.parametrize("fmt", FORMATS)
def test_grid_inputs_quantise_back_to_their_bytes(fmt):
    g = ops.mxq_make_inputs("grid", fmt, 128, 256, N=256, seed=0x4B3B, W=1)
    for side in "ab":
        p, s = ops.mxq_quantize_bits(g["x" + side], fmt)
        assert np.array_equal(p, g[side]) and np.array_equal(s, g["s" + side])
        assert np.array_equal(mxq.bf16_round_bits(g["x" + side]).astype(np.uint32) << 16, g["x" + side])   # exact in bf16
        _, eb, mb, _, _ = mxq._LAYOUT[fmt]
        field = (ops.mx_unpack(g[side], fmt).reshape(-1, 32) >> mb) & (2 ** eb - 1)
        assert (field == (ops.MXQ_MAX_CODE[fmt] >> mb)).any(axis=1).all()                                  # a top-binade element per block
    d = ops.mx_make_inputs("dense", fmt, 128, 256, 256, seed=0x4B3B, W=1)
    assert np.array_equal(d["sa"], g["sa"]) and np.mean(d["a"] != g["a"]) < 0.05                       # make_dense, a few raised


def test_end_to_end_shapes_are_exact_where_the_bound_allows():
    for K in (128, 512):
        for fmt in ("e2m1", "e2m3"):
            W = ops.mx_max_spread(fmt, K)
            assert W >= 0 and ops.mx_dense_exact(fmt, K, W)
    # e4m3's largest product alone is 2^35.6 product quanta: no K and no spread is exact by the
    # bound, so the e4m3 end-to-end product runs at spread 0 and its bitwise equality with the
    # reference kernel is what the GPU shows, not what mx_dense_exact promises
    assert ops.mx_max_spread("e4m3", 128) == -1 and not ops.mx_dense_exact("e4m3", 128, 0)


def test_block_rows_hold_the_special_blocks():
    for fmt in FORMATS:
        x = mxq.mxq_block_rows(fmt, 3, 96, 160, seed=5)
        assert (x[:, 96:] == mxq.MXQ_PAD).all()
        s = ops.mxq_scale_bytes(x[:, :96], fmt).ravel()
        blocks = x[:, :96].reshape(9, 32)
        assert s[3] == 127 and not blocks[3].any() and np.count_nonzero(blocks[5]) == 1 and s[7] == 1
    assert (mxq.mxq_block_rows("e2m1", 2, 64, seed=1, bf16=True) & 0xFFFF == 0).all()


# ------------------------------------------------- the plan header, sanitized
PLAN_MAIN = r"""
#include "ntm/mxq_plan.hpp"
using namespace ntm;
#define REQUIRE(c) do { if (!(c)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #c); std::exit(1); } } while (0)
static uint32_t crc32(const void* q, size_t n) {
  const uint8_t* p = (const uint8_t*)q;
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
  }
  return ~c;
}
int main() {
  for (int f = 0; f < mx::kFormats; ++f) {
    const char* n = mx::format_name(f);
    // the sweeps: inputs, scale bytes and the quantised bytes
    for (int bf = 0; bf < 2; ++bf) {
      const mxq::Sweep s = bf ? mxq::make_down_bf16(f) : mxq::make_down_sweep(f);
      const mxq::Quantized q = mxq::quantize_rows(f, s.x.data(), s.blocks(), 32, 32, s.scales.data());
      std::printf("down %s %d %d %08x %08x %08x\n", n, bf, s.blocks(), crc32(s.x.data(), s.x.size() * 4),
                  crc32(s.scales.data(), s.scales.size()), crc32(q.packed.data(), q.packed.size()));
    }
    const mxq::UpSweep u = mxq::make_up_sweep(f);
    const std::vector<uint32_t> y = mxq::dequantize_rows(f, u.packed.data(), u.scales.data(), u.R, u.K);
    int kept = 0;
    for (int b = 1; b <= 254; ++b)
      for (int c = 0; c < mx::format_codes(f); ++c) kept += mxq::up_kept(f, c, b);
    std::printf("up %s %d %d %08x %08x %08x\n", n, u.K, kept, crc32(u.packed.data(), u.packed.size()),
                crc32(u.scales.data(), u.scales.size()), crc32(y.data(), y.size() * 4));
    // block rows, strided, both sources; quantised by the rule
    for (int bf = 0; bf < 2; ++bf) {
      const std::vector<uint32_t> x = mxq::make_block_rows(f, 37, 96, 160, 0x4B3B, bf != 0);
      const mxq::Quantized q = mxq::quantize_rows(f, x.data(), 37, 96, 160);
      std::printf("block %s %d %08x %08x %08x\n", n, bf, crc32(x.data(), x.size() * 4),
                  crc32(q.packed.data(), q.packed.size()), crc32(q.scales.data(), q.scales.size()));
    }
    // generator (d)
    const mx::Inputs in = mx::make_dense(f, 128, 256, 256, 0x4B3B, 1);
    const mxq::Grid ga = mxq::make_grid(f, in.a, in.sa, 128, 256, 0x4B3B), gb = mxq::make_grid(f, in.b, in.sb, 256, 256, 0x4B3C);
    const mxq::Quantized qa = mxq::quantize_rows(f, ga.x.data(), 128, 256, 256);
    REQUIRE(qa.packed == ga.packed && qa.scales == ga.scales);
    std::printf("grid %s %08x %08x %08x %08x\n", n, crc32(ga.packed.data(), ga.packed.size()),
                crc32(ga.x.data(), ga.x.size() * 4), crc32(gb.packed.data(), gb.packed.size()),
                crc32(gb.x.data(), gb.x.size() * 4));
  }
  REQUIRE(mxq::shape_ok(1, 32, 32) && mxq::shape_ok(3, 96, 160) && !mxq::shape_ok(1, 48, 48) && !mxq::shape_ok(1, 64, 32) &&
          !mxq::shape_ok(0, 32, 32));
  REQUIRE(mxq::f32_to_bf16_rne(0x3F808000u) == 0x3F80 && mxq::f32_to_bf16_rne(0x3F818000u) == 0x3F82 &&
          mxq::f32_to_bf16_rne(0x3F808001u) == 0x3F81);
  mx::Mismatch m;
  mx::mismatch_init(m);
  m.count = 1, m.first_index = 5 * 512 + 8, m.expected = 0x00000021, m.got = 0x00000031;
  std::printf("%s\n", mxq::failure_message(3, mx::kFmtE2M1, "block", m, 512, 4).c_str());
  m.count = 7, m.first_index = 2 * 6 + 1;
  std::printf("%s\n", mxq::failure_message(0, mx::kFmtE2M3, "down", m, 6, 6).c_str());
  return 0;
}
"""


def _crc(a) -> str:
    return f"{zlib.crc32(np.ascontiguousarray(a).tobytes()):08x}"


def test_plan_header_matches_numpy_under_sanitizers(tmp_path):
    """Stand-alone program with its own main against mxq_plan.hpp, built with AddressSanitizer
    and UBSan (host code only; nothing is loaded into Python): its generators' bytes, its
    quantised bytes and its dequantised bits must be numpy's."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src, exe = tmp_path / "mxq_main.cpp", tmp_path / "mxq_main"
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
    at = 0
    for fmt in FORMATS:
        for bf, gen in enumerate((mxq.mxq_down_sweep, mxq.mxq_down_bf16)):
            x, s = gen(fmt)
            packed, _ = ops.mxq_quantize_bits(x, fmt, s[:, None])
            assert lines[at].split() == ["down", fmt, str(bf), str(x.shape[0]), _crc(x), _crc(s), _crc(packed)], lines[at]
            at += 1
        packed, scales, kept = mxq.mxq_up_sweep(fmt)
        y = ops.mxq_dequantize_bits(packed, scales, fmt)
        assert lines[at].split() == ["up", fmt, str(kept.shape[1]), str(int(kept.sum())), _crc(packed), _crc(scales), _crc(y)], lines[at]
        at += 1
        for bf in (0, 1):
            x = mxq.mxq_block_rows(fmt, 37, 96, 160, seed=0x4B3B, bf16=bool(bf))
            packed, scales = ops.mxq_quantize_bits(x[:, :96], fmt)
            assert lines[at].split() == ["block", fmt, str(bf), _crc(x), _crc(packed), _crc(scales)], lines[at]
            at += 1
        g = ops.mxq_make_inputs("grid", fmt, 128, 256, N=256, seed=0x4B3B, W=1)
        assert lines[at].split() == ["grid", fmt, _crc(g["a"]), _crc(g["xa"]), _crc(g["b"]), _crc(g["xb"])], lines[at]
        at += 1
    assert lines[at] == ops.mxq_failure_message(3, "e2m1", "block", 1, 5 * 512 + 8, 0x21, 0x31, 512, 4)
    assert lines[at] == ("gpu3: mxq e2m1 block: 1 bad word(s), first at row 5 element 64: expected 0x00000021, "
                         "got 0x00000031, bad bits 0x00000010")
    assert lines[at + 1] == ops.mxq_failure_message(0, "e2m3", "down", 7, 13, 0x21, 0x31, 6, 6)
    assert all(len(line) < 200 for line in lines[at:at + 2])
