"""K12 host side (no GPU): the numpy twin ``ops.wave`` equals ``wave_paths_plan.hpp`` byte for byte
through a sanitized stand-alone program; spot values of the lane maps written by hand from the
ISA's wording; the brackets; the truth tables."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from nvidia_terraform_modules_amd.ops import wave as w

ROOT = Path(__file__).resolve().parents[1]
INCLUDE = ROOT / "validation" / "include"

DUMP_MAIN = r"""
#include <cstdio>
#include "ntm/wave_paths_plan.hpp"
namespace wv = ntm::wave;
static void put(const void* p, size_t n) { std::fwrite(p, 1, n, stdout); }
static void put32(uint32_t v) { put(&v, 4); }
int main() {
  put32((uint32_t)wv::kLaneOps);
  for (int i = 0; i < wv::kLaneOps; ++i) {
    const wv::LaneOp op = wv::lane_op(i);
    for (int l = 0; l < 64; ++l) { const int16_t s = (int16_t)wv::src_lane(op, l); put(&s, 2); }
    const std::string n = wv::lane_op_name(op);
    put32((uint32_t)n.size()); put(n.data(), n.size());
  }
  for (uint32_t l = 0; l < 64; ++l) put32(wv::hash32(0x4B3C, 1, 2, 3, l));
  const int shapes[6][3] = {{16, 4, 32}, {8, 8, 32}, {4, 16, 72}, {6, 16, 48}, {16, 64, 136}, {6, 32, 128}};
  for (auto& sh : shapes) {
    wv::TrShape s;
    if (!wv::tr_shape(sh[0], sh[1], sh[2], &s)) return 3;
    const auto img = wv::tr_make_image(sh[0], sh[1], sh[2], 77);
    put(img.data(), img.size());
    for (int it = 0; it < s.iters; ++it)
      for (int d = 0; d < 3; ++d)
        for (int t = 0; t < 256; ++t) put32(wv::tr_expected_word(s, img.data(), it, d, t));
  }
  for (int op = 0; op < wv::kSfuOps; ++op) {
    const wv::SfuList L = wv::sfu_inputs(op);
    put32((uint32_t)L.x.size()); put32((uint32_t)L.exact_from);
    put(L.x.data(), L.x.size() * 4);
    for (uint32_t x : L.x) { uint32_t lo, hi; wv::sfu_bracket(op, x, &lo, &hi); put32(lo); put32(hi); }
  }
  for (uint32_t t = 0; t < 256; ++t) put32(wv::bitop3_expected(wv::h32(t), wv::h32(t + 999), wv::h32(t * 7 + 5), t));
  const auto cv = wv::cvt_inputs(5, 100);
  put32((uint32_t)cv.size());
  for (size_t i = 0; i + 1 < cv.size(); i += 2) { put32(cv[i]); put32(cv[i + 1]); put32(wv::cvt_pk_expected(cv[i], cv[i + 1])); }
  return 0;
}
"""


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("wave")
    (d / "dump.cpp").write_text(DUMP_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{INCLUDE}", str(d / "dump.cpp"), "-o", str(d / "dump")], check=True, timeout=300)
    p = subprocess.run([str(d / "dump")], capture_output=True, timeout=300)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    return p.stdout


def test_numpy_twin_equals_the_header(dump):
    at = 0

    def take(n):
        nonlocal at
        at += n
        return dump[at - n:at]

    def u32(n=1):
        return np.frombuffer(take(4 * n), np.uint32)

    ops = w.wave_lane_ops()
    assert int(u32()[0]) == len(ops) == 547
    for op in ops:
        assert np.array_equal(np.frombuffer(take(128), np.int16), w.wave_src_lane(op).astype(np.int16)), op
        assert take(int(u32()[0])).decode() == w.wave_lane_op_name(op)
    assert np.array_equal(u32(64), w.wave_hash32(0x4B3C, 1, 2, 3, np.arange(64)))
    for bits, rows, stride in ((16, 4, 32), (8, 8, 32), (4, 16, 72), (6, 16, 48), (16, 64, 136), (6, 32, 128)):
        img = w.wave_make_image(bits, rows, stride, 77)
        assert take(rows * stride) == img.tobytes(), (bits, rows, stride)
        exp = w.wave_expected_tr_read(bits, img, rows, stride)
        assert np.array_equal(u32(len(exp)), exp), (bits, rows, stride)
    for op in range(7):
        n, exact = (int(v) for v in u32(2))
        x, e = w.wave_sfu_inputs(op)
        assert (n, exact) == (len(x), e)
        assert np.array_equal(u32(n), x)
        lo, hi = w.wave_sfu_brackets(op, x)
        assert np.array_equal(u32(2 * n).reshape(-1, 2), np.stack([lo, hi], 1)), w.WAVE_SFU_OPS[op]
    t = np.arange(256, dtype=np.uint32)
    h = w._h32
    assert np.array_equal(u32(256), np.array([w.wave_expected_bitop3(h(i), h(i + 999), h(i * 7 + 5), int(i)) for i in t]))
    cv = w.wave_cvt_inputs(5, 100)
    assert int(u32()[0]) == len(cv)
    trip = u32(3 * (len(cv) // 2)).reshape(-1, 3)
    assert np.array_equal(trip[:, 0], cv[0::2]) and np.array_equal(trip[:, 1], cv[1::2])
    assert np.array_equal(trip[:, 2], w.wave_expected_cvt_pk(cv[0::2], cv[1::2]))
    assert at == len(dump)


def _src(name):
    return w.wave_src_lane(w.wave_lane_ops()[w.wave_lane_op_index(name)])


def test_lane_maps_spot_values_from_the_isa_wording():
    s = _src("row_shr:1 bound_ctrl:0")
    assert s[17] == 16 and s[16] == w.WAVE_OLD
    assert _src("row_shr:1 bound_ctrl:1")[16] == w.WAVE_ZERO
    assert _src("row_mirror bound_ctrl:0")[3] == 12
    assert _src("row_bcast:15 bound_ctrl:0")[16] == 15
    assert _src("wave_ror:1 bound_ctrl:0")[0] == 63
    assert list(_src("quad_perm:[3,2,1,0] bound_ctrl:0")[4:8]) == [7, 6, 5, 4]
    assert list(_src("ds_swizzle 0x041f")[:4]) == [1, 0, 3, 2] and _src("ds_swizzle 0x041f")[62] == 63
    a, b = _src("permlane32_swap 0"), _src("permlane32_swap 1")
    assert a[5] == 5 and a[37] == 64 + 5 and b[5] == 37 and b[37] == 64 + 37
    # a lane that row_mask 0x5 disables (row 1) keeps old
    assert _src("row_shl:1 bound_ctrl:1 row_mask:0x5")[20] == w.WAVE_OLD
    assert _src("row_shl:1 bound_ctrl:1 bank_mask:0x6")[0] == w.WAVE_OLD and _src("row_shl:1 bound_ctrl:1 bank_mask:0x6")[4] == 5


def test_every_permute_index_list_is_a_bijection():
    for variant in (0, 2):
        dst = sorted((w.wave_bpermute_index(variant, l) >> 2) & 63 for l in range(64))
        assert dst == list(range(64))
    for name in ("ds_permute 0", "ds_permute 1"):
        assert sorted(_src(name)) == list(range(64))


def test_tr_b16_map_is_the_guides_on_a_4_by_16_block():
    # lane 4q+p supplies row q, columns 4p .. 4p+3; lane i receives column i, row q in element q
    block = np.arange(64, dtype=np.uint16).reshape(4, 16) + 0x100
    img = block.view(np.uint8).reshape(-1)
    got = w.wave_expected_tr_read(16, img, 4, 32).reshape(1, 3, 256)[0]
    for i in range(16):
        elems = np.array([got[0, i] & 0xFFFF, got[0, i] >> 16, got[1, i] & 0xFFFF, got[1, i] >> 16])
        assert list(elems) == list(block[:, i]), i
    for i in range(16):
        for q in range(4):
            assert w.wave_tr_src(16, i, q) == (4 * q + i // 4, i % 4)


def test_brackets():
    for op, name in enumerate(w.WAVE_SFU_OPS):
        x, exact = w.wave_sfu_inputs(op)
        lo, hi = w.wave_sfu_brackets(op, x)
        flo, fhi = lo.view(np.float32), hi.view(np.float32)
        assert (flo <= fhi).all(), name
        step = w.wave_ordered(hi).astype(np.int64) - w.wave_ordered(lo).astype(np.int64)
        assert ((step == 0) | (step == 1)).all(), name
        assert (lo[exact:] == hi[exact:]).all(), name
        for v in (x, lo, hi):
            e = (v >> 23) & 0xFF
            assert ((e != 0) & (e != 255)).all(), name
        assert len(x) > 8192
        if op < 5:
            assert len(x) > exact


def test_the_256_truth_tables_against_a_bit_loop():
    rng = np.random.default_rng(12)
    a, b, c = (int(v) for v in rng.integers(0, 2**32, 3, dtype=np.uint64))
    for table in range(256):
        want = 0
        for i in range(32):
            idx = (((a >> i) & 1) << 2) | (((b >> i) & 1) << 1) | ((c >> i) & 1)
            want |= ((table >> idx) & 1) << i
        assert int(w.wave_expected_bitop3(a, b, c, table)) == want, table


def test_bf16_rounding_ties_to_even():
    assert int(w.wave_bf16_rne(0x3F808000)) == 0x3F80 and int(w.wave_bf16_rne(0x3F818000)) == 0x3F82
    assert int(w.wave_bf16_rne(0x3F808001)) == 0x3F81 and int(w.wave_bf16_rne(0x3F807FFF)) == 0x3F80


MESSAGES_MAIN = r"""
#include <cstdio>
#include "ntm/wave_paths_plan.hpp"
namespace wv = ntm::wave;
int main() {
  // xcd 3, se 2, sh 1, cu 7; the four waves on SIMDs 0, 2, 1, 3
  wv::Record r{};
  r.hw_id = (2u << 13) | (1u << 12) | (7u << 8), r.xcc_id = 3, r.magic = wv::kMagic;
  r.simd[0] = 0, r.simd[1] = 2, r.simd[2] = 1, r.simd[3] = 3;
  std::vector<wv::Record> recs(5, r);
  for (int i = 0; i < 5; ++i) recs[i].digest[2] = i == 3 ? 0xBADull : 0x600Dull;
  recs[4].magic = 0;                      // an unwritten record has no vote
  recs[4].digest[2] = 0xBADull;
  std::printf("%llx\n", (unsigned long long)wv::majority_digest(recs, 2));
  r.bad = 1, r.first = ~(uint32_t)(25 * 256 + 2 * 64 + 19), r.expected = 0x12345678u, r.got = 0x12345278u;
  std::printf("%s\n", wv::lane_failure(2, r).c_str());
  r.first = ~(uint32_t)70;
  std::printf("%s\n", wv::indexed_failure(0, wv::kFamLdstr, "tr_b6 stride 144", r).c_str());
  std::printf("%s\n", wv::sfu_failure(1, wv::kSfuRsq, r, 1000, 0x3f800000u, 0x3f800000u, 0x3f800400u).c_str());
  std::printf("%s\n", wv::sfu_digest_failure(1, 2, recs[3], 0x600D, "not seen again in a second launch").c_str());
  wv::SfuDistance d;
  wv::distance_init(d);
  std::printf("%u %u %u %u\n", d.max_d, d.max_index, wv::sfu_distance(0x3f800005u, 0x3f800000u, 0x3f800001u),
              wv::sfu_distance(0xbf800005u, 0xbf800001u, 0xbf800000u));
  return 0;
}
"""


def test_majority_digest_and_the_failure_lines_on_fabricated_records(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    (tmp_path / "m.cpp").write_text(MESSAGES_MAIN)
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-I{INCLUDE}", str(tmp_path / "m.cpp"), "-o", str(tmp_path / "m")], check=True, timeout=300)
    p = subprocess.run([str(tmp_path / "m")], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert lines[0] == "600d"
    assert lines[1] == ("gpu2: wave lane row_shr:3 bound_ctrl:0: xcd 3 se 2 sh 1 cu 7 simd 1 lane 19: expected 0x12345678, "
                        "got 0x12345278, bad bits 0x00000400")
    assert lines[1] == w.wave_failure_message(2, "lane", "row_shr:3 bound_ctrl:0", (3, 2, 1, 7, 1), "lane", 19, 0x12345678, 0x12345278)
    assert lines[2] == ("gpu0: wave ldstr tr_b6 stride 144: xcd 3 se 2 sh 1 cu 7 simd 2 element 70: expected 0x12345678, "
                        "got 0x12345278, bad bits 0x00000400")
    assert lines[3] == ("gpu1: wave sfu v_rsq_f32: xcd 3 se 2 sh 1 cu 7 simd 3 element 1000 input 0x3f800000: expected 0x3f800000, "
                        "got 0x3f800400, bad bits 0x00000400")
    assert lines[4] == ("gpu1: wave sfu v_rcp_f32: xcd 3 se 2 sh 1 cu 7: digest 0xbad differs from 0x600d of the other workgroups "
                        "(not seen again in a second launch)")
    assert lines[5] == "0 4294967295 4 4"
    assert all(len(x) < 200 for x in lines)
