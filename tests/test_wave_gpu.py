"""K12 on the GPU: every instruction kernel against its reference kernel bitwise (and both against
the numpy twin), one sfu digest across workgroups, the measured distances within the recorded
bounds, a planted bit, refusals, and ``models.wave_check``."""
import numpy as np
import pytest
import torch

from nvidia_terraform_modules_amd import ops as o
from nvidia_terraform_modules_amd.models import wave_check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _np(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.fixture(scope="module")
def words():
    l = np.arange(256)
    x, y = o.wave_hash32(0x4B3C, 0, l // 64, 0, l % 64), o.wave_hash32(0x4B3C, 1, l // 64, 0, l % 64)
    return x, y, o.wave_to_device(x, DEV), o.wave_to_device(y, DEV)


def test_lane_every_op_equals_the_reference_and_the_twin(words):
    x, y, dx, dy = words
    bad = []
    for i, op in enumerate(o.wave_lane_ops()):
        got, ref = _np(o.wave_lane(i, None, dx, dy)), _np(o.wave_lane_reference_gpu(i, None, dx, dy))
        if not (np.array_equal(got, ref) and np.array_equal(ref, o.wave_expected_lane(op, x, y))):
            lane = int(np.flatnonzero(got != ref)[0]) if not np.array_equal(got, ref) else -1
            bad.append((o.wave_lane_op_name(op), lane))
    print("lane ops that differ:", bad)
    assert not bad


# the 6-bit form needs 16-byte aligned addresses (the probe log), so its padded stride is 144, not 136
# R = 4 rows is one block of the 16-bit form; the 8-, 4- and 6-bit forms' blocks are 8, 16 and 16
# rows, so their smallest image is one block high
@pytest.mark.parametrize("bits,rows,stride", [(16, 4, 32), (8, 8, 32), (4, 16, 32), (6, 16, 32), (16, 64, 136), (8, 64, 136),
                                              (4, 64, 136), (6, 64, 128), (6, 64, 144), (16, 16, 64), (8, 16, 72), (4, 32, 128)])
def test_ldstr_equals_the_reference_and_the_twin(bits, rows, stride):
    img = o.wave_make_image(bits, rows, stride, 91)
    d = torch.from_numpy(img.copy()).to(DEV)
    got, ref = _np(o.wave_tr_read(bits, d, stride)), _np(o.wave_tr_read_reference_gpu(bits, d, stride))
    exp = o.wave_expected_tr_read(bits, img, rows, stride)
    diff = np.flatnonzero(got != ref)
    print(f"tr_b{bits} {rows}x{stride}: {len(diff)} of {len(got)} words differ", diff[:4])
    assert np.array_equal(ref, exp)
    assert np.array_equal(got, ref)


def test_valu_equals_the_reference_and_the_twin(words):
    x, y, dx, dy = words
    c = o.wave_hash32(0x4B3C, 2, np.arange(256) // 64, 0, np.arange(256) % 64)
    dc = o.wave_to_device(c, DEV)
    got, ref = _np(o.wave_valu("bitop3", dx, dy, dc)), _np(o.wave_valu("bitop3", dx, dy, dc, reference=True))
    assert np.array_equal(got, ref)
    for table in (0x00, 0x96, 0xE8, 0xCA, 0xFF):
        assert np.array_equal(ref[table], o.wave_expected_bitop3(x, y, c, table))
    cv = o.wave_cvt_inputs(9, 1024)
    a, b = o.wave_to_device(cv, DEV), o.wave_to_device(cv[::-1].copy(), DEV)
    got, ref = _np(o.wave_valu("cvt_pk_bf16", a, b)), _np(o.wave_valu("cvt_pk_bf16", a, b, reference=True))
    assert np.array_equal(ref, o.wave_expected_cvt_pk(cv, cv[::-1]))
    assert np.array_equal(got, ref)


def test_sfu_one_digest_per_instruction_across_two_workgroups_per_cu():
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    recs, digests = o.wave_sfu_digest(DEV, 2 * cus)
    assert (recs["magic"] == 0x4B31324B).all()
    for op, name in enumerate(o.WAVE_SFU_OPS):
        assert len(np.unique(digests[:, op])) == 1, name
    assert len(np.unique(digests[0])) == 7


def test_sfu_distance_within_the_recorded_bound():
    for op, name in enumerate(o.WAVE_SFU_OPS):
        x, _ = o.wave_sfu_inputs(op)
        dx = o.wave_to_device(x, DEV)
        y = o.wave_sfu(op, dx)
        d = o.wave_sfu_distance(op, dx, y, o.WAVE_SFU_BOUND[name])
        lo, hi = o.wave_sfu_brackets(op, x)
        host = o.wave_expected_sfu_distance(_np(y), lo, hi)
        print(name, "max d", d["max_d"], "input", hex(int(x[d["max_index"]])) if d["max_d"] else None, "bound", o.WAVE_SFU_BOUND[name])
        assert d["max_d"] == int(host.max())
        if o.WAVE_SFU_BOUND[name] is not None:
            assert d["beyond"] == 0 and d["max_d"] <= o.WAVE_SFU_BOUND[name], name


def test_a_planted_bit_is_reported_with_its_index_and_bits(words):
    x, y, dx, dy = words
    i = o.wave_lane_op_index("row_ror:5 bound_ctrl:0")
    got = o.wave_lane(i, None, dx, dy)
    ref = o.wave_lane_reference_gpu(i, None, dx, dy)
    got[77] ^= 1 << 21
    rep = o.mx_compare(ref, got)
    assert rep.count == 1 and rep.first_index == 77 and rep.expected ^ rep.got == 1 << 21
    dx2 = o.wave_to_device(o.wave_sfu_inputs(2)[0][:512], DEV)
    yy = o.wave_sfu(2, dx2)
    yy[300] += 64
    d = o.wave_sfu_distance(2, dx2, yy, bound=4)
    lo, hi = o.wave_sfu_brackets(2, o.wave_sfu_inputs(2)[0][:512])
    host = o.wave_expected_sfu_distance(_np(yy), lo, hi)
    assert int(host.argmax()) == 300 and 60 <= int(host.max()) <= 64
    assert d == {"max_d": int(host.max()), "max_index": 300, "beyond": 1, "first_beyond": 300}


def test_bad_arguments_are_refused_and_outputs_untouched(words):
    _, _, dx, dy = words
    out = torch.full((256,), 0x55, dtype=torch.int32, device=DEV)
    lib = o._lib.lib()
    h = o._lib.stream_handle()
    assert lib.ntm_wave_lane(0, 547, 1, dx.data_ptr(), dy.data_ptr(), out.data_ptr(), 256, h) != 0
    assert lib.ntm_wave_lane(0, -1, 1, dx.data_ptr(), dy.data_ptr(), out.data_ptr(), 256, h) != 0
    assert lib.ntm_wave_sfu(7, dx.data_ptr(), out.data_ptr(), 256, h) != 0
    img = torch.zeros(4 * 32 + 16, dtype=torch.uint8, device=DEV)
    assert lib.ntm_wave_tr_read(0, 16, img.data_ptr() + 4, 4, 32, out.data_ptr(), h) != 0      # misaligned image
    assert lib.ntm_wave_tr_read(0, 16, img.data_ptr(), 4, 36, out.data_ptr(), h) != 0          # stride not a multiple of 8
    assert lib.ntm_wave_tr_read(0, 6, img.data_ptr(), 16, 40, out.data_ptr(), h) != 0          # 6-bit: not a multiple of 16
    assert lib.ntm_wave_tr_read(0, 5, img.data_ptr(), 4, 32, out.data_ptr(), h) != 0
    torch.cuda.synchronize()
    assert (out == 0x55).all()
    with pytest.raises(ValueError):
        o.wave_tr_read(16, img[:128], 36)
    with pytest.raises(ValueError):
        o.wave_lane("no_such_op", None, dx, dy)


def test_wave_check_clean_and_corrupt():
    r = wave_check(DEV)
    print({k: v for k, v in r.items() if k.startswith("wave_")})
    assert r["ok"], r["failures"]
    assert r["wave_lane_bad"] == r["wave_ldstr_bad"] == r["wave_valu_bad"] == r["wave_sfu_inconsistent"] == 0
    assert r["wave_cus_covered"] == torch.cuda.get_device_properties(DEV).multi_processor_count
    r = wave_check(DEV, corrupt="lane")
    assert not r["ok"] and r["wave_lane_bad"] == 1 and len(r["failures"]) == 1
    assert "wave lane row_shr:3 bound_ctrl:0: xcd" in r["failures"][0] and r["failures"][0].endswith("bad bits 0x00000400")
    assert " lane 19: " in r["failures"][0]


def test_wave_check_names_the_input_behind_an_inconsistent_digest():
    import re
    r = wave_check(DEV, corrupt="sfu")
    print(r["failures"])
    assert not r["ok"] and r["wave_sfu_inconsistent"] >= 1 and len(r["failures"]) == 1
    assert r["wave_lane_bad"] == r["wave_ldstr_bad"] == r["wave_valu_bad"] == r["wave_sfu_beyond_bound"] == 0
    m = re.match(r"gpu0: wave sfu v_exp_f32: xcd \d+ se \d+ sh \d+ cu \d+ simd \d+ element 1000 input (0x[0-9a-f]{8}): "
                 r"expected (0x[0-9a-f]{8}), got (0x[0-9a-f]{8}), bad bits 0x00000400$", r["failures"][0])
    assert m, r["failures"][0]
    x = o.wave_sfu_inputs(0)[0]
    assert int(m.group(1), 16) == int(x[1000])
    assert int(m.group(2), 16) == int(_np(o.wave_sfu(0, o.wave_to_device(x[1000:1001], DEV)))[0])
    assert int(m.group(2), 16) ^ int(m.group(3), 16) == 0x400
