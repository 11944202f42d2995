"""The Python side after its split by check (``ops.gpu``, ``models.checks``): the public names are
those recorded before the split (tests/fixtures/python_surface.json), every C entry of an opt-in
check is called from that check's module only, and the struct reader decodes device result records
to what the hand-sliced ``int.from_bytes`` / ``ctypes`` code before it gave for the same bytes. No
GPU and no native library needed."""
import importlib
import json
import re
import types
from pathlib import Path

import pytest
import torch

from nvidia_terraform_modules_amd import ops
from nvidia_terraform_modules_amd.ops import _lib, kernels
from nvidia_terraform_modules_amd.ops.gpu import _common, hbm_pattern

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "nvidia_terraform_modules_amd"
RECORDED = json.loads((ROOT / "tests" / "fixtures" / "python_surface.json").read_text())


@pytest.mark.parametrize("name", ["ops", "models", "models.validation_job", "ops.reference"])
def test_public_names_are_the_recorded_ones(name):
    """The fixture holds ``sorted(n for n in dir(module) if not n.startswith('_'))`` from before the
    split, and which of those names were modules (submodules and ``import x`` lines: the layout,
    which the split changes on purpose). Everything else must be there, and nothing new."""
    mod = importlib.import_module("nvidia_terraform_modules_amd." + name)
    now = {n for n in dir(mod) if not n.startswith("_") and not isinstance(getattr(mod, n), types.ModuleType)}
    assert now == set(RECORDED[name]) - set(RECORDED["modules_among_them"][name])


def test_each_name_has_one_home():
    assert ops.MxCompareReport is ops.McoreCompareReport
    for moved in ("mx_gemm", "cu_sweep", "atomics_rmw", "wave_lane"):
        assert not hasattr(kernels, moved), moved
    # bench.py calls kernels.gemm_clock_stable and a test patches kernels.gemm_clock_ghz beneath it
    assert kernels.gemm_clock_stable.__module__ == kernels.gemm_clock_ghz.__module__ == kernels.__name__
    assert kernels.gemm_clock_stable.__globals__["gemm_clock_ghz"] is kernels.gemm_clock_ghz


CHECK_HOMES = {"ntm_mx_": "mx", "ntm_mcore_": "mcore", "ntm_mxq_": "mxq", "ntm_wave_": "wave",
               "ntm_atomics_": "atomics", "ntm_xcd_sweep_": "xcd_sweep", "ntm_cu_sweep_": "cu_sweep",
               "ntm_host_link_": "host_link", "ntm_hbm_pattern_": "hbm_pattern"}


def test_c_entries_are_called_from_their_check_module_only():
    """A plain text search of the package's own .py files: an ``ntm_<check>_*`` row of
    ``_lib.SIGNATURES`` is named, outside the table itself, in ops/gpu/<check>.py and nowhere else
    (a few rows serve the Job binary alone and are named nowhere)."""
    sources = {p.relative_to(PKG).as_posix(): p.read_text() for p in PKG.rglob("*.py")}
    assert "ops/gpu/_common.py" in sources
    called = {m: 0 for m in CHECK_HOMES.values()}
    for entry in _lib.SIGNATURES:
        home = next((m for prefix, m in CHECK_HOMES.items() if entry.startswith(prefix)), None)
        if home is None:
            continue
        users = {path for path, text in sources.items() if re.search(rf"\b{entry}\b", text)} - {"ops/_lib.py"}
        assert users <= {f"ops/gpu/{home}.py"}, (entry, sorted(users))
        called[home] += len(users)
    assert all(n >= 3 for n in called.values()), called     # every check's module calls its entries


# Hand-built records, little-endian, with junk in the padding. The expected values below are what the
# slicing code before the struct reader (int.from_bytes(raw[a:b], "little"),
# ctypes.c_float / c_double.from_buffer_copy) returned for these bytes; they were computed with that
# code once and are literals here.
def _u64(v):
    return v.to_bytes(8, "little")


def _u32(v):
    return v.to_bytes(4, "little")


def test_abft_result_decodes_as_before():
    raw = _u64(3) + _u64(0x100000002) + _u32(0x3A83126F) + _u32(0x3C23D70A) + b"\xAA" * 8
    rep = kernels._abft_report(raw, 512)
    assert rep.as_dict() == {"rows": 512, "bad_acc": 3, "bad_store": 4294967298,
                             "max_rel_acc": 0.0010000000474974513,
                             "max_rel_store": 0.009999999776482582, "ok": False}


def test_verify_result_decodes_as_before():
    raw = _u64(7) + _u32(0x3DCCCCCD) + _u32(0xDEADBEEF) + _u64(0x4004000000000000) + _u64(0x4024000000000000)
    rep = kernels._verify_report(raw, 4096)
    assert (rep.n, rep.bad, rep.max_abs_err, rep.rel_rms_err, rep.ok) == (4096, 7, 0.10000000149011612, 0.5, False)
    clean = kernels._verify_report(bytes(32), 16)        # sum of squares of the reference 0: infinite
    assert (clean.bad, clean.max_abs_err, clean.rel_rms_err, clean.ok) == (0, 0.0, float("inf"), True)


def test_pattern_result_decodes_as_before():
    raw = (_u64(5) + _u64(0xFF00FF00FF00FF00) + _u64(0x1000) + _u32(6) + _u32(0xFFFFFFFF)   # 6 asked, 4 slots
           + _u64(0x3000) + _u64(0x11) + _u64(0x12) + _u64(0x1000) + _u64(0x21) + _u64(0x22)
           + _u64(0x4000) + _u64(0x31) + _u64(0x32) + _u64(0x2000) + _u64(2**64 - 1) + _u64(0))
    assert len(raw) == 128
    assert hbm_pattern.read_pattern_result(raw).as_dict() == {
        "bad_words": 5, "bad_bits": 18374966859414961920, "first_bad_offset": 4096, "ok": False,
        "records": [{"offset": 4096, "expected": 33, "got": 34},
                    {"offset": 8192, "expected": 18446744073709551615, "got": 0},
                    {"offset": 12288, "expected": 17, "got": 18},
                    {"offset": 16384, "expected": 49, "got": 50}]}
    clean = _u64(0) + _u64(0) + _u64(2**64 - 1) + _u32(0) + _u32(0) + bytes(96)
    assert hbm_pattern.read_pattern_result(clean).as_dict() == {
        "bad_words": 0, "bad_bits": 0, "first_bad_offset": None, "records": [], "ok": True}


def test_pattern_result_decodes_from_a_tensor():
    res = torch.zeros(16, dtype=torch.int64)
    res[0], res[1], res[2], res[3] = 1, 4, 64, 1
    res[4], res[5], res[6] = 64, 8, 12
    assert hbm_pattern.read_pattern_result(res).as_dict() == {
        "bad_words": 1, "bad_bits": 4, "first_bad_offset": 64, "ok": False,
        "records": [{"offset": 64, "expected": 8, "got": 12}]}


def test_mismatch_records_decode_as_before():
    four = _u64(2) + _u64(9) + _u32(0x3F800000) + _u32(0x3F800001)                 # K7: 4-byte words at 16, 20
    assert _common.compare_report(four, 4).as_dict() == {
        "count": 2, "first_index": 9, "expected": 1065353216, "got": 1065353217, "ok": False}
    eight = _u64(1) + _u64(2**33 + 1) + _u64(0x400921FB54442D18) + _u64(0x400921FB54442D19)   # K10: 8-byte at 16, 24
    assert _common.compare_report(eight, 8).as_dict() == {
        "count": 1, "first_index": 8589934593, "expected": 4614256656552045848,
        "got": 4614256656552045849, "ok": False}
    for raw, width in ((_u64(0) + _u64(2**64 - 1) + bytes(8), 4), (_u64(0) + _u64(2**64 - 1) + bytes(16), 8)):
        assert _common.compare_report(raw, width).as_dict() == {
            "count": 0, "first_index": None, "expected": None, "got": None, "ok": True}
