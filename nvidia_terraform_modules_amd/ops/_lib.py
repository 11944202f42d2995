"""ctypes binding to ``libntm_validation.so`` (the gfx950 HIP kernels) and,
on demand, ``libntm_experimental.so`` (non-default K1 builds and diagnostics,
for tests and tools only).

The library is loaded AFTER ``torch`` so that its ``libamdhip64.so.7``
dependency binds to the HIP runtime PyTorch already mapped (same soname): one
runtime, one set of streams. Loading fails loudly - there is deliberately no
eager/PyTorch fallback for the validation kernels.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import torch  # noqa: F401  (must be imported before the HIP library)

_HERE = Path(__file__).resolve().parent
LIB_PATH = _HERE / "libntm_validation.so"
EXP_LIB_PATH = _HERE / "libntm_experimental.so"

_lib: ctypes.CDLL | None = None
_exp: ctypes.CDLL | None = None


class NativeLibraryMissing(RuntimeError):
    pass


# The ctypes view of the C ABI that validation/include/ntm/abi.h declares: name ->
# (argument types, result type). Module-level tables, readable without a built
# library; tests/test_abi_header.py holds them to the header. SIGNATURES is what
# this module binds on load, XGMI_SIGNATURES what parallel/xgmi.py adds for C2.
c_int, c_size, c_float, c_vp = ctypes.c_int, ctypes.c_size_t, ctypes.c_float, ctypes.c_void_p
c_uint, c_u64, c_double = ctypes.c_uint, ctypes.c_ulonglong, ctypes.c_double
_c_vpp = ctypes.POINTER(c_vp)

SIGNATURES = {
    "ntm_version": ([], ctypes.c_char_p),
    "ntm_gemm_shape_ok": ([c_int, c_int, c_int], c_int),
    "ntm_gemm_bf16": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp], c_int),
    "ntm_gemm_bf16_variant": (
        [c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp], c_int),
    "ntm_gemm_fp8": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp], c_int),
    "ntm_gemm_fp8_shape_ok": ([c_int, c_int, c_int], c_int),
    "ntm_gemm_fp8_variant": ([c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_vp], c_int),
    "ntm_k1_fp8_plan": ([c_int, c_int, c_int, c_vp, c_vp, c_vp], c_int),
    "ntm_k1_fp8_plan_splitk": ([c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp], c_int),
    "ntm_fp8_splitk_ws_bytes": ([c_int, c_int, c_int, c_int], c_size),
    "ntm_gemm_fp8_splitk": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int,
                             c_int, c_vp, c_size, c_vp], c_int),
    "ntm_gemm_fp8_ex": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                         c_size, c_vp], c_int),
    "ntm_gemm_bf16_rowsum": (
        [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp], c_int),
    "ntm_abft_check": ([c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                        c_vp, c_vp, c_vp], c_int),
    "ntm_abft_result_bytes": ([], c_int),
    "ntm_gemm_fp8_rowsum": (
        [c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp], c_int),
    "ntm_abft_check_fp8": ([c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                            c_vp, c_vp, c_vp], c_int),
    "ntm_fill_uniform_bf16": ([c_vp, c_size, c_u64, c_float, c_vp], c_int),
    "ntm_k1_plan": ([c_int, c_int, c_int, c_vp, c_vp, c_vp], c_int),
    "ntm_k1_plan_splitk": ([c_int, c_int, c_int, c_vp, c_vp, c_vp, c_vp], c_int),
    "ntm_gemm_bf16_ex": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                          c_size, c_vp], c_int),
    "ntm_splitk_ws_bytes": ([c_int, c_int, c_int, c_int], c_size),
    "ntm_sk_ws_bytes": ([c_int, c_int, c_int], c_size),
    "ntm_skh_ws_bytes": ([c_int, c_int, c_int, c_int], c_size),
    "ntm_gemm_bf16_skh": ([c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                           c_vp, c_size, c_vp], c_int),
    "ntm_k1_plan_times": ([c_int, c_int, c_int, c_vp, c_vp], c_int),
    "ntm_gemm_bf16_sk": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                          c_size, c_vp], c_int),
    "ntm_gemm_bf16_splitk": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int,
                              c_int, c_int, c_vp, c_size, c_vp], c_int),
    "ntm_fill_uniform_e4m3": ([c_vp, c_size, c_u64, c_float, c_vp], c_int),
    "ntm_ref_gemm_f32_e4m3": (
        [c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp], c_int),
    "ntm_ref_gemm_f32": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp], c_int),
    "ntm_verify_bf16": ([c_vp, c_vp, c_size, c_float, c_float, c_vp, c_vp], c_int),
    "ntm_verify_result_bytes": ([], c_int),
    "ntm_clock_probe": ([c_int, c_int, c_vp, c_vp, c_vp], c_int),
    "ntm_gemm_bf16_clock_grid": ([c_int, c_int], c_int),
    "ntm_gemm_bf16_clock_words": ([], c_int),
    "ntm_sk_error_word_index": ([], c_int),
    "ntm_set_sk_fault_inject": ([c_int], None),
    "ntm_gemm_bf16_skh_ex": ([c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                              c_vp, c_size, c_int, c_vp], c_int),
    "ntm_plan_cus": ([], c_int),
    "ntm_set_cus_override": ([c_int], None),
    "ntm_set_plan_pp_tiles": ([c_int], None),
    "ntm_set_plan_splitk": ([c_double, c_int, c_int], None),
    "ntm_set_plan_splitk_ragged": ([c_int], None),
    "ntm_pp3h_vmcnt": ([c_int, c_int, c_int], c_int),
    "ntm_gemm_bf16_clock": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp,
                             c_vp], c_int),
    "ntm_stream_copy": ([c_vp, c_vp, c_size, c_vp], c_int),
    "ntm_stream_read": ([c_vp, c_size, c_vp, c_vp], c_int),
    "ntm_stream_copy_ex": ([c_vp, c_vp, c_size, c_int, c_int, c_int, c_vp], c_int),
    "ntm_stream_read_ex": ([c_vp, c_size, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_hbm_pattern_write": ([c_vp, c_size, c_u64, c_int, c_u64, c_int,
                               c_vp], c_int),
    "ntm_hbm_pattern_verify": ([c_vp, c_size, c_u64, c_int, c_u64, c_int,
                                c_int, c_vp, c_vp], c_int),
    "ntm_hbm_pattern_result_bytes": ([], c_int),
    "ntm_host_link_default_blocks": ([c_int], c_int),
    "ntm_host_link_tile_bytes": ([c_int], c_int),
    "ntm_host_link_push": ([c_vp, c_size, c_u64, c_int, c_u64, c_int,
                            c_int, c_vp], c_int),
    "ntm_host_link_push_ex": ([c_vp, c_size, c_u64, c_int, c_u64, c_int,
                               c_int, c_int, c_int, c_vp], c_int),
    "ntm_host_link_pull": ([c_vp, c_size, c_u64, c_int, c_u64, c_int,
                            c_vp, c_int, c_vp, c_vp], c_int),
    "ntm_host_link_pull_ex": ([c_vp, c_size, c_u64, c_int, c_u64, c_int,
                               c_vp, c_int, c_int, c_int, c_vp, c_vp], c_int),
    "ntm_host_link_chase": ([c_vp, c_u64, c_u64, c_uint, c_vp,
                             c_vp], c_int),
    "ntm_host_link_clock_khz": ([c_int], c_int),
    "ntm_mx_shape_ok": ([c_int, c_int, c_int], c_int),
    "ntm_mx_gemm": ([c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_mx_reference": ([c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_mx_compare": ([c_vp, c_vp, c_size, c_vp, c_vp], c_int),
    "ntm_mx_mismatch_bytes": ([], c_int),
    "ntm_cu_sweep_record_bytes": ([], c_int),
    "ntm_cu_sweep_expected_bytes": ([c_int], c_size),
    "ntm_cu_sweep_expected": ([c_int, c_uint, c_vp, c_size], c_int),
    "ntm_cu_sweep_lds_words": ([c_uint, c_uint, c_uint, c_uint, c_vp],
                               c_int),
    "ntm_cu_sweep_max_lds_bytes": ([c_int], c_int),
    "ntm_cu_sweep_launch": ([c_vp, c_vp, c_uint, c_int, c_size, c_uint,
                             c_uint, c_int, c_vp], c_int),
    "ntm_cu_sweep_decode": ([c_uint, c_uint, c_vp], None),
    "ntm_cu_sweep_summarize": ([c_vp, c_size, c_uint, c_uint, c_int, c_vp, c_size],
                               c_size),
    "ntm_xcd_sweep_record_bytes": ([], c_int),
    "ntm_xcd_sweep_heads_bytes": ([], c_int),
    "ntm_xcd_sweep_tile_bytes": ([], c_int),
    "ntm_xcd_sweep_mfma_per_batch": ([], c_int),
    "ntm_xcd_sweep_gated": ([c_int, c_int], c_int),
    "ntm_xcd_sweep_read_launch": ([c_vp, c_size, c_uint, c_uint, c_uint, c_int,
                                   c_u64, c_uint, c_int, c_uint, c_vp, c_vp,
                                   c_vp], c_int),
    "ntm_xcd_sweep_mfma_launch": ([c_uint, c_uint, c_uint, c_uint,
                                   c_uint, c_int, c_uint, c_vp, c_vp, c_vp], c_int),
    "ntm_xcd_sweep_summarize": ([c_vp, c_size, c_int, c_int, c_uint, c_uint,
                                 c_u64, c_double, c_int, c_vp, c_size], c_size),
    "ntm_atomics_ops": ([], c_int),
    "ntm_atomics_op_name": ([c_int], ctypes.c_char_p),
    "ntm_atomics_slot_bytes": ([c_int], c_int),
    "ntm_atomics_record_bytes": ([], c_int),
    "ntm_atomics_exact": ([c_int, c_u64, c_u64], c_int),
    "ntm_atomics_rmw_shape_ok": ([c_int, c_u64, c_uint, c_uint, c_u64], c_int),
    "ntm_atomics_expected": ([c_int, c_u64, c_u64, c_u64, c_u64, c_vp], c_int),
    "ntm_atomics_rmw_launch": ([c_int, c_vp, c_u64, c_uint, c_uint, c_u64, c_u64, c_vp], c_int),
    "ntm_atomics_rmw_reference_launch": ([c_int, c_vp, c_u64, c_uint, c_uint, c_u64, c_u64, c_vp], c_int),
    "ntm_atomics_ticket_claim_bytes": ([c_uint, c_uint, c_uint], c_size),
    "ntm_atomics_counter_bytes": ([c_uint], c_size),
    "ntm_atomics_ticket_launch": ([c_vp, c_vp, c_uint, c_uint, c_uint, c_uint, c_vp], c_int),
    "ntm_atomics_handoff_slab_bytes": ([c_uint, c_uint], c_size),
    "ntm_atomics_handoff_init": ([c_vp, c_uint, c_uint, c_u64, c_uint, c_vp], c_int),
    "ntm_atomics_handoff_launch": ([c_vp, c_vp, c_vp, c_uint, c_uint, c_u64, c_uint, c_uint, c_vp], c_int),
    "ntm_atomics_summarize_rmw": ([c_int, c_vp, c_vp, c_u64, c_int, c_vp, c_size], c_size),
    "ntm_atomics_summarize_tickets": ([c_vp, c_vp, c_uint, c_uint, c_uint, c_int, c_vp, c_size], c_size),
    "ntm_atomics_summarize_handoff": ([c_vp, c_size, c_uint, c_uint, c_uint, c_uint, c_int, c_vp, c_size], c_size),
    "ntm_mcore_gemm": ([c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_mcore_reference": ([c_int, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_mcore_compare": ([c_vp, c_vp, c_size, c_int, c_vp, c_vp], c_int),
    "ntm_mcore_mismatch_bytes": ([], c_int),
    "ntm_mxq_shape_ok": ([c_int, c_int, c_int], c_int),
    "ntm_mxq_quantize": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_u64, c_vp], c_int),
    "ntm_mxq_dequantize": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_mxq_cvt": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_u64, c_vp], c_int),
    "ntm_mxq_reference_quantize": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_mxq_reference_dequantize": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_mxq_reference_cvt": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_vp], c_int),
    "ntm_wave_lane_ops": ([], c_int),
    "ntm_wave_record_bytes": ([], c_int),
    "ntm_wave_lane": ([c_int, c_int, c_int, c_vp, c_vp, c_vp, c_size, c_vp], c_int),
    "ntm_wave_tr_out_words": ([c_int, c_int, c_int], c_int),
    "ntm_wave_tr_read": ([c_int, c_int, c_vp, c_int, c_int, c_vp, c_vp], c_int),
    "ntm_wave_sfu": ([c_int, c_vp, c_vp, c_size, c_vp], c_int),
    "ntm_wave_sfu_distance": ([c_vp, c_vp, c_vp, c_size, ctypes.c_uint, c_vp, c_vp], c_int),
    "ntm_wave_sfu_locate": ([c_int, c_vp, ctypes.c_uint, ctypes.c_uint, c_int, c_vp, c_vp, c_vp, c_int, ctypes.c_uint,
                             ctypes.c_uint, c_vp], c_int),
    "ntm_wave_valu": ([c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_size, c_vp], c_int),
    "ntm_wave_sweep": ([c_int, c_vp, c_size, c_vp, c_vp, c_vp, c_int, ctypes.c_uint, ctypes.c_uint, c_vp], c_int),
    "ntm_attn_shape_ok": ([c_int, c_int, c_int, c_int, c_int, c_int], c_int),
    "ntm_attn_table_bytes": ([c_int, c_int, c_int], c_size),
    "ntm_attn_lds_bytes": ([], c_int),
    "ntm_attn_fwd": ([c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_float,
                      c_vp], c_int),
    "ntm_attn_reference": ([c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                            c_float, c_vp], c_int),
    "ntm_attn_compare": ([c_vp, c_vp, c_size, c_vp, c_vp], c_int),
    "ntm_attn_mismatch_bytes": ([], c_int),
    "ntm_pda_shape_ok": ([c_int, c_int, c_int, c_int, c_int, c_int, c_int], c_int),
    "ntm_pda_workspace_bytes": ([c_int, c_int, c_int], c_size),
    "ntm_pda_table_bytes": ([c_int, c_int, c_int], c_size),
    "ntm_pda_lds_bytes": ([], c_int),
    "ntm_pda_default_splits": ([c_int, c_int, c_int, c_int], c_int),
    "ntm_pda_fwd": ([c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int,
                     c_int, c_int, c_float, c_vp], c_int),
}

XGMI_SIGNATURES = {
    "ntm_xgmi_allreduce_bf16": ([_c_vpp, _c_vpp, _c_vpp, c_int, c_int, c_int, c_int, c_size,
                                 c_uint, c_vp, c_int, c_vp], c_int),
    "ntm_xgmi_allreduce_bf16_ex": ([_c_vpp, _c_vpp, _c_vpp, c_int, c_int, c_int, c_int, c_size,
                                    c_uint, c_vp, c_int, c_uint, c_uint, c_vp], c_int),
    "ntm_xgmi_signal_bytes": ([c_int], c_size),
    "ntm_malloc": ([_c_vpp, c_size, c_int], c_int),
    "ntm_free": ([c_vp], c_int),
    "ntm_memset_async": ([c_vp, c_int, c_size, c_vp], c_int),
    "ntm_ipc_handle": ([c_vp, c_vp], c_int),
    "ntm_ipc_open": ([c_vp, _c_vpp], c_int),
    "ntm_ipc_close": ([c_vp], c_int),
}


def declare(lib: ctypes.CDLL, signatures: dict) -> None:
    for name, (argt, rest) in signatures.items():
        fn = getattr(lib, name)
        fn.argtypes = argt
        fn.restype = rest


def _declare(lib: ctypes.CDLL) -> None:
    declare(lib, SIGNATURES)


def lib() -> ctypes.CDLL:
    """Return the loaded library, raising if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise NativeLibraryMissing(
            f"{LIB_PATH} not found. Build it with "
            "`python -m nvidia_terraform_modules_amd.ops.build` (needs hipcc, gfx950)."
        )
    mode = os.RTLD_NOW | getattr(os, "RTLD_GLOBAL", 0)
    _lib = ctypes.CDLL(str(LIB_PATH), mode=mode)
    _declare(_lib)
    return _lib


def _declare_experimental(lib: ctypes.CDLL) -> None:
    gemm = [c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp]
    sig = {
        "ntm_experimental_version": ([], ctypes.c_char_p),
        "ntm_gemm_bf16_experimental": (gemm, c_int),
        "ntm_gemm_bf16_knob": (gemm, c_int),
        "ntm_gemm_bf16_ws_knob": ([c_int] + gemm, c_int),
        "ntm_gemm_bf16_stamp": (
            [c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_vp, c_vp], c_int),
        "ntm_mfma_f8_probe": ([c_vp, c_vp, c_vp, c_vp], c_int),
        "ntm_mx_mfma_probe": ([c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp], c_int),
        "ntm_mcore_mfma_probe": ([c_int, c_vp, c_vp, c_vp, c_int, c_int, c_vp, c_vp], c_int),
        "ntm_mxq_cvt_probe": ([c_int, c_int, c_vp, c_vp, c_vp, c_vp, c_vp, c_int, c_vp], c_int),
        "ntm_wave_tr_probe": ([c_int, c_vp, c_vp, c_vp, c_vp], c_int),
        "ntm_mfma_rate": ([c_int, c_int, c_int, c_vp, c_vp, c_vp], c_int),
        "ntm_mfma_toggle": ([c_int, c_int, c_int, c_vp, c_vp, c_vp], c_int),
        "ntm_dma_probe": ([c_int, c_vp, c_int, c_int, c_int, c_int, c_vp], c_int),
        "ntm_gemm_fp8_knob": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int, c_int,
                               c_vp], c_int),
        "ntm_gemm_bf16_sk_rev": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                                  c_vp, c_size, c_vp], c_int),
        "ntm_gemm_bf16_sk_nopair": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                                     c_vp, c_size, c_vp], c_int),
        "ntm_gemm_bf16_sk_stamp": ([c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int, c_int, c_int,
                                    c_vp, c_size, c_vp, c_vp], c_int),
        "ntm_gemm_bf16_pp6_stamp": ([c_int, c_int, c_vp, c_vp, c_vp, c_int, c_int, c_int, c_int,
                                     c_int, c_int, c_vp, c_vp], c_int),
    }
    declare(lib, sig)


def lib_experimental() -> ctypes.CDLL:
    """The experimental/diagnostic library (non-default K1 builds, schedule
    knobs, probes). Loaded on first use; the shipping paths never touch it."""
    global _exp
    if _exp is not None:
        return _exp
    lib()  # HIP runtime binding order: the shipping library (and torch) first
    if not EXP_LIB_PATH.exists():
        raise NativeLibraryMissing(
            f"{EXP_LIB_PATH} not found. Build it with "
            "`python -m nvidia_terraform_modules_amd.ops.build`.")
    _exp = ctypes.CDLL(str(EXP_LIB_PATH), mode=os.RTLD_NOW | getattr(os, "RTLD_GLOBAL", 0))
    _declare_experimental(_exp)
    return _exp


def available() -> bool:
    try:
        lib()
        return True
    except (NativeLibraryMissing, OSError):
        return False


def check(rc: int, what: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{what} failed with hipError {rc}")


def stream_handle(stream: "torch.cuda.Stream | None" = None) -> int:
    if stream is None:
        stream = torch.cuda.current_stream()
    return int(stream.cuda_stream)


def version() -> str:
    return lib().ntm_version().decode()
