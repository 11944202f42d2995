"""MI355X (gfx950) HIP kernels used by the post-provision validation Job.

K1 ``gemm_bf16``      - 256x256x64 LDS-DMA + MFMA bf16 GEMM (the headline; small,
                        mid-size and ragged C also on 128x128 / 256x128 / 160x160 /
                        160x128 / 128x160 tiles, skinny long-K C split-K; see
                        ``k1_plan`` / ``k1_splitk_plan``);
   ``gemm_bf16_rowsum`` - same kernel with the fused ABFT row-checksum epilogue;
   ``gemm_fp8``         - the same kernels on OCP e4m3 operands (f8f6f4 MFMA; 256x256
                          and the wave-specialised tiles, ``k1_fp8_plan``).
K2 ``stream_copy``, ``stream_read`` - tuned float4 HBM streams.
K4 ``hbm_pattern_write``, ``hbm_pattern_verify`` - address / hash pattern fill and
   on-device compare for the full-capacity HBM test.
K5 ``cu_sweep``, ``cu_sweep_decode``, ``cu_sweep_summarize`` - known-answer LDS / VALU /
   MFMA sub-tests per workgroup, tied to the CU that ran them.
K6 ``host_link_push``, ``host_link_pull``, ``host_link_chase`` - the same pattern written to and
   read from pinned host memory over the host link (PCIe), and its read round-trip latency.
K7 ``mx_gemm``, ``mx_reference_gpu``, ``mx_compare`` - a block-scaled GEMM in the MX formats
   (e4m3, e5m2, e2m3, e3m2, e2m1 with E8M0 scales) on the scaled f8f6f4 matrix instruction, a
   reference without matrix cores and a bitwise compare; ``mx_pack``, ``mx_unpack``,
   ``mx_make_inputs``, ``mx_dense_exact`` - the host side (numpy, ``ops.mx``).
K8 ``xcd_sweep_read``, ``xcd_sweep_mfma``, ``xcd_sweep_summarize`` - a verified read and an
   MFMA clock probe per XCD, each XCD timed against its own stamps.
K9 ``atomics_rmw``, ``atomics_rmw_reference``, ``atomics_tickets``, ``atomics_handoff``,
   ``atomics_summarize`` - every kind of global atomic with a checked answer, and plain stores
   handed from one XCD to another under agent-scope release / acquire.
K10 ``mcore_gemm``, ``mcore_reference_gpu``, ``mcore_compare`` - the fp64, fp32, fp16 and int8
   MFMAs and the 2:4-sparse bf16 / int8 SMFMACs with exact answers, a reference without
   matrix instructions and a bitwise compare; ``mcore_make_inputs``, ``mcore_matmul_bits``,
   ``mcore_exact``, ``mcore_compress``, ``mcore_expand`` - the host side (numpy, ``ops.mcore``).
K11 ``mx_quantize``, ``mx_dequantize``, ``mxq_cvt`` - MX quantise / dequantise on the device with
   the scaled-conversion instructions, producing what ``mx_gemm`` takes;
   ``mx_quantize_reference_gpu``, ``mx_dequantize_reference_gpu`` - the same by integer
   arithmetic; ``mxq_quantize_bits``, ``mxq_dequantize_bits``, ``mxq_make_inputs`` - the host
   side (numpy, ``ops.mxq``).
K12 ``wave_lane``, ``wave_tr_read``, ``wave_sfu``, ``wave_sfu_digest``, ``wave_sfu_distance``,
   ``wave_sfu_locate``, ``wave_valu``, ``wave_sweep`` - cross-lane movement, the gfx950 transposed LDS reads, the fp32
   transcendentals and v_bitop3 / v_cvt_pk_bf16 on the device; ``wave_lane_reference_gpu``,
   ``wave_tr_read_reference_gpu`` - the same without the instructions under test;
   ``wave_expected_*``, ``wave_sfu_inputs``, ``wave_sfu_brackets`` - the host side (numpy, ``ops.wave``).
K3 ``fill_uniform_``, ``ref_gemm_f32``, ``verify_bf16``, ``abft_check`` - synthetic
   data, full fp32 reference check and the O(n^2) checksum check;
   ``clock_probe_ghz`` - the shader clock held under a dense MFMA load;
   ``gemm_clock_ghz`` - the clock K1's own 8192^3-class launches run at
   (``gemm_clock_stable``: the same, re-stamped until a batch is transient-free).
K1 - K3 and the clocks are in ``ops.kernels``, each of K4 - K12 in its own ``ops.gpu`` module.
Import is cheap; the native library is loaded on first kernel call and raises
``NativeLibraryMissing`` if it was not built (no silent fallback).
"""
from ._lib import NativeLibraryMissing, available, version  # noqa: F401
from .kernels import (  # noqa: F401
    AbftReport, VerifyReport, abft_check, clock_probe_ghz, fill_uniform_, gemm_bf16,
    gemm_bf16_rowsum, clock_summary, gemm_clock_ghz, gemm_clock_stable, gemm_fp8, gemm_fp8_rowsum,
    gemm_fp8_shape_ok, gemm_shape_ok, gemm_tolerance, FP8_VARIANTS, k1_fp8_plan, k1_fp8_splitk_plan,
    k1_candidates, k1_plan, k1_splitk_plan, ref_gemm_f32, set_plan_pp_tiles, set_plan_splitk,
    set_plan_splitk_ragged, set_cus_override, sk_ws_bytes, sk_xcc_error, SkPlacementError,
    set_sk_fault_inject, sk_check_enabled, stream_copy, stream_read, verify_bf16,
)
from .gpu.hbm_pattern import (  # noqa: F401
    HBM_PATTERN_ADDR, HBM_PATTERN_HASH, HbmPatternReport, hbm_pattern_verify, hbm_pattern_write,
)
from .gpu.host_link import (  # noqa: F401
    host_link_chase, host_link_default_blocks, host_link_pull, host_link_push, host_link_tile_bytes,
)
from .gpu.mx import (  # noqa: F401
    MxCompareReport, mx_compare, mx_gemm, mx_reference_gpu,
)
from .gpu.mxq import (  # noqa: F401
    mx_dequantize, mx_dequantize_reference_gpu, mx_quantize, mx_quantize_reference_gpu, mxq_cvt,
    mxq_to_device,
)
from .gpu.mcore import (  # noqa: F401
    McoreCompareReport, mcore_compare, mcore_gemm, mcore_reference_gpu, mcore_to_device,
)
from .gpu.cu_sweep import (  # noqa: F401
    CU_SWEEP_SUBTESTS, cu_sweep, cu_sweep_decode, cu_sweep_max_lds_bytes, cu_sweep_record_dtype,
    cu_sweep_summarize,
)
from .gpu.xcd_sweep import (  # noqa: F401
    XCD_SWEEP_LEVELS, XCD_SWEEP_MODES, xcd_sweep_gated, xcd_sweep_mfma, xcd_sweep_read,
    xcd_sweep_record_dtype, xcd_sweep_summarize, xcd_sweep_xcds,
)
from .gpu.atomics import (  # noqa: F401
    ATOMIC_OPS, atomics_exact, atomics_handoff, atomics_record_dtype, atomics_rmw,
    atomics_rmw_expected, atomics_rmw_reference, atomics_summarize, atomics_tickets,
)
from .gpu.wave import (  # noqa: F401
    wave_cu_key, wave_lane, wave_lane_reference_gpu, wave_sfu, wave_sfu_digest, wave_sfu_distance,
    wave_sfu_locate, wave_sweep, wave_to_device, wave_tr_read, wave_tr_read_reference_gpu, wave_valu,
)
from .wave import (  # noqa: F401
    WAVE_FAMILIES, WAVE_FAULT_BIT, WAVE_SFU_BOUND, WAVE_SFU_OPS, WAVE_TR_BITS, wave_bf16_rne,
    wave_bpermute_index, wave_cvt_inputs, wave_expected_bitop3, wave_expected_cvt_pk,
    wave_expected_lane, wave_expected_sfu_distance, wave_expected_tr_read, wave_failure_message,
    wave_hash32, wave_lane_op_index, wave_lane_op_name, wave_lane_ops, wave_make_image,
    wave_sfu_brackets, wave_sfu_inputs, wave_src_lane, wave_tr_shape, wave_tr_src,
)
from .mxq import (  # noqa: F401
    MXQ_EMAX, MXQ_MAX_CODE, mx_bits, mxq_dequantize_bits, mxq_failure_message, mxq_make_inputs,
    mxq_quantize_bits, mxq_quantize_codes, mxq_scale_bytes, mxq_shape_ok,
)
from .mcore import (  # noqa: F401
    MCORE_FORMATS, mcore_compress, mcore_decode_windows, mcore_exact, mcore_expand,
    mcore_failure_message, mcore_format, mcore_make_inputs, mcore_matmul_bits, mcore_max_abits,
)
from .mx import (  # noqa: F401
    MX_FORMATS, mx_dense_exact, mx_make_inputs, mx_matmul_bits, mx_max_spread, mx_pack, mx_shape_ok,
    mx_unpack,
)
