/* The C ABI of the shipping native code: every function that ntm_validation.hip
 * and xgmi_allreduce.hip export, declared once.
 *
 * Three users read this file:
 *   - the two .hip files include it, so a definition that disagrees with its
 *     prototype does not compile;
 *   - the Job binary (validation/src/validate/) includes it instead of
 *     re-declaring what it calls;
 *   - tests/test_abi_header.py parses it and holds the ctypes tables of
 *     ops/_lib.py (SIGNATURES, XGMI_SIGNATURES) to it, name by name and
 *     argument by argument.
 *
 * Plain C: no HIP type appears here. Streams and device buffers cross as
 * void*; an int result is a hipError_t (0 = success) unless the name says
 * otherwise (*_bytes, *_ok, *_index ...). One prototype per statement, each
 * starting with NTM_API, so the test's small parser can read them.
 */
#ifndef NTM_ABI_H
#define NTM_ABI_H

#include <stddef.h>

#ifdef __cplusplus
#define NTM_API extern "C" __attribute__((visibility("default")))
#else
#define NTM_API __attribute__((visibility("default")))
#endif

/* ranks of one C2 communicator: the length of the pointer arrays below */
#define NTM_XGMI_MAX_RANKS 8

/* ---- library */
NTM_API const char* ntm_version(void);

/* ---- K1 dispatch plan (ntm/k1_plan.hpp) and its knobs */
NTM_API int ntm_gemm_shape_ok(int M, int N, int K);
NTM_API void ntm_set_plan_pp_tiles(int on);
NTM_API void ntm_set_plan_splitk(double margin, int long_k, int fp8_long);
NTM_API void ntm_set_plan_splitk_ragged(int on);
NTM_API int ntm_pp3h_vmcnt(int ah, int bh, int phase);
NTM_API int ntm_k1_plan_times(int M, int N, int K, double* unsplit_s, double* sk_s);
NTM_API int ntm_k1_plan(int M, int N, int K, int* top_rows, int* top_variant, int* rest_variant);
NTM_API int ntm_k1_plan_splitk(int M, int N, int K, int* top_rows, int* top_variant, int* rest_variant, int* splits);
NTM_API int ntm_plan_cus(void);
NTM_API void ntm_set_cus_override(int cus);

/* ---- K1 bf16 GEMM, C = A B^T */
NTM_API int ntm_gemm_bf16(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* stream);
NTM_API int ntm_gemm_bf16_ex(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes, void* stream);
NTM_API int ntm_gemm_bf16_variant(int variant, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* stream);
NTM_API size_t ntm_splitk_ws_bytes(int M, int N, int K, int splits);
NTM_API int ntm_gemm_bf16_splitk(int variant, int splits, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes, void* stream);

/* ---- K1 stream-K */
NTM_API int ntm_sk_error_word_index(void);
NTM_API void ntm_set_sk_fault_inject(int v);
NTM_API size_t ntm_sk_ws_bytes(int M, int N, int K);
NTM_API int ntm_gemm_bf16_sk(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes, void* stream);
NTM_API size_t ntm_skh_ws_bytes(int variant, int M, int N, int K);
NTM_API int ntm_gemm_bf16_skh(int variant, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes, void* stream);
NTM_API int ntm_gemm_bf16_skh_ex(int variant, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes, int fault, void* stream);

/* ---- K1-fp8 (e4m3 operands) */
NTM_API int ntm_gemm_fp8_shape_ok(int M, int N, int K);
NTM_API int ntm_k1_fp8_plan(int M, int N, int K, int* top_rows, int* top_variant, int* rest_variant);
NTM_API int ntm_k1_fp8_plan_splitk(int M, int N, int K, int* top_rows, int* top_variant, int* rest_variant, int* splits);
NTM_API int ntm_gemm_fp8(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* stream);
NTM_API int ntm_gemm_fp8_ex(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes, void* stream);
NTM_API int ntm_gemm_fp8_variant(int variant, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* stream);
NTM_API size_t ntm_fp8_splitk_ws_bytes(int M, int N, int K, int splits);
NTM_API int ntm_gemm_fp8_splitk(int variant, int splits, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* ws, size_t ws_bytes, void* stream);

/* ---- K1 with the fused ABFT row checksum */
NTM_API int ntm_gemm_bf16_rowsum(const void* A, const void* B, void* C, float* rowsum, int M, int N, int K, int lda, int ldb, int ldc, void* stream);
NTM_API int ntm_gemm_fp8_rowsum(const void* A, const void* B, void* C, float* rowsum, int M, int N, int K, int lda, int ldb, int ldc, void* stream);
NTM_API int ntm_abft_check(const void* A, const void* B, const void* C, const float* rowsum, int M, int N, int K, int lda, int ldb, int ldc, double* scratch, void* result, void* stream);
NTM_API int ntm_abft_check_fp8(const void* A, const void* B, const void* C, const float* rowsum, int M, int N, int K, int lda, int ldb, int ldc, double* scratch, void* result, void* stream);
NTM_API int ntm_abft_result_bytes(void);

/* ---- fills, fp32 reference GEMMs, element-wise verification */
NTM_API int ntm_fill_uniform_bf16(void* out, size_t n, unsigned long long seed, float scale, void* stream);
NTM_API int ntm_fill_uniform_e4m3(void* out, size_t n, unsigned long long seed, float scale, void* stream);
NTM_API int ntm_ref_gemm_f32(const void* A, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, void* stream);
NTM_API int ntm_ref_gemm_f32_e4m3(const void* A, const void* B, float* C, int M, int N, int K, int lda, int ldb, int ldc, void* stream);
NTM_API int ntm_verify_bf16(const void* C, const float* R, size_t n, float atol, float rtol, void* result, void* stream);
NTM_API int ntm_verify_result_bytes(void);

/* ---- clock probes */
NTM_API int ntm_clock_probe(int grid, int iters, void* out, float* sink, void* stream);
NTM_API int ntm_gemm_bf16_clock_words(void);
NTM_API int ntm_gemm_bf16_clock_grid(int M, int N);
NTM_API int ntm_gemm_bf16_clock(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc, void* stamps, void* stream);

/* ---- K2 HBM stream copy / read */
NTM_API int ntm_stream_copy(const void* src, void* dst, size_t bytes, void* stream);
NTM_API int ntm_stream_read(const void* src, size_t bytes, float* sink, void* stream);
NTM_API int ntm_stream_copy_ex(const void* src, void* dst, size_t bytes, int unroll, int policy, int grid, void* stream);
NTM_API int ntm_stream_read_ex(const void* src, size_t bytes, float* sink, int unroll, int policy, int grid, void* stream);

/* ---- K4 HBM pattern test (ntm/hbm_pattern.hpp) */
NTM_API int ntm_hbm_pattern_result_bytes(void);
NTM_API int ntm_hbm_pattern_write(void* ptr, size_t bytes, unsigned long long base_bytes, int pattern, unsigned long long seed, int invert, void* stream);
NTM_API int ntm_hbm_pattern_verify(void* ptr, size_t bytes, unsigned long long base_bytes, int pattern, unsigned long long seed, int invert, int invert_after, void* result, void* stream);

/* ---- K5 per-CU compute sweep (ntm/cu_sweep.hpp, ntm/cu_sweep_plan.hpp) */
NTM_API int ntm_cu_sweep_record_bytes(void);
NTM_API size_t ntm_cu_sweep_expected_bytes(int iters);
NTM_API int ntm_cu_sweep_expected(int iters, unsigned seed, void* out, size_t out_bytes);
NTM_API int ntm_cu_sweep_lds_words(unsigned seed, unsigned round, unsigned first, unsigned count, unsigned* out);
NTM_API int ntm_cu_sweep_max_lds_bytes(int device);
NTM_API int ntm_cu_sweep_launch(void* records, const void* expected, unsigned grid, int iters, size_t lds_bytes, unsigned seed, unsigned fault_key, int fault_subtest, void* stream);
NTM_API void ntm_cu_sweep_decode(unsigned hw_id, unsigned xcc_id, unsigned* out);
NTM_API size_t ntm_cu_sweep_summarize(const void* records, size_t n, unsigned cus, unsigned launches, int gpu, char* json, size_t cap);

/* ---- K6 host-link check (ntm/host_link.hpp, ntm/host_link_plan.hpp) */
NTM_API int ntm_host_link_default_blocks(int pull);
NTM_API int ntm_host_link_tile_bytes(int pull);
NTM_API int ntm_host_link_push(void* host, size_t bytes, unsigned long long base_bytes, int pattern, unsigned long long seed, int invert, int blocks, void* stream);
NTM_API int ntm_host_link_push_ex(void* host, size_t bytes, unsigned long long base_bytes, int pattern, unsigned long long seed, int invert, int blocks, int unroll, int nt, void* stream);
NTM_API int ntm_host_link_pull(const void* host, size_t bytes, unsigned long long base_bytes, int pattern, unsigned long long seed, int invert, void* dst, int blocks, void* result, void* stream);
NTM_API int ntm_host_link_pull_ex(const void* host, size_t bytes, unsigned long long base_bytes, int pattern, unsigned long long seed, int invert, void* dst, int blocks, int unroll, int nt, void* result, void* stream);
NTM_API int ntm_host_link_chase(const void* host, unsigned long long nslots, unsigned long long start, unsigned hops, void* out, void* stream);
NTM_API int ntm_host_link_clock_khz(int device);

/* ---- K7 MX block-scaled matrix check (ntm/mx_gemm.hpp, ntm/mx_plan.hpp) */
NTM_API int ntm_mx_shape_ok(int M, int N, int K);
NTM_API int ntm_mx_gemm(int fmt, const void* A, const void* B, const void* SA, const void* SB, void* C, int M, int N, int K, void* stream);
NTM_API int ntm_mx_reference(int fmt, const void* A, const void* B, const void* SA, const void* SB, void* C, int M, int N, int K, void* stream);
NTM_API int ntm_mx_compare(const void* expected, const void* got, size_t n, void* out, void* stream);
NTM_API int ntm_mx_mismatch_bytes(void);

/* ---- K8 per-XCD sweep (ntm/xcd_sweep.hpp, ntm/xcd_sweep_plan.hpp) */
NTM_API int ntm_xcd_sweep_record_bytes(void);
NTM_API int ntm_xcd_sweep_heads_bytes(void);
NTM_API int ntm_xcd_sweep_tile_bytes(void);
NTM_API int ntm_xcd_sweep_mfma_per_batch(void);
NTM_API int ntm_xcd_sweep_gated(int level, int mode);
NTM_API int ntm_xcd_sweep_read_launch(const void* buf, size_t slice_bytes, unsigned xcds, unsigned xcd_mask, unsigned passes, int pattern, unsigned long long seed, unsigned grid, int slow_xcd, unsigned slow_factor, void* heads, void* records, void* stream);
NTM_API int ntm_xcd_sweep_mfma_launch(unsigned grid, unsigned batches, unsigned seed, unsigned xcds, unsigned xcd_mask, int slow_xcd, unsigned slow_factor, void* records, float* sink, void* stream);
NTM_API size_t ntm_xcd_sweep_summarize(const void* records, size_t n, int level, int mode, unsigned xcds, unsigned mask, unsigned long long expected_tiles, double ratio, int gpu, char* json, size_t cap);

/* ---- K9 atomics and cross-XCD hand-off check (ntm/atomics.hpp, ntm/atomics_plan.hpp) */
NTM_API int ntm_atomics_ops(void);
NTM_API const char* ntm_atomics_op_name(int op);
NTM_API int ntm_atomics_slot_bytes(int op);
NTM_API int ntm_atomics_record_bytes(void);
NTM_API int ntm_atomics_exact(int op, unsigned long long adds_per_slot, unsigned long long max_abs);
NTM_API int ntm_atomics_rmw_shape_ok(int op, unsigned long long slots, unsigned grid, unsigned iters, unsigned long long max_abs);
NTM_API int ntm_atomics_expected(int op, unsigned long long slots, unsigned long long total, unsigned long long seed, unsigned long long max_abs, void* out);
NTM_API int ntm_atomics_rmw_launch(int op, void* table, unsigned long long slots, unsigned grid, unsigned iters, unsigned long long seed, unsigned long long max_abs, void* stream);
NTM_API int ntm_atomics_rmw_reference_launch(int op, void* table, unsigned long long slots, unsigned grid, unsigned iters, unsigned long long seed, unsigned long long max_abs, void* stream);
NTM_API size_t ntm_atomics_ticket_claim_bytes(unsigned heads, unsigned grid, unsigned iters);
NTM_API size_t ntm_atomics_counter_bytes(unsigned counters);
NTM_API int ntm_atomics_ticket_launch(void* counters, void* claim, unsigned heads, unsigned grid, unsigned iters, unsigned inject_gid, void* stream);
NTM_API size_t ntm_atomics_handoff_slab_bytes(unsigned episodes, unsigned episode_size);
NTM_API int ntm_atomics_handoff_init(void* slabs, unsigned episodes, unsigned episode_size, unsigned long long seed, unsigned round, void* stream);
NTM_API int ntm_atomics_handoff_launch(void* slabs, void* counters, void* records, unsigned episodes, unsigned episode_size, unsigned long long seed, unsigned round, unsigned inject_wg, void* stream);
NTM_API size_t ntm_atomics_summarize_rmw(int op, const void* got, const void* expected, unsigned long long slots, int gpu, char* json, size_t cap);
NTM_API size_t ntm_atomics_summarize_tickets(const void* counters, const void* claim, unsigned heads, unsigned grid, unsigned iters, int gpu, char* json, size_t cap);
NTM_API size_t ntm_atomics_summarize_handoff(const void* records, size_t n, unsigned episodes, unsigned episode_size, unsigned xcds, unsigned launches, int gpu, char* json, size_t cap);

/* ---- K10 fp64 / fp32 / fp16 / int8 / 2:4-sparse matrix-core check (ntm/mcore.hpp, ntm/mcore_plan.hpp) */
NTM_API int ntm_mcore_gemm(int fmt, const void* A, const void* AI, const void* B, void* C, int M, int N, int K, void* stream);
NTM_API int ntm_mcore_reference(int fmt, const void* A, const void* AI, const void* B, void* C, int M, int N, int K, void* stream);
NTM_API int ntm_mcore_compare(const void* expected, const void* got, size_t n, int word_bytes, void* out, void* stream);
NTM_API int ntm_mcore_mismatch_bytes(void);

/* ---- K11 MX quantise / dequantise on the device (ntm/mxq.hpp, ntm/mxq_plan.hpp) */
NTM_API int ntm_mxq_shape_ok(int R, int K, int ldx);
NTM_API int ntm_mxq_quantize(int fmt, int src_dtype, const void* x, void* packed, void* scales, int R, int K, int ldx, int rounding, unsigned long long seed, void* stream);
NTM_API int ntm_mxq_dequantize(int fmt, int dst_dtype, const void* packed, const void* scales, void* y, int R, int K, int ldx, void* stream);
NTM_API int ntm_mxq_cvt(int fmt, int src_dtype, const void* x, const void* scales, void* packed, int R, int K, int ldx, int rounding, unsigned long long seed, void* stream);
NTM_API int ntm_mxq_reference_quantize(int fmt, int src_dtype, const void* x, void* packed, void* scales, int R, int K, int ldx, void* stream);
NTM_API int ntm_mxq_reference_dequantize(int fmt, int dst_dtype, const void* packed, const void* scales, void* y, int R, int K, int ldx, void* stream);
NTM_API int ntm_mxq_reference_cvt(int fmt, int src_dtype, const void* x, const void* scales, void* packed, int R, int K, int ldx, void* stream);

/* ---- K12 wave data-path and special-function check (ntm/wave_paths.hpp, ntm/wave_paths_plan.hpp) */
NTM_API int ntm_wave_lane_ops(void);
NTM_API int ntm_wave_record_bytes(void);
NTM_API int ntm_wave_lane(int reference, int op_first, int op_count, const void* x, const void* y, void* out, size_t n, void* stream);
NTM_API int ntm_wave_tr_out_words(int bits, int rows, int stride);
NTM_API int ntm_wave_tr_read(int reference, int bits, const void* image, int rows, int stride, void* out, void* stream);
NTM_API int ntm_wave_sfu(int op, const void* x, void* y, size_t n, void* stream);
NTM_API int ntm_wave_sfu_distance(const void* y, const void* lo, const void* hi, size_t n, unsigned bound, void* out, void* stream);
NTM_API int ntm_wave_sfu_locate(int op, const void* x, unsigned n, unsigned cu_key, int on_key, void* claim, void* y, void* record, int grid, unsigned fault_key, unsigned fault_index, void* stream);
NTM_API int ntm_wave_valu(int reference, int op, const void* a, const void* b, const void* c, void* out, size_t n, void* stream);
NTM_API int ntm_wave_sweep(int family, const void* in, size_t in_words, const unsigned* layout, const void* expected, void* records, int grid, unsigned fault_wg, unsigned fault_index, void* stream);

/* ---- K13 fused attention forward (ntm/attn.hpp, ntm/attn_plan.hpp) */
NTM_API int ntm_attn_shape_ok(int B, int Hq, int Hkv, int Sq, int Sk, int causal);
NTM_API size_t ntm_attn_table_bytes(int B, int Hq, int Sq);
NTM_API int ntm_attn_lds_bytes(void);
NTM_API int ntm_attn_fwd(const void* Q, const void* K, const void* V, void* O, float* m, float* l, unsigned* table, int B, int Hq, int Hkv, int Sq, int Sk, int causal, float scale_log2, void* stream);
NTM_API int ntm_attn_reference(const void* Q, const void* K, const void* V, void* O, float* O32, float* absum, float* m, float* l, int B, int Hq, int Hkv, int Sq, int Sk, int causal, float scale_log2, void* stream);
NTM_API int ntm_attn_compare(const void* expected, const void* got, size_t n, void* out, void* stream);
NTM_API int ntm_attn_mismatch_bytes(void);

/* ---- K14 paged-KV decode attention (ntm/pda.hpp, ntm/pda_plan.hpp) */
NTM_API int ntm_pda_shape_ok(int B, int Hq, int Hkv, int T, int max_pages, int pages, int splits);
NTM_API size_t ntm_pda_workspace_bytes(int B, int Hkv, int splits);
NTM_API size_t ntm_pda_table_bytes(int B, int Hkv, int splits);
NTM_API int ntm_pda_lds_bytes(void);
NTM_API int ntm_pda_default_splits(int B, int Hkv, int max_len, int cus);
NTM_API int ntm_pda_fwd(const void* Q, const void* Kpool, const void* Vpool, const int* block_table, const int* seq_lens, void* O, float* m, float* l, void* workspace, unsigned* table, int B, int Hq, int Hkv, int T, int max_pages, int pages, int splits, float scale_log2, void* stream);

/* ---- C2 hand-written xGMI all-reduce (xgmi_allreduce.hip, ntm/xgmi_allreduce.hpp)
 * and the allocation / HIP IPC helpers its Python side needs */
NTM_API int ntm_xgmi_allreduce_bf16(const void* const* in_ptrs, void* const* out_ptrs, unsigned* const* sig_ptrs, int nranks, int rank_base, int nranks_here, int nblk, size_t count, unsigned epoch, unsigned* err, int one_shot, void* stream);
NTM_API int ntm_xgmi_allreduce_bf16_ex(const void* const* in_ptrs, void* const* out_ptrs, unsigned* const* sig_ptrs, int nranks, int rank_base, int nranks_here, int nblk, size_t count, unsigned epoch, unsigned* err, int one_shot, unsigned spin_limit, unsigned entry_spin_limit, void* stream);
NTM_API size_t ntm_xgmi_signal_bytes(int nblk);
NTM_API int ntm_malloc(void** p, size_t bytes, int uncached);
NTM_API int ntm_free(void* p);
NTM_API int ntm_memset_async(void* p, int v, size_t bytes, void* stream);
NTM_API int ntm_ipc_handle(void* p, void* out64);
NTM_API int ntm_ipc_open(const void* in64, void** p);
NTM_API int ntm_ipc_close(void* p);
NTM_API int ntm_ipc_handle_bytes(void);

#endif /* NTM_ABI_H */
