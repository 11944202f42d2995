// amdgpu-validate: one GPU's thread. K1 (bf16 GEMM, the ABFT build, the stream-K
// split-mode self-check, K1-fp8) and K2 (HBM stream copy / read) live here; each
// opt-in check (K4-K8) is one line at the end of run_gpu and a source file of its own.
#include <cmath>
#include <cstring>

#include "check.hpp"

namespace ntm::job {
namespace {

// The split-mode self-check shape: 48 x 5 of 192x256 tiles, half a round on
// 256 CUs, so each tile is cut into K slices combined through the workspace (the
// ragged shape round 5 moved from 0.82-0.89 to 1.03 of hipBLASLt).
constexpr int kSkM = 4152, kSkN = 1096, kSkK = 16056;

bool run_sk_check(const GpuCtx& g, void* V, SkResult& r) {
  const int dev = g.dev;
  hipStream_t s = g.s;
  int top = 0, tv = 0, rest = 0, sp = 0;
  int variant = 0;
  if (ntm_k1_plan_splitk(kSkM, kSkN, kSkK, &top, &tv, &rest, &sp) == 0 &&
      (tv == 54 || tv == 55) && ntm_skh_ws_bytes(tv, kSkM, kSkN, kSkK) > 0)
    variant = tv;  // what the default dispatch runs for this shape
  for (int v : {54, 55})
    if (!variant && ntm_skh_ws_bytes(v, kSkM, kSkN, kSkK) > 0) variant = v;
  if (!variant) return true;  // a partition with other CU counts: not served, not run
  r.variant = variant;
  const size_t ea = (size_t)kSkM * kSkK, eb = (size_t)kSkN * kSkK, ec = (size_t)kSkM * kSkN;
  const size_t wsb = ntm_skh_ws_bytes(variant, kSkM, kSkN, kSkK);
  void *A, *B, *C, *W;
  float* R;
  CK(hipMalloc(&A, ea * 2));
  CK(hipMalloc(&B, eb * 2));
  CK(hipMalloc(&C, ec * 2));
  CK(hipMalloc(&R, ec * 4));
  CK(hipMalloc(&W, wsb));
  CK(hipMemsetAsync(W, 0, wsb, s));  // counters zero on entry (each launch leaves them zero)
  CK(ntm_fill_uniform_bf16(A, ea, 5000 + 2 * dev, 1.0f, s));
  CK(ntm_fill_uniform_bf16(B, eb, 5001 + 2 * dev, 1.0f, s));
  const int fault = g.fault("sk_xcc") ? 1 : 0;
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipEventRecord(e0, s));
  CK(ntm_gemm_bf16_skh_ex(variant, A, B, C, kSkM, kSkN, kSkK, kSkK, kSkK, kSkN, W, wsb, fault, s));
  CK(hipEventRecord(e1, s));
  CK(ntm_ref_gemm_f32(A, B, R, kSkM, kSkN, kSkK, kSkK, kSkK, kSkN, s));
  CK(hipMemsetAsync(V, 0, 64, s));
  const float atol = 1e-3f + 4.0f * std::sqrt((float)kSkK) * std::ldexp(1.0f, -20);
  CK(ntm_verify_bf16(C, R, ec, atol, std::ldexp(1.0f, -7), V, s));
  unsigned char vr[64];
  CK(hipMemcpyAsync(vr, V, ntm_verify_result_bytes(), hipMemcpyDeviceToHost, s));
  CK(hipMemcpyAsync(&r.word, (unsigned*)W + ntm_sk_error_word_index(), 4, hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  std::memcpy(&r.bad, vr, 8);
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  r.ms = ms;
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  CK(hipFree(A));
  CK(hipFree(B));
  CK(hipFree(C));
  CK(hipFree(R));
  CK(hipFree(W));
  return true;
}

double gemm_tflops(int n, double ms_per_call) { return 2.0 * n * (double)n * n / (ms_per_call * 1e-3) / 1e12; }

}  // namespace

bool run_gpu(int dev, bool last, const Opts& o, GpuResult& r) {
  r.device = dev;
  CK(hipSetDevice(dev));
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, dev));
  r.name = prop.name;
  r.arch = prop.gcnArchName;
  if (r.arch.find("gfx950") == std::string::npos) {
    fail("device " + std::to_string(dev) + " is " + r.arch + ", not gfx950 (MI355X)");
    return false;
  }
  size_t fre = 0, tot = 0;
  CK(hipMemGetInfo(&fre, &tot));
  r.total_gb = tot / 1e9;
  r.free_gb = fre / 1e9;
  hipStream_t s;
  CK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  const GpuCtx g{dev, last, o, s};
  r.t_init = wall_now();

  // ---- K1
  const int n = o.size;
  if (!ntm_gemm_shape_ok(n, n, n)) {
    fail("--size must be a multiple of 256 (>= 256)");
    return false;
  }
  const size_t e = (size_t)n * n;
  void *A, *B, *C, *V;
  float* R;
  CK(hipMalloc(&A, e * 2));
  CK(hipMalloc(&B, e * 2));
  CK(hipMalloc(&C, e * 2));
  CK(hipMalloc(&R, e * 4));
  CK(hipMalloc(&V, 64));
  CK(ntm_fill_uniform_bf16(A, e, 1000 + 2 * dev, 1.0f, s));
  CK(ntm_fill_uniform_bf16(B, e, 1001 + 2 * dev, 1.0f, s));
  auto gemm = [&] { return ntm_gemm_bf16(A, B, C, n, n, n, n, n, n, s); };
  CK(gemm());  // warm-up + verified result
  // corrupt_gemm: flip one output element's exponent
  if (g.fault("corrupt_gemm") && !flip_bits((uint16_t*)C + 4321, 2, 0x0100, &s)) return false;
  CK(ntm_ref_gemm_f32(A, B, R, n, n, n, n, n, n, s));
  CK(hipMemsetAsync(V, 0, 64, s));
  const float atol = 1e-3f + 4.0f * std::sqrt((float)n) * std::ldexp(1.0f, -20);
  CK(ntm_verify_bf16(C, R, e, atol, std::ldexp(1.0f, -7), V, s));
  unsigned char vr[64];
  CK(hipMemcpyAsync(vr, V, ntm_verify_result_bytes(), hipMemcpyDeviceToHost, s));
  CK(hipStreamSynchronize(s));
  std::memcpy(&r.k1.bad, vr, 8);
  std::memcpy(&r.k1.max_err, vr + 8, 4);
  CK(hipFree(R));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float ms = 0;
  if (!settle(s, o.settle_s, gemm) || !timed_ms(s, e0, e1, o.iters, ms, gemm)) return false;
  r.k1.ms = ms / o.iters;
  r.k1.tflops = gemm_tflops(n, r.k1.ms);

  // ---- K1 + fused ABFT row checksum, checked in O(n^2) (every launch of a
  // long-running health check can afford this; the fp32 reference cannot)
  {
    float* rowsum;
    double* scratch;
    void* ab;
    CK(hipMalloc(&rowsum, sizeof(float) * n));
    CK(hipMalloc(&scratch, sizeof(double) * n));
    CK(hipMalloc(&ab, 64));
    const int it = std::max(1, o.iters / 5);
    if (!timed_ms(s, e0, e1, it, ms, [&] {
          const hipError_t z = hipMemsetAsync(rowsum, 0, sizeof(float) * n, s);
          return z != hipSuccess ? (int)z : ntm_gemm_bf16_rowsum(A, B, C, rowsum, n, n, n, n, n, n, s);
        }))
      return false;
    r.k1.abft_tflops = gemm_tflops(n, ms / it);
    if (g.fault("corrupt_abft")) {
      const float bump = 64.0f;
      float v;
      CK(hipMemcpyAsync(&v, rowsum + 7, 4, hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      v += bump;
      CK(hipMemcpyAsync(rowsum + 7, &v, 4, hipMemcpyHostToDevice, s));
    }
    CK(ntm_abft_check(A, B, C, rowsum, n, n, n, n, n, n, scratch, ab, s));
    unsigned char abr[64];
    CK(hipMemcpyAsync(abr, ab, ntm_abft_result_bytes(), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    std::memcpy(&r.k1.abft_bad_acc, abr, 8);
    std::memcpy(&r.k1.abft_bad_store, abr + 8, 8);
    std::memcpy(&r.k1.abft_max_rel_acc, abr + 16, 4);
    CK(hipFree(rowsum));
    CK(hipFree(scratch));
    CK(hipFree(ab));
  }
  CK(hipFree(A));
  CK(hipFree(B));

  // ---- stream-K split mode on a 192-wide tile: the one K1 path
  // whose correctness rests on a placement invariant (every part of a split tile
  // on one XCD, gemm_bf16_sk.hpp) - checked against the fp32 reference, and the
  // kernel's own placement error word must stay zero. fault "sk_xcc" makes the
  // last GPU's launch claim a wrong XCC and must fail the Job.
  if (!run_sk_check(g, V, r.sk)) return false;

  // ---- K1-fp8: the same schedule on e4m3 operands (MX-scaled MFMA, unit
  // scales), checked element-wise against the fp32 reference of the e4m3 values
  if (o.fp8 && ntm_gemm_fp8_shape_ok(n, n, n)) {
    void *A8, *B8;
    CK(hipMalloc(&A8, e));
    CK(hipMalloc(&B8, e));
    CK(hipMalloc(&R, e * 4));
    CK(ntm_fill_uniform_e4m3(A8, e, 3000 + 2 * dev, 1.0f, s));
    CK(ntm_fill_uniform_e4m3(B8, e, 3001 + 2 * dev, 1.0f, s));
    auto gemm8 = [&] { return ntm_gemm_fp8(A8, B8, C, n, n, n, n, n, n, s); };
    CK(gemm8());
    if (g.fault("corrupt_fp8") && !flip_bits((uint16_t*)C + 777, 2, 0x0100, &s)) return false;
    CK(ntm_ref_gemm_f32_e4m3(A8, B8, R, n, n, n, n, n, n, s));
    CK(hipMemsetAsync(V, 0, 64, s));
    CK(ntm_verify_bf16(C, R, e, atol, std::ldexp(1.0f, -7), V, s));
    CK(hipMemcpyAsync(vr, V, ntm_verify_result_bytes(), hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    std::memcpy(&r.fp8.bad, vr, 8);
    std::memcpy(&r.fp8.max_err, vr + 8, 4);
    CK(hipFree(R));
    if (!settle(s, o.settle_s, gemm8) || !timed_ms(s, e0, e1, o.iters, ms, gemm8)) return false;
    r.fp8.ms = ms / o.iters;
    r.fp8.tflops = gemm_tflops(n, r.fp8.ms);
    if (n % 256 == 0) {
      // the fp8 build with the fused ABFT row checksum, checked in O(n^2)
      float* rowsum;
      double* scratch;
      void* ab;
      CK(hipMalloc(&rowsum, sizeof(float) * n));
      CK(hipMalloc(&scratch, sizeof(double) * n));
      CK(hipMalloc(&ab, 64));
      CK(hipMemsetAsync(rowsum, 0, sizeof(float) * n, s));
      CK(ntm_gemm_fp8_rowsum(A8, B8, C, rowsum, n, n, n, n, n, n, s));
      // corrupt_fp8_abft: an exponent bit, a large stored-output error
      if (g.fault("corrupt_fp8_abft") && !flip_bits((uint16_t*)C + 4242, 2, 0x4000, &s)) return false;
      CK(ntm_abft_check_fp8(A8, B8, C, rowsum, n, n, n, n, n, n, scratch, ab, s));
      unsigned char abr[64];
      CK(hipMemcpyAsync(abr, ab, ntm_abft_result_bytes(), hipMemcpyDeviceToHost, s));
      CK(hipStreamSynchronize(s));
      unsigned long long bad_acc, bad_store;
      std::memcpy(&bad_acc, abr, 8);
      std::memcpy(&bad_store, abr + 8, 8);
      r.fp8.abft_bad = bad_acc + bad_store;
      CK(hipFree(rowsum));
      CK(hipFree(scratch));
      CK(hipFree(ab));
    }
    CK(hipFree(A8));
    CK(hipFree(B8));
  }
  CK(hipFree(C));
  CK(hipFree(V));
  r.t_gemm = wall_now();

  // ---- K2: 2 GiB float4 copy
  const size_t hb = std::min<size_t>((size_t)2 << 30, fre / 4) / 16 * 16;
  void *src, *dst;
  CK(hipMalloc(&src, hb));
  CK(hipMalloc(&dst, hb));
  CK(ntm_fill_uniform_bf16(src, hb / 2, 77 + dev, 1.0f, s));
  auto copy = [&] { return ntm_stream_copy(src, dst, hb, s); };
  CK(copy());
  if (!timed_ms(s, e0, e1, 10, ms, copy)) return false;
  r.k2.copy_gbps = 2.0 * hb * 10 / (ms * 1e-3) / 1e9;
  {
    float* sink;
    CK(hipMalloc(&sink, sizeof(float) * 8192));
    auto read = [&] { return ntm_stream_read(src, hb, sink, s); };
    CK(read());
    if (!timed_ms(s, e0, e1, 10, ms, read)) return false;
    r.k2.read_gbps = (double)hb * 10 / (ms * 1e-3) / 1e9;
    CK(hipFree(sink));
  }
  {  // byte-exact copy check on a sample window (first + last 16 MiB)
    const size_t w = std::min<size_t>(hb, 16u << 20);
    std::vector<unsigned char> h0(w), h1(w);
    bool ok = true;
    for (size_t off : {(size_t)0, hb - w}) {
      CK(hipMemcpy(h0.data(), (char*)src + off, w, hipMemcpyDeviceToHost));
      CK(hipMemcpy(h1.data(), (char*)dst + off, w, hipMemcpyDeviceToHost));
      ok = ok && std::memcmp(h0.data(), h1.data(), w) == 0;
    }
    r.k2.copy_ok = ok;
  }
  CK(hipFree(src));
  CK(hipFree(dst));

  // ---- the opt-in checks: one line each
  if (o.hbm_test_gb != 0 && !run_hbm_test(g, r.hbm_test)) return false;
  if (o.cu_sweep && !run_cu_sweep(g, r.cu_sweep)) return false;
  if (o.host_link_mib > 0 && !run_host_link(g, r.host_link)) return false;
  if (o.mx_check && !run_mx_check(g, r.mx)) return false;
  if (o.xcd_sweep && !run_xcd_sweep(g, r.xcd)) return false;
  if (o.atomics_check && !run_atomics(g, r.atomics)) return false;
  if (o.mcore_check && !run_mcore(g, r.mcore)) return false;
  if (o.mxq_check && !run_mxq(g, r.mxq)) return false;
  if (o.wave_check && !run_wave(g, r.wave)) return false;
  if (o.attn_check && !run_attn(g, r.attn)) return false;
  if (o.pda_check && !run_pda(g, r.pda)) return false;
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  CK(hipStreamDestroy(s));
  r.t_hbm = wall_now();  // after the opt-in checks: phases_s.hbm_done includes them
  return true;
}

}  // namespace ntm::job
