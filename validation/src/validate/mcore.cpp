// amdgpu-validate K10: fp64 / fp32 / fp16 / int8 / 2:4-sparse matrix-core check (ntm/mcore.hpp,
// host side in ntm/mcore_plan.hpp). On for NTM_MCORE_CHECK=1. Every answer is exact and every
// compare bitwise, against mcore_ref_kernel (no matrix instruction):
//   1. per format, the decode sweep, 256 x 128 x 128, one non-zero per row of A, all windows;
//   2. per format, dense 512^3 with the widest operands the bound allows at K = 512;
//   3. dense 4096^3 for f64 and i8 with mcore_max_abits at K = 4096, verified, then timed: the
//      settle of the other GEMM stages, then o.iters launches. Rates are reported, never judged.
// corrupt_mcore: bit 9 of one element of the LAST GPU's dense 512^3 f64 result is flipped
// before the compare.
#include "check.hpp"
#include "ntm/mcore_plan.hpp"

namespace ntm::job {

bool run_mcore(const GpuCtx& g, McoreResult& r) {
  namespace mc = ntm::mc;
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  const auto t_begin = Clock::now();
  r.ran = true;
  constexpr int kBig = 4096, kDense = 512;
  const size_t big = (size_t)kBig * kBig * 8;
  unsigned char *dA = nullptr, *dAI = nullptr, *dB = nullptr, *dC = nullptr, *dE = nullptr;
  mc::Mismatch init, got;
  mc::mismatch_init(init);
  mc::Mismatch* dres = nullptr;
  CK(hipMalloc(&dA, big));
  CK(hipMalloc(&dB, big));
  CK(hipMalloc(&dC, big));
  CK(hipMalloc(&dE, big));
  CK(hipMalloc(&dAI, (size_t)kBig * kBig / 4));
  CK(hipMalloc(&dres, sizeof init));

  // One product: upload, run the GEMM and the reference kernel, compare on the device.
  auto product = [&](const mc::Inputs& in, const char* mode, bool inject) -> bool {
    const size_t nc = (size_t)in.M * in.N, wb = (size_t)mc::kFormatTable[in.fmt].acc_bytes;
    CK(hipMemcpyAsync(dA, in.a.data(), in.a.size(), hipMemcpyHostToDevice, s));
    if (!in.ai.empty()) CK(hipMemcpyAsync(dAI, in.ai.data(), in.ai.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dB, in.b.data(), in.b.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(dC, 0xFF, nc * wb, s));
    CK(ntm_mcore_gemm(in.fmt, dA, dAI, dB, dC, in.M, in.N, in.K, s));
    CK(ntm_mcore_reference(in.fmt, dA, dAI, dB, dE, in.M, in.N, in.K, s));
    if (inject && !flip_bits(dC + (nc / 2 + 5) * wb, 4, 1u << 9, &s)) return false;
    CK(ntm_mcore_compare(dE, dC, nc, (int)wb, dres, s));
    CK(hipMemcpyAsync(&got, dres, sizeof got, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (got.count) {
      r.bad[in.fmt] += got.count;
      // one line per format and mode: the first failing product names the element
      const std::string head = "gpu" + std::to_string(dev) + ": mcore: " + mc::format_name(in.fmt) + " " + mode + ":";
      bool seen = false;
      for (auto& f : r.failures) seen = seen || f.compare(0, head.size(), head) == 0;
      if (!seen) r.failures.push_back(mc::failure_message(dev, in.fmt, mode, got, in.N));
    }
    return true;
  };

  const unsigned long long seed = 0x4B3Aull + (unsigned)dev;
  for (int fmt = 0; fmt < mc::kFormats; ++fmt) {
    for (int w = 0; w < mc::decode_windows(fmt); ++w)
      if (!product(mc::make_decode(fmt, mc::kDecodeRows, 128, 128, w), "decode", false)) return false;
    if (!product(mc::make_dense(fmt, kDense, kDense, kDense, seed, mc::mcore_max_abits(fmt, kDense)), "dense",
                 fmt == mc::kF64 && g.fault("corrupt_mcore")))
      return false;
  }

  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int fmt : {mc::kF64, mc::kI8}) {
    if (!product(mc::make_dense(fmt, kBig, kBig, kBig, seed, mc::mcore_max_abits(fmt, kBig)), "dense", false))
      return false;
    auto gemm = [&] { return ntm_mcore_gemm(fmt, dA, dAI, dB, dC, kBig, kBig, kBig, s); };
    float ms = 0;
    if (!settle(s, o.settle_s, gemm) || !timed_ms(s, e0, e1, o.iters, ms, gemm)) return false;
    const double rate = ms > 0 ? 2.0 * kBig * (double)kBig * kBig / (ms / o.iters * 1e-3) / 1e12 : 0;
    (fmt == mc::kF64 ? r.f64_tflops : r.i8_tops) = rate;
  }
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  for (void* p : {(void*)dA, (void*)dAI, (void*)dB, (void*)dC, (void*)dE, (void*)dres}) CK(hipFree(p));
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
