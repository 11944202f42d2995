// amdgpu-validate K7: MX block-scaled matrix check (ntm/mx_gemm.hpp, host side in ntm/mx_plan.hpp).
// Every answer is exact and every compare bitwise:
//   1. the decode sweep of all five formats, 256 x 128 x 128, one non-zero per row of A,
//      all 15 windows of A scale bytes 0 .. 254, against the host's integer table;
//   2. dense e2m3, mx-size x mx-size x 512, and
//   3. dense e2m1, mx-size^3, both with non-unit scales of the largest spread W <= 3
//      the bound allows, against mx_ref_kernel (no matrix core);
//   4. the e2m1 product timed: the settle of the other GEMM stages, then o.iters launches.
// corrupt_mx: one bit of one element of the dense e2m1 result is flipped before the compare.
#include "check.hpp"
#include "ntm/mx_plan.hpp"

namespace ntm::job {

bool run_mx_check(const GpuCtx& g, MxResult& r) {
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  namespace mx = ntm::mx;
  const auto t_begin = Clock::now();
  r.ran = true;
  const int S = o.mx_size;
  mx::Mismatch init, got;
  mx::mismatch_init(init);
  mx::Mismatch* dres = nullptr;
  CK(hipMalloc(&dres, sizeof init));
  bool fmt_clean[mx::kFormats] = {true, true, true, true, true};
  unsigned char *dA = nullptr, *dB = nullptr, *dSA = nullptr, *dSB = nullptr;
  float *dC = nullptr, *dE = nullptr;
  // One product: upload, run the GEMM, get the expected bits (host table or reference
  // kernel), compare on the device. The buffers stay allocated for the timed loop.
  auto product = [&](const mx::Inputs& in, const char* mode, bool host_table, bool inject) -> bool {
    const size_t nc = (size_t)in.M * in.N;
    CK(hipMalloc(&dA, in.a.size()));
    CK(hipMalloc(&dB, in.b.size()));
    CK(hipMalloc(&dSA, in.sa.size()));
    CK(hipMalloc(&dSB, in.sb.size()));
    CK(hipMalloc(&dC, nc * 4));
    CK(hipMalloc(&dE, nc * 4));
    CK(hipMemcpyAsync(dA, in.a.data(), in.a.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dB, in.b.data(), in.b.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dSA, in.sa.data(), in.sa.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dSB, in.sb.data(), in.sb.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s));
    CK(hipMemsetAsync(dC, 0xFF, nc * 4, s));
    CK(ntm_mx_gemm(in.fmt, dA, dB, dSA, dSB, dC, in.M, in.N, in.K, s));
    std::vector<uint32_t> bits;
    if (host_table) {
      if (!mx::host_reference(in, bits)) {
        fail("mx host reference: scale spread too wide");
        return false;
      }
      CK(hipMemcpyAsync(dE, bits.data(), nc * 4, hipMemcpyHostToDevice, s));
    } else {
      CK(ntm_mx_reference(in.fmt, dA, dB, dSA, dSB, dE, in.M, in.N, in.K, s));
    }
    if (inject && !flip_bits(dC + (nc / 2 + 5), 4, 1u << 3, &s)) return false;
    CK(ntm_mx_compare(dE, dC, nc, dres, s));
    CK(hipMemcpyAsync(&got, dres, sizeof got, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (got.count) {
      r.bad_elements += got.count;
      fmt_clean[in.fmt] = false;
      // one line per format and mode: the first failing product names the element
      const std::string head = "gpu" + std::to_string(dev) + ": mx " + mx::format_name(in.fmt) + " " + mode + ":";
      bool seen = false;
      for (auto& f : r.failures) seen = seen || f.compare(0, head.size(), head) == 0;
      if (!seen) r.failures.push_back(mx::failure_message(dev, in.fmt, mode, got, in.N));
    }
    return true;
  };
  auto release = [&]() -> bool {
    CK(hipFree(dA));
    CK(hipFree(dB));
    CK(hipFree(dSA));
    CK(hipFree(dSB));
    CK(hipFree(dC));
    CK(hipFree(dE));
    dA = dB = dSA = dSB = nullptr;
    dC = dE = nullptr;
    return true;
  };
  for (int fmt = 0; fmt < mx::kFormats; ++fmt)
    for (int w = 0; w < mx::kDecodeWindows; ++w) {
      if (!product(mx::make_decode(fmt, 256, 128, 128, w), "decode", true, false)) return false;
      if (!release()) return false;
    }
  const unsigned long long seed = 0x4B37ull + (unsigned)dev;
  const int w6 = mx::dense_max_spread(mx::kFmtE2M3, 512);
  if (w6 >= 0) {
    if (!product(mx::make_dense(mx::kFmtE2M3, S, S, 512, seed, w6), "dense", false, false)) return false;
    if (!release()) return false;
  }
  const int w4 = mx::dense_max_spread(mx::kFmtE2M1, S);
  if (w4 < 0) {
    r.failures.push_back("gpu" + std::to_string(dev) + ": mx e2m1 dense: no exact scale spread at size " +
                         std::to_string(S));
    fmt_clean[mx::kFmtE2M1] = false;
  } else {
    r.scale_spread = w4;
    if (!product(mx::make_dense(mx::kFmtE2M1, S, S, S, seed, w4), "dense", false, g.fault("corrupt_mx")))
      return false;
    // timed: the buffers of the dense e2m1 product are still in place
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto gemm = [&] { return ntm_mx_gemm(mx::kFmtE2M1, dA, dB, dSA, dSB, dC, S, S, S, s); };
    float ms = 0;
    if (!settle(s, o.settle_s, gemm) || !timed_ms(s, e0, e1, o.iters, ms, gemm)) return false;
    r.fp4_tflops = 2.0 * S * (double)S * S / (ms / o.iters * 1e-3) / 1e12;
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    if (!release()) return false;
    if (o.mx_tflops_floor > 0 && r.fp4_tflops < o.mx_tflops_floor)
      r.failures.push_back("gpu" + std::to_string(dev) + ": mx e2m1 GEMM " + jnum(r.fp4_tflops) +
                           " TFLOP/s below floor " + jnum(o.mx_tflops_floor));
  }
  CK(hipFree(dres));
  for (int fmt = 0; fmt < mx::kFormats; ++fmt)
    if (fmt_clean[fmt]) r.formats.push_back(mx::format_name(fmt));
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
