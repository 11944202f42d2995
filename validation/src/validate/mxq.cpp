// amdgpu-validate K11: MX quantise / dequantise on the device (ntm/mxq.hpp, host side in
// ntm/mxq_plan.hpp). On for NTM_MXQ_CHECK=1. Every compare is bitwise through ntm_mx_compare,
// on buffers of whole zero-filled 4-byte words:
//   1. per format, the conversion sweeps against the reference kernels (integer arithmetic, no
//      conversion instruction): down from fp32 and from every finite normal bf16 code with
//      given scale bytes (ntm_mxq_cvt), up for every finite code at every scale byte 1 .. 254;
//   2. per format, a block quantise of a 1024 x 4096 fp32 and bf16 matrix: packed bytes
//      ("block") and scale bytes ("scale");
//   3. end to end for e2m1, e2m3 and e4m3 at 512^3: both operands quantised on the device from
//      the grid inputs, then ntm_mx_gemm, against ntm_mx_reference on the host-packed operands
//      (e4m3, for which no product is exact by the bound: against ntm_mx_gemm on them);
//   4. the fp32 -> e2m1 quantise of 8192 x 8192 timed, GB/s of bytes read + written, reported
//      beside K2's copy rate of the same run and never judged.
// corrupt_mxq: bit 4 of one packed e2m1 byte of the LAST GPU's fp32 block quantise is flipped
// before the compare.
#include "check.hpp"
#include "ntm/mxq_plan.hpp"

namespace ntm::job {

bool run_mxq(const GpuCtx& g, MxqResult& r) {
  namespace mx = ntm::mx;
  namespace q = ntm::mxq;
  const int dev = g.dev;
  const Opts& o = g.o;
  hipStream_t s = g.s;
  const auto t_begin = Clock::now();
  r.ran = true;
  constexpr int kRows = 1024, kCols = 4096, kE2e = 512, kBig = 8192;
  const size_t x_bytes = (size_t)kBig * kBig * 4, p_bytes = (size_t)kBig * kBig / 2, s_bytes = (size_t)kBig * kBig / 32;
  unsigned char *dX = nullptr, *dP = nullptr, *dPr = nullptr, *dS = nullptr, *dSr = nullptr, *dY = nullptr,
                *dYr = nullptr, *dP2 = nullptr, *dS2 = nullptr;
  mx::Mismatch init, got;
  mx::mismatch_init(init);
  mx::Mismatch* dres = nullptr;
  CK(hipMalloc(&dX, x_bytes));
  for (unsigned char** p : {&dP, &dPr, &dP2}) CK(hipMalloc(p, p_bytes));
  for (unsigned char** p : {&dS, &dSr, &dS2}) CK(hipMalloc(p, s_bytes));
  const size_t y_bytes = (size_t)kE2e * kE2e * 4 > 254 * 256 * 4 ? (size_t)kE2e * kE2e * 4 : 254 * 256 * 4;
  CK(hipMalloc(&dY, y_bytes));
  CK(hipMalloc(&dYr, y_bytes));
  CK(hipMalloc(&dres, sizeof init));

  // compare `bytes` (a multiple of 4) of two device buffers; a mismatch adds to `bad` and gives one line per
  // format and sub-test
  auto compare = [&](int fmt, const char* sub, const void* expected, const void* have, size_t bytes, size_t row_words,
                     int elem_bits, unsigned long long& bad) -> bool {
    CK(hipMemcpyAsync(dres, &init, sizeof init, hipMemcpyHostToDevice, s));
    CK(ntm_mx_compare(expected, have, bytes / 4, dres, s));
    CK(hipMemcpyAsync(&got, dres, sizeof got, hipMemcpyDeviceToHost, s));
    CK(hipStreamSynchronize(s));
    if (got.count) {
      bad += got.count;
      const std::string head = "gpu" + std::to_string(dev) + ": mxq " + mx::format_name(fmt) + " " + sub + ":";
      bool seen = false;
      for (auto& f : r.failures) seen = seen || f.compare(0, head.size(), head) == 0;
      if (!seen) r.failures.push_back(q::failure_message(dev, fmt, sub, got, row_words, elem_bits));
    }
    return true;
  };
  auto zero_out = [&](size_t packed, size_t scales) -> bool {
    for (unsigned char* p : {dP, dPr}) CK(hipMemsetAsync(p, 0, (packed + 3) & ~(size_t)3, s));
    for (unsigned char* p : {dS, dSr}) CK(hipMemsetAsync(p, 0, (scales + 3) & ~(size_t)3, s));
    return true;
  };
  // upload fp32 bit patterns as fp32, or their upper halves as bf16
  std::vector<uint16_t> half;
  auto upload = [&](const std::vector<uint32_t>& x, bool bf16) -> bool {
    if (bf16) {
      half.resize(x.size());
      for (size_t i = 0; i < x.size(); ++i) half[i] = (uint16_t)(x[i] >> 16);
      CK(hipMemcpyAsync(dX, half.data(), half.size() * 2, hipMemcpyHostToDevice, s));
    } else {
      CK(hipMemcpyAsync(dX, x.data(), x.size() * 4, hipMemcpyHostToDevice, s));
    }
    return true;
  };

  const unsigned long long seed = 0x4B3Bull + (unsigned)dev;
  for (int fmt = 0; fmt < mx::kFormats; ++fmt) {
    const int bits = mx::format_bits(fmt);
    // 1. down sweeps: rows = blocks, K = 32
    for (int bf16 = 0; bf16 < 2; ++bf16) {
      const q::Sweep sw = bf16 ? q::make_down_bf16(fmt) : q::make_down_sweep(fmt);
      const int R = sw.blocks();
      const size_t pb = (size_t)R * mx::kBlock * bits / 8;
      if (!zero_out(pb, (size_t)R) || !upload(sw.x, bf16 != 0)) return false;
      CK(hipMemcpyAsync(dS, sw.scales.data(), (size_t)R, hipMemcpyHostToDevice, s));
      CK(ntm_mxq_cvt(fmt, bf16, dX, dS, dP, R, mx::kBlock, mx::kBlock, q::kRne, 0, s));
      CK(ntm_mxq_reference_cvt(fmt, bf16, dX, dS, dPr, R, mx::kBlock, mx::kBlock, s));
      if (!compare(fmt, "down", dPr, dP, pb, (size_t)mx::kBlock * bits / 32, bits, r.bad_down[fmt])) return false;
    }
    // up sweep: row = scale byte - 1
    {
      const q::UpSweep up = q::make_up_sweep(fmt);
      CK(hipMemcpyAsync(dP, up.packed.data(), up.packed.size(), hipMemcpyHostToDevice, s));
      CK(hipMemcpyAsync(dS, up.scales.data(), up.scales.size(), hipMemcpyHostToDevice, s));
      CK(hipMemsetAsync(dY, 0, y_bytes, s));
      CK(hipMemsetAsync(dYr, 0, y_bytes, s));
      CK(ntm_mxq_dequantize(fmt, q::kF32, dP, dS, dY, up.R, up.K, up.K, s));
      CK(ntm_mxq_reference_dequantize(fmt, q::kF32, dP, dS, dYr, up.R, up.K, up.K, s));
      if (!compare(fmt, "up", dYr, dY, (size_t)up.R * up.K * 4, (size_t)up.K, 32, r.bad_up[fmt])) return false;
    }
    // 2. block quantise
    for (int bf16 = 0; bf16 < 2; ++bf16) {
      const size_t pb = (size_t)kRows * mx::row_bytes(fmt, kCols), sb = (size_t)kRows * kCols / mx::kBlock;
      if (!zero_out(pb, sb) || !upload(q::make_block_rows(fmt, kRows, kCols, kCols, seed, bf16 != 0), bf16 != 0))
        return false;
      CK(ntm_mxq_quantize(fmt, bf16, dX, dP, dS, kRows, kCols, kCols, q::kRne, 0, s));
      CK(ntm_mxq_reference_quantize(fmt, bf16, dX, dPr, dSr, kRows, kCols, kCols, s));
      if (fmt == mx::kFmtE2M1 && !bf16 && g.fault("corrupt_mxq") && !flip_bits(dP + (pb / 2 & ~(size_t)3) + 64, 4, 1u << 4, &s))
        return false;
      if (!compare(fmt, "block", dPr, dP, pb, mx::row_bytes(fmt, kCols) / 4, bits, r.bad_block[fmt]) ||
          !compare(fmt, "scale", dSr, dS, sb, (size_t)kCols / mx::kBlock / 4, 8, r.bad_block[fmt]))
        return false;
    }
  }

  // 3. end to end
  for (int fmt : {mx::kFmtE2M1, mx::kFmtE2M3, mx::kFmtE4M3}) {
    const mx::Inputs in = mx::make_dense(fmt, kE2e, kE2e, kE2e, seed, std::max(mx::dense_max_spread(fmt, kE2e), 0));
    const q::Grid ga = q::make_grid(fmt, in.a, in.sa, kE2e, kE2e, seed), gb = q::make_grid(fmt, in.b, in.sb, kE2e, kE2e, seed + 1);
    unsigned char* dXb = dX + (size_t)kE2e * kE2e * 4;
    CK(hipMemcpyAsync(dX, ga.x.data(), ga.x.size() * 4, hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dXb, gb.x.data(), gb.x.size() * 4, hipMemcpyHostToDevice, s));
    CK(ntm_mxq_quantize(fmt, q::kF32, dX, dP, dS, kE2e, kE2e, kE2e, q::kRne, 0, s));
    CK(ntm_mxq_quantize(fmt, q::kF32, dXb, dP2, dS2, kE2e, kE2e, kE2e, q::kRne, 0, s));
    CK(ntm_mx_gemm(fmt, dP, dP2, dS, dS2, dY, kE2e, kE2e, kE2e, s));
    CK(hipMemcpyAsync(dPr, ga.packed.data(), ga.packed.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dSr, ga.scales.data(), ga.scales.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dP, gb.packed.data(), gb.packed.size(), hipMemcpyHostToDevice, s));
    CK(hipMemcpyAsync(dS, gb.scales.data(), gb.scales.size(), hipMemcpyHostToDevice, s));
    // no e4m3 product is exact by mx::dense_exact (its largest product alone passes 2^24 product
    // quanta), so the reference kernel's fp32 sums round differently from the matrix core's; the
    // e4m3 answer is ntm_mx_gemm itself on the host-packed operands
    if (fmt == mx::kFmtE4M3) CK(ntm_mx_gemm(fmt, dPr, dP, dSr, dS, dYr, kE2e, kE2e, kE2e, s));
    else CK(ntm_mx_reference(fmt, dPr, dP, dSr, dS, dYr, kE2e, kE2e, kE2e, s));
    if (!compare(fmt, "e2e", dYr, dY, (size_t)kE2e * kE2e * 4, (size_t)kE2e, 32, r.bad_e2e[fmt])) return false;
  }

  // 4. the rate: every fp32 of the source is 0x3C3C3C3C (0.0115), a normal value
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  CK(hipMemsetAsync(dX, 0x3C, x_bytes, s));
  auto quantize = [&] { return ntm_mxq_quantize(mx::kFmtE2M1, q::kF32, dX, dP, dS, kBig, kBig, kBig, q::kRne, 0, s); };
  float ms = 0;
  if (!settle(s, o.settle_s, quantize) || !timed_ms(s, e0, e1, o.iters, ms, quantize)) return false;
  r.quantize_gbps = ms > 0 ? (double)(x_bytes + p_bytes + s_bytes) * o.iters / (ms * 1e-3) / 1e9 : 0;
  CK(hipEventDestroy(e0));
  CK(hipEventDestroy(e1));
  for (void* p : {(void*)dX, (void*)dP, (void*)dPr, (void*)dP2, (void*)dS, (void*)dSr, (void*)dS2, (void*)dY, (void*)dYr,
                  (void*)dres})
    CK(hipFree(p));
  r.seconds = since(t_begin);
  return true;
}

}  // namespace ntm::job
