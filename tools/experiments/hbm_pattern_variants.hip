// K4 kernel templates (ntm/hbm_pattern.hpp) at 1 / 2 / 4 / 8 float4 per lane, for
// tools/hbm_pattern_rates.py only: the shipping C ABI instantiates just
// kWriteUnroll and kVerifyUnroll. Built by that tool into validation/build/;
// never linked into a shipping artifact. Pattern: plain, seed 1, base 0.
#include "ntm/hbm_pattern.hpp"
using namespace ntm::hbm;
static unsigned grid_for(size_t n4, int U) {
  size_t tiles = n4 / (256 * (size_t)U);
  return (unsigned)(tiles < 1 ? 1 : (tiles > 0x7fffffffu ? 0x7fffffffu : tiles));
}
template <int PAT, int U>
static void w(void* p, size_t n4, hipStream_t s) {
  hipLaunchKernelGGL((hbm_pattern_write_kernel<PAT, U>), dim3(grid_for(n4, U)), dim3(256), 0, s, (u32x4*)p, n4, (uint64_t)0, (uint64_t)1, 0u);
}
template <int PAT, int U, bool INV>
static void v(void* p, size_t n4, void* r, hipStream_t s) {
  hipLaunchKernelGGL((hbm_pattern_verify_kernel<PAT, U, INV>), dim3(grid_for(n4, U)), dim3(256), 0, s, (u32x4*)p, n4, (uint64_t)0, (uint64_t)1, 0u, (PatternResult*)r);
}
#define DISPATCH_U(F, ...) switch (U) { case 1: F<1>(__VA_ARGS__); break; case 2: F<2>(__VA_ARGS__); break; case 4: F<4>(__VA_ARGS__); break; case 8: F<8>(__VA_ARGS__); break; default: return 1; }
template <int U> static void w_any(int pat, void* p, size_t n4, hipStream_t s) { if (pat) w<1, U>(p, n4, s); else w<0, U>(p, n4, s); }
template <int U> static void v_any(int pat, int inv, void* p, size_t n4, void* r, hipStream_t s) {
  if (pat) { if (inv) v<1, U, true>(p, n4, r, s); else v<1, U, false>(p, n4, r, s); }
  else { if (inv) v<0, U, true>(p, n4, r, s); else v<0, U, false>(p, n4, r, s); }
}
extern "C" __attribute__((visibility("default"))) int k4v_write(int U, void* p, size_t bytes, int pat, void* s) {
  DISPATCH_U(w_any, pat, p, bytes / 16, (hipStream_t)s);
  return (int)hipGetLastError();
}
// the pattern written here is plain (inv = 0), seed 1; after an inverting verify the buffer holds ~pattern,
// so the caller rewrites before the next verify
extern "C" __attribute__((visibility("default"))) int k4v_verify(int U, void* p, size_t bytes, int pat, int inv_after, void* r, void* s) {
  DISPATCH_U(v_any, pat, inv_after, p, bytes / 16, r, (hipStream_t)s);
  return (int)hipGetLastError();
}
