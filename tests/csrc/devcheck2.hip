// devcheck2.hip -- TEST SHIM: the gfx950 build of the second operation table (devcheck_ops2.hpp), one element per lane, built with the
// HIPCC / ARCH / CXXFLAGS of csrc/Makefile (tests/devcheck.py).  Entry points as in devcheck.hip: device pointers, the null stream,
// a synchronisation, the HIP error code returned.  Lanes beyond the last element clamp their index and do not store.  The wider
// wrappers (the affine group: 353 words in) keep their operands in scratch; the product's flags and launch bounds are unchanged.
// Not part of the product; not a fallback.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include "devcheck_ops2.hpp"

namespace {

int finish() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}

#define X(name, fn, IW, OW)                                                                                                 \
  __global__ void __launch_bounds__(256) k_dc_##name(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) { \
    const uint32_t gt = blockIdx.x * 256u + threadIdx.x, i = min(gt, n - 1u);                                               \
    uint32_t a[IW], r[OW];                                                                                                  \
    _Pragma("unroll") for (int j = 0; j < IW; j++) a[j] = in[(size_t)i * IW + j];                                           \
    fn(a, r);                                                                                                               \
    if (gt < n) { _Pragma("unroll") for (int j = 0; j < OW; j++) out[(size_t)i * OW + j] = r[j]; }                          \
  }
DC_OPS2(X)
#undef X

}  // namespace

extern "C" {

#define X(name, fn, IW, OW)                                                                             \
  int dc_##name(const uint32_t* in, uint32_t* out, uint32_t n) {                                        \
    if (n == 0) return 0;                                                                               \
    hipLaunchKernelGGL(k_dc_##name, dim3((n + 255u) / 256u), dim3(256), 0, 0, in, out, n);              \
    return finish();                                                                                    \
  }
DC_OPS2(X)
#undef X
#define X(name, fn, IW, OW) #name ":" #IW ":" #OW ";"
const char* dc_table() { return DC_OPS2(X); }
#undef X

}  // extern "C"
