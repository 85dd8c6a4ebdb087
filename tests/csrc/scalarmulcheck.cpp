// scalarmulcheck.cpp -- TEST SHIM: compiles the product's batch scalar multiplication (csrc/scalar_mul.hip.hpp) for the host, so that
// the exact per-lane code of k_scalar_mul and k_scalar_mul_affine is compared with the bigint models on the CPU box
// (tests/test_scalar_mul_host.py).  Not part of the product; not a fallback.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/scalar_mul.hip.hpp"

using namespace te;

namespace {
// n points and scalars -> n affine results, as the two kernels do it: one lane per point, then groups of SM_AFF_GROUP
template <int CURVE> void run(const uint8_t* pts, const uint8_t* ks, uint64_t n, int shared, uint8_t* out) {
  using Z = sm_sizes<CURVE>;
  constexpr int SB = CURVE == 1 ? 48 : 32;
  std::vector<uint32_t> proj((size_t)n * Z::JW), res((size_t)n * Z::PW);
  naf_t kn = {};
  if (shared) {
    uint32_t k[8];
    memcpy(k, ks, 32);
    kn = sm_shared_naf(k, CURVE);
  }
  for (uint64_t i = 0; i < n; i++) {
    uint32_t w[Z::PW], k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    memcpy(w, pts + i * Z::PW * 4, Z::PW * 4);
    if (shared) sm_point<CURVE, true>(w, k, kn, &proj[i * Z::JW]);
    else { memcpy(k, ks + i * SB, 32); sm_point<CURVE, false>(w, k, kn, &proj[i * Z::JW]); }
  }
  for (uint64_t lo = 0; lo < n; lo += SM_AFF_GROUP)
    sm_affine_group<CURVE>(&proj[lo * Z::JW], (uint32_t)std::min<uint64_t>(SM_AFF_GROUP, n - lo), &res[lo * Z::PW], CURVE == 1 ? kInvExp377 : kInvExpTe);
  memcpy(out, res.data(), (size_t)n * Z::PW * 4);
}
}  // namespace

extern "C" {

// curve 0: 64-byte points, 32-byte scalars; curve 1: 96-byte points, 48-byte scalar records.  shared: ks holds one scalar.
void sm_mul(int curve, const uint8_t* pts, const uint8_t* ks, uint64_t n, int shared, uint8_t* out) {
  if (curve == 1) run<1>(pts, ks, n, shared, out);
  else run<0>(pts, ks, n, shared, out);
}
// the NAF of the shared scalar: pos / neg words (8 each) and top
int sm_naf(int curve, const uint8_t* k32, uint32_t* pos, uint32_t* neg) {
  uint32_t k[8];
  memcpy(k, k32, 32);
  const naf_t r = sm_shared_naf(k, curve);
  memcpy(pos, r.pos, 32); memcpy(neg, r.neg, 32);
  return r.top;
}
// te_msm_mul_x's two steps on the Twisted-Edwards curve: recovery (from_x_te), then the per-point multiply; returns the reason code
int sm_mul_x_te(const uint8_t* x32, const uint8_t* k32, uint8_t* out64) {
  uint32_t xw[8], p[16];
  memcpy(xw, x32, 32);
  const int r = from_x_te(xw, p, kRootExpTe, kNafTeOrder);
  uint8_t pb[64];
  memcpy(pb, p, 64);
  run<0>(pb, k32, 1, 0, out64);
  return r;
}

}
