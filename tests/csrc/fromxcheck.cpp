// fromxcheck.cpp -- TEST SHIM: compiles the product's x-only point recovery (csrc/from_x.hip.hpp) for the host, so that the exact
// code that k_points_from_x runs on gfx950 is compared with the bigint models on the CPU box (tests/test_points_from_x_host.py).
// Not part of the product; not a fallback.
#include <stdint.h>
#include <string.h>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/from_x.hip.hpp"

using namespace te;

extern "C" {

// x: 32 bytes -> out: 64 bytes (x || y), returns the reason code (0 = recovered)
int fx_from_x_te(const uint8_t* x32, uint8_t* out64) {
  uint32_t xw[8], o[16];
  memcpy(xw, x32, 32);
  const int r = from_x_te(xw, o, kRootExpTe, kNafTeOrder);
  memcpy(out64, o, 64);
  return r;
}
// x with flags: 48 bytes -> out: 96 bytes
int fx_from_x_377(const uint8_t* x48, uint8_t* out96) {
  uint32_t xw[12], o[24];
  memcpy(xw, x48, 48);
  const int r = from_x_377(xw, o, kRootExp377);
  memcpy(out96, o, 96);
  return r;
}
// the square roots alone, canonical little-endian in and out: returns 1 when u / v (u) is a non-zero square, root in y
int fx_sqrt_ratio_te(const uint8_t* u32, const uint8_t* v32, uint8_t* y32) {
  uint32_t uw[8], vw[8], yw[8];
  memcpy(uw, u32, 32); memcpy(vw, v32, 32);
  fp y;
  const bool qr = fe_sqrt_ratio<9, true>(fe_from_canon(uw), fe_from_canon(vw), kRootExpTe, y);
  fe_to_canon<9, 8>(y, yw);
  memcpy(y32, yw, 32);
  return qr ? 1 : 0;
}
int fx_sqrt_377(const uint8_t* u48, uint8_t* y48) {
  uint32_t uw[12], yw[12];
  memcpy(uw, u48, 48);
  te377::fq y;
  const te377::fq u = fe_from_canon(uw);
  const bool qr = fe_sqrt_ratio<14, false>(u, u, kRootExp377, y);
  fe_to_canon<14, 12>(y, yw);
  memcpy(y48, yw, 48);
  return qr ? 1 : 0;
}

}
