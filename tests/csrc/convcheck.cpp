// convcheck.cpp -- TEST SHIM: the record conversion of the Twisted-Edwards curve (csrc/curve.hpp pnt_from_affine_raw) and its
// small-constant product by d (csrc/fp.hpp fp_mul_d), compiled for the host so tests/test_record_conversion_host.py can check the
// exact limb code k_prep_points / k_part_scatter_prep run on gfx950 against bigints.  Not part of the product; not a fallback.
#include <stdint.h>
#include <string.h>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/curve.hpp"

using namespace te;

extern "C" {

void cc_mul_d(const uint32_t a[9], uint32_t out[9]) { fp x; memcpy(x.v, a, 36); const fp r = fp_mul_d(x); memcpy(out, r.v, 36); }
uint32_t cc_kd_q() { return KD_Q; }
uint32_t cc_kd_small() { return KD_SMALL; }
// x, y: 32 little-endian bytes each (any 256-bit value); out: hm | hp | dt, 27 limbs
void cc_from_affine(const uint8_t xy_le[64], uint32_t out[27]) {
  uint32_t xw[8], yw[8];
  memcpy(xw, xy_le, 32); memcpy(yw, xy_le + 32, 32);
  const pnt r = pnt_from_affine_raw(fp_from_words32(xw), fp_from_words32(yw));
  memcpy(out, &r, 108);
}

}  // extern "C"
