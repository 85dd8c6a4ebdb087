// pairstart.cpp -- TEST SHIM: the two-record bucket start of k_accumulate (csrc/curve.hpp ete_from_pair) and the conversion +
// addition it replaces, compiled for the host so tests/test_bucket_start_host.py can check the exact limb code the GPU runs against
// bigints, for both curves and every record kind the kernel is instantiated with.  The 14-limb products run with every column sum
// checked against 2^64 (g_fq377_overflow).  Not part of the product; not a fallback.
#include <stdint.h>
#include <string.h>
#define TE377_CHECK_COLUMNS 1
#include "../../webgpu-msm-twisted-edwards_amd/csrc/curve.hpp"

int g_fq377_overflow = 0;

using namespace te;

extern "C" {

// ---- Twisted-Edwards BLS12, 9 limbs: record = hm | hp | dt (27 words), accumulator = x | y | z | t (36 words)
// x, y: 32 little-endian bytes each
void ps_record(const uint8_t xy_le[64], uint32_t out[27]) {
  uint32_t xw[8], yw[8];
  memcpy(xw, xy_le, 32); memcpy(yw, xy_le + 32, 32);
  const pnt r = pnt_from_affine_raw(fp_from_words32(xw), fp_from_words32(yw));
  memcpy(out, &r, 108);
}
// both signs are applied with pnt_cneg before the call, as k_accumulate does
void ps_pair(const uint32_t a[27], int neg_a, const uint32_t b[27], int neg_b, uint32_t out[36]) {
  pnt x, y; memcpy(&x, a, 108); memcpy(&y, b, 108);
  const ete r = ete_from_pair(pnt_cneg(x, neg_a != 0), pnt_cneg(y, neg_b != 0)); memcpy(out, &r, 144);
}
void ps_convert_add(const uint32_t a[27], int neg_a, const uint32_t b[27], int neg_b, uint32_t out[36]) {
  pnt x, y; memcpy(&x, a, 108); memcpy(&y, b, 108);
  const ete r = ete_madd(ete_from_pnt(pnt_cneg(x, neg_a != 0)), pnt_cneg(y, neg_b != 0)); memcpy(out, &r, 144);
}

// ---- BLS12-377 G1, 14 limbs: projective record hm | hp | dt | z (56 words), affine record hm | hp | dt (42 words),
// accumulator x | y | z | t (56 words)
int ps377_overflow_and_reset() { const int v = g_fq377_overflow; g_fq377_overflow = 0; return v; }
// [R, 2d R, s R^2, f R]: what maps the Edwards form back to y^2 = x^3 + 1
void ps377_constants(uint32_t out[4 * 14]) {
  using namespace te377;
  const fq c[4] = {fq_R1(), fq_K2D_MONT(), fq_S_R2(), fq_F_MONT()};
  memcpy(out, c, sizeof c);
}
// short-Weierstrass x, y: 48 little-endian bytes each
void ps377_record(const uint8_t xy_le[96], uint32_t out[56]) {
  uint32_t xw[12], yw[12]; memcpy(xw, xy_le, 48); memcpy(yw, xy_le + 48, 48);
  const pnt_t<14> r = pnt_from_sw377(te377::fq_from_words32(xw), te377::fq_from_words32(yw));
  memcpy(out, &r, 224);
}
void ps377_pair(const uint32_t a[56], int neg_a, const uint32_t b[56], int neg_b, uint32_t out[56]) {
  pnt_t<14> x, y; memcpy(&x, a, 224); memcpy(&y, b, 224);
  const ete_t<14> r = ete_from_pair(pnt_cneg(x, neg_a != 0), pnt_cneg(y, neg_b != 0)); memcpy(out, &r, 224);
}
void ps377_convert_add(const uint32_t a[56], int neg_a, const uint32_t b[56], int neg_b, uint32_t out[56]) {
  pnt_t<14> x, y; memcpy(&x, a, 224); memcpy(&y, b, 224);
  const ete_t<14> r = ete_madd(ete_from_pnt(pnt_cneg(x, neg_a != 0)), pnt_cneg(y, neg_b != 0)); memcpy(out, &r, 224);
}
void ps377_pair_aff(const uint32_t a[42], int neg_a, const uint32_t b[42], int neg_b, uint32_t out[56]) {
  pnt_aff377 x, y; memcpy(&x, a, 168); memcpy(&y, b, 168);
  const ete_t<14> r = ete_from_pair(pnt_cneg(x, neg_a != 0), pnt_cneg(y, neg_b != 0)); memcpy(out, &r, 224);
}
void ps377_convert_add_aff(const uint32_t a[42], int neg_a, const uint32_t b[42], int neg_b, uint32_t out[56]) {
  pnt_aff377 x, y; memcpy(&x, a, 168); memcpy(&y, b, 168);
  const ete_t<14> r = ete_madd(ete_from_pnt(pnt_cneg(x, neg_a != 0)), pnt_cneg(y, neg_b != 0)); memcpy(out, &r, 224);
}

}  // extern "C"
