// scalarform.cpp -- TEST SHIM: csrc/scalar_form.hpp (the Montgomery reduction the digit kernels run on option "scalars_montgomery") and the
// Montgomery-input instantiations of the bind path's record conversions (csrc/curve.hpp, option "points_montgomery"), compiled for the host
// so tests/test_scalar_form_host.py checks the exact word and limb code of the kernels against Python integers.  Not part of the product;
// not a fallback.  Also a program of its own (main below): the same functions over edge values, checked by re-encoding -- what the test
// builds and runs once with -fsanitize=address,undefined.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/scalar_form.hpp"
#include "../../webgpu-msm-twisted-edwards_amd/csrc/curve.hpp"

using namespace te;

namespace {
void decode(int form, const uint8_t in[32], uint8_t out[32]) {
  uint32_t a[8];
  memcpy(a, in, 32);
  if (form == SCALAR_FORM_377) scalar_from_montgomery<SCALAR_FORM_377>(a);
  else scalar_from_montgomery<SCALAR_FORM_TE>(a);
  memcpy(out, a, 32);
}
const uint32_t* modulus(int form) { return form == SCALAR_FORM_377 ? SF_MOD_377 : SF_MOD_TE; }
}  // namespace

extern "C" {

// form: 1 = modulo L (Twisted-Edwards BLS12), 2 = modulo r (BLS12-377); n records of 32 little-endian bytes
void sf_decode(int form, const uint8_t* in, uint64_t n, uint8_t* out) {
  for (uint64_t i = 0; i < n; i++) decode(form, in + 32 * i, out + 32 * i);
}
void sf_modulus(int form, uint32_t out[8], uint32_t* ninv) {
  memcpy(out, modulus(form), 32);
  *ninv = form == SCALAR_FORM_377 ? SF_NINV_377 : SF_NINV_TE;
}
// [R_e^2 / R_a / 2, R_e^2 / R_a] mod p (9 limbs each), [s, 1, f] R_e^2 / R_a mod q (14 limbs each)
void sf_point_constants(uint32_t te_out[2 * 9], uint32_t q_out[3 * 14]) {
  const fp a[2] = {fp_R2_HALF_A(), fp_R2_A()};
  memcpy(te_out, a, sizeof a);
  const te377::fq b[3] = {te377::fq_S_R2_A(), te377::fq_R2_A(), te377::fq_F_R2_A()};
  memcpy(q_out, b, sizeof b);
}
// x || y, 32 bytes each -> hm | hp | dt (27 limbs); mont: the coordinates are x 2^256 mod p
void sf_from_affine(int mont, const uint8_t xy_le[64], uint32_t out[27]) {
  uint32_t xw[8], yw[8];
  memcpy(xw, xy_le, 32); memcpy(yw, xy_le + 32, 32);
  const pnt r = mont ? pnt_from_affine_raw<true>(fp_from_words32(xw), fp_from_words32(yw)) : pnt_from_affine_raw<false>(fp_from_words32(xw), fp_from_words32(yw));
  memcpy(out, &r, 108);
}
// x || y, 48 bytes each -> hm | hp | dt | z (56 limbs); mont: the coordinates are x 2^384 mod q
void sf_from_sw377(int mont, const uint8_t xy_le[96], uint32_t out[56]) {
  uint32_t xw[12], yw[12];
  memcpy(xw, xy_le, 48); memcpy(yw, xy_le + 48, 48);
  const te377::fq x = te377::fq_from_words32(xw), y = te377::fq_from_words32(yw);
  const pnt_t<14> r = mont ? pnt_from_sw377<true>(x, y) : pnt_from_sw377<false>(x, y);
  memcpy(out, &r, 224);
}

}  // extern "C"

// ---- the stand-alone program: decode(a) is below m and 2^256 decode(a) = a (mod m), by plain add-and-subtract arithmetic on 8 words
namespace {
bool ge(const uint32_t a[8], const uint32_t m[8]) {
  for (int i = 7; i >= 0; i--) if (a[i] != m[i]) return a[i] > m[i];
  return true;
}
void sub(uint32_t a[8], const uint32_t m[8]) {
  uint64_t b = 0;
  for (int i = 0; i < 8; i++) { const uint64_t s = (uint64_t)a[i] - m[i] - b; a[i] = (uint32_t)s; b = (s >> 32) & 1u; }
}
// a = 2 a mod m for a < m < 2^255
void dbl(uint32_t a[8], const uint32_t m[8]) {
  uint32_t c = 0;
  for (int i = 0; i < 8; i++) { const uint32_t n = a[i] >> 31; a[i] = (a[i] << 1) | c; c = n; }
  if (ge(a, m)) sub(a, m);
}
int check_one(int form, const uint32_t a_in[8]) {
  const uint32_t* m = modulus(form);
  uint8_t in[32], out[32];
  memcpy(in, a_in, 32);
  decode(form, in, out);
  uint32_t k[8], a[8];
  memcpy(k, out, 32); memcpy(a, a_in, 32);
  if (ge(k, m)) return 1;                               // not canonical
  for (int i = 0; i < 256; i++) dbl(k, m);              // k 2^256 mod m
  while (ge(a, m)) sub(a, m);                           // a mod m (at most 2^256 / m < 64 rounds)
  return memcmp(k, a, 32) != 0;
}
}  // namespace

int main() {
  int bad = 0, cases = 0;
  for (int form = SCALAR_FORM_TE; form <= SCALAR_FORM_377; form++) {
    const uint32_t* m = modulus(form);
    uint32_t v[8];
    auto run = [&]() { bad += check_one(form, v); cases++; };
    memset(v, 0, 32); run();
    v[0] = 1; run();
    memcpy(v, m, 32); run();
    v[0] -= 1; run();
    v[0] += 2; run();
    memset(v, 0xff, 32); run();
    for (int j = 0; j < 8; j++) {
      memset(v, 0, 32); v[j] = 0xffffffffu; run();
      memset(v, 0xff, 32); v[j] = 0; run();
    }
    uint64_t s = 0x9e3779b97f4a7c15ull + (uint64_t)form;
    for (int i = 0; i < 2000; i++) {
      for (int j = 0; j < 8; j++) { s = s * 6364136223846793005ull + 1442695040888963407ull; v[j] = (uint32_t)(s >> 32); }
      run();
    }
  }
  // the record conversions in both forms (their values are the test's business; here they run under the sanitizers)
  uint8_t xy[96];
  for (int i = 0; i < 96; i++) xy[i] = (uint8_t)(37 * i + 11);
  xy[47] = 0; xy[95] = 0;
  uint32_t rec[56];
  uint32_t sum = 0;
  for (int mont = 0; mont < 2; mont++) {
    sf_from_affine(mont, xy, rec); sum += rec[0];
    sf_from_sw377(mont, xy, rec); sum += rec[0];
  }
  printf("scalarform: %d cases, %d bad (conversion word %08x)\n", cases, bad, sum);
  return bad ? 1 : 0;
}
