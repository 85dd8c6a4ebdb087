// pointcheck.cpp -- TEST SHIM: compiles the product's point checks (csrc/check.hip.hpp) for the host, so that the verdicts of
// the exact code that k_check_form / k_check_subgroup run on gfx950 are compared with the bigint models on the CPU box
// (tests/test_point_checks_host.py).  Not part of the product; not a fallback.
#include <stdint.h>
#include <string.h>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/check.hip.hpp"

using namespace te;

extern "C" {

// level 1: form only; level 2: form, then the subgroup.  Returns the reason code (0 = the point passes).
int pc_check_te(const uint8_t* p64, int level) {
  uint32_t w[16];
  memcpy(w, p64, 64);
  const int r = check_form_te(w);
  if (r || level < 2) return r;
  return in_subgroup_te(w, kNafTeOrder) ? 0 : 3;
}
int pc_check_377(const uint8_t* p96, int level) {
  uint32_t w[24];
  memcpy(w, p96, 96);
  const int r = check_form_377(w);
  if (r || level < 2) return r;
  return in_subgroup_377(w, kNaf377Order) ? 0 : 3;
}
// the report word: the code of (n, i, reason) and its decoding
uint64_t pc_code(uint64_t n, uint64_t i, int reason) { return check_code(n, i, reason); }
void pc_decode(uint64_t code, uint64_t n, int64_t* index, int* reason) { check_decode(code, n, index, reason); }

}
