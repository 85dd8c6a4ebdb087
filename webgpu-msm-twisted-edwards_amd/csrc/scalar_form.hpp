// scalar_form.hpp -- scalars in a native prover's Montgomery form (option "scalars_montgomery", include/te_msm.h).
//
// arkworks and snarkVM keep a scalar k as a = k * 2^256 mod m in four u64 limbs: in memory a 32-byte little-endian integer.  The digit
// kernels (kernels.hip.hpp: digits_block, k_fb_digits) decode it where they load it, k = a * 2^-256 mod m, one Montgomery reduction per
// scalar: 8 rounds of u = t_0 * (-m^-1) mod 2^32, t = (t + u m) / 2^32 over 32-bit words (64 multiply-accumulates and 8 low products)
// and one conditional subtraction.  m is the scalar field of the curve in force:
//   SCALAR_FORM_TE   L, the prime-order subgroup of the Twisted-Edwards BLS12 curve (251 bits)
//   SCALAR_FORM_377  r of BLS12-377 (253 bits)
// ANY 256-bit a is accepted and stands for its residue; the result is canonical (< m).  Bounds: t < 2^256 before round 1 and
// t_i < t_{i-1} / 2^32 + m after round i, so t_i < 2^(256 - 32 i) + m (1 + 2^-32 + ...) < 2^256 for both moduli (m < 2^253): eight words
// hold every intermediate, and t_8 < 1 + m (1 + 2^-31), an integer congruent to a 2^-256, is at most m -- one subtraction (t_8 = m happens:
// a = m).
// HIP-free: the same text compiles for the host (tests/csrc/scalarform.cpp; a caller's CPU pass is what the option removes,
// tools/montgomery_inputs.py times it).  The constants come from tools/gen_constants.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef TE_HD
#define TE_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef TE_HD
#define TE_HD inline
#endif
#endif

namespace te {

#include "scalar_form_constants.inc"

// what a scalar record holds: the integer itself, or its Montgomery form modulo one of the two scalar fields
enum { SCALAR_FORM_CANONICAL = 0, SCALAR_FORM_TE = 1, SCALAR_FORM_377 = 2 };

// word j of the modulus of FORM and its -m^-1 mod 2^32 (compile-time j: the constants become immediates)
template <int FORM> TE_HD uint32_t sf_mod_word(int j) { return FORM == SCALAR_FORM_377 ? SF_MOD_377[j] : SF_MOD_TE[j]; }
template <int FORM> TE_HD uint32_t sf_ninv() { return FORM == SCALAR_FORM_377 ? SF_NINV_377 : SF_NINV_TE; }

// a (8 little-endian 32-bit words, any value) -> a * 2^-256 mod m, canonical, in place
template <int FORM> TE_HD void scalar_from_montgomery(uint32_t (&a)[8]) {
  static_assert(FORM == SCALAR_FORM_TE || FORM == SCALAR_FORM_377, "a Montgomery form");
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 8; i++) {
    const uint32_t u = a[0] * sf_ninv<FORM>();
    uint64_t c = ((uint64_t)u * sf_mod_word<FORM>(0) + a[0]) >> 32;        // the low word is 0 by the choice of u
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = 1; j < 8; j++) {
      c += (uint64_t)u * sf_mod_word<FORM>(j) + a[j];
      a[j - 1] = (uint32_t)c;
      c >>= 32;
    }
    a[7] = (uint32_t)c;                                                   // (below 2^32: the bound above)
  }
  // t >= m ? t - m : t
  uint32_t d[8];
  uint64_t borrow = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 8; j++) {
    const uint64_t s = (uint64_t)a[j] - sf_mod_word<FORM>(j) - borrow;
    d[j] = (uint32_t)s;
    borrow = (s >> 32) & 1u;
  }
  const uint32_t keep = (uint32_t)0 - (uint32_t)borrow;                   // all ones: t < m
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 8; j++) a[j] = (a[j] & keep) | (d[j] & ~keep);
}

}  // namespace te
