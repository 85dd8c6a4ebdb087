// devcheck_ops2.hpp -- TEST SHIM: the second operation table, over the per-lane functions of csrc/check.hip.hpp, from_x.hip.hpp and
// scalar_mul.hip.hpp -- the zero test, the canonical conversions, the Fermat inverse, the uniform square root, the complete
// short-Weierstrass formulas, the negating addition, the order chain, the offset recoding, the affine group and the verdicts.
// Same mechanism as devcheck_ops.hpp: one wrapper form  void op(const uint32_t* in, uint32_t* out)  with fixed word counts, compiled
// by g++ into libdevcheck2_host.so (devcheck2_host.cpp) and by hipcc for gfx950 into libdevcheck2.so (devcheck2.hip), a library pair
// of its own so that neither translation unit grows slow to compile.  Exponents and orders are the product's constants; a chain
// whose digits are operands (mul_order_te) takes them as words.  HIP-free; the product's headers are included unchanged.
// Not part of the product; not a fallback.
#pragma once
#include <stdint.h>
#include "devcheck_ops.hpp"
#include "../../webgpu-msm-twisted-edwards_amd/csrc/scalar_mul.hip.hpp"

namespace dcop {

template <class T, int K> TE_HD void ldw(const uint32_t* p, T (&w)[K]) {
#pragma unroll
  for (int i = 0; i < K; i++) w[i] = p[i];
}
template <int N> TE_HD const uint32_t* modulus_words() { if constexpr (N == 9) return P_W32; else return te377::Q_W32; }

// ---- field helpers
template <int N> TE_HD void is_zero(const uint32_t* in, uint32_t* out) { out[0] = fe_is_zero(ld<fel<N>>(in)) ? 1u : 0u; }
template <int N, int W> TE_HD void to_canon(const uint32_t* in, uint32_t* out) {
  uint32_t w[W];
  fe_to_canon<N, W>(ld<fel<N>>(in), w);
#pragma unroll
  for (int i = 0; i < W; i++) out[i] = w[i];
}
template <int N, int W> TE_HD void from_canon(const uint32_t* in, uint32_t* out) {
  uint32_t w[W];
  ldw(in, w);
  st(out, fe_from_canon(w));
}
template <int N> TE_HD void inv(const uint32_t* in, uint32_t* out) { st(out, fe_inv<N>(ld<fel<N>>(in), N == 9 ? kInvExpTe : kInvExp377)); }
// u | v -> flag | y
TE_HD void sqrt_ratio_9(const uint32_t* in, uint32_t* out) {
  fp y;
  out[0] = fe_sqrt_ratio<9, true>(ld<fp>(in), ld<fp>(in + 9), kRootExpTe, y) ? 1u : 0u;
  st(out + 1, y);
}
// u -> flag | y
TE_HD void sqrt_14(const uint32_t* in, uint32_t* out) {
  const fel<14> u = ld<fel<14>>(in);
  fel<14> y;
  out[0] = fe_sqrt_ratio<14, false>(u, u, kRootExp377, y) ? 1u : 0u;
  st(out + 1, y);
}
template <int N, int W> TE_HD void words_lt_m(const uint32_t* in, uint32_t* out) {
  uint32_t a[W];
  ldw(in, a);
  out[0] = words_lt<W>(a, modulus_words<N>()) ? 1u : 0u;
}
template <int N, int W> TE_HD void words_neg_m(const uint32_t* in, uint32_t* out) {
  uint32_t a[W], r[W];
  ldw(in, a);
  words_neg<W>(a, modulus_words<N>(), r);
#pragma unroll
  for (int i = 0; i < W; i++) out[i] = r[i];
}
// ---- the complete short-Weierstrass formulas: (X : Y : Z) of 14 limbs each
TE_HD void sw_add(const uint32_t* in, uint32_t* out) { st(out, sw377_add(ld<sw377>(in), ld<sw377>(in + 42))); }
TE_HD void sw_dbl(const uint32_t* in, uint32_t* out) { st(out, sw377_dbl(ld<sw377>(in))); }
TE_HD void sw_cneg(const uint32_t* in, uint32_t* out) { st(out, sw377_cneg(ld<sw377>(in), in[42] != 0u)); }      // point | sign word
// ---- Twisted-Edwards chains.  a | b | sign word
TE_HD void add_cneg(const uint32_t* in, uint32_t* out) { st(out, ete_add_cneg(ld<ete>(in), ld<ete>(in + 36), in[72] != 0u)); }
TE_HD naf_t ld_naf(const uint32_t* p) {                                 // pos[8] | neg[8] | top (0 .. 255)
  naf_t k;
#pragma unroll
  for (int i = 0; i < 8; i++) { k.pos[i] = p[i]; k.neg[i] = p[8 + i]; }
  k.top = (int)(p[16] & 255u);
  return k;
}
TE_HD void mul_order(const uint32_t* in, uint32_t* out) { st(out, mul_order_te(ld<fp>(in), ld<fp>(in + 9), ld_naf(in + 18))); }   // X | Y | naf
// naf | i -> the digit as a two's-complement word;  exponent words[12] | top | i -> the bit
TE_HD void naf_digit_at(const uint32_t* in, uint32_t* out) { out[0] = (uint32_t)naf_digit(ld_naf(in), (int)(in[17] & 255u)); }
TE_HD void exp_bit_at(const uint32_t* in, uint32_t* out) {
  exp_t e;
#pragma unroll
  for (int i = 0; i < 12; i++) e.w[i] = in[i];
  e.top = (int)in[12];
  out[0] = exp_bit(e, (int)(in[13] % 384u)) ? 1u : 0u;
}
// k (8 words) -> K (9 words) | the M signed digits as two's-complement words (W = 2 on both curves)
TE_HD void sm_digits(const uint32_t* in, uint32_t* out) {
  using S = sm_win<0>;
  static_assert(sm_win<0>::W == sm_win<1>::W && sm_win<0>::M == sm_win<1>::M && S::M == 129, "one operation serves both curves");
  uint32_t k[8], K[9];
  ldw(in, k);
  sm_recode<S::W, S::M>(k, K);
#pragma unroll
  for (int j = 0; j < 9; j++) out[j] = K[j];
#pragma unroll 1
  for (int i = 0; i < S::M; i++) out[9 + i] = (uint32_t)sm_digit<S::W>(K, i);
}
// ---- affine output: 8 projective slots | cnt (1 .. 8) -> 8 points; the words of the points past cnt stay DC_AFF_FILL
#define DC_AFF_FILL 0xA5A5A5A5u
template <int CURVE> TE_HD void aff_group(const uint32_t* in, uint32_t* out) {
  using Z = sm_sizes<CURVE>;
  for (int i = 0; i < 8 * Z::PW; i++) out[i] = DC_AFF_FILL;
  uint32_t cnt = in[8 * Z::JW];
  cnt = cnt < 1u ? 1u : (cnt > SM_AFF_GROUP ? SM_AFF_GROUP : cnt);
  sm_affine_group<CURVE>(in, cnt, out, CURVE == 1 ? kInvExp377 : kInvExpTe);
}
// ---- verdicts on wire words
template <bool MONT> TE_HD void form_te(const uint32_t* in, uint32_t* out) { uint32_t w[16]; ldw(in, w); out[0] = (uint32_t)check_form_te<MONT>(w); }
template <bool MONT> TE_HD void form_377(const uint32_t* in, uint32_t* out) { uint32_t w[24]; ldw(in, w); out[0] = (uint32_t)check_form_377<MONT>(w); }
TE_HD void subgroup_te(const uint32_t* in, uint32_t* out) { uint32_t w[16]; ldw(in, w); out[0] = in_subgroup_te(w, kNafTeOrder) ? 1u : 0u; }
TE_HD void subgroup_377(const uint32_t* in, uint32_t* out) { uint32_t w[24]; ldw(in, w); out[0] = in_subgroup_377(w, kNaf377Order) ? 1u : 0u; }
}  // namespace dcop

// The second table: X(name, function, words in, words out), exported as dc_<name> like the first
#define DC_OPS2(X)                                                                                      \
  X(is_zero_9, (dcop::is_zero<9>), 9, 1)                     X(is_zero_14, (dcop::is_zero<14>), 14, 1)  \
  X(to_canon_9, (dcop::to_canon<9, 8>), 9, 8)                X(to_canon_14, (dcop::to_canon<14, 12>), 14, 12)     \
  X(from_canon_9, (dcop::from_canon<9, 8>), 8, 9)            X(from_canon_14, (dcop::from_canon<14, 12>), 12, 14) \
  X(inv_9, (dcop::inv<9>), 9, 9)                             X(inv_14, (dcop::inv<14>), 14, 14)         \
  X(sqrt_ratio_9, dcop::sqrt_ratio_9, 18, 10)                X(sqrt_14, dcop::sqrt_14, 14, 15)          \
  X(words_lt_8, (dcop::words_lt_m<9, 8>), 8, 1)              X(words_lt_12, (dcop::words_lt_m<14, 12>), 12, 1)    \
  X(words_neg_8, (dcop::words_neg_m<9, 8>), 8, 8)            X(words_neg_12, (dcop::words_neg_m<14, 12>), 12, 12) \
  X(sw_add, dcop::sw_add, 84, 42)                            X(sw_dbl, dcop::sw_dbl, 42, 42)            \
  X(sw_cneg, dcop::sw_cneg, 43, 42)                          X(add_cneg, dcop::add_cneg, 73, 36)        \
  X(mul_order_te, dcop::mul_order, 35, 36)                   X(sm_digits, dcop::sm_digits, 8, 138)      \
  X(naf_digit, dcop::naf_digit_at, 18, 1)                    X(exp_bit, dcop::exp_bit_at, 14, 1)        \
  X(aff_group_te, (dcop::aff_group<0>), 225, 128)            X(aff_group_377, (dcop::aff_group<1>), 353, 192)     \
  X(check_form_te, (dcop::form_te<false>), 16, 1)            X(check_form_te_mont, (dcop::form_te<true>), 16, 1)  \
  X(check_form_377, (dcop::form_377<false>), 24, 1)          X(check_form_377_mont, (dcop::form_377<true>), 24, 1)\
  X(in_subgroup_te, dcop::subgroup_te, 16, 1)                X(in_subgroup_377, dcop::subgroup_377, 24, 1)
