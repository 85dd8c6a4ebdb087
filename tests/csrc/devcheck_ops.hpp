// devcheck_ops.hpp -- TEST SHIM: one table of the engine's arithmetic primitives (csrc/fp.hpp, fq377.hpp, curve.hpp,
// scalar_form.hpp), each behind a wrapper of one form,  void op(const uint32_t* in, uint32_t* out)  with fixed word counts.
// The table is compiled twice from this one text: by g++ into libdevcheck_host.so (devcheck_host.cpp, a loop over elements) and by
// hipcc for gfx950 inside devcheck.hip (one element per lane), so the device compilation of every function -- its chain() markers,
// v_bitop3 selections, unrolled loops -- is compared bit for bit with the host build that the host tests pin to bigints.
// HIP-free; the product's headers are included unchanged.  Not part of the product; not a fallback.
#pragma once
#include <stdint.h>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/curve.hpp"
#include "../../webgpu-msm-twisted-edwards_amd/csrc/scalar_form.hpp"

namespace dcop {
using namespace te;

// a struct of 32-bit words (fel, pnt_t, pnt_aff377, ete_t) <-> consecutive words
template <class T> TE_HD T ld(const uint32_t* p) {
  T r; uint32_t* w = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; i++) w[i] = p[i];
  return r;
}
template <class T> TE_HD void st(uint32_t* p, const T& a) {
  const uint32_t* w = reinterpret_cast<const uint32_t*>(&a);
#pragma unroll
  for (unsigned i = 0; i < sizeof(T) / 4; i++) p[i] = w[i];
}

// ---- products.  mul_x: a0 | b0 | a1 | b1 | ...  ->  r0 | r1 | ...  (different operands in every chain)
template <int N> TE_HD void mul(const uint32_t* in, uint32_t* out) { st(out, fe_mul(ld<fel<N>>(in), ld<fel<N>>(in + N))); }
template <int N, int M> TE_HD void mul_x(const uint32_t* in, uint32_t* out) {
  fel<N> a[M], b[M], r[M];
#pragma unroll
  for (int m = 0; m < M; m++) { a[m] = ld<fel<N>>(in + 2 * N * m); b[m] = ld<fel<N>>(in + 2 * N * m + N); }
  fe_mul_x<M>(a, b, r);
#pragma unroll
  for (int m = 0; m < M; m++) st(out + N * m, r[m]);
}
// ---- small multiplies and carries
TE_HD void mul_k2d(const uint32_t* in, uint32_t* out) { st(out, fp_mul_k2d(ld<fp>(in))); }
TE_HD void mul_d(const uint32_t* in, uint32_t* out) { st(out, fp_mul_d(ld<fp>(in))); }
TE_HD void mul3(const uint32_t* in, uint32_t* out) { st(out, te377::fq_mul3(ld<fel<14>>(in))); }
template <int N> TE_HD void norm(const uint32_t* in, uint32_t* out) { st(out, fe_norm(ld<fel<N>>(in))); }
// ---- subtractions and negations in offset form
template <int N, int K> TE_HD void sub(const uint32_t* in, uint32_t* out) { st(out, fe_sub<K>(ld<fel<N>>(in), ld<fel<N>>(in + N))); }
template <int N, int K> TE_HD void neg(const uint32_t* in, uint32_t* out) { st(out, fe_neg<K>(ld<fel<N>>(in))); }
// ---- loads and selection
TE_HD void from_words_9(const uint32_t* in, uint32_t* out) {
  uint32_t w[8]; for (int i = 0; i < 8; i++) w[i] = in[i];
  st(out, fp_from_words32(w));
}
TE_HD void from_words_14(const uint32_t* in, uint32_t* out) {
  uint32_t w[12]; for (int i = 0; i < 12; i++) w[i] = in[i];
  st(out, te377::fq_from_words32(w));
}
TE_HD void select(const uint32_t* in, uint32_t* out) { out[0] = mask_select(in[0], in[1], in[2]); }          // m | b | a
// ---- records.  Coordinates come in as limbs (class N, any 256- / 384-bit value): x | y
template <bool MONT> TE_HD void rec_te(const uint32_t* in, uint32_t* out) { st(out, pnt_from_affine_raw<MONT>(ld<fp>(in), ld<fp>(in + 9))); }
template <bool MONT> TE_HD void rec_sw(const uint32_t* in, uint32_t* out) { st(out, pnt_from_sw377<MONT>(ld<fel<14>>(in), ld<fel<14>>(in + 14))); }
// record | sign word (0: keep, anything else: negate)
template <class REC> TE_HD void cneg(const uint32_t* in, uint32_t* out) { st(out, pnt_cneg(ld<REC>(in), in[sizeof(REC) / 4] != 0u)); }
// ---- point formulas
template <class REC, class ACC> TE_HD void from_pnt(const uint32_t* in, uint32_t* out) { const ACC r = ete_from_pnt(ld<REC>(in)); st(out, r); }
template <class REC, class ACC> TE_HD void from_pair(const uint32_t* in, uint32_t* out) {
  const ACC r = ete_from_pair(ld<REC>(in), ld<REC>(in + sizeof(REC) / 4)); st(out, r);
}
template <class REC, class ACC> TE_HD void madd(const uint32_t* in, uint32_t* out) {                           // accumulator | record
  const ACC r = ete_madd(ld<ACC>(in), ld<REC>(in + sizeof(ACC) / 4)); st(out, r);
}
template <int N> TE_HD void add(const uint32_t* in, uint32_t* out) { st(out, ete_add<N>(ld<ete_t<N>>(in), ld<ete_t<N>>(in + 4 * N))); }
// ---- scalar decoding
template <int FORM> TE_HD void scalar(const uint32_t* in, uint32_t* out) {
  uint32_t a[8]; for (int i = 0; i < 8; i++) a[i] = in[i];
  scalar_from_montgomery<FORM>(a);
  for (int i = 0; i < 8; i++) out[i] = a[i];
}
}  // namespace dcop

// The table: X(name, function, words in, words out).  Both builds export  int dc_<name>(const uint32_t* in, uint32_t* out, uint32_t n)
// over n elements laid out back to back (host pointers in libdevcheck_host.so, device pointers in libdevcheck.so).
#define DC_R9 te::pnt_t<9>
#define DC_R14 te::pnt_t<14>
#define DC_RA te::pnt_aff377
#define DC_A9 te::ete_t<9>
#define DC_A14 te::ete_t<14>
#define DC_OPS(X)                                                                         \
  X(mul_9, (dcop::mul<9>), 18, 9)                  X(mul_14, (dcop::mul<14>), 28, 14)     \
  X(mul_x2_9, (dcop::mul_x<9, 2>), 36, 18)         X(mul_x2_14, (dcop::mul_x<14, 2>), 56, 28)   \
  X(mul_x3_9, (dcop::mul_x<9, 3>), 54, 27)         X(mul_x3_14, (dcop::mul_x<14, 3>), 84, 42)   \
  X(mul_x4_9, (dcop::mul_x<9, 4>), 72, 36)         X(mul_x4_14, (dcop::mul_x<14, 4>), 112, 56)  \
  X(mul_k2d_9, dcop::mul_k2d, 9, 9)                X(mul_d_9, dcop::mul_d, 9, 9)          \
  X(mul3_14, dcop::mul3, 14, 14)                                                          \
  X(norm_9, (dcop::norm<9>), 9, 9)                 X(norm_14, (dcop::norm<14>), 14, 14)   \
  X(sub2_9, (dcop::sub<9, 2>), 18, 9)              X(sub2_14, (dcop::sub<14, 2>), 28, 14) \
  X(sub4_9, (dcop::sub<9, 4>), 18, 9)              X(sub4_14, (dcop::sub<14, 4>), 28, 14) \
  X(sub16_9, (dcop::sub<9, 16>), 18, 9)            X(sub16_14, (dcop::sub<14, 16>), 28, 14)     \
  X(neg2_9, (dcop::neg<9, 2>), 9, 9)               X(neg2_14, (dcop::neg<14, 2>), 14, 14) \
  X(neg4_9, (dcop::neg<9, 4>), 9, 9)               X(neg4_14, (dcop::neg<14, 4>), 14, 14) \
  X(from_words_9, dcop::from_words_9, 8, 9)        X(from_words_14, dcop::from_words_14, 12, 14)\
  X(select, dcop::select, 3, 1)                                                           \
  X(rec_te, (dcop::rec_te<false>), 18, 27)         X(rec_te_mont, (dcop::rec_te<true>), 18, 27) \
  X(rec_sw, (dcop::rec_sw<false>), 28, 56)         X(rec_sw_mont, (dcop::rec_sw<true>), 28, 56) \
  X(cneg_9, (dcop::cneg<DC_R9>), 28, 27)           X(cneg_14, (dcop::cneg<DC_R14>), 57, 56)     \
  X(cneg_aff, (dcop::cneg<DC_RA>), 43, 42)                                                \
  X(from_pnt_9, (dcop::from_pnt<DC_R9, DC_A9>), 27, 36)      X(from_pnt_14, (dcop::from_pnt<DC_R14, DC_A14>), 56, 56)    \
  X(from_pnt_aff, (dcop::from_pnt<DC_RA, DC_A14>), 42, 56)                                \
  X(from_pair_9, (dcop::from_pair<DC_R9, DC_A9>), 54, 36)    X(from_pair_14, (dcop::from_pair<DC_R14, DC_A14>), 112, 56) \
  X(from_pair_aff, (dcop::from_pair<DC_RA, DC_A14>), 84, 56)                              \
  X(madd_9, (dcop::madd<DC_R9, DC_A9>), 63, 36)              X(madd_14, (dcop::madd<DC_R14, DC_A14>), 112, 56)           \
  X(madd_aff, (dcop::madd<DC_RA, DC_A14>), 98, 56)                                        \
  X(add_9, (dcop::add<9>), 72, 36)                 X(add_14, (dcop::add<14>), 112, 56)    \
  X(scalar_te, (dcop::scalar<te::SCALAR_FORM_TE>), 8, 8)     X(scalar_377, (dcop::scalar<te::SCALAR_FORM_377>), 8, 8)
