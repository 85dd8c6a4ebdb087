// from_x.hip.hpp -- x-only points: the point of each x-coordinate, recovered on the device (te_msm_points_from_x*,
// te_msm_bind_points_x, te_msm_run_x; include/te_msm.h "x-only points").
//
// Like check.hip.hpp, every verdict is a pure function of the input bytes, and the header compiles for the host as well
// (tests/csrc/fromxcheck.cpp runs the exact code of k_points_from_x on the CPU).  Reason codes are TE_MSM_POINT_*.
//
// TWISTED-EDWARDS BLS12 (an Aleo `group`: the value IS its x-coordinate).  y^2 = (a x^2 - 1) / (d x^2 - 1) = (1 + x^2) / (1 - d x^2),
// a = -1, d = 3021.  d is a non-square, so the denominator never vanishes.  Of the two roots +-y the point must lie in the subgroup of
// order L.  The curve group is Z/L x Z/4 (one point of order 2, T2 = (0, -1); two of order 4, (+-sqrt(-1), 0)), so with
// P = (x, y) = S + T, S in the subgroup and T of order dividing 4, ONE chain decides: Q = [L] P = [L] T has T's order (L is odd).
//   Q = O        T = O: take y
//   Q = T2       (x, -y) = -P + T2 = -S - T + T2 = -S: take -y
//   Q of order 4 (x, -y) has torsion T2 - T, of order 4 as well: neither root is in the subgroup, reason 3 (this covers y = 0)
// The chain is check.hip.hpp's (mul_order_te, the complete ete_add).  getPointFromX of the reference (FieldMath.ts:31-55) returns
// (x, -y) in the last case; reason 3 is what Address.msm does instead -- it cannot build such a group.
//
// BLS12-377 G1 (48 bytes; the flags of compressed short-Weierstrass points as arkworks / snarkVM lay them out -- not verifiable
// offline, pinned as written here): bit 7 of byte 47 = y is the larger root (y > q - y), bit 6 = the point at infinity (reason 2, as
// the uncompressed form), bits 377..381 must be 0 (reason 1, as x >= q).  y = sqrt(x^3 + 1), no root: reason 2; the predicates of
// check_form_377 apply to the recovered point, so y = 0 and s x + s + 1 = 0 (the engine's map undefined) are reason 2 exactly as there.  Both
// roots share subgroup membership: that stays the job of option "check_points" = 2.  (The predicates are check_form_377's, computed
// around the root rather than by calling it on the result: its lockstep products beside the root's live values cost the kernel
// 500 registers.)
//
// THE SQUARE ROOT: RFC 9380's sqrt_ratio for any field (appendix F.2.1.1), lane-uniform.  p - 1 = 2^47 t, q - 1 = 2^46 t: the
// fixed exponent (t - 1) / 2 runs as a square-and-multiply chain over compile-time bits (a kernel argument read through selects, as
// the NAF chain); the 2-adic part is S - 1 steps whose squaring counts depend on the step only, with selects -- every lane of a wave
// runs the same instructions.  No table: the roots of unity are powers of one constant, squared step by step.  The division by
// 1 - d x^2 is folded into the one exponentiation (no inversion).  u = 0 comes out as (false, 0): callers treat it as the root 0.
// COST (field products): TE  v^(2^47-1) 92 + exponent ~305 + test 46 + steps 1035 squarings + 3 x 46 = ~1 630, the chain ~3 000;
//                         377 exponent ~495 + 45 + 990 + 3 x 45 = ~1 670, no chain.
// LIMBS: every operand of a product is a product output (class N, value < 1.1 p) or a normalised sum; selects keep the class.
#pragma once
#include "check.hip.hpp"

namespace te {

// bits of a fixed exponent, little-endian words; top = index of the leading one
struct exp_t { uint32_t w[12]; int top; };
// (t - 1) / 2 with p - 1 = 2^47 t (205 bits)
constexpr exp_t kRootExpTe = {{0x00010a11u, 0x76fed000u, 0xb00159aau, 0x4d1e5c37u, 0xa55660b4u, 0x655e9a2cu, 0x000012abu, 0u, 0u, 0u, 0u, 0u}, 204};
// (t - 1) / 2 with q - 1 = 2^46 t (330 bits)
constexpr exp_t kRootExp377 = {{0x00010a11u, 0xba886000u, 0x90002e16u, 0xc45f7412u, 0x271e3de6u, 0xb3e601eau, 0x92763445u, 0x0b80d942u,
                                0x21d58c76u, 0x748c2f8au, 0x0000035cu, 0u}, 329};
// ... by the kernels' CURVE parameter
template <int CURVE> constexpr const exp_t& root_exp_of() { return CURVE == 1 ? kRootExp377 : kRootExpTe; }
TE_HD bool exp_bit(const exp_t& e, int i) {
  uint32_t r = 0;
  const int w = i >> 5;
#pragma unroll
  for (int k = 0; k < 12; k++) r = k == w ? e.w[k] : r;
  return (r >> (i & 31)) & 1u;
}

// per field: 2-adicity S, c6 = Z^t, c7 = Z^((t + 1) / 2) for the smallest non-square Z (11 mod p, 5 mod q), canonical words
template <int N> struct root_field;
template <> struct root_field<9> {
  static constexpr int S = 47, W = 8;
  static constexpr uint32_t c6[8] = {0xa623875cu, 0x726869aau, 0x4059d4cdu, 0xe5c1f1b8u, 0x8d4ff39bu, 0x480b0da0u, 0xb338db36u, 0x0f4f58d6u};
  static constexpr uint32_t c7[8] = {0x16212b4bu, 0xcce70cb6u, 0x60d36af1u, 0x359c9492u, 0x6054a6dbu, 0x81b2d614u, 0x27981a1au, 0x0f0808a3u};
};
template <> struct root_field<14> {
  static constexpr int S = 46, W = 12;
  static constexpr uint32_t c6[12] = {0x6b00bbe8u, 0xba6b5ef2u, 0xcc795186u, 0x1ea03d28u, 0x56228ac4u, 0xc6eaa2bcu, 0x7022110eu, 0xd14fcacau,
                                      0xaa914b0au, 0x8fe9dee6u, 0x99cdbc5du, 0x00382d3du};
  static constexpr uint32_t c7[12] = {0x428ffcf8u, 0x190e6a04u, 0x8aca3083u, 0x888d7ad5u, 0x9ca4f459u, 0x8a522d81u, 0x4928e7d9u, 0x85de7572u,
                                      0xbc0164c2u, 0x85502bb8u, 0x4ddd14ccu, 0x01603f9bu};
};
// (q + 1) / 2: y > q - y exactly when y >= (q + 1) / 2
constexpr uint32_t Q_HALF1_W32[12] = {0x00000001u, 0x42846000u, 0x18000000u, 0x0b85aea2u, 0xdd04a400u, 0x8f79b117u, 0x807a89c7u, 0x8d116cf9u,
                                      0x3650a49du, 0x631d82e0u, 0x0be28875u, 0x00d71d23u};

// canonical words <-> Montgomery form (any input below 2^256 / 2^384: w R^2 / R < 1.04 p, < 1.1 q)
TE_HD fel<9> fe_from_canon(const uint32_t (&w)[8]) { return mont_mul(fp_from_words32(w), fp_R2()); }
TE_HD fel<14> fe_from_canon(const uint32_t (&w)[12]) { return te377::mont_mul(te377::fq_from_words32(w), te377::fq_R2()); }
template <int N> TE_HD fel<N> fe_modulus() { if constexpr (N == 9) return fp_P(); else return te377::fq_Q(); }
// class N (value < 1.1 modulus)  ->  the canonical value as W little-endian words.  v / R (one product with the integer 1) is at
// most the modulus, which it equals only for 0: one conditional subtraction, with the borrow in the sign bit of each limb.
template <int N, int W> TE_HD void fe_to_canon(const fel<N>& a, uint32_t (&w)[W]) {
  fel<N> one = fe_zero<N>(); one.v[0] = 1u;
  const fel<N> t = fe_mul(a, one), m = fe_modulus<N>();
  fel<N> d;
  uint32_t br = 0;
#pragma unroll
  for (int i = 0; i < N; i++) { const uint32_t s = t.v[i] - m.v[i] - br; br = s >> 31; d.v[i] = s & LM; }
  const uint32_t keep = br ? 0xffffffffu : 0u;                     // t < modulus
  fel<N> c;
#pragma unroll
  for (int i = 0; i < N; i++) c.v[i] = mask_select(keep, t.v[i], d.v[i]);
#pragma unroll
  for (int j = 0; j < W; j++) {
    const int bit = 32 * j, i = bit / 29, s = bit % 29;
    uint32_t v = i < N ? c.v[i] >> s : 0u;
    if (i + 1 < N) v |= c.v[i + 1] << (29 - s);
    if (i + 2 < N && 58 - s < 32) v |= c.v[i + 2] << (58 - s);
    w[j] = v;
  }
}
// m - a for canonical a != 0 (words); 0 stays 0
template <int W> TE_HD void words_neg(const uint32_t (&a)[W], const uint32_t* m, uint32_t (&r)[W]) {
  uint32_t nz = 0;
#pragma unroll
  for (int i = 0; i < W; i++) nz |= a[i];
  uint64_t br = 0;
#pragma unroll
  for (int i = 0; i < W; i++) {
    const uint64_t s = (uint64_t)m[i] - a[i] - br;
    br = (s >> 63) & 1u;
    r[i] = nz ? (uint32_t)s : 0u;
  }
}

template <int N> TE_HD fel<N> fe_select(bool c, const fel<N>& a, const fel<N>& b) {     // c ? a : b
  const uint32_t m = c ? 0xffffffffu : 0u;
  fel<N> r;
#pragma unroll
  for (int i = 0; i < N; i++) r.v[i] = mask_select(m, a.v[i], b.v[i]);
  return r;
}
// two independent products: in lockstep where the field's registers allow it (9 limbs); one after the other with 14 limbs, where a
// lockstep pair pushes the kernel past 256 VGPRs into scratch
template <int N> TE_HD void fe_mul2(const fel<N>& a0, const fel<N>& b0, const fel<N>& a1, const fel<N>& b1, fel<N>& r0, fel<N>& r1) {
  if constexpr (fe_wide_ok<N>()) {
    const fel<N> a[2] = {a0, a1}, b[2] = {b0, b1};
    fel<N> o[2];
    fe_mul_x<2>(a, b, o);
    r0 = o[0]; r1 = o[1];
  } else {
    r0 = fe_mul(a0, b0); r1 = fe_mul(a1, b1);
  }
}
template <int N> TE_HD bool fe_is_one(const fel<N>& a) { return fe_is_zero(fe_sub<2>(a, fe_one<N>())); }
template <int N> TE_HD fel<N> fe_sqr_n(fel<N> a, int k) {           // a^(2^k), k uniform
#pragma unroll 1
  for (int i = 0; i < k; i++) a = fe_mul(a, a);
  return a;
}

// sqrt_ratio(u, v) (RATIO) or sqrt(u) (v = 1 dropped): returns whether u / v is a non-zero square; y = sqrt(u / v) then, else
// sqrt(Z u / v).  u, v: class N, values < 3.3 p / q (sums normalised).  y: class N, value < 1.1 p / q.
template <int N, bool RATIO> TE_HD bool fe_sqrt_ratio(const fel<N>& u, const fel<N>& v, const exp_t& e, fel<N>& y) {
  using F = root_field<N>;
  constexpr int S = F::S;
  fel<N> tv1 = fe_from_canon(F::c6), tv2, tv3, tv4, tv5;
  if constexpr (RATIO) {
    tv2 = v;                                                       // v^(2^S - 1)
#pragma unroll 1
    for (int k = 1; k < S; k++) { tv2 = fe_mul(tv2, tv2); tv2 = fe_mul(tv2, v); }
    tv3 = fe_mul(fe_mul(tv2, tv2), v);                             // v^(2^(S+1) - 1)
    tv5 = fe_mul(u, tv3);
  } else {
    tv5 = u;
  }
  {                                                                // tv5 ^ ((t - 1) / 2), the top bit is 1
    const fel<N> base = tv5;
#pragma unroll 1
    for (int i = e.top - 1; i >= 0; i--) {
      tv5 = fe_mul(tv5, tv5);
      if (exp_bit(e, i)) tv5 = fe_mul(tv5, base);
    }
  }
  if constexpr (RATIO) {
    tv5 = fe_mul(tv5, tv2);
    fe_mul2(tv5, v, tv5, u, tv2, tv3);                             // tv5 v, tv5 u
  } else {
    tv2 = tv5; tv3 = fe_mul(tv5, u);
  }
  tv4 = fe_mul(tv3, tv2);
  const bool is_qr = fe_is_one(fe_sqr_n(tv4, S - 1));
  {
    fel<N> o0, o1;
    fe_mul2(tv3, fe_from_canon(F::c7), tv4, tv1, o0, o1);
    tv3 = fe_select(is_qr, tv3, o0);
    tv4 = fe_select(is_qr, tv4, o1);
  }
#pragma unroll 1
  for (int i = S; i >= 2; i--) {
    const bool e1 = fe_is_one(fe_sqr_n(tv4, i - 2));
    fel<N> t31;
    fe_mul2(tv3, tv1, tv1, tv1, t31, tv1);                         // tv3 tv1, tv1^2
    tv5 = fe_mul(tv4, tv1);
    tv3 = fe_select(e1, tv3, t31);
    tv4 = fe_select(e1, tv4, tv5);
  }
  y = tv3;
  return is_qr;
}

// ---- Twisted-Edwards BLS12: x (8 words) -> x || y (16 words) -----------------------------------------------------------------
// 0 or TE_MSM_POINT_*; out is written either way (meaningless on a failure)
TE_HD int from_x_te(const uint32_t (&xw)[8], uint32_t (&out)[16], const exp_t& e, const naf_t& order) {
  const bool canon = words_lt<8>(xw, P_W32);
  const fp X = fe_from_canon(xw);
  const fp x2 = mont_mul(X, X);
  const fp u = fp_norm(fp_add(fp_R1(), x2));                       // 1 + x^2     (< 2.2 p)
  const fp v = fp_norm(fp_sub<2>(fp_R1(), mont_mul(x2, fp_D_MONT())));   // 1 - d x^2   (< 3.1 p)
  fp Y;
  const bool square = fe_sqrt_ratio<9, true>(u, v, e, Y) || fe_is_zero(u);
  const ete Q = mul_order_te(X, Y, order);
  const bool x0 = fe_is_zero(Q.x) && !fe_is_zero(Q.z);
  const bool is_o = x0 && fe_is_zero(fp_sub<2>(Q.y, Q.z));
  const bool is_t2 = x0 && fe_is_zero(fp_add(Q.y, Q.z));
  uint32_t yc[8], yn[8];
  fe_to_canon<9, 8>(Y, yc);
  words_neg<8>(yc, P_W32, yn);
#pragma unroll
  for (int i = 0; i < 8; i++) { out[i] = xw[i]; out[8 + i] = is_t2 ? yn[i] : yc[i]; }
  return !canon ? 1 : (!square ? 2 : ((is_o || is_t2) ? 0 : 3));
}

// ---- BLS12-377 G1: x with flags (12 words) -> x || y (24 words) ------------------------------------------------------------
TE_HD int from_x_377(const uint32_t (&xw)[12], uint32_t (&out)[24], const exp_t& e) {
  using namespace te377;
  const uint32_t top = xw[11];
  const bool larger = (top >> 31) & 1u, infinity = (top >> 30) & 1u, reserved = (top >> 25) & 0x1fu;
  uint32_t xc[12];
#pragma unroll
  for (int i = 0; i < 12; i++) xc[i] = i == 11 ? top & 0x01ffffffu : xw[i];       // bits 0 .. 376
  const bool canon = !reserved && words_lt<12>(xc, Q_W32);
  const fq xl = fq_from_words32(xc);
  const fq a[2] = {xl, xl}, b[2] = {fq_R2(), fq_S_R2()};
  fq o2[2];
  fe_mul_x<2>(a, b, o2);                                          // x, s x   (Montgomery form, as c377_coords)
  const fq X = o2[0];
  // check_form_377's "defined" before the root (only a flag stays live across it): w = s x + s + 1 != 0 here, y != 0 below
  const bool w_zero = fe_is_zero(fq_norm(fq_add(o2[1], fq_SP1_MONT())));
  const fq u = fq_norm(fq_add(te377::mont_mul(te377::mont_mul(X, X), X), fq_R1()));   // x^3 + 1   (< 2.2 q)
  fq Y;
  const bool square = fe_sqrt_ratio<14, false>(u, u, e, Y);       // false for u = 0 as well: y = 0, undefined map, reason 2 either way
  uint32_t yc[12], yn[12];
  fe_to_canon<14, 12>(Y, yc);
  words_neg<12>(yc, Q_W32, yn);
  const bool take_yc = larger == !words_lt<12>(yc, Q_HALF1_W32);  // the flag asks for the larger root, and yc is the larger one
#pragma unroll
  for (int i = 0; i < 12; i++) { out[i] = xc[i]; out[12 + i] = take_yc ? yc[i] : yn[i]; }
  // the curve equation holds (a root exists) and y != 0 (u != 0, a square): check_form_377's verdict is 2 exactly when this is
  return !canon ? 1 : ((infinity || !square || w_zero) ? 2 : 0);
}

#if defined(__HIPCC__)
// one lane per x-coordinate of a piece [base, base + m) of n; out holds the piece's points.  The report word is check_code over the
// whole buffer (n, base + i): pieces may share one word, the lowest index wins.  No early exit: a wave's instructions are uniform.
template <int CURVE> __global__ __launch_bounds__(256) void k_points_from_x(const uint4* __restrict__ xs, uint32_t m, uint4* __restrict__ out,
                                                                            unsigned long long* word, uint64_t n, uint64_t base, exp_t e, naf_t order) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int XQ = CURVE == 1 ? 3 : 2, PQ = 2 * XQ;               // 16-byte words of one x / one point
  constexpr int XW = 4 * XQ;
  uint32_t xw[XW], o[2 * XW];
#pragma unroll
  for (int k = 0; k < XQ; k++) { const uint4 v = xs[(size_t)i * XQ + k]; xw[4 * k] = v.x; xw[4 * k + 1] = v.y; xw[4 * k + 2] = v.z; xw[4 * k + 3] = v.w; }
  int reason;
  if constexpr (CURVE == 1) reason = from_x_377(xw, o, e);
  else reason = from_x_te(xw, o, e, order);
#pragma unroll
  for (int k = 0; k < PQ; k++) out[(size_t)i * PQ + k] = make_uint4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
  if (reason) atomicMax(word, (unsigned long long)check_code(n, base + i, reason));
}
#endif

}  // namespace te
