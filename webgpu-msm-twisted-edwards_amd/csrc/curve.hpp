// curve.hpp -- point arithmetic on a twisted Edwards curve -x^2 + y^2 = 1 + d x^2 y^2 (a = -1) over fel<N>:
//   N = 9   the Twisted-Edwards BLS12 curve of the competition, d = 3021 (reference/params/AleoConstants.ts:2-4,
//           reference/utils/FieldMath.ts:104-137)
//   N = 14  BLS12-377 G1 in its twisted-Edwards form (BASELINE config 5; the reference has no code for this curve,
//           README.md:57-73,279-287).  d = -(A - 2) / (A + 2) for the Montgomery form of y^2 = x^3 + 1 (tools/gen_constants.py);
//           d is a square there, so the addition law is complete on the subgroup of odd prime order r only -- where MSM
//           inputs live -- not on the cofactor part.
//
// Replaces add_points / double_point / negate_point of the reference (wgsl/curve/ec.template.wgsl:7-66,
// wgsl/cuzk/smvp.template.wgsl:47-56).  The reference adds two full extended points with add-2008-hwcd (10 field products
// + T = x*y recomputed per gathered point, smvp.template.wgsl:107-108).  Here the n input points are converted ONCE into a
// RECORD and bucket accumulation is a 7-product (N = 9: affine record) or 8-product (N = 14: projective record, no
// inversion in the conversion) addition with no reduction modulo p at all (limb-magnitude rules in fp.hpp / fq377.hpp).
// Any correct group law gives the same affine result, which is the only thing compared with the reference.
#pragma once
#include "field.hpp"

namespace te {

// Extended twisted Edwards accumulator (X : Y : Z : T), x = X/Z, y = Y/Z, T = XY/Z.
// Every coordinate is a product output: limb class N, value < 1.1p.  4 N words, x | y | z | t.
template <int N> struct ete_t { fel<N> x, y, z, t; };
using ete = ete_t<9>;            // 144 bytes

// Record of an input point, up to a common factor of its coordinates (projectively the result of an addition does not
// depend on it):  hm ~ (Y - X)/2,  hp ~ (Y + X)/2,  dt ~ -d T,  z ~ Z  of the extended point (X : Y : Z : T).
//   N = 9 : affine, z = 1 is not stored: ((y-x)/2, (y+x)/2, -d*x*y), 27 words in a 128-byte slot.
//   N = 14: projective (converted from short Weierstrass without a division, see pnt_from_sw377): 56 words = 224 bytes.
// Products of class N, values < 1.1p; a negated record holds 4p - dt with limbs < 2^30.6.
// dt carries the MINUS sign so that F = D' + C' below is a sum and no product meets two differences.
template <int N> struct pnt_t;
template <> struct pnt_t<9> { fel<9> hm, hp, dt; };
template <> struct pnt_t<14> { fel<14> hm, hp, dt, z; };
using pnt = pnt_t<9>;
// BLS12-377 G1, AFFINE record of a BOUND point set (te_msm_bind_points: the conversion is paid once, so its one inversion per
// point -- Montgomery's trick, k_affine377 -- costs nothing per MSM): the projective record divided by its z,
// ((y-x)/2, (y+x)/2, -d x y) of the Edwards point like pnt_t<9>, z = 1 not stored.  42 words = 168 bytes instead of 224, and
// an addition of 7 products instead of 8 (ete_madd below).  Products of class N, values < 1.1q.
struct pnt_aff377 { fel<14> hm, hp, dt; };

template <int N> TE_HD ete_t<N> ete_identity_t() { ete_t<N> r; r.x = fe_zero<N>(); r.y = fe_one<N>(); r.z = fe_one<N>(); r.t = fe_zero<N>(); return r; }
TE_HD ete ete_identity() { return ete_identity_t<9>(); }

// -(x, y) = (-x, y): swaps hm and hp, negates dt.  The selection is bitwise under a per-lane mask: gfx950 does
// (b & m) | (a & ~m) in one v_bitop3_b32 at full rate (2.7 cycles per wave, tools/ubench); v_cndmask_b32 and v_bfi_b32
// cost 4.3.
TE_HD uint32_t mask_select(uint32_t m, uint32_t b, uint32_t a) {          // m ? b : a, bit by bit
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_bitop3_b32(m, b, a, 0xCA);
#else
  return (b & m) | (a & ~m);
#endif
}
template <int N> TE_HD pnt_t<N> pnt_cneg(const pnt_t<N>& a, bool neg) {
  pnt_t<N> r = a; const fel<N> ndt = fe_neg<4>(a.dt);
  const uint32_t m = neg ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < N; i++) {
    r.hm.v[i] = mask_select(m, a.hp.v[i], a.hm.v[i]);
    r.hp.v[i] = mask_select(m, a.hm.v[i], a.hp.v[i]);
    r.dt.v[i] = mask_select(m, ndt.v[i], a.dt.v[i]);
  }
  return r;
}

TE_HD pnt_aff377 pnt_cneg(const pnt_aff377& a, bool neg) {
  pnt_aff377 r = a; const fel<14> ndt = fe_neg<4>(a.dt);
  const uint32_t m = neg ? 0xffffffffu : 0u;
#pragma unroll
  for (int i = 0; i < 14; i++) {
    r.hm.v[i] = mask_select(m, a.hp.v[i], a.hm.v[i]);
    r.hp.v[i] = mask_select(m, a.hm.v[i], a.hp.v[i]);
    r.dt.v[i] = mask_select(m, ndt.v[i], a.dt.v[i]);
  }
  return r;
}

// Affine (x, y) as plain integers (class N, ANY 256-bit value) -> record, in three products and a small-constant pass:
//   hm = (y - x + 16p) * (R^2/2) / R,   hp = (y + x) * (R^2/2) / R     (Montgomery forms of (y - x)/2 and (y + x)/2),
//   then hp + hm = y R and hm - hp = -x R, so  (hp + hm) (hm - hp + 2p) / R = -x y R,  and  dt = d * (-x y R)  (fp_mul_d, two
//   multiply-accumulates per limb instead of the fourth product by -d R^3 of rounds 1-6).
// The constant folds the conversion to Montgomery form and the halving into the first two products (16p > 2^256 keeps y - x
// non-negative for non-canonical inputs).  Limb classes: hp + hm is S, hm - hp + 2p is D (S x D is exact, fp.hpp).  Values: hm, hp
// < 1.07p; the third product is below 2.14p * 3.07p / R + p < 1.02p, and dt < 1.0001p.
// MONT (option "points_montgomery", bind time only): x and y are the caller's Montgomery residues x R_a, R_a = 2^256, again ANY 256-bit
// value; the constant becomes R^2 / R_a / 2 and the products give the same (y -+ x) R / 2.  Every bound above carries over unchanged: they
// use of the inputs only "below 2^256, limbs of class N" and of the constant only "a canonical residue (< p) in class N" -- both still
// hold, so hm, hp < 1.07p as before and everything behind the first two products sees the same classes and ranges.
template <bool MONT = false> TE_HD pnt pnt_from_affine_raw(const fp& x, const fp& y) {
  const fp k = MONT ? fp_R2_HALF_A() : fp_R2_HALF();
  const fp a[2] = {fp_sub<16>(y, x), fp_add(y, x)}, b[2] = {k, k};
  fp o[2];
  mont_mul_x<2>(a, b, o);
  pnt r;
  r.hm = o[0]; r.hp = o[1];
  r.dt = fp_mul_d(mont_mul(fp_add(o[1], o[0]), fp_sub<2>(o[0], o[1])));
  return r;
}

// BLS12-377 G1: short-Weierstrass affine (x, y) as plain integers (class N, any 384-bit value) -> projective twisted-Edwards
// record, 8 products and no division.  With s = 1/sqrt(3), f = sqrt(-(A+2)/B) (tools/gen_constants.py):
//   Montgomery  u = s (x + 1), v = s y;   Edwards  X = f u / v = f (x + 1) / y,   Y = (u - 1)/(u + 1) = (s x + s - 1)/(s x + s + 1).
//   With a = f (x + 1), b = s x + s - 1, w = s x + s + 1:  X = a / y, Y = b / w, and the extended point is simply
//   (X : Y : Z : T) = (a w : b y : y w : a b)   (X Y / Z = a b).
//   record, times 2:  hm = Y - X,  hp = Y + X,  dt = -2 d T,  z = 2 Z.
// Undefined (all-zero record, the neutral element's weight is lost) for y = 0 or w = 0: points of order 2 and 4, never in G1.
// MONT (option "points_montgomery", bind time only): x and y are x R_a, R_a = 2^384 (any 384-bit value); the three constants of the first
// products carry 1 / R_a and o1 is s x, y, f x in the engine's Montgomery form exactly as before.  The inputs are still "below 2^384, class
// N" and the constants still canonical residues (< q) in class N, so o1 has the bounds it had; the constants added to o1 and the last
// product's act on the engine's own Montgomery values and stay.
template <bool MONT = false> TE_HD pnt_t<14> pnt_from_sw377(const fel<14>& x, const fel<14>& y) {
  using namespace te377;
  const fq a1[3] = {x, y, x}, b1[3] = {MONT ? fq_S_R2_A() : fq_S_R2(), MONT ? fq_R2_A() : fq_R2(), MONT ? fq_F_R2_A() : fq_F_R2()};
  fq o1[3];
  fe_mul_x<3>(a1, b1, o1);                                   // s x, y, f x   (Montgomery form, class N)
  const fq w = fe_norm(fe_add(o1[0], fq_SP1_MONT())), bb = fe_add(o1[0], fq_SM1_MONT()), aa = fe_norm(fe_add(o1[2], fq_F_MONT()));
  const fq a2[4] = {w, o1[1], o1[1], aa}, b2[4] = {aa, bb, w, bb};
  fq o2[4];
  fe_mul_x<4>(a2, b2, o2);                                   // X = a w,  Y = b y,  Z = y w,  T = a b
  pnt_t<14> r;
  r.hm = fe_norm(fe_sub<2>(o2[1], o2[0]));
  r.hp = fe_norm(fe_add(o2[1], o2[0]));
  r.z = fe_norm(fe_add(o2[2], o2[2]));
  r.dt = fe_mul(o2[3], fq_NEG_2D_MONT());
  return r;
}

// The neutral element (X : Y : Z : T) = (0 : 1 : 1 : 0) as a record of the form above (times 2: hm = Y - X, hp = Y + X, dt = -2 d T,
// z = 2 Z): (1, 1, 0, 2) in Montgomery form -- what a point flagged "at infinity" converts to (option "point_infinity_flag").  Its affine
// record is (hm / z, hp / z, dt / z) = (1/2, 1/2, 0): k_affine377's shared inversion handles it like any other record (z = 2 is a unit).
TE_HD pnt_t<14> pnt_identity377() {
  pnt_t<14> r;
  r.hm = r.hp = fe_one<14>();
  r.dt = fe_zero<14>();
  r.z = fe_norm(fe_add(fe_one<14>(), fe_one<14>()));
  return r;
}

// the four closing products of every addition: (X3, Y3, T3, Z3) = (E F, H G, E H, G F) with E, G differences (offset form)
// and H, F sums.  N = 9: every product is "difference x sum", 9 * 2^30.6 * 2^30 + 8 * 2^58 = 0.9 * 2^64: nothing is
// normalised.  N = 14: one operand of every product must be normalised -- E and G are.
template <int N> TE_HD ete_t<N> ete_close(const fel<N>& E, const fel<N>& H, const fel<N>& F, const fel<N>& G) {
  const fel<N> En = fe_norm_if_needed(E), Gn = fe_norm_if_needed(G);
  const fel<N> l[4] = {En, H, En, Gn}, rr[4] = {F, Gn, H, F};
  fel<N> o[4];
  fe_mul_x<4>(l, rr, o);
  ete_t<N> r;
  r.x = o[0]; r.y = o[1]; r.t = o[2]; r.z = o[3];
  return r;
}

// Mixed addition acc + b with an affine record, 7 products, unified and complete (a = -1 is a square, d is not).
// With A' = (Y1-X1)(y2-x2)/2, B' = (Y1+X1)(y2+x2)/2:  E = B'-A' = X1 y2 + Y1 x2,
// H = B'+A' = Y1 y2 + X1 x2, C = d T1 x2 y2, F = Z1 - C, G = Z1 + C;  (X3,Y3,T3,Z3) = (EF, HG, EH, GF).
// The record holds -d x2 y2, so the product below is C' = -C and F = Z1 + C' is a SUM, G = Z1 - C' the difference.
//
// The accumulator enters the addition OPENED: (U, V, Z, T) with U = Y1 - X1 (offset form, + 2p) and V = Y1 + X1, the first operands
// of A' and B' -- ete_open, 27 limb operations right behind the closing products of the addition before.  In this form the NEGATIVE
// of the accumulator is cheap: -(X, Y) = (-X, Y) swaps U and V and negates T (ete_uv_neg: 2p - T in offset form), and that is how
// k_accumulate subtracts a point: Q - P = -((-Q) + P).  A lane keeps a flag "my accumulator stands for its negative", negates the
// opened accumulator only where an entry's sign differs from the flag, and ALWAYS adds the record as loaded (no pnt_cneg, whose 9
// subtractions and 27 selects every entry paid).
// Limb classes: U is D (limbs < 2^30.6), V is S (< 2^30) -- or the other way round behind a negation -- and T is N or, negated,
// 2p - T with limbs < 2^30 (T is a product output below 1.1p < 2p); each meets a record field, class N ALWAYS (no negated dt any
// more): D x N, S x N, (< 2^30) x N, the pairings of the addition so far with the wide operand on the accumulator's side.  Every
// addition closes into fresh product outputs (class N, below 1.1p), so nothing accumulates from one negation to the next, and
// with 14 limbs the rule "one operand of every product normalised" is met by the record.  E and G are D, H and F are S as before.
// Values: everything is below 5p before a product and below 1.1p after it; nothing is reduced mod p.
template <int N> struct ete_uv_t { fel<N> u, v, z, t; };
template <int N> TE_HD ete_uv_t<N> ete_open(const ete_t<N>& a) {
  ete_uv_t<N> r;
  r.u = fe_sub<2>(a.y, a.x); r.v = fe_add(a.y, a.x); r.z = a.z; r.t = a.t;
  return r;
}
// the opened form of -a.  Twice in a row (not what k_accumulate does: an addition stands between two negations) gives u, v and
// t back limb for limb: 2p - (2p - t) in offset form has no borrow.
// In place, and on the device the swap is v_swap_b32 by name: written as two assignments the compiler copies U to nine more
// registers in FRONT of the branch (nine moves that every addition pays, and 168 VGPRs with spills instead of 138).
template <int N> TE_HD void ete_uv_neg(ete_uv_t<N>& a) {
#pragma unroll
  for (int i = 0; i < N; i++) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm("v_swap_b32 %0, %1" : "+v"(a.u.v[i]), "+v"(a.v.v[i]));
#else
    const uint32_t w = a.u.v[i]; a.u.v[i] = a.v.v[i]; a.v.v[i] = w;
#endif
  }
  a.t = fe_neg<2>(a.t);
}
// What a lane STORES is the sum itself, never its negative, and always four fresh product outputs (class N, below 1.1p -- the form
// the buckets and seg_out have always had; 2p - X carried into class N would be a value up to 2p, whose top limb the offset of the
// next fe_sub<2> does not cover).  The negation rides on the segment's LAST addition instead: (X3, Y3, T3, Z3) = (E F, H G, E H, G F),
// so -(X3, Y3) = (-X3 : Y3 : Z3 : -T3) is the same closing with -E = A' - B' in the place of E = B' - A'.  SGN = true variants of the
// additions and segment starts below take that choice per lane (`neg`): the operands of the one subtraction are selected under a
// mask, 2 N selects, once or twice per segment; E has the same class and range either way (A' and B' are both class N below 1.1p).
template <bool SGN, int N> TE_HD fel<N> fe_diff(const fel<N>& b, const fel<N>& a, bool neg) {          // b - a, or a - b where neg
  if constexpr (!SGN) return fe_sub<2>(b, a);
  else {
    const uint32_t m = neg ? 0xffffffffu : 0u;
    fel<N> hi, lo;
#pragma unroll
    for (int i = 0; i < N; i++) { hi.v[i] = mask_select(m, a.v[i], b.v[i]); lo.v[i] = mask_select(m, b.v[i], a.v[i]); }
    return fe_sub<2>(hi, lo);
  }
}
template <bool SGN = false> TE_HD ete ete_madd_raw(const ete_uv_t<9>& a, const pnt& b, bool neg = false) {
  const fp in1[3] = {a.u, a.v, a.t}, in2[3] = {b.hm, b.hp, b.dt};
  fp abc[3];
  mont_mul_x<3>(in1, in2, abc);
  const fp &A = abc[0], &B = abc[1], &Cn = abc[2];
  return ete_close<9>(fe_diff<SGN, 9>(B, A, neg), fp_add(B, A), fp_add(a.z, Cn), fp_sub<2>(a.z, Cn));
}
// The same with a projective record: D' = Z1 z2 takes the place of Z1 -- 8 products.
template <bool SGN = false> TE_HD ete_t<14> ete_madd_raw(const ete_uv_t<14>& a, const pnt_t<14>& b, bool neg = false) {
  const fel<14> in1[4] = {a.u, a.v, a.t, a.z}, in2[4] = {b.hm, b.hp, b.dt, b.z};
  fel<14> p[4];
  fe_mul_x<4>(in1, in2, p);
  const fel<14> &A = p[0], &B = p[1], &Cn = p[2], &D = p[3];
  return ete_close<14>(fe_diff<SGN, 14>(B, A, neg), fe_add(B, A), fe_add(D, Cn), fe_sub<2>(D, Cn));
}
// BLS12-377 with an AFFINE record (bound bases): the 7-product form of the other curve under the 14-limb rule -- one operand of
// every product normalised: the record's coordinates are, E and G are normalised by ete_close; F = Z1 + C' is a sum of two product
// outputs (limbs < 2^30), H likewise.
template <bool SGN = false> TE_HD ete_t<14> ete_madd_raw(const ete_uv_t<14>& a, const pnt_aff377& b, bool neg = false) {
  const fel<14> in1[3] = {a.u, a.v, a.t}, in2[3] = {b.hm, b.hp, b.dt};
  fel<14> p[3];
  fe_mul_x<3>(in1, in2, p);
  const fel<14> &A = p[0], &B = p[1], &Cn = p[2];
  return ete_close<14>(fe_diff<SGN, 14>(B, A, neg), fe_add(B, A), fe_add(a.z, Cn), fe_sub<2>(a.z, Cn));
}
// acc + b from the closed form (X : Y : Z : T); b may be a record negated by pnt_cneg (its dt then has limbs < 2^30.6 and meets T1,
// class N)
TE_HD ete ete_madd(const ete& a, const pnt& b) { return ete_madd_raw(ete_open<9>(a), b); }
TE_HD ete_t<14> ete_madd(const ete_t<14>& a, const pnt_t<14>& b) { return ete_madd_raw(ete_open<14>(a), b); }
TE_HD ete_t<14> ete_madd(const ete_t<14>& a, const pnt_aff377& b) { return ete_madd_raw(ete_open<14>(a), b); }

// neutral element + b without the products whose result is known: with (X1 : Y1 : Z1 : T1) = (0 : 1 : 1 : 0) the mixed addition
// has A' = hm, B' = hp, C' = 0, D' = z2, i.e. (X3, Y3, T3, Z3) = (E z2, H z2, E H, z2^2) with E = hp - hm, H = hp + hm: three
// products for an affine record (z2 = 1: E and H only pass through a product by one to become class N below 2p), four for a
// projective one, instead of 7 / 8.  k_accumulate starts a segment of ONE entry with this step, and every segment of projective
// records (ete_from_pair below); k_fb_ext_from_recs converts whole point sets with it.
template <bool SGN = false> TE_HD ete ete_from_pnt(const pnt& b, bool neg = false) {
  const fp one = fp_R1();
  const fp E = fe_diff<SGN, 9>(b.hp, b.hm, neg), H = fp_add(b.hp, b.hm);
  const fp l[3] = {E, H, E}, rr[3] = {one, one, H};
  fp o[3];
  mont_mul_x<3>(l, rr, o);
  ete r;
  r.x = o[0]; r.y = o[1]; r.t = o[2]; r.z = one;
  return r;
}
template <bool SGN = false> TE_HD ete_t<14> ete_from_pnt(const pnt_t<14>& b, bool neg = false) {
  const fel<14> En = fe_norm(fe_diff<SGN, 14>(b.hp, b.hm, neg)), H = fe_add(b.hp, b.hm);
  const fel<14> l[4] = {En, H, En, b.z}, rr[4] = {b.z, b.z, H, b.z};
  fel<14> o[4];
  fe_mul_x<4>(l, rr, o);
  ete_t<14> r;
  r.x = o[0]; r.y = o[1]; r.t = o[2]; r.z = o[3];
  return r;
}

template <bool SGN = false> TE_HD ete_t<14> ete_from_pnt(const pnt_aff377& b, bool neg = false) {          // z2 = 1: (E, H, E H, 1), three products
  const fel<14> one = fe_one<14>();
  const fel<14> En = fe_norm(fe_diff<SGN, 14>(b.hp, b.hm, neg)), H = fe_add(b.hp, b.hm);
  const fel<14> l[3] = {En, H, En}, rr[3] = {one, one, H};
  fel<14> o[3];
  fe_mul_x<3>(l, rr, o);
  ete_t<14> r;
  r.x = o[0]; r.y = o[1]; r.t = o[2]; r.z = one;
  return r;
}

// a + b of two RECORDS: the first two entries of a segment of k_accumulate, in 1 + 7 products instead of the 3 + 7 of
// ete_madd(ete_from_pnt(a), b).  ete_from_pnt's X1 = E 1 and Y1 = H 1 (E = hp1 - hm1, H = hp1 + hm1) are products by one whose only
// purpose is to bring E and H into class N for the next addition's Y1 - X1 and Y1 + X1 -- which are H - E = 2 hm1 and H + E = 2 hp1
// of the record itself.  So with T1 = E H (the one real product of the conversion) and Z1 = 1 the mixed addition opens with
//   A' = (2 hm1) hm2,   B' = (2 hp1) hp2,   C' = T1 dt2
// and closes as ete_madd does with a.z = 1: F = 1 + C', G = 1 - C'.  Unified and complete like ete_madd (b = a, b = -a and the
// neutral element as either operand are ordinary inputs); a's dt is not used.  The result is congruent mod p, coordinate by
// coordinate, to ete_madd(ete_from_pnt(a), b).
// Limb classes (N = 9): E = fp_sub<2>(hp1, hm1) is D (hm1 is a record field: class N, value < 1.1p < 2p), H is S, T1 = H x E is S x D
// (the pairing of pnt_from_affine_raw); 2 hm1 and 2 hp1 are S and meet the class-N hm2, hp2; T1 (N) meets dt2 (N, or limbs < 2^30.6
// when b is negated); 1 is class N, so F is S and G is D as in ete_madd, and ete_close sees what it sees there.  Output: class N.
// Values: E < 3.1p, H < 2.2p, T1 < 1.02p; 2 hm1, 2 hp1 < 2.2p; A', B', C' < 1.02p; E3, G < 3.1p, H3, F < 2.1p; outputs < 1.02p.
template <bool SGN = false> TE_HD ete ete_from_pair(const pnt& a, const pnt& b, bool neg = false) {
  const fp one = fp_R1();
  const fp T1 = mont_mul(fp_add(a.hp, a.hm), fp_sub<2>(a.hp, a.hm));
  const fp in1[3] = {fp_add(a.hm, a.hm), fp_add(a.hp, a.hp), T1}, in2[3] = {b.hm, b.hp, b.dt};
  fp abc[3];
  mont_mul_x<3>(in1, in2, abc);
  const fp &A = abc[0], &B = abc[1], &Cn = abc[2];
  return ete_close<9>(fe_diff<SGN, 9>(B, A, neg), fp_add(B, A), fp_add(one, Cn), fp_sub<2>(one, Cn));
}
// The same for the affine BLS12-377 record under the 14-limb rule (one operand of every product normalised): E is normalised before
// it meets H (as in ete_from_pnt); the second record's fields are class N (a negated dt, limbs < 2^30.6, meets T1, class N) and meet
// the sums 2 hm1, 2 hp1 (limbs < 2^30); ete_close normalises E3 and G.  Values as above with q for p.
template <bool SGN = false> TE_HD ete_t<14> ete_from_pair(const pnt_aff377& a, const pnt_aff377& b, bool neg = false) {
  const fel<14> one = fe_one<14>();
  const fel<14> T1 = fe_mul(fe_add(a.hp, a.hm), fe_norm(fe_sub<2>(a.hp, a.hm)));
  const fel<14> in1[3] = {fe_add(a.hm, a.hm), fe_add(a.hp, a.hp), T1}, in2[3] = {b.hm, b.hp, b.dt};
  fel<14> p[3];
  fe_mul_x<3>(in1, in2, p);
  const fel<14> &A = p[0], &B = p[1], &Cn = p[2];
  return ete_close<14>(fe_diff<SGN, 14>(B, A, neg), fe_add(B, A), fe_add(one, Cn), fe_sub<2>(one, Cn));
}
// The projective BLS12-377 record keeps the rule it had, 4 + 8 products.  With z1 != 1 the shortcut does not exist: Y1 - X1 of the
// converted point is 2 hm1 z1, a product in its own right, and forming the addition from the two records directly (A' = hm1 hm2,
// B' = hp1 hp2, D' = z1 z2) leaves C' = d T1 T2 to be had from dt1 dt2 = d^2 T1 T2 -- a product by 1/d, and one by 1/2 to put D' on
// the records' common scale: 6 + 4 against 12, for a record kind that only per-call BLS12-377 MSMs use (bound point sets gather the
// affine record above), with two constants and a limb-bound analysis of their own.  Not taken.
template <bool SGN = false> TE_HD ete_t<14> ete_from_pair(const pnt_t<14>& a, const pnt_t<14>& b, bool neg = false) {
  return ete_madd_raw<SGN>(ete_open<14>(ete_from_pnt(a)), b, neg);
}

// Full addition a + b of two accumulators (add-2008-hwcd-3 shape, k = 2d), 9 products.
// One operand of the opening product of two differences and F are normalised, so that no product sees two wide operands:
// with F of class N the closing products are E F (difference x N), H G (sum x sum-of-a-sum, limbs 2^30 x 2^30.6: the same
// "difference x sum" column bound as the mixed addition, 0.97 * 2^64 in tests/test_limb_bounds_te.py), E H and F G.  With 14
// limbs one operand of EVERY product must be normalised: E and G are as well.  (Until round 4 all three were normalised for
// N = 9 too: two carry chains of 27 dependent instructions per addition that nothing needed.)
template <int N> TE_HD ete_t<N> ete_add(const ete_t<N>& a, const ete_t<N>& b) {
  const fel<N> in1[4] = {fe_norm(fe_sub<2>(a.y, a.x)), fe_norm_if_needed(fe_add(a.y, a.x)), a.t, a.z};
  const fel<N> in2[4] = {fe_sub<2>(b.y, b.x), fe_add(b.y, b.x), b.t, b.z};
  fel<N> p1[4];
  fe_mul_x<4>(in1, in2, p1);
  const fel<N> &A = p1[0], &B = p1[1];
  const fel<N> C = fe_mul_k2d(p1[2]);                 // N = 9: the 13-bit constant applied limb-wise, not a product
  const fel<N> D = fe_add(p1[3], p1[3]);
  const fel<N> E = fe_norm_if_needed(fe_sub<2>(B, A));
  const fel<N> H = fe_add(B, A);
  const fel<N> F = fe_norm(fe_sub<2>(D, C));
  const fel<N> G = fe_norm_if_needed(fe_add(D, C));
  const fel<N> l[4] = {E, H, E, F}, rr[4] = {F, G, H, G};
  fel<N> o[4];
  fe_mul_x<4>(l, rr, o);
  ete_t<N> r;
  r.x = o[0]; r.y = o[1]; r.t = o[2]; r.z = o[3];
  return r;
}

}  // namespace te
