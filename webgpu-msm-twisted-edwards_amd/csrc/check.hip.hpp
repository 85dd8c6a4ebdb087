// check.hip.hpp -- validation of input points (option "check_points", te_msm_check_points; include/te_msm.h).
//
// Two verdicts per point, each a pure function of the point's wire bytes, so that the CPU build (tests/csrc/pointcheck.cpp)
// runs the exact code of the kernels:
//   form       both coordinates canonical (a word compare against p / q, no arithmetic), the curve equation holds, and --
//              BLS12-377 only -- the engine's map to the twisted-Edwards form is defined (pnt_from_sw377: Z = 2 y w != 0)
//   subgroup   [order] P = O with the order a compile-time constant, in signed digits (NAF): every lane runs the same chain
// The reason codes are TE_MSM_POINT_* of include/te_msm.h: 1 non-canonical, 2 off the curve / map undefined, 3 outside the subgroup.
//
// THE GROUP LAWS OF THE SUBGROUP CHAIN.  The input is not known to lie in the subgroup -- that is the question -- so the law
// must be complete on the whole curve E(F), cofactor part included:
//   Twisted-Edwards BLS12: -x^2 + y^2 = 1 + d x^2 y^2 with a = -1 a square and d = 3021 a non-square mod p.  By Bernstein-Lange
//     (and Hisil-Wong-Carter-Dawson for the extended coordinates) the unified addition is then complete on all of E(F_p): the
//     engine's own ete_add (curve.hpp) serves as it is, doubling included.
//   BLS12-377 G1: the engine's twisted-Edwards form has a SQUARE d -- its law is complete on the subgroup of order r only, and
//     the map from y^2 = x^3 + 1 is undefined at the points of order 2 and 4.  The chain therefore stays on the short-Weierstrass
//     curve, in projective (X : Y : Z) with the complete formulas of Renes-Costello-Batina 2016 for a = 0 (their algorithms 7
//     and 9, b3 = 3).  Their exceptional pairs need a difference of order 2; a chain over a point of G1 (odd order r) never meets
//     one.  A chain that does meet one turns into (0 : 0 : 0) and stays there -- the test below demands Y != 0 as well as Z = 0,
//     so such a point is rejected, which is right: it is not in G1.
#pragma once
#include "curve.hpp"
#include "strided.hip.hpp"

namespace te {

// NAF digits of an order: bit i of pos / neg is digit +1 / -1 at 2^i; top = index of the leading digit (always +1)
struct naf_t { uint32_t pos[8], neg[8]; int top; };
// L = 2111115437357092606062206234695386632838870926408408195193685246394721360383 (251 bits, 133 ones; 88 non-zero digits)
constexpr naf_t kNafTeOrder = {{0x04400200u, 0x020000a0u, 0x04409000u, 0x52942400u, 0x20100000u, 0x20411448u, 0x28902a00u, 0x05000200u},
                               {0x41002801u, 0x48a51205u, 0x40040501u, 0x00008050u, 0x89021400u, 0x88140100u, 0x820500aau, 0x005528a8u}, 250};
// r = 8444461749428370424248824938781546531375899335154063827935233455917409239041 (253 bits, 88 ones; 69 non-zero digits)
constexpr naf_t kNaf377Order = {{0x00000001u, 0x0a120000u, 0x10000001u, 0x022a8000u, 0x80400002u, 0x81045120u, 0xa240a800u, 0x14000800u},
                                {0x00000000u, 0x00008000u, 0x40000000u, 0xa8800901u, 0x24085000u, 0x20500402u, 0x081402aau, 0x0154a2a2u}, 252};
// ... by the kernels' CURVE parameter (0 Twisted-Edwards BLS12, 1 BLS12-377 G1): what a launch passes beside k_*<CURVE>
template <int CURVE> constexpr const naf_t& order_naf_of() { return CURVE == 1 ? kNaf377Order : kNafTeOrder; }

// word w of a, w uniform: a chain of selects instead of a dynamically indexed array (which would live in scratch memory)
TE_HD uint32_t naf_word(const uint32_t (&a)[8], int w) {
  uint32_t r = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) r = k == w ? a[k] : r;
  return r;
}
// digit at 2^i: +1, -1 or 0
TE_HD int naf_digit(const naf_t& k, int i) {
  const uint32_t b = 1u << (i & 31);
  return (naf_word(k.pos, i >> 5) & b) ? 1 : ((naf_word(k.neg, i >> 5) & b) ? -1 : 0);
}

// a < m for little-endian K-word integers
template <int K> TE_HD bool words_lt(const uint32_t* a, const uint32_t* m) {
  bool lt = false, decided = false;
#pragma unroll
  for (int i = K - 1; i >= 0; i--) {
    if (!decided && a[i] != m[i]) { lt = a[i] < m[i]; decided = true; }
  }
  return lt;
}

// v == 0 mod the field's modulus, for limbs below 2^30.6 and values far below R: v / R (one product with the integer 1) is below
// 2 p and a multiple of p exactly when v is -- 0 or p, both in class N, compared limb by limb
TE_HD bool fe_is_zero(const fp& v) {
  fp one = fp_zero(); one.v[0] = 1u;
  const fp t = mont_mul(v, one), p = fp_P();
  bool z = true, e = true;
#pragma unroll
  for (int i = 0; i < 9; i++) { z = z && t.v[i] == 0u; e = e && t.v[i] == p.v[i]; }
  return z || e;
}
TE_HD bool fe_is_zero(const te377::fq& v) {
  te377::fq one = te377::fq_zero(); one.v[0] = 1u;
  const te377::fq t = te377::mont_mul(v, one), q = te377::fq_Q();
  bool z = true, e = true;
#pragma unroll
  for (int i = 0; i < 14; i++) { z = z && t.v[i] == 0u; e = e && t.v[i] == q.v[i]; }
  return z || e;
}

// ---- Twisted-Edwards BLS12: 16 words, x = w[0..7], y = w[8..15] --------------------------------------------------------------
// coordinates in Montgomery form (any 256-bit input: x R^2 / R < 1.04 p).  MONT (option "points_montgomery"): the words hold x 2^256
// mod p, decoded by the constant R^2 / 2^256 -- also a canonical residue: the same bound
template <bool MONT = false> TE_HD void te_coords(const uint32_t (&w)[16], fp& X, fp& Y) {
  uint32_t xw[8], yw[8];
#pragma unroll
  for (int i = 0; i < 8; i++) { xw[i] = w[i]; yw[i] = w[8 + i]; }
  const fp k = MONT ? fp_R2_A() : fp_R2();
  const fp a[2] = {fp_from_words32(xw), fp_from_words32(yw)}, b[2] = {k, k};
  fp o[2];
  mont_mul_x<2>(a, b, o);
  X = o[0]; Y = o[1];
}
// 0, TE_MSM_POINT_NONCANONICAL (1) or TE_MSM_POINT_OFF_CURVE (2).  MONT: "canonical" stays "the stored value is below p"; the curve
// equation is checked on the decoded coordinates
template <bool MONT = false> TE_HD int check_form_te(const uint32_t (&w)[16]) {
  const bool canon = words_lt<8>(w, P_W32) && words_lt<8>(w + 8, P_W32);
  fp X, Y;
  te_coords<MONT>(w, X, Y);
  const fp a1[2] = {X, Y};
  fp sq[2];
  mont_mul_x<2>(a1, a1, sq);                                       // x^2, y^2
  const fp xy2 = mont_mul(sq[0], sq[1]);
  const fp dxy2 = mont_mul(xy2, fp_D_MONT());
  const fp lhs = fp_norm(fp_sub<2>(sq[1], sq[0]));                 // y^2 - x^2       (< 3.1 p)
  const fp rhs = fp_norm(fp_add(fp_R1(), dxy2));                   // 1 + d x^2 y^2   (< 2.2 p)
  const bool on = fe_is_zero(fp_sub<4>(lhs, rhs));
  return !canon ? 1 : (!on ? 2 : 0);
}
// [k] (X, Y) in extended coordinates, X and Y in Montgomery form (product outputs); also the root choice of from_x.hip.hpp
TE_HD ete mul_order_te(const fp& X, const fp& Y, const naf_t& k) {
  ete P;
  P.x = X; P.y = Y; P.z = fp_R1(); P.t = mont_mul(X, Y);
  ete N = P;                                                       // -P = (-x, y, 1, -t), reduced to class N below 1.1 p
  {
    const fp a[2] = {fp_neg<2>(P.x), fp_neg<2>(P.t)}, b[2] = {fp_R1(), fp_R1()};
    fp o[2];
    mont_mul_x<2>(a, b, o);
    N.x = o[0]; N.t = o[1];
  }
  ete acc = P;
#pragma unroll 1
  for (int i = k.top - 1; i >= 0; i--) {
    acc = ete_add<9>(acc, acc);
    const int dg = naf_digit(k, i);
    if (dg) acc = ete_add<9>(acc, dg > 0 ? P : N);
  }
  return acc;
}
// [L] P = O on the whole curve (ete_add is complete there: a square, d not)
template <bool MONT = false> TE_HD bool in_subgroup_te(const uint32_t (&w)[16], const naf_t& k) {
  fp X, Y;
  te_coords<MONT>(w, X, Y);
  const ete acc = mul_order_te(X, Y, k);
  // the neutral element (0 : Z : Z : 0), Z != 0
  return fe_is_zero(acc.x) && fe_is_zero(fp_sub<2>(acc.y, acc.z)) && !fe_is_zero(acc.z);
}

// ---- BLS12-377 G1: 24 words, x = w[0..11], y = w[12..23] ----------------------------------------------------------------------
// MONT (option "points_montgomery"): the words hold x 2^384 mod q; R^2 / 2^384 and s R^2 / 2^384 decode them
template <bool MONT = false> TE_HD void c377_coords(const uint32_t (&w)[24], te377::fq& X, te377::fq& Y, te377::fq& sx) {
  using namespace te377;
  uint32_t xw[12], yw[12];
#pragma unroll
  for (int i = 0; i < 12; i++) { xw[i] = w[i]; yw[i] = w[12 + i]; }
  const fq xl = fq_from_words32(xw);
  const fq k = MONT ? fq_R2_A() : fq_R2();
  const fq a[3] = {xl, fq_from_words32(yw), xl}, b[3] = {k, k, MONT ? fq_S_R2_A() : fq_S_R2()};
  fq o[3];
  fe_mul_x<3>(a, b, o);
  X = o[0]; Y = o[1]; sx = o[2];                                   // x, y, s x   (Montgomery form, as in pnt_from_sw377)
}
template <bool MONT = false> TE_HD int check_form_377(const uint32_t (&w)[24]) {
  using namespace te377;
  const bool canon = words_lt<12>(w, Q_W32) && words_lt<12>(w + 12, Q_W32);
  fq X, Y, sx;
  c377_coords<MONT>(w, X, Y, sx);
  const fq a1[2] = {X, Y};
  fq sq[2];
  fe_mul_x<2>(a1, a1, sq);                                       // x^2, y^2
  const fq x3 = te377::mont_mul(sq[0], X);
  const fq rhs = fq_norm(fq_add(x3, fq_R1()));                     // x^3 + 1   (< 2.2 q)
  const bool on = fe_is_zero(fq_sub<4>(sq[1], rhs));
  // the conversion's Z = 2 y w with w = s x + s + 1 (pnt_from_sw377)
  const fq wv = fq_norm(fq_add(sx, fq_SP1_MONT()));
  const bool defined = !fe_is_zero(Y) && !fe_is_zero(wv);
  return !canon ? 1 : ((!on || !defined) ? 2 : 0);
}

// projective short-Weierstrass point of y^2 = x^3 + 1 and the complete formulas (Renes-Costello-Batina 2016, a = 0, b3 = 3).
// Every operand of a product is normalised (class N); differences take 16 q (subtrahends stay below 10 q); values stay below
// 20 q, far inside the 29 spare bits of R = 2^406.
struct sw377 { te377::fq x, y, z; };
namespace rcb {
using te377::fq;
TE_HD fq mul(const fq& a, const fq& b) { return te377::mont_mul(a, b); }
TE_HD fq add(const fq& a, const fq& b) { return te377::fq_norm(te377::fq_add(a, b)); }
TE_HD fq sub(const fq& a, const fq& b) { return te377::fq_norm(te377::fq_sub<16>(a, b)); }
TE_HD fq mul3(const fq& a) { return te377::fq_norm(te377::fq_mul3(a)); }
}  // namespace rcb
// algorithm 7: P + Q, 12 products
TE_HD sw377 sw377_add(const sw377& P, const sw377& Q) {
  using namespace rcb;
  fq t0 = mul(P.x, Q.x), t1 = mul(P.y, Q.y), t2 = mul(P.z, Q.z);
  fq t3 = mul(add(P.x, P.y), add(Q.x, Q.y));
  fq t4 = add(t0, t1);
  t3 = sub(t3, t4);
  t4 = mul(add(P.y, P.z), add(Q.y, Q.z));
  fq X3 = add(t1, t2);
  t4 = sub(t4, X3);
  X3 = mul(add(P.x, P.z), add(Q.x, Q.z));
  fq Y3 = add(t0, t2);
  Y3 = sub(X3, Y3);
  X3 = add(t0, t0);
  t0 = add(X3, t0);
  t2 = mul3(t2);
  fq Z3 = add(t1, t2);
  t1 = sub(t1, t2);
  Y3 = mul3(Y3);
  X3 = mul(t4, Y3);
  t2 = mul(t3, t1);
  X3 = sub(t2, X3);
  Y3 = mul(Y3, t0);
  t1 = mul(t1, Z3);
  Y3 = add(t1, Y3);
  t0 = mul(t0, t3);
  Z3 = mul(Z3, t4);
  Z3 = add(Z3, t0);
  sw377 r; r.x = X3; r.y = Y3; r.z = Z3;
  return r;
}
// algorithm 9: 2 P, 8 products
TE_HD sw377 sw377_dbl(const sw377& P) {
  using namespace rcb;
  fq t0 = mul(P.y, P.y);
  fq Z3 = add(t0, t0); Z3 = add(Z3, Z3); Z3 = add(Z3, Z3);
  fq t1 = mul(P.y, P.z), t2 = mul(P.z, P.z);
  t2 = mul3(t2);
  fq X3 = mul(t2, Z3);
  fq Y3 = add(t0, t2);
  Z3 = mul(t1, Z3);
  t1 = add(t2, t2);
  t2 = add(t1, t2);
  t0 = sub(t0, t2);
  Y3 = mul(t0, Y3);
  Y3 = add(X3, Y3);
  t1 = mul(P.x, P.y);
  X3 = mul(t0, t1);
  X3 = add(X3, X3);
  sw377 r; r.x = X3; r.y = Y3; r.z = Z3;
  return r;
}
// [r] P = O on y^2 = x^3 + 1 (never in the engine's twisted-Edwards form: see the top of this file)
template <bool MONT = false> TE_HD bool in_subgroup_377(const uint32_t (&w)[24], const naf_t& k) {
  using namespace te377;
  fq X, Y, sx;
  c377_coords<MONT>(w, X, Y, sx);
  sw377 P; P.x = X; P.y = Y; P.z = fq_R1();
  sw377 N = P; N.y = te377::mont_mul(fq_neg<4>(Y), fq_R1());       // -P = (x, -y, 1)
  sw377 acc = P;
#pragma unroll 1
  for (int i = k.top - 1; i >= 0; i--) {
    acc = sw377_dbl(acc);
    const int dg = naf_digit(k, i);
    if (dg) acc = sw377_add(acc, dg > 0 ? P : N);
  }
  return fe_is_zero(acc.z) && !fe_is_zero(acc.y);                  // (0 : Y : 0), Y != 0
}

// the report word of one check launch: the LOWEST failing index i of n wins an atomicMax over (n - i) << 2 | (3 - reason) (0 = no
// failure); at one index the lowest reason wins, so a point that fails its form is never reported as "outside the subgroup"
TE_HD uint64_t check_code(uint64_t n, uint64_t i, int reason) { return ((n - i) << 2) | (uint64_t)(3 - reason); }
TE_HD void check_decode(uint64_t code, uint64_t n, int64_t* index, int* reason) { *index = (int64_t)(n - (code >> 2)); *reason = 3 - (int)(code & 3u); }

#if defined(__HIPCC__)
// one lane per point; every lane of a launch runs the same instructions (no early exit: a wave's chain is uniform)
template <int CURVE, bool MONT = false> __global__ __launch_bounds__(256) void k_check_form(const uint4* __restrict__ pts, uint32_t n, unsigned long long* word) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int Q4 = CURVE == 1 ? 6 : 4;                            // 16-byte words of one point (96 / 64 bytes)
  uint32_t w[Q4 * 4];
#pragma unroll
  for (int k = 0; k < Q4; k++) { const uint4 v = pts[(size_t)i * Q4 + k]; w[4 * k] = v.x; w[4 * k + 1] = v.y; w[4 * k + 2] = v.z; w[4 * k + 3] = v.w; }
  int reason;
  if constexpr (CURVE == 1) reason = check_form_377<MONT>(w);
  else reason = check_form_te<MONT>(w);
  if (reason) atomicMax(word, (unsigned long long)check_code(n, i, reason));
}
template <int CURVE, bool MONT = false> __global__ __launch_bounds__(256) void k_check_subgroup(const uint4* __restrict__ pts, uint32_t n, unsigned long long* word, naf_t k) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int Q4 = CURVE == 1 ? 6 : 4;
  uint32_t w[Q4 * 4];
#pragma unroll
  for (int j = 0; j < Q4; j++) { const uint4 v = pts[(size_t)i * Q4 + j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
  bool in;
  if constexpr (CURVE == 1) in = in_subgroup_377<MONT>(w, k);
  else in = in_subgroup_te<MONT>(w, k);
  if (!in) atomicMax(word, (unsigned long long)check_code(n, i, 3));
}
// The same two checks over records at a stride (options "point_stride" / "point_infinity_flag"; strided.hip.hpp): the block's tile through
// LDS, then the packed kernels' verdict per lane.  flag (BLS12-377): a record whose flag byte is 1 is the point at infinity and passes both
// levels without its coordinates being looked at; a flag byte other than 0 or 1 is TE_MSM_POINT_NONCANONICAL at its index.
template <int CURVE, bool MONT = false> __global__ __launch_bounds__(256) void k_check_form_strided(const uint64_t* __restrict__ src, uint32_t stride, uint32_t flag, uint32_t n,
                                                                                                    unsigned long long* word) {
  __shared__ uint64_t tile[TE_STRIDE_TILE * TE_STRIDE_MAX / 8u];
  strided_stage(tile, src, blockIdx.x, n, stride);
  const uint32_t t = threadIdx.x, i = blockIdx.x * TE_STRIDE_TILE + t;
  if (i >= n) return;
  constexpr int PW = CURVE == 1 ? 24 : 16;
  uint32_t w[PW];
  const uint32_t fb = strided_pick<PW>(tile, t, stride, w, CURVE == 1 && flag != 0u);
  int reason;
  if constexpr (CURVE == 1) reason = check_form_377<MONT>(w);
  else reason = check_form_te<MONT>(w);
  if (fb) reason = fb == 1u ? 0 : 1;
  if (reason) atomicMax(word, (unsigned long long)check_code(n, i, reason));
}
template <int CURVE, bool MONT = false> __global__ __launch_bounds__(256) void k_check_subgroup_strided(const uint64_t* __restrict__ src, uint32_t stride, uint32_t flag, uint32_t n,
                                                                                                        unsigned long long* word, naf_t k) {
  __shared__ uint64_t tile[TE_STRIDE_TILE * TE_STRIDE_MAX / 8u];
  strided_stage(tile, src, blockIdx.x, n, stride);
  const uint32_t t = threadIdx.x, i = blockIdx.x * TE_STRIDE_TILE + t;
  if (i >= n) return;
  constexpr int PW = CURVE == 1 ? 24 : 16;
  uint32_t w[PW];
  const uint32_t fb = strided_pick<PW>(tile, t, stride, w, CURVE == 1 && flag != 0u);
  bool in;
  if constexpr (CURVE == 1) in = in_subgroup_377<MONT>(w, k);
  else in = in_subgroup_te<MONT>(w, k);
  if (!in && !fb) atomicMax(word, (unsigned long long)check_code(n, i, 3));      // (a flagged record: the form check has spoken)
}
#endif

}  // namespace te
