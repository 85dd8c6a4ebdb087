// field_ops.hip.hpp -- batched field arithmetic out[i] = a_i op b_i (te_msm_field_op*; include/te_msm.h "batched field arithmetic",
// DESIGN.md section 21).  The reference's bulkAddFields / bulkSubFields / bulkMulFields / bulkDoubleFields / bulkInvertFields /
// bulkPowFields / bulkPowFields17 / bulkSqrtFields (utils/wasmFunctions.ts), over either base field of the engine:
//   N = 9   p, 32-byte elements: Aleo's `field`, the Twisted-Edwards base field, BLS12-377's scalar field Fr
//   N = 14  q, 48-byte elements: BLS12-377's base field
//
// Like group_add.hip.hpp, the per-lane functions are TE_HD and the kernels sit under __HIPCC__: tests/csrc/fieldopscheck.cpp runs the
// exact code of the kernels on the CPU, a block of k_field_inv as plain loops over its lanes.
//
// VALUES.  Any 256- / 384-bit input stands for its residue; outputs are canonical.  MONT: inputs and outputs are a A mod m with
// A = 2^256 / 2^384 (a native prover's residues).  Two routes through the arithmetic of fp.hpp / fq377.hpp (R = 2^261 / 2^406):
//   add, sub, neg, mul (k_field_map) work on the RAW limbs of the input words.  A product with the integer R mod m leaves the residue
//     of its other operand below 2 m (w (R mod m) / R + m), and one conditional subtraction makes it canonical: add is one product,
//     and the same product in both forms ((a + b) A = a A + b A).  mul is two: a b / R, then the constant R^2 (canonical) or R^2 / A
//     (MONT: a A b A / A = a b A) -- the one constant te_coords<MONT> swaps for points.  double and square are add / mul with b = a.
//   inv, pow, sqrt decode to the Montgomery form of the field (one product with R^2 or R^2 / A, fo_decode), run their chain there and
//     encode with the integer 1 or A (fo_encode).
// LIMBS: every product takes a class N operand (raw limbs of fe_from_words32, or a product output) and one more of class N or a
//   normalised sum / difference; value bounds: raw inputs are below 2^256 = 13.8 p / 2^384 = 153 q, so w c / R stays below m / 16
//   for any canonical constant c, and the product of two raw inputs below 2^251 + p / 2^362 + q.
//
// INVERSION (k_field_inv): Montgomery's trick.  A lane owns the `group` elements 256 apart inside its block's tile of 256 x group
//   (every load and store of a wave covers consecutive elements).  Forward it multiplies them up, writing the product BEFORE each
//   element to a slab of the call's own (plane-major 16-byte words: coalesced); one Fermat chain (fe_inv) inverts the total; backward
//   it reads the element again, its prefix from the slab, writes inv x prefix and takes the element into inv.  A zero residue is left
//   out of the chain (a select) and written as 0.  An index at or past m ends the lane's walk: a partial last tile and a partial last
//   chain are the same code.  The element is read again before the lane's own write of the same record: d_out may be d_a.
//   Products per element: decode twice, one forward, two backward, encode.
// POWERS (k_field_pow): per-element exponents in fixed 2-bit windows over 256 bits with the table a, a^2, a^3 (384 products, every
//   lane the same instructions); a SHARED exponent is a kernel argument, square-and-multiply from its top set bit with uniform branches.
//   The exponent is a plain 256-bit integer on both fields, never reduced.  0^0 = 1.
// SQUARE ROOT (k_field_sqrt): from_x.hip.hpp's fe_sqrt_ratio<N, false>, then the numerically smaller root: r <= (m - 1) / 2, decided on
//   the canonical words (words_lt against (m + 1) / 2, words_neg).  0 has the root 0; a non-square is reported.
// FAILURES go to the check lane's report word as check_code(n, index, reason): reason 1 TE_MSM_FIELD_ZERO, 2 TE_MSM_FIELD_NOT_SQUARE.
//
// Every address is an affine function of the thread id, bounded by m.
#pragma once
#include "scalar_mul.hip.hpp"
#include "../../include/te_msm.h"

namespace te {

enum { FO_ADD = 0, FO_SUB = 1, FO_MUL = 2, FO_NEG = 3 };            // k_field_map's OP
enum { FO_B_ARRAY = 0, FO_B_SHARED = 1, FO_B_IS_A = 2 };           // ... and where its second operand comes from
#define FO_INV_GROUP_DEFAULT TE_MSM_FIELD_INV_GROUP                // elements of one inversion chain (measured: include/te_msm.h)
#define FO_INV_GROUP_MAX 64u

template <int N> struct fo_sizes {
  static constexpr int W = N == 9 ? 8 : 12, Q4 = W / 4;            // words and 16-byte words of one element
  static constexpr int SQ = N == 9 ? 3 : 4;                        // 16-byte words of one slab entry (N limbs, padded)
};
// one record that every lane of a launch shares: b under TE_MSM_FIELD_SHARED_B (W words), or the exponent (8 words; top = index of its
// leading one, -1 for 0)
struct fo_rec { uint32_t w[12]; int top; };

// (p + 1) / 2: r > p - r exactly when r >= (p + 1) / 2   (Q_HALF1_W32 for q: from_x.hip.hpp)
constexpr uint32_t P_HALF1_W32[8] = {0x00000001u, 0x8508c000u, 0x68000000u, 0xacd53b7fu, 0x2e1bd800u, 0x305a268fu, 0x4d1652abu, 0x0955b2afu};

TE_HD fel<9> fo_limbs(const uint32_t (&w)[8]) { return fp_from_words32(w); }
TE_HD fel<14> fo_limbs(const uint32_t (&w)[12]) { return te377::fq_from_words32(w); }
template <int N> TE_HD const uint32_t* fo_mod_words() { if constexpr (N == 9) return P_W32; else return te377::Q_W32; }
template <int N> TE_HD const uint32_t* fo_half1_words() { if constexpr (N == 9) return P_HALF1_W32; else return Q_HALF1_W32; }
// the constant of a decoding product: R^2, or R^2 / A for words that hold a A
template <int N, bool MONT> TE_HD fel<N> fo_decode_const() {
  if constexpr (N == 9) return MONT ? fp_R2_A() : fp_R2();
  else return MONT ? te377::fq_R2_A() : te377::fq_R2();
}
// the integer A = 2^256 / 2^384 as limbs (class N: only the top limb is set)
template <int N> TE_HD fel<N> fo_A() {
  fel<N> r = fe_zero<N>();
  r.v[N - 1] = N == 9 ? 1u << (256 - 29 * 8) : 1u << (384 - 29 * 13);
  return r;
}
// class N, value below 2 m  ->  the canonical value as W words (fe_to_canon's tail: one conditional subtraction, then the packing)
template <int N, int W> TE_HD void fo_words(const fel<N>& t, uint32_t (&w)[W]) {
  const fel<N> m = fe_modulus<N>();
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
// the residue of a raw value (limbs of class N or a normalised sum, value below 2^258 / 2^386) as class N below 1.1 m
template <int N> TE_HD fel<N> fo_residue(const fel<N>& raw) { return fe_mul(raw, fe_one<N>()); }
// words -> Montgomery form of the field, class N, value below 1.1 m; and back (MONT: the words of y A)
template <int N, bool MONT, int W> TE_HD fel<N> fo_decode(const uint32_t (&w)[W]) { return fe_mul(fo_limbs(w), fo_decode_const<N, MONT>()); }
template <int N, bool MONT, int W> TE_HD void fo_encode(const fel<N>& y, uint32_t (&w)[W]) {
  fel<N> k = fe_zero<N>(); k.v[0] = 1u;
  if constexpr (MONT) k = fo_A<N>();
  fo_words<N, W>(fe_mul(y, k), w);
}
// a product output (class N, value below 2 m) is 0 mod m exactly when it is 0 or m: class N has one representation of a value
template <int N> TE_HD bool fo_is_zero(const fel<N>& t) {
  const fel<N> m = fe_modulus<N>();
  bool z = true, e = true;
#pragma unroll
  for (int i = 0; i < N; i++) { z = z && t.v[i] == 0u; e = e && t.v[i] == m.v[i]; }
  return z || e;
}
// is the residue of these words 0?  (k_field_zero_scan: one product, then compares)
template <int N, int W> TE_HD bool fo_words_zero(const uint32_t (&w)[W]) { return fo_is_zero(fo_residue(fo_limbs(w))); }

// ---- one lane of k_field_map ----------------------------------------------------------------------------------------------------
// MONT changes the second constant of FO_MUL only: add, sub and neg are the same map on a and on a A
template <int N, int OP, bool MONT, int W> TE_HD void fo_map(const uint32_t (&wa)[W], const uint32_t (&wb)[W], uint32_t (&o)[W]) {
  const fel<N> a = fo_limbs(wa);
  if constexpr (OP == FO_ADD) {
    fo_words<N, W>(fo_residue(fe_norm(fe_add(a, fo_limbs(wb)))), o);
  } else if constexpr (OP == FO_SUB) {
    const fel<N> b = fo_residue(fo_limbs(wb));                     // class N, below 1.1 m: what the offset form of 2 m takes
    fo_words<N, W>(fo_residue(fe_norm(fe_sub<2>(a, b))), o);
  } else if constexpr (OP == FO_NEG) {
    uint32_t c[W];
    fo_words<N, W>(fo_residue(a), c);
    words_neg<W>(c, fo_mod_words<N>(), o);
  } else {
    fo_words<N, W>(fe_mul(fe_mul(a, fo_limbs(wb)), fo_decode_const<N, MONT>()), o);
  }
}

// ---- one lane of k_field_inv: a step forward, the inversion, a step backward -------------------------------------------------------
// run: the product of the lane's non-zero elements so far; before: run as it was
template <int N, bool MONT, int W> TE_HD void fo_inv_forward(const uint32_t (&wa)[W], fel<N>& run, fel<N>& before) {
  const fel<N> x = fo_decode<N, MONT>(wa);
  before = run;
  run = fe_select(fo_is_zero(x), run, fe_mul(run, x));
}
// inv: the inverse of the product of the lane's non-zero elements up to and including this one; out = 1 / a (0 for a zero)
template <int N, bool MONT, int W> TE_HD void fo_inv_backward(const uint32_t (&wa)[W], const fel<N>& before, fel<N>& inv, uint32_t (&o)[W]) {
  const fel<N> x = fo_decode<N, MONT>(wa);
  const bool skip = fo_is_zero(x);
  fel<N> r, nx;
  fe_mul2(inv, before, inv, x, r, nx);
  uint32_t e[W];
  fo_encode<N, MONT>(r, e);
#pragma unroll
  for (int j = 0; j < W; j++) o[j] = skip ? 0u : e[j];
  inv = fe_select(skip, inv, nx);
}
// slab entries: N limbs in SQ 16-byte words
template <int N> TE_HD void fo_slab_pack(const fel<N>& v, uint32_t (&s)[4 * fo_sizes<N>::SQ]) {
#pragma unroll
  for (int i = 0; i < 4 * fo_sizes<N>::SQ; i++) s[i] = i < N ? v.v[i] : 0u;
}
template <int N> TE_HD fel<N> fo_slab_unpack(const uint32_t (&s)[4 * fo_sizes<N>::SQ]) {
  fel<N> v;
#pragma unroll
  for (int i = 0; i < N; i++) v.v[i] = s[i];
  return v;
}

// ---- one lane of k_field_pow -----------------------------------------------------------------------------------------------------
TE_HD uint32_t fo_exp_word(const uint32_t (&e)[8], int k) {        // e[k], k uniform or not: read through selects, never indexed
  uint32_t r = 0;
#pragma unroll
  for (int j = 0; j < 8; j++) r = j == k ? e[j] : r;
  return r;
}
// the leading one of a 256-bit exponent (-1: the exponent is 0); the host fills fo_rec::top with it
inline int fo_exp_top(const uint32_t (&e)[8]) {
  for (int i = 255; i >= 0; i--)
    if ((e[i >> 5] >> (i & 31)) & 1u) return i;
  return -1;
}
template <int N, bool MONT, int W> TE_HD void fo_pow(const uint32_t (&wa)[W], const uint32_t (&e)[8], uint32_t (&o)[W]) {
  const fel<N> x = fo_decode<N, MONT>(wa), one = fe_one<N>();
  const fel<N> x2 = fe_mul(x, x), x3 = fe_mul(x2, x);
  fel<N> acc = one;
#pragma unroll 1
  for (int i = 127; i >= 0; i--) {
    acc = fe_mul(acc, acc);
    acc = fe_mul(acc, acc);
    const uint32_t d = (fo_exp_word(e, i >> 4) >> (2 * (i & 15))) & 3u;
    acc = fe_mul(acc, fe_select((d & 2u) != 0u, fe_select((d & 1u) != 0u, x3, x2), fe_select((d & 1u) != 0u, x, one)));
  }
  fo_encode<N, MONT>(acc, o);
}
template <int N, bool MONT, int W> TE_HD void fo_pow_shared(const uint32_t (&wa)[W], const fo_rec& e, uint32_t (&o)[W]) {
  const fel<N> x = fo_decode<N, MONT>(wa);
  fel<N> acc = e.top < 0 ? fe_one<N>() : x;
  uint32_t ew[8];
#pragma unroll
  for (int j = 0; j < 8; j++) ew[j] = e.w[j];
#pragma unroll 1
  for (int i = e.top - 1; i >= 0; i--) {
    acc = fe_mul(acc, acc);
    if ((fo_exp_word(ew, i >> 5) >> (i & 31)) & 1u) acc = fe_mul(acc, x);
  }
  fo_encode<N, MONT>(acc, o);
}

// ---- one lane of k_field_sqrt: 0 or TE_MSM_FIELD_NOT_SQUARE (2); o is written either way (meaningless on a failure) ------------------
// larger_root (false in every real use): the test shim's deliberate mistake
template <int N, bool MONT, int W> TE_HD int fo_sqrt(const uint32_t (&wa)[W], const exp_t& root_exp, uint32_t (&o)[W], bool larger_root = false) {
  const fel<N> x = fo_decode<N, MONT>(wa);
  const bool zero = fo_is_zero(x);
  fel<N> y;
  const bool square = fe_sqrt_ratio<N, false>(x, x, root_exp, y);
  uint32_t rc[W], rn[W];
  fe_to_canon<N, W>(y, rc);
  const bool flip = words_lt<W>(rc, fo_half1_words<N>()) == larger_root;
  if constexpr (MONT) fo_encode<N, true>(y, rc);                   // (m - r A = (m - r) A mod m: the choice carries over)
  words_neg<W>(rc, fo_mod_words<N>(), rn);
#pragma unroll
  for (int j = 0; j < W; j++) o[j] = zero ? 0u : flip ? rn[j] : rc[j];
  return square || zero ? 0 : 2;
}

#if defined(__HIPCC__)
template <int Q4> __device__ __forceinline__ void fo_load(const uint4* __restrict__ src, size_t at, uint32_t (&w)[Q4 * 4]) {
#pragma unroll
  for (int j = 0; j < Q4; j++) { const uint4 v = src[at + j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
}
template <int Q4> __device__ __forceinline__ void fo_store(uint4* dst, size_t at, const uint32_t (&w)[Q4 * 4]) {
#pragma unroll
  for (int j = 0; j < Q4; j++) dst[at + j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
}
// (a, b and out are not __restrict__: out may be a or b -- a lane reads its own records before it writes its own)
// one lane per element of m; BSRC: b holds m records, or the launch's one record sb, or b is a (double, square)
template <int N, int OP, bool MONT, int BSRC> __global__ __launch_bounds__(256) void k_field_map(const uint4* a, const uint4* b, fo_rec sb, uint32_t m, uint4* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int W = fo_sizes<N>::W, Q4 = fo_sizes<N>::Q4;
  uint32_t wa[W], wb[W], o[W];
  fo_load<Q4>(a, (size_t)i * Q4, wa);
  if constexpr (BSRC == FO_B_ARRAY) fo_load<Q4>(b, (size_t)i * Q4, wb);
  else {
#pragma unroll
    for (int j = 0; j < W; j++) wb[j] = BSRC == FO_B_SHARED ? sb.w[j] : wa[j];
  }
  fo_map<N, OP, MONT>(wa, wb, o);
  fo_store<Q4>(out, (size_t)i * Q4, o);
}
// in front of a strict inversion: the piece [base, base + m) of n; reports the lowest zero residue
template <int N> __global__ __launch_bounds__(256) void k_field_zero_scan(const uint4* __restrict__ a, uint32_t m, unsigned long long* word, uint64_t n, uint64_t base) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int W = fo_sizes<N>::W, Q4 = fo_sizes<N>::Q4;
  uint32_t wa[W];
  fo_load<Q4>(a, (size_t)i * Q4, wa);
  if (fo_words_zero<N>(wa)) atomicMax(word, (unsigned long long)check_code(n, base + i, 1));
}
// grid = ceil(m / (256 group)) blocks; slab: SQ planes of cap >= m 16-byte words, the call's own
template <int N, bool MONT> __global__ __launch_bounds__(256) void k_field_inv(const uint4* a, uint32_t m, uint32_t group, uint4* __restrict__ slab, uint32_t cap, uint4* out,
                                                                              exp_t inv_exp) {
  constexpr int W = fo_sizes<N>::W, Q4 = fo_sizes<N>::Q4, SQ = fo_sizes<N>::SQ;
  const uint64_t first = (uint64_t)blockIdx.x * 256u * group + threadIdx.x;
  fel<N> run = fe_one<N>();
#pragma unroll 1
  for (uint32_t j = 0; j < group; j++) {
    const uint64_t e = first + (uint64_t)j * 256u;
    if (e >= m) break;
    uint32_t wa[W], s[4 * SQ];
    fo_load<Q4>(a, (size_t)e * Q4, wa);
    fel<N> before;
    fo_inv_forward<N, MONT>(wa, run, before);
    fo_slab_pack<N>(before, s);
#pragma unroll
    for (int q = 0; q < SQ; q++) slab[(size_t)q * cap + e] = make_uint4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
  }
  if (first >= m) return;
  fel<N> inv = fe_inv(run, inv_exp);
#pragma unroll 1
  for (uint32_t j = group; j-- > 0u;) {
    const uint64_t e = first + (uint64_t)j * 256u;
    if (e >= m) continue;
    uint32_t wa[W], s[4 * SQ], o[W];
    fo_load<Q4>(a, (size_t)e * Q4, wa);
#pragma unroll
    for (int q = 0; q < SQ; q++) { const uint4 v = slab[(size_t)q * cap + e]; s[4 * q] = v.x; s[4 * q + 1] = v.y; s[4 * q + 2] = v.z; s[4 * q + 3] = v.w; }
    fo_inv_backward<N, MONT>(wa, fo_slab_unpack<N>(s), inv, o);
    fo_store<Q4>(out, (size_t)e * Q4, o);
  }
}
// one lane per element; SHARED: the exponent is se (b is not read), else record i of b: 32 bytes on both fields
template <int N, bool MONT, bool SHARED> __global__ __launch_bounds__(256) void k_field_pow(const uint4* a, const uint4* b, fo_rec se, uint32_t m, uint4* out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int W = fo_sizes<N>::W, Q4 = fo_sizes<N>::Q4;
  uint32_t wa[W], o[W];
  fo_load<Q4>(a, (size_t)i * Q4, wa);
  if constexpr (SHARED) fo_pow_shared<N, MONT>(wa, se, o);
  else {
    uint32_t e[8];
    fo_load<2>(b, (size_t)i * 2, e);
    fo_pow<N, MONT>(wa, e, o);
  }
  fo_store<Q4>(out, (size_t)i * Q4, o);
}
// one lane per element of the piece [base, base + m) of n; reports the lowest non-square
template <int N, bool MONT> __global__ __launch_bounds__(256) void k_field_sqrt(const uint4* a, uint32_t m, uint4* out, unsigned long long* word, uint64_t n, uint64_t base,
                                                                               exp_t root_exp) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int W = fo_sizes<N>::W, Q4 = fo_sizes<N>::Q4;
  uint32_t wa[W], o[W];
  fo_load<Q4>(a, (size_t)i * Q4, wa);
  const int reason = fo_sqrt<N, MONT>(wa, root_exp, o);
  fo_store<Q4>(out, (size_t)i * Q4, o);
  if (reason) atomicMax(word, (unsigned long long)check_code(n, base + i, reason));
}
#endif

}  // namespace te
