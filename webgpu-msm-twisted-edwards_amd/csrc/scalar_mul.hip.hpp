// scalar_mul.hip.hpp -- batch scalar multiplication out[i] = [k_i] P_i, no sum (te_msm_mul*, include/te_msm.h "batch scalar
// multiplication").  The reference's bulkGroupScalarMul / FieldMath.multiply.
//
// Like check.hip.hpp, the per-lane functions are TE_HD and the kernels sit under __HIPCC__: tests/csrc/scalarmulcheck.cpp runs the
// exact code of k_scalar_mul and k_scalar_mul_affine on the CPU.
//
// THE GROUP LAWS are check.hip.hpp's, for the same reason: the result must be exactly [k] P for ANY k below 2^256.
//   Twisted-Edwards BLS12: the engine's ete_add is complete on the whole curve (a = -1 a square, d a non-square), cofactor part
//     included, doubling included.  #E = 4 L, so k mod 4 L is the only reduction allowed -- and only the shared scalar takes it.
//   BLS12-377 G1: the complete Renes-Costello-Batina formulas on y^2 = x^3 + 1 (sw377_add / sw377_dbl): 12 / 8 products against the
//     10 of the twisted-Edwards form, 42 words a point against 56, and no map back.  Inputs must lie in G1 (as for the MSM); the
//     shared scalar is reduced mod r.
// Adding the neutral element is correct under both laws: a digit 0 adds it, and no lane ever branches on its digit.
//
// PER-POINT SCALARS (k_scalar_mul<CURVE, false>): signed fixed windows of W bits.  K = k + C with C = sum_i 2^(W-1) 2^(W i) makes
// every window u_i of K an unsigned W-bit value and d_i = u_i - 2^(W-1) in [-2^(W-1), 2^(W-1)) the signed digit -- no carry to
// propagate, digit i is bits [W i, W i + W) of K.  A per-lane table of [1 .. 2^(W-1)] P in registers (indexed by unrolled compile-time
// selects, never a runtime index: that would put it in scratch), the addend chosen by compare chains and negated inside the addition.
// Chain: M = ceil(257 / W) digits, (M - 1) W doublings and M additions (W = 2: 256 and 129).
// SHARED SCALAR (k_scalar_mul<CURVE, true>): the NAF of k (mod 4 L, mod r), built on the host, a kernel argument: every lane of the
// launch runs the same digits, so the `if (digit)` of mul_order_te's chain is uniform.  k = 0 is top = -1: the neutral element.
//
// AFFINE OUTPUT (k_scalar_mul_affine): the chain writes projective (X : Y : Z); one thread then takes SM_AFF_GROUP consecutive points,
// Montgomery's trick over them (one Fermat inversion a group), and writes canonical little-endian x || y.  Z = 0 (the BLS12-377 point
// at infinity) keeps the factor 1 in the prefix products and gives 96 zero bytes, as the MSM result encodes infinity.
#pragma once
#include "from_x.hip.hpp"

namespace te {

// window bits: W = 2 on both curves, the widest whose table of 2^(W-1) points fits beside the accumulator and an addition's
// temporaries without scratch (measured).  Twisted-Edwards: 185 VGPRs, 2 waves per SIMD (W = 3: scratch).
// BLS12-377: 256 VGPRs + 7 AGPRs, 1 wave -- 8 % faster than W = 1 (double-and-always-add over the bits, 236 VGPRs, 2 waves).
// W >= 2 here: with W = 1 every digit u_i - 1 would be <= 0, so the offset recoding needs at least two bits.
template <int CURVE> struct sm_win {
  static constexpr int W = 2;
  static constexpr int M = (257 + W - 1) / W;                     // digits of K (K < 2^(W M))
  static constexpr int H = 1 << (W - 1);                           // table entries [1 .. H] P
};
// word j of C = sum_{i < M} 2^(W-1) 2^(W i)
constexpr uint32_t sm_offset_word(int W, int M, int j) {
  uint32_t r = 0;
  for (int i = 0; i < M; i++) {
    const int b = W * i + W - 1;
    if (b >> 5 == j) r |= 1u << (b & 31);
  }
  return r;
}
// K = k + C, 9 words
template <int W, int M> TE_HD void sm_recode(const uint32_t (&k)[8], uint32_t (&K)[9]) {
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    c += (uint64_t)(j < 8 ? k[j] : 0u) + sm_offset_word(W, M, j);
    K[j] = (uint32_t)c;
    c >>= 32;
  }
}
// the signed digit i (i uniform: the words are read through selects)
template <int W> TE_HD int sm_digit(const uint32_t (&K)[9], int i) {
  const int b = W * i, w = b >> 5, s = b & 31;
  uint32_t lo = 0, hi = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) { lo = j == w ? K[j] : lo; hi = j == w + 1 ? K[j] : hi; }
  const uint64_t v = ((uint64_t)hi << 32 | lo) >> s;
  return (int)(v & ((1u << W) - 1u)) - (1 << (W - 1));
}

// p - 2 and q - 2: Fermat's inverse
constexpr exp_t kInvExpTe = {{0xffffffffu, 0x0a117fffu, 0xd0000001u, 0x59aa76feu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu, 0u, 0u, 0u, 0u}, 252};
constexpr exp_t kInvExp377 = {{0xffffffffu, 0x8508bfffu, 0x30000000u, 0x170b5d44u, 0xba094800u, 0x1ef3622fu, 0x00f5138fu, 0x1a22d9f3u,
                               0x6ca1493bu, 0xc63b05c0u, 0x17c510eau, 0x01ae3a46u}, 376};
// ... by the kernels' CURVE parameter
template <int CURVE> constexpr const exp_t& inv_exp_of() { return CURVE == 1 ? kInvExp377 : kInvExpTe; }
// a^(modulus - 2), e uniform (a square-and-multiply chain over the bits of a kernel argument)
template <int N> TE_HD fel<N> fe_inv(const fel<N>& a, const exp_t& e) {
  fel<N> r = a;
#pragma unroll 1
  for (int i = e.top - 1; i >= 0; i--) {
    r = fe_mul(r, r);
    if (exp_bit(e, i)) r = fe_mul(r, a);
  }
  return r;
}

// ---- Twisted-Edwards BLS12 -----------------------------------------------------------------------------------------------------
// a + (neg ? -b : b), ete_add with -b = (-x, y, z, -t) folded in: -b swaps (y - x) and (y + x) and negates C, which swaps F and G.
// Every product sees the operand classes of ete_add (the swapped difference meets the sum of in1[1]: "difference x sum", allowed with
// 9 limbs); F and G are both normalised.
TE_HD ete ete_add_cneg(const ete& a, const ete& b, bool neg) {
  const fp ymx = fp_sub<2>(b.y, b.x), ypx = fp_add(b.y, b.x);
  const fp in1[4] = {fp_norm(fp_sub<2>(a.y, a.x)), fp_add(a.y, a.x), a.t, a.z};
  const fp in2[4] = {fe_select(neg, ypx, ymx), fe_select(neg, ymx, ypx), b.t, b.z};
  fp p1[4];
  mont_mul_x<4>(in1, in2, p1);
  const fp &A = p1[0], &B = p1[1];
  const fp C = fp_mul_k2d(p1[2]);
  const fp D = fp_add(p1[3], p1[3]);
  const fp E = fp_sub<2>(B, A);
  const fp H = fp_add(B, A);
  const fp Fs = fp_norm(fp_sub<2>(D, C)), Ga = fp_add(D, C);
  const fp F = fe_select(neg, fp_norm(Ga), Fs), G = fe_select(neg, Fs, Ga);
  const fp l[4] = {E, H, E, F}, rr[4] = {F, G, H, G};
  fp o[4];
  mont_mul_x<4>(l, rr, o);
  ete r;
  r.x = o[0]; r.y = o[1]; r.t = o[2]; r.z = o[3];
  return r;
}
TE_HD ete ete_select(bool c, const ete& a, const ete& b) {
  ete r;
  r.x = fe_select(c, a.x, b.x); r.y = fe_select(c, a.y, b.y); r.z = fe_select(c, a.z, b.z); r.t = fe_select(c, a.t, b.t);
  return r;
}
// (X, Y) in Montgomery form (product outputs) -> the extended point
TE_HD ete ete_of(const fp& X, const fp& Y) {
  ete P;
  P.x = X; P.y = Y; P.z = fp_R1(); P.t = mont_mul(X, Y);
  return P;
}
// [k] P by signed windows; K = sm_recode(k)
TE_HD ete sm_chain_te(const fp& X, const fp& Y, const uint32_t (&K)[9]) {
  using S = sm_win<0>;
  ete T[S::H];                                                     // [j + 1] P
  T[0] = ete_of(X, Y);
#pragma unroll
  for (int j = 1; j < S::H; j++) T[j] = (j & 1) ? ete_add<9>(T[j / 2], T[j / 2]) : ete_add<9>(T[j - 1], T[0]);
  auto addend = [&](int d, bool& neg) {
    const int mag = d < 0 ? -d : d;
    neg = d < 0;
    ete e = ete_identity();
#pragma unroll
    for (int j = 0; j < S::H; j++) e = ete_select(mag == j + 1, T[j], e);
    return e;
  };
  bool neg;
  ete e = addend(sm_digit<S::W>(K, S::M - 1), neg);
  ete acc = ete_add_cneg(ete_identity(), e, neg);
#pragma unroll 1
  for (int i = S::M - 2; i >= 0; i--) {
#pragma unroll 1
    for (int s = 0; s < S::W; s++) acc = ete_add<9>(acc, acc);    // (a whole addition per step: no unrolling)
    e = addend(sm_digit<S::W>(K, i), neg);
    acc = ete_add_cneg(acc, e, neg);
  }
  return acc;
}
// [k] P for a uniform k given as its NAF (top = -1: k = 0)
TE_HD ete sm_naf_te(const fp& X, const fp& Y, const naf_t& k) {
  if (k.top < 0) return ete_identity();
  return mul_order_te(X, Y, k);
}

// ---- BLS12-377 G1 (short Weierstrass, projective) -----------------------------------------------------------------------------
TE_HD sw377 sw377_identity() { sw377 r; r.x = te377::fq_zero(); r.y = te377::fq_R1(); r.z = te377::fq_zero(); return r; }
TE_HD sw377 sw377_select(bool c, const sw377& a, const sw377& b) {
  sw377 r;
  r.x = fe_select(c, a.x, b.x); r.y = fe_select(c, a.y, b.y); r.z = fe_select(c, a.z, b.z);
  return r;
}
TE_HD sw377 sw377_cneg(const sw377& a, bool neg) {                 // (X : -Y : Z), -Y = 16 q - Y normalised (rcb's difference)
  sw377 r = a;
  r.y = fe_select(neg, rcb::sub(te377::fq_zero(), a.y), a.y);
  return r;
}
TE_HD sw377 sw377_of(const te377::fq& X, const te377::fq& Y) { sw377 P; P.x = X; P.y = Y; P.z = te377::fq_R1(); return P; }
TE_HD sw377 sm_chain_377(const te377::fq& X, const te377::fq& Y, const uint32_t (&K)[9]) {
  using S = sm_win<1>;
  sw377 T[S::H];
  T[0] = sw377_of(X, Y);
#pragma unroll
  for (int j = 1; j < S::H; j++) T[j] = (j & 1) ? sw377_dbl(T[j / 2]) : sw377_add(T[j - 1], T[0]);
  auto addend = [&](int d) {
    const int mag = d < 0 ? -d : d;
    sw377 e = sw377_identity();
#pragma unroll
    for (int j = 0; j < S::H; j++) e = sw377_select(mag == j + 1, T[j], e);
    return sw377_cneg(e, d < 0);
  };
  sw377 acc = addend(sm_digit<S::W>(K, S::M - 1));
#pragma unroll 1
  for (int i = S::M - 2; i >= 0; i--) {
#pragma unroll 1
    for (int s = 0; s < S::W; s++) acc = sw377_dbl(acc);
    acc = sw377_add(acc, addend(sm_digit<S::W>(K, i)));
  }
  return acc;
}
TE_HD sw377 sm_naf_377(const te377::fq& X, const te377::fq& Y, const naf_t& k) {
  if (k.top < 0) return sw377_identity();
  const sw377 P = sw377_of(X, Y), N = sw377_cneg(P, true);
  sw377 acc = P;
#pragma unroll 1
  for (int i = k.top - 1; i >= 0; i--) {
    acc = sw377_dbl(acc);
    const int dg = naf_digit(k, i);
    if (dg) acc = sw377_add(acc, dg > 0 ? P : N);
  }
  return acc;
}

// ---- the shared scalar, on the host: k (8 words) reduced mod 4 L (Twisted-Edwards: the exponent of the whole curve group) or mod r
// (BLS12-377: inputs in G1), then its NAF -- at most 254 digits below 2^253.  k = 0 mod the order gives top = -1.
constexpr uint32_t kTe4L_W32[8] = {0x0cff67fcu, 0xe56bba6bu, 0x10f22bfau, 0x4a4e8ebfu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu};
constexpr uint32_t kR377_W32[8] = {0x00000001u, 0x0a118000u, 0xd0000001u, 0x59aa76feu, 0x5c37b001u, 0x60b44d1eu, 0x9a2ca556u, 0x12ab655eu};
inline naf_t sm_shared_naf(const uint32_t (&k)[8], int curve) {
  const uint32_t* m = curve == 1 ? kR377_W32 : kTe4L_W32;
  uint32_t v[9];
  for (int i = 0; i < 8; i++) v[i] = k[i];
  v[8] = 0;
  while (!words_lt<8>(v, m)) {                                     // k < 2^256 < 9 m: a few subtractions
    uint64_t br = 0;
    for (int i = 0; i < 8; i++) { const uint64_t s = (uint64_t)v[i] - m[i] - br; v[i] = (uint32_t)s; br = (s >> 63) & 1u; }
  }
  naf_t r = {};
  r.top = -1;
  for (int i = 0; i < 256; i++) {                                  // v >= 0 throughout; v + 1 never leaves 9 words
    bool nz = false;
    for (int j = 0; j < 9; j++) nz = nz || v[j];
    if (!nz) break;
    if (v[0] & 1u) {
      const bool minus = (v[0] & 3u) == 3u;                        // digit -1: v + 1; digit +1: v - 1
      if (minus) { r.neg[i >> 5] |= 1u << (i & 31); for (int j = 0; j < 9 && ++v[j] == 0u; j++) {} }
      else { r.pos[i >> 5] |= 1u << (i & 31); v[0] -= 1u; }
      r.top = i;
    }
    for (int j = 0; j < 9; j++) v[j] = (v[j] >> 1) | (j < 8 ? v[j + 1] << 31 : 0u);
  }
  return r;
}

// ---- one lane: point words and scalar words -> projective result (3 N words: X, Y, Z) --------------------------------------------
template <int CURVE> struct sm_sizes {
  static constexpr int N = CURVE == 1 ? 14 : 9;                    // limbs
  static constexpr int PW = CURVE == 1 ? 24 : 16;                  // words of an input / output point
  static constexpr int JW = CURVE == 1 ? 44 : 28;                  // words of a projective slot (3 N, rounded up to 16 bytes)
};
template <int CURVE, bool SHARED> TE_HD void sm_point(const uint32_t (&w)[sm_sizes<CURVE>::PW], const uint32_t (&k)[8], const naf_t& kn,
                                                      uint32_t* proj) {
  constexpr int N = sm_sizes<CURVE>::N;
  fel<N> X, Y, Z;
  uint32_t K[9];
  if constexpr (!SHARED) sm_recode<sm_win<CURVE>::W, sm_win<CURVE>::M>(k, K);
  if constexpr (CURVE == 1) {
    te377::fq sx;
    c377_coords(w, X, Y, sx);
    sw377 r;
    if constexpr (SHARED) r = sm_naf_377(X, Y, kn); else r = sm_chain_377(X, Y, K);
    X = r.x; Y = r.y; Z = r.z;
  } else {
    te_coords(w, X, Y);
    ete r;
    if constexpr (SHARED) r = sm_naf_te(X, Y, kn); else r = sm_chain_te(X, Y, K);
    X = r.x; Y = r.y; Z = r.z;
  }
#pragma unroll
  for (int i = 0; i < N; i++) { proj[i] = X.v[i]; proj[N + i] = Y.v[i]; proj[2 * N + i] = Z.v[i]; }
}

// ---- affine output: cnt (<= SM_AFF_GROUP) consecutive projective slots -> canonical x || y; Montgomery's trick, one inversion ------
// The prefix products wait in the first N words of the output slots, which are written last (backwards), as in k_affine377.
#define SM_AFF_GROUP 8u
template <int CURVE> TE_HD void sm_affine_group(const uint32_t* proj, uint32_t cnt, uint32_t* out, const exp_t& inv_exp) {
  constexpr int N = sm_sizes<CURVE>::N, PW = sm_sizes<CURVE>::PW, JW = sm_sizes<CURVE>::JW, CW = PW / 2;
  const fel<N> one = fe_one<N>();
  fel<N> run = one;
  for (uint32_t j = 0; j < cnt; j++) {
    fel<N> z;
#pragma unroll
    for (int i = 0; i < N; i++) z.v[i] = proj[(size_t)j * JW + 2 * N + i];
    run = fe_mul(run, fe_select(fe_is_zero(z), one, z));
#pragma unroll
    for (int i = 0; i < N; i++) out[(size_t)j * PW + i] = run.v[i];
  }
  fel<N> inv = fe_inv(run, inv_exp);
  for (uint32_t jj = cnt; jj-- > 0u;) {
    fel<N> x, y, z, pre = one;
#pragma unroll
    for (int i = 0; i < N; i++) { x.v[i] = proj[(size_t)jj * JW + i]; y.v[i] = proj[(size_t)jj * JW + N + i]; z.v[i] = proj[(size_t)jj * JW + 2 * N + i]; }
    if (jj > 0u) {
#pragma unroll
      for (int i = 0; i < N; i++) pre.v[i] = out[(size_t)(jj - 1u) * PW + i];
    }
    const bool inf = fe_is_zero(z);
    const fel<N> zi = fe_mul(inv, pre);                            // 1 / z_jj (1 for a stand-in)
    inv = fe_mul(inv, fe_select(inf, one, z));
    fel<N> ax, ay;
    fe_mul2(x, zi, y, zi, ax, ay);
    uint32_t cx[CW], cy[CW];
    fe_to_canon<N, CW>(ax, cx);
    fe_to_canon<N, CW>(ay, cy);
#pragma unroll
    for (int i = 0; i < CW; i++) { out[(size_t)jj * PW + i] = inf ? 0u : cx[i]; out[(size_t)jj * PW + CW + i] = inf ? 0u : cy[i]; }
  }
}

#if defined(__HIPCC__)
// one lane per point of a piece of m points; the scalars are per point (sc[i]) or one (SHARED: kn, the NAF).  No early exit inside the
// chain: a wave's instructions are uniform.
// SQ: 16-byte words of a scalar record -- the curve's own unless named: 2 on BLS12-377 reads 32-byte records (option "scalar_record_bytes";
// the shared-scalar form reads no record).  Lane i < m reads words [i SQ, i SQ + 2): the record's first 32 bytes, inside m records of 16 SQ.
template <int CURVE, bool SHARED, int SQ = (CURVE == 1 ? 3 : 2)> __global__ __launch_bounds__(256) void k_scalar_mul(const uint4* __restrict__ pts, const uint4* __restrict__ sc,
                                                                                     uint32_t m, uint4* __restrict__ proj, naf_t kn) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int PQ = sm_sizes<CURVE>::PW / 4, JQ = sm_sizes<CURVE>::JW / 4;                           // 16-byte words of a point / slot
  uint32_t w[4 * PQ], k[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < PQ; j++) { const uint4 v = pts[(size_t)i * PQ + j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
  if constexpr (!SHARED) {
#pragma unroll
    for (int j = 0; j < 2; j++) { const uint4 v = sc[(size_t)i * SQ + j]; k[4 * j] = v.x; k[4 * j + 1] = v.y; k[4 * j + 2] = v.z; k[4 * j + 3] = v.w; }
  }
  uint32_t o[4 * JQ];
  sm_point<CURVE, SHARED>(w, k, kn, o);
#pragma unroll
  for (int j = 0; j < JQ; j++) proj[(size_t)i * JQ + j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
}
// one thread per SM_AFF_GROUP consecutive results
template <int CURVE> __global__ __launch_bounds__(256) void k_scalar_mul_affine(const uint32_t* __restrict__ proj, uint32_t m, uint32_t* __restrict__ out,
                                                                                exp_t inv_exp) {
  const uint32_t lo = (blockIdx.x * blockDim.x + threadIdx.x) * SM_AFF_GROUP;
  if (lo >= m) return;
  sm_affine_group<CURVE>(proj + (size_t)lo * sm_sizes<CURVE>::JW, min(SM_AFF_GROUP, m - lo), out + (size_t)lo * sm_sizes<CURVE>::PW, inv_exp);
}
#endif

}  // namespace te
