// mul_base.hip.hpp -- fixed-base batch scalar multiplication out[i] = [k_i] P over ONE bound point (te_msm_bind_base / te_msm_mul_base*,
// include/te_msm.h "fixed-base batch scalar multiplication").  arkworks' FixedBase::msm / batch_mul.
//
// Like scalar_mul.hip.hpp, the per-lane functions are TE_HD and the kernels sit under __HIPCC__: tests/csrc/mulbasecheck.cpp runs the
// exact code of k_mul_base and k_mul_base_entries on the CPU, through a table accessor that asserts its index.
//
// RECODING: scalar_mul.hip.hpp's offset recoding with a RUN-TIME window W in [4, 12].  K = k + C with C = sum_{i < M} 2^(W-1) 2^(W i),
// M = ceil(257 / W): window i of K is an unsigned W-bit value u_i and d_i = u_i - 2^(W-1) in [-2^(W-1), 2^(W-1)) the signed digit,
// sum d_i 2^(W i) = k.  K < 2^256 + 2^(W M - 1) (1 + 2^-W + ...) < 2^(W M) because W M >= 258 for every W in [4, 12] (257 is prime), so
// the top window takes small non-negative digits and nothing is carried out of it; W M <= 264: nine words.  The words of C are made on
// the host (mb_geometry) and travel as a kernel argument.
//
// TABLE: entry (i, j) = [j 2^(W i)] P for i < M, j = 0 .. H = 2^(W-1): H + 1 entries a window, entry 0 the neutral element where the form
// has one, so the index inside a window is the digit's magnitude itself.  128-byte slots:
//   Twisted-Edwards BLS12  the engine's affine record hm | hp | dt of 9 words each (pnt_from_affine_raw; te_msm_bases_read's layout);
//                          entry 0 is the record of (0, 1): the complete mixed addition adds it like any other
//   BLS12-377 G1           affine short-Weierstrass x | y of 14 words each, Montgomery form (c377_coords); entry 0 holds x = y = 0 mod q (the
//                          affine pass writes infinity as zeros) and never reaches the result: a digit 0 SELECTS the accumulator
// It is built from what is already pinned by tests: the scalars j 2^(W i), reduced on the host mod 4 L (the exponent of the whole
// Twisted-Edwards curve group) or mod r (BLS12-377 G1) -- exact on the whole curve, and they pass 2^256 in the top window --, go through
// k_scalar_mul and k_scalar_mul_affine over the point replicated, and k_mul_base_entries writes the entry form.
//
// THE LANE (mb_lane): one table look-up and one mixed addition a window, no doubling, no branch on the digit.
//   Twisted-Edwards: ete_madd_raw<true>, 7 products.  Its SGN form returns -(a + b) where `neg`; with the opened accumulator negated
//     under the same mask (u and v swapped, t -> 2 p - t: ete_uv_neg's classes, selected instead of branched) that is
//     -((-acc) + e) = acc - e -- the way k_accumulate subtracts.
//   BLS12-377: sw377_add(acc, sw377_cneg(sw377_of(x, y), neg)), the complete law; the accumulator starts at sw377_identity().
//
// ADDRESSING: an entry's index is i (H + 1) + mag, where i < M is the loop counter and mag <= H follows from a digit MASKED to W bits
// (u < 2^W, mag = |u - H| <= H).  M (H + 1) is the table's entry count by construction (mb_geom::entries), so no scalar, whatever
// its bytes, addresses memory outside the table.
#pragma once
#include "scalar_mul.hip.hpp"
#include "scalar_form.hpp"

namespace te {

constexpr int MB_SLOT_WORDS = 32;                                  // a table entry: 128 bytes
constexpr int MB_ENTRY_WORDS = 28;                                 // ... of which a lane reads 7 x 16 (27 used: Twisted-Edwards, 28: BLS12-377)

// what the window bits fix (host-made, a kernel argument): M windows of H + 1 entries, the words of C
struct mb_geom {
  int W, M;
  uint32_t H, entries;                                             // 2^(W-1); M (H + 1)
  uint32_t C[9];
};
inline mb_geom mb_geometry(int W) {
  mb_geom g = {};
  g.W = W; g.M = (257 + W - 1) / W;
  g.H = 1u << (W - 1); g.entries = (uint32_t)g.M * (g.H + 1u);
  for (int j = 0; j < 9; j++) g.C[j] = sm_offset_word(W, g.M, j);
  return g;
}

// K = k + C, 9 words
TE_HD void mb_recode(const uint32_t (&k)[8], const uint32_t (&C)[9], uint32_t (&K)[9]) {
  uint64_t c = 0;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    c += (uint64_t)(j < 8 ? k[j] : 0u) + C[j];
    K[j] = (uint32_t)c;
    c >>= 32;
  }
}
// the lowest window of K as (magnitude, sign) of its signed digit, then K >>= W: called M times it walks the windows upwards.
// The window is masked to W bits, so mag <= H whatever K holds.
TE_HD uint32_t mb_next_digit(uint32_t (&K)[9], int W, uint32_t H, bool& neg) {
  const uint32_t u = K[0] & ((1u << W) - 1u);
#pragma unroll
  for (int j = 0; j < 8; j++) K[j] = (K[j] >> W) | (K[j + 1] << (32 - W));
  K[8] >>= W;
  neg = u < H;
  return neg ? H - u : u - H;
}
// index of entry (i, mag) in the table
TE_HD uint32_t mb_index(const mb_geom& g, int i, uint32_t mag) { return (uint32_t)i * (g.H + 1u) + mag; }

// ---- one window's addition ------------------------------------------------------------------------------------------------------
// acc + (neg ? -e : e), e the affine record in w[0 .. 27)
TE_HD ete mb_step_te(const ete& acc, const uint32_t (&w)[MB_ENTRY_WORDS], bool neg) {
  pnt e;
#pragma unroll
  for (int i = 0; i < 9; i++) { e.hm.v[i] = w[i]; e.hp.v[i] = w[9 + i]; e.dt.v[i] = w[18 + i]; }
  const ete_uv_t<9> a = ete_open<9>(acc);
  const fp nt = fe_neg<2>(a.t);
  const uint32_t m = neg ? 0xffffffffu : 0u;
  ete_uv_t<9> s;
  s.z = a.z;
#pragma unroll
  for (int i = 0; i < 9; i++) {
    s.u.v[i] = mask_select(m, a.v.v[i], a.u.v[i]);
    s.v.v[i] = mask_select(m, a.u.v[i], a.v.v[i]);
    s.t.v[i] = mask_select(m, nt.v[i], a.t.v[i]);
  }
  return ete_madd_raw<true>(s, e, neg);
}
// acc + (neg ? -e : e) for mag != 0, acc for mag == 0 (selected); e = (x, y) in w[0 .. 28)
TE_HD sw377 mb_step_377(const sw377& acc, const uint32_t (&w)[MB_ENTRY_WORDS], uint32_t mag, bool neg) {
  te377::fq x, y;
#pragma unroll
  for (int i = 0; i < 14; i++) { x.v[i] = w[i]; y.v[i] = w[14 + i]; }
  const sw377 s = sw377_add(acc, sw377_cneg(sw377_of(x, y), neg));
  return sw377_select(mag == 0u, acc, s);
}

// ---- one lane: scalar words -> projective result in k_scalar_mul's slot layout (3 N words: X, Y, Z) ------------------------------------
// TAB: load(index, w) reads the first MB_ENTRY_WORDS words of entry `index`.  FORM: what the scalar record holds (scalar_form.hpp).
template <int CURVE, int FORM, class TAB> TE_HD void mb_lane(uint32_t (&k)[8], const mb_geom& g, const TAB& tab, uint32_t* proj) {
  constexpr int N = sm_sizes<CURVE>::N;
  if constexpr (FORM != SCALAR_FORM_CANONICAL) scalar_from_montgomery<FORM>(k);
  uint32_t K[9];
  mb_recode(k, g.C, K);
  fel<N> X, Y, Z;
  if constexpr (CURVE == 1) {
    sw377 acc = sw377_identity();
#pragma unroll 1
    for (int i = 0; i < g.M; i++) {
      bool neg;
      const uint32_t mag = mb_next_digit(K, g.W, g.H, neg);
      uint32_t w[MB_ENTRY_WORDS];
      tab.load(mb_index(g, i, mag), w);
      acc = mb_step_377(acc, w, mag, neg);
    }
    X = acc.x; Y = acc.y; Z = acc.z;
  } else {
    ete acc = ete_identity();
#pragma unroll 1
    for (int i = 0; i < g.M; i++) {
      bool neg;
      const uint32_t mag = mb_next_digit(K, g.W, g.H, neg);
      uint32_t w[MB_ENTRY_WORDS];
      tab.load(mb_index(g, i, mag), w);
      acc = mb_step_te(acc, w, neg);
    }
    X = acc.x; Y = acc.y; Z = acc.z;
  }
#pragma unroll
  for (int i = 0; i < N; i++) { proj[i] = X.v[i]; proj[N + i] = Y.v[i]; proj[2 * N + i] = Z.v[i]; }
}

// ---- a table entry from the canonical affine point k_scalar_mul_affine wrote (wire format), MB_SLOT_WORDS words ---------------------
template <int CURVE> TE_HD void mb_entry(const uint32_t (&w)[sm_sizes<CURVE>::PW], uint32_t (&e)[MB_SLOT_WORDS]) {
#pragma unroll
  for (int i = 0; i < MB_SLOT_WORDS; i++) e[i] = 0u;
  if constexpr (CURVE == 1) {
    te377::fq X, Y, sx;
    c377_coords(w, X, Y, sx);
#pragma unroll
    for (int i = 0; i < 14; i++) { e[i] = X.v[i]; e[14 + i] = Y.v[i]; }
  } else {
    uint32_t xw[8], yw[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { xw[i] = w[i]; yw[i] = w[8 + i]; }
    const pnt r = pnt_from_affine_raw(fp_from_words32(xw), fp_from_words32(yw));
#pragma unroll
    for (int i = 0; i < 9; i++) { e[i] = r.hm.v[i]; e[9 + i] = r.hp.v[i]; e[18 + i] = r.dt.v[i]; }
  }
}

// ---- the table's scalars, on the host: j 2^(W i) mod 4 L (curve 0) or mod r (curve 1), 8 words each, entry order --------------------
// a = a + b mod m for a, b < m < 2^253
inline void mb_add_mod(uint32_t (&a)[8], const uint32_t (&b)[8], const uint32_t* m) {
  uint64_t c = 0;
  for (int j = 0; j < 8; j++) { c += (uint64_t)a[j] + b[j]; a[j] = (uint32_t)c; c >>= 32; }
  if (words_lt<8>(a, m)) return;
  uint64_t br = 0;
  for (int j = 0; j < 8; j++) { const uint64_t s = (uint64_t)a[j] - m[j] - br; a[j] = (uint32_t)s; br = (s >> 63) & 1u; }
}
inline void mb_table_scalars(int curve, const mb_geom& g, uint32_t* out) {
  const uint32_t* m = curve == 1 ? kR377_W32 : kTe4L_W32;
  uint32_t base[8] = {1u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};           // 2^(W i) mod m
  for (int i = 0; i < g.M; i++) {
    uint32_t cur[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (uint32_t j = 0; j <= g.H; j++) {
      memcpy(out + (size_t)mb_index(g, i, j) * 8, cur, 32);
      mb_add_mod(cur, base, m);
    }
    for (int s = 0; s < g.W; s++) { uint32_t twice[8]; memcpy(twice, base, 32); mb_add_mod(base, twice, m); }
  }
}

#if defined(__HIPCC__)
// the table in device memory: entry `index` < g.entries by construction (ADDRESSING above) -- i is the loop counter, mag a masked digit
struct mb_device_table {
  const uint4* t;
  __device__ __forceinline__ void load(uint32_t index, uint32_t (&w)[MB_ENTRY_WORDS]) const {
    const uint4* e = t + (size_t)index * (MB_SLOT_WORDS / 4);
#pragma unroll
    for (int j = 0; j < MB_ENTRY_WORDS / 4; j++) { const uint4 v = e[j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
  }
};
// one lane per scalar of a piece of m; no early exit inside the window loop.  SQ: 16-byte words of a scalar record, as k_scalar_mul's
template <int CURVE, int FORM, int SQ = (CURVE == 1 ? 3 : 2)> __global__ __launch_bounds__(256) void k_mul_base(const uint4* __restrict__ table, const uint4* __restrict__ sc, uint32_t m,
                                                                                 uint4* __restrict__ proj, mb_geom g) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int JQ = sm_sizes<CURVE>::JW / 4;
  uint32_t k[8];
#pragma unroll
  for (int j = 0; j < 2; j++) { const uint4 v = sc[(size_t)i * SQ + j]; k[4 * j] = v.x; k[4 * j + 1] = v.y; k[4 * j + 2] = v.z; k[4 * j + 3] = v.w; }
  uint32_t o[4 * JQ];
#pragma unroll
  for (int j = 0; j < 4 * JQ; j++) o[j] = 0u;
  const mb_device_table tab = {table};
  mb_lane<CURVE, FORM>(k, g, tab, o);
#pragma unroll
  for (int j = 0; j < JQ; j++) proj[(size_t)i * JQ + j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
}
// one lane per table entry: the m canonical affine points of k_scalar_mul_affine -> m entries
template <int CURVE> __global__ __launch_bounds__(256) void k_mul_base_entries(const uint4* __restrict__ pts, uint32_t m, uint4* __restrict__ table) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int PQ = sm_sizes<CURVE>::PW / 4;
  uint32_t w[4 * PQ], e[MB_SLOT_WORDS];
#pragma unroll
  for (int j = 0; j < PQ; j++) { const uint4 v = pts[(size_t)i * PQ + j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
  mb_entry<CURVE>(w, e);
#pragma unroll
  for (int j = 0; j < MB_SLOT_WORDS / 4; j++) table[(size_t)i * (MB_SLOT_WORDS / 4) + j] = make_uint4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
}
#endif

}  // namespace te
