// poly.hip.hpp -- evaluate polynomials over p and divide them by X - z (te_msm_poly_divide*; include/te_msm.h "polynomial openings",
// DESIGN.md section 23): with h_(n-1) = a_(n-1), h_i = a_i + z h_(i+1), evals = h_0 = a(z) and q_i = h_(i+1), q_(n-1) = 0 -- the
// witness polynomial of a KZG opening.  poly_plan.hpp says which levels a call runs and forms every index; this file is the arithmetic
// of one lane in each phase of a block, and the two kernels.
//
// Like ntt.hip.hpp, the per-lane functions are TE_HD and the kernels sit under __HIPCC__: tests/csrc/polycheck.cpp runs a block on the
// CPU as plain loops over its lanes, one loop per phase (a loop boundary is the block's barrier).
//
// THE RECURRENCE IS LINEAR in the coefficients.  z is held in the Montgomery form of fp.hpp (z R, one product with R^2 or R^2 / A on the
// host), and mont_mul(z R, h) = z h: coefficients and partial values never enter that form, and the same code serves canonical records
// and MONTGOMERY ones (a A in, h A out).  A step is  h' = norm(a + mont_mul(z R, h))  -- one product and one normalised sum.
// TWO KERNELS, a block of 256 lanes on a tile of T = 256 chunk coefficients (chunk is a run-time argument):
//   k_poly_sums   lane l walks the coefficients l + 256 j of its tile from the top with the point z^256 (every load of a wave covers 64
//                 consecutive records), then 8 log-steps through LDS combine the lanes with z^(2^s): lane 0 holds S_b = sum a_(bT+k) z^k
//                 and writes it canonical (one product more a TILE).  One product a coefficient; nothing else is read or written.
//   k_poly_apply  the tile goes through LDS: loaded as k_poly_sums loads it and stored as its 8 words; behind the barrier lane l owns the
//                 chunk CONSECUTIVE coefficients l chunk .. l chunk + chunk - 1.  It walks them once for its own sum L_l (point z), the top
//                 lane takes the tile's carry H_(b+1) in (z^chunk), 8 Hillis-Steele steps with z^(chunk 2^s) leave in lane l the value h at
//                 its first coefficient, and lane l takes lane l + 1's: h just past its last coefficient.  It then walks its chunk again:
//                 h_(i+1) is made canonical (one product) and stored over a_i in LDS, then h_i = a_i + z h_(i+1).  Behind a second barrier
//                 the tile is stored as it was loaded.  A block reads its tile before its first barrier and writes behind its last: q may be a.
//   PRODUCTS a coefficient: sums 1; apply 3 (own sum, walk, canonical output) + 17 / chunk.  The issue's sketch has 3 in all: it would keep
//   the lanes' sums of the first kernel (n / chunk records of scratch written and read) where this file computes them again in the apply
//   kernel from the copy of the tile it holds in LDS anyway; lanes 256 apart cannot apply the carry without a scan ACROSS lanes for every
//   row (8 products a coefficient), so the apply kernel owns consecutive coefficients and pays LDS for the transposition.
// LIMBS AND VALUES of everything stored.  LDS tile: the 8 words of a record as loaded, any 256-bit value (below 13.8 p), and behind the
//   walk canonical words.  Powers (device table, 9 limbs in 48 bytes): product outputs, class N below 1.2 p.  A step takes a (class N,
//   below 2^256) and h below B and leaves norm(a + t), t = z R h / R + p < B / 405 + p (R = 446 p): class N below 2^256 + p + B / 405, so
//   B < 14.9 p for any walk from a value below 40 p.  A combine adds t < p + B' / 405 to a value of class N: the 8 steps of a scan (and the
//   carry's) take a lane's sum from 14.9 p to below 14.9 p + 9 (p + 40 p / 405) < 25 p -- what the scan area holds (9 limbs, class N), far
//   below class N's 2^261 and below the 2^258 = 55 p that fo_residue takes.  Sums, carries and evaluations in the scratch buffer:
//   canonical words (fo_words of fo_residue), read back as coefficients.  Every product takes a class N operand below 1.2 p and a
//   class N one below 25 p.
// Every global index is poly_plan.hpp's tile_of / sum_of, guarded by the tile's `fill`; every LDS index its lds_word.  All offsets are 64 bits wide.
#pragma once
#include <string.h>
#include "field_ops.hip.hpp"
#include "poly_plan.hpp"

namespace te {

TE_HD fel<9> poly_pow(const uint32_t* t, uint32_t e) {
  fel<9> r;
  const uint32_t* p = t + (size_t)te_poly::kPowWords * e;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = p[k];
  return r;
}
// h' = a + z h: one product, one normalised sum
TE_HD void poly_step(const uint32_t (&w)[8], const fel<9>& zp, fel<9>& h) { h = fe_norm(fe_add(fp_from_words32(w), fe_mul(zp, h))); }
// v + z^k u
TE_HD fel<9> poly_combine(const fel<9>& v, const fel<9>& zp, const fel<9>& u) { return fe_norm(fe_add(v, fe_mul(zp, u))); }
// a partial value (class N below 2^258) -> canonical words
TE_HD void poly_out(const fel<9>& h, uint32_t (&w)[8]) { fo_words<9, 8>(fo_residue(h), w); }
TE_HD void poly_scan_put(uint32_t* scan, uint32_t lane, const fel<9>& v) {
#pragma unroll
  for (int k = 0; k < 9; k++) scan[lane * te_poly::kScanLimbs + k] = v.v[k];
}
TE_HD fel<9> poly_scan_get(const uint32_t* scan, uint32_t lane) {
  fel<9> r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = scan[lane * te_poly::kScanLimbs + k];
  return r;
}
TE_HD void poly_lds_put(uint32_t* lds, uint32_t word, const uint32_t (&w)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) lds[word + k] = w[k];
}
TE_HD void poly_lds_get(const uint32_t* lds, uint32_t word, uint32_t (&w)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = lds[word + k];
}
// step s of the tree of k_poly_sums: lane l takes lane l + 2^s in when l is a multiple of 2^(s+1)
TE_HD bool poly_tree_takes(uint32_t lane, uint32_t s) { return (lane & ((2u << s) - 1u)) == 0u; }
// step s of the scan of k_poly_apply: lane l takes lane l + 2^s in when there is one
TE_HD bool poly_scan_takes(uint32_t lane, uint32_t s) { return lane + (1u << s) < te_poly::kLanes; }

// ---- what a call computes on the host before it launches (points.hip; the shim of the CPU tests calls the same functions) ------------
struct poly_req { uint64_t n = 0, count = 0; bool mont = false, shared = false; uint32_t chunk = te_poly::kChunkDefault; };
enum { POLY_OK = 0, POLY_BAD_N, POLY_BAD_FLAGS, POLY_NO_OUTPUT, POLY_TOO_LARGE, POLY_NULL };
// what every te_msm_poly_divide* call checks first: POLY_OK with r filled, or why it is refused
inline int poly_check(const void* a, uint64_t n, uint64_t count, const uint8_t* z, int flags, const void* evals, const void* q, poly_req& r) {
  if (n == 0 || n > TE_MSM_POLY_MAX_N) return POLY_BAD_N;
  if (flags & ~(TE_MSM_POLY_MONTGOMERY | TE_MSM_POLY_SHARED_Z)) return POLY_BAD_FLAGS;
  if (!evals && !q) return POLY_NO_OUTPUT;
  if (count > (UINT64_MAX >> 5) / n) return POLY_TOO_LARGE;
  if (count > 0 && (!a || !z)) return POLY_NULL;
  r.n = n; r.count = count; r.mont = (flags & TE_MSM_POLY_MONTGOMERY) != 0; r.shared = (flags & TE_MSM_POLY_SHARED_Z) != 0;
  return POLY_OK;
}
// the kPowEntries powers of one level from its point (Montgomery form): z^(2^j), j = 0 .. 8, and z^(chunk 2^j), j = 0 .. 8; the last
// one, z^T, is the point of the next level.  25 products
inline void poly_level_pows(const fel<9>& zr, uint32_t chunk, fel<9> (&e)[te_poly::kPowEntries]) {
  e[te_poly::kPowZ] = zr;
  for (uint32_t j = 1; j <= te_poly::kPowLog; j++) e[te_poly::kPowZ + j] = fe_mul(e[te_poly::kPowZ + j - 1], e[te_poly::kPowZ + j - 1]);
  fel<9> c = fe_one<9>();
  for (int b = 4; b >= 0; b--) {
    c = fe_mul(c, c);
    if ((chunk >> b) & 1u) c = fe_mul(c, zr);
  }
  e[te_poly::kPowC] = c;
  for (uint32_t j = 1; j <= te_poly::kPowLog; j++) e[te_poly::kPowC + j] = fe_mul(e[te_poly::kPowC + j - 1], e[te_poly::kPowC + j - 1]);
}
// the table of a call: for every point (one under SHARED_Z) and level, the entries above as kPowWords words each
inline void poly_pow_table(const te_poly::plan& P, const uint8_t* z, bool mont, uint32_t* out) {
  for (uint32_t k = 0; k < P.points; k++) {
    uint32_t w[8];
    memcpy(w, z + (size_t)32 * k, 32);
    fel<9> zr = mont ? fo_decode<9, true>(w) : fo_decode<9, false>(w);
    for (uint32_t l = 0; l < P.levels; l++) {
      fel<9> e[te_poly::kPowEntries];
      poly_level_pows(zr, P.chunk, e);
      for (uint32_t i = 0; i < te_poly::kPowEntries; i++) {
        uint32_t* o = out + te_poly::pow_word(P, k, l, i);
        for (uint32_t j = 0; j < te_poly::kPowWords; j++) o[j] = j < 9u ? e[i].v[j] : 0u;
      }
      zr = e[te_poly::kPowC + te_poly::kPowLog];
    }
  }
}

#if defined(__HIPCC__)
// grid = count x tiles of the level; a: the level's coefficients, sums: record (poly, b) of the next level; pw: the level's entries of
// polynomial 0, pow_stride words from one polynomial's to the next's (0 under SHARED_Z)
__global__ __launch_bounds__(256) void k_poly_sums(const uint4* __restrict__ a, uint4* __restrict__ sums, te_poly::level v, uint32_t chunk, const uint32_t* __restrict__ pw,
                                                   uint64_t pow_stride) {
  __shared__ uint32_t scan[te_poly::kLanes * te_poly::kScanLimbs];
  const uint32_t lane = threadIdx.x;
  const te_poly::tile t = te_poly::tile_of(v, te_poly::kLanes * chunk, blockIdx.x);
  const uint32_t* pows = pw + (size_t)t.poly * pow_stride;
  const fel<9> z256 = poly_pow(pows, te_poly::kPowZ + te_poly::kPowLog);
  fel<9> acc = fe_zero<9>();
#pragma unroll 1
  for (uint32_t j = chunk; j-- > 0u;) {
    const uint32_t x = te_poly::wide_x(lane, j);
    if (x >= t.fill) continue;
    uint32_t w[8];
    fo_load<2>(a, (size_t)(t.base + x) * 2, w);
    poly_step(w, z256, acc);
  }
#pragma unroll 1
  for (uint32_t s = 0; s < te_poly::kPowLog; s++) {
    poly_scan_put(scan, lane, acc);
    __syncthreads();
    if (poly_tree_takes(lane, s)) acc = poly_combine(acc, poly_pow(pows, te_poly::kPowZ + s), poly_scan_get(scan, lane + (1u << s)));
    __syncthreads();
  }
  if (lane == 0u) {
    uint32_t w[8];
    poly_out(acc, w);
    fo_store<2>(sums, (size_t)(t.poly * v.tiles + t.b) * 2, w);
  }
}
// the same grid; carries: record (poly, b) of the next level's quotient, or nullptr at the last level (one tile: its carry is 0).  a and
// q are not __restrict__: q may be a.  Dynamic LDS: te_poly::lds_bytes_apply(chunk)
__global__ __launch_bounds__(256) void k_poly_apply(const uint4* a, uint4* q, const uint4* carries, te_poly::level v, uint32_t chunk, const uint32_t* __restrict__ pw,
                                                    uint64_t pow_stride) {
  extern __shared__ uint32_t poly_lds[];
  uint32_t* const lds = poly_lds;
  uint32_t* const scan = poly_lds + te_poly::lds_data_words(chunk);
  const uint32_t lane = threadIdx.x;
  const te_poly::tile t = te_poly::tile_of(v, te_poly::kLanes * chunk, blockIdx.x);
  const uint32_t* pows = pw + (size_t)t.poly * pow_stride;
#pragma unroll 1
  for (uint32_t j = 0; j < chunk; j++) {
    const uint32_t x = te_poly::wide_x(lane, j);
    uint32_t w[8] = {};
    if (x < t.fill) fo_load<2>(a, (size_t)(t.base + x) * 2, w);
    poly_lds_put(lds, te_poly::lds_word(x, chunk), w);
  }
  uint32_t cw[8] = {};
  if (carries && lane == te_poly::kLanes - 1u) fo_load<2>(carries, (size_t)(t.poly * v.tiles + t.b) * 2, cw);
  __syncthreads();
  const fel<9> z1 = poly_pow(pows, te_poly::kPowZ);
  fel<9> acc = fe_zero<9>();
#pragma unroll 1
  for (uint32_t j = chunk; j-- > 0u;) {
    uint32_t w[8];
    poly_lds_get(lds, te_poly::lds_word(te_poly::own_x(lane, j, chunk), chunk), w);
    poly_step(w, z1, acc);
  }
  if (lane == te_poly::kLanes - 1u) acc = poly_combine(acc, poly_pow(pows, te_poly::kPowC), fp_from_words32(cw));
#pragma unroll 1
  for (uint32_t s = 0; s < te_poly::kPowLog; s++) {
    poly_scan_put(scan, lane, acc);
    __syncthreads();
    if (poly_scan_takes(lane, s)) acc = poly_combine(acc, poly_pow(pows, te_poly::kPowC + s), poly_scan_get(scan, lane + (1u << s)));
    __syncthreads();
  }
  poly_scan_put(scan, lane, acc);
  __syncthreads();
  fel<9> h = lane == te_poly::kLanes - 1u ? fp_from_words32(cw) : poly_scan_get(scan, lane + 1u);
#pragma unroll 1
  for (uint32_t j = chunk; j-- > 0u;) {
    const uint32_t at = te_poly::lds_word(te_poly::own_x(lane, j, chunk), chunk);
    uint32_t w[8], o[8];
    poly_lds_get(lds, at, w);
    poly_out(h, o);
    poly_lds_put(lds, at, o);
    poly_step(w, z1, h);
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t j = 0; j < chunk; j++) {
    const uint32_t x = te_poly::wide_x(lane, j);
    if (x >= t.fill) continue;
    uint32_t w[8];
    poly_lds_get(lds, te_poly::lds_word(x, chunk), w);
    fo_store<2>(q, (size_t)(t.base + x) * 2, w);
  }
}
#endif

}  // namespace te
