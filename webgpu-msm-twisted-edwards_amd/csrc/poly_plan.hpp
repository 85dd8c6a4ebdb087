// poly_plan.hpp -- the plan of te_msm_poly_divide* (kernels in poly.hip.hpp): evaluation of `count` polynomials
// of n coefficients over p at a point each, and their quotients by X - z.  The levels of the recursion, what a block's tile is, every
// global, scratch and LDS index a lane forms, the size of the device's scratch buffer and the launch geometry.  HIP-free: points.hip,
// the kernels and the host shim (tests/csrc/polycheck.cpp) take their numbers from here, and the bounds replay of
// tests/test_poly_host.py walks exactly these functions.
//
// With h_(n-1) = a_(n-1), h_i = a_i + z h_(i+1):  a(z) = h_0 and q_i = h_(i+1).  A block of 256 lanes owns a tile of T = 256 chunk
// consecutive coefficients of ONE polynomial (the last tile of a polynomial may be partly filled; no tile spans two polynomials).
//   sums    tile b of level l computes S_b = sum_(k < T) a_(bT + k) z^k  ->  record b of the level's sums
//   carry   H_b = h_(bT) = S_b + z^T H_(b+1): the carries are the quotient of S(X) by X - z^T and a(z) its remainder -- the same problem on
//           tiles = ceil(n / T) coefficients at the point z^T: level l + 1.  The recursion ends at the level with one tile; its one sum
//           is a(z), and its one carry is 0.
//   apply   tile b of level l takes H_(b+1) = record b of level l + 1's quotient and writes h_(i+1) at i.
// Level 0 reads a and writes q (which may be a); level l >= 1 lives in region l of the device's scratch buffer: count x n_l records,
// n_l = tiles of level l - 1, quotient written over the sums.  Region `levels` holds one record a polynomial: the evaluations.
// Behind the regions: the powers of every point, kPowEntries entries of kPowWords words for each (point, level).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "plan_arith.hpp"      // TE_HD

namespace te_poly {

constexpr uint64_t kMaxN = 1ull << 30;             // TE_MSM_POLY_MAX_N
constexpr uint32_t kLanes = 256u;
constexpr uint32_t kChunkMin = 1u, kChunkMax = 16u, kChunkDefault = 8u;        // coefficients of a lane (TE_MSM_POLY_CHUNK: measured)
constexpr uint32_t kMaxLevels = 4u;                // chunk 1: 2^30 -> 2^22 -> 2^14 -> 2^6 -> 1
constexpr uint32_t kRecWords = 8u;                 // a record in LDS: its 8 words, as loaded
constexpr uint32_t kLanePad = 4u;                  // words between the chunks of two lanes: lane pitch 8 chunk + 4, an odd number of 16-byte words
constexpr uint32_t kScanLimbs = 9u;                // a lane's partial value in the scan area: 9 limbs (an odd pitch over the 64 banks)
constexpr uint32_t kPowEntries = 18u, kPowWords = 12u;   // z^(2^j), j = 0 .. 8, then z^(chunk 2^j), j = 0 .. 8 (the last: z^T); 9 limbs in 48 bytes
constexpr uint32_t kPowZ = 0u, kPowC = 9u, kPowLog = 8u;

struct level {
  uint64_t n, tiles;          // coefficients and tiles of one polynomial at this level
  uint64_t src, dst;          // record offsets in the scratch buffer of the level's coefficients (level 0: a itself) and of its sums
};
struct plan {
  uint32_t chunk, T, levels, points;   // points: 1 under SHARED_Z, else count
  uint64_t n, count;
  level lv[kMaxLevels];
  uint64_t records;           // records of all regions
  uint64_t pow_words;         // words of the powers behind them
  uint64_t scratch_bytes;
};

TE_HD uint32_t clamp_chunk(long v) { return v >= (long)kChunkMin && v <= (long)kChunkMax ? (uint32_t)v : kChunkDefault; }
// the chunk of a call: kChunkDefault, or what TE_MSM_POLY_CHUNK names (kChunkMin .. kChunkMax: tools/poly_cost.py measures the candidates
// with it, and the tests reach a deep recursion at small sizes)
inline uint32_t chunk_in_force() {
  const char* e = getenv("TE_MSM_POLY_CHUNK");
  return clamp_chunk(e ? atol(e) : 0);
}
// the chunk a call of polynomials of n coefficients runs at: the chunk in force, but no more than one tile needs to cover n -- a batch of
// polynomials shorter than a tile (1024 x 2^10 at chunk 8) then fills its blocks instead of leaving half of every tile idle
TE_HD uint32_t chunk_for(uint64_t n, uint32_t chunk) {
  const uint64_t need = (n + kLanes - 1) / kLanes;
  return need < chunk ? (need ? (uint32_t)need : 1u) : chunk;
}
TE_HD uint32_t levels_for(uint64_t n, uint32_t chunk) {
  const uint64_t T = (uint64_t)kLanes * chunk;
  uint32_t l = 1;
  for (uint64_t m = (n + T - 1) / T; m > 1; m = (m + T - 1) / T) l++;
  return l;
}
// false: n, count or the chunk is outside what a call may ask, or the grid of a launch would not fit
TE_HD bool make_plan(uint64_t n, uint64_t count, uint32_t chunk, bool shared_z, plan& P) {
  if (n == 0 || n > kMaxN || chunk < kChunkMin || chunk > kChunkMax || count == 0 || count > (UINT64_MAX >> 5) / n) return false;
  P.chunk = chunk; P.T = kLanes * chunk; P.n = n; P.count = count; P.points = shared_z ? 1u : (uint32_t)count;
  if (!shared_z && count >> 31) return false;
  P.levels = levels_for(n, chunk);
  uint64_t m = n, at = 0;
  for (uint32_t l = 0; l < P.levels; l++) {
    level& v = P.lv[l];
    v.n = m; v.tiles = (m + P.T - 1) / P.T;
    if (count > 0x7fffffffull / v.tiles) return false;              // blocks of one launch
    v.src = l ? P.lv[l - 1].dst : 0; v.dst = at;
    at += count * v.tiles;
    m = v.tiles;
  }
  P.records = at;
  P.pow_words = (uint64_t)P.points * P.levels * kPowEntries * kPowWords;
  P.scratch_bytes = P.records * 32u + P.pow_words * 4u;
  return true;
}

// ---- indices -------------------------------------------------------------------------------------------------------------------
// block -> polynomial and tile
struct tile { uint64_t poly, b, base, fill; };     // base: record offset of the tile's first coefficient; fill: coefficients it holds (1 .. T)
TE_HD tile tile_of(const level& v, uint32_t T, uint64_t block) {
  tile t;
  t.poly = block / v.tiles; t.b = block % v.tiles;
  t.base = t.poly * v.n + t.b * T;
  const uint64_t rest = v.n - t.b * T;
  t.fill = rest < T ? rest : T;
  return t;
}
// where tile t's sum goes, and where its carry comes from: record (poly, b) of the next level
TE_HD uint64_t sum_of(const level& v, const tile& t) { return v.dst + t.poly * v.tiles + t.b; }
// coefficient x of a tile as the block loads and stores it: lane + 256 j (every load of a wave covers consecutive records)
TE_HD uint32_t wide_x(uint32_t lane, uint32_t j) { return lane + kLanes * j; }
// ... and as a lane owns it in the apply kernel: chunk consecutive coefficients
TE_HD uint32_t own_x(uint32_t lane, uint32_t j, uint32_t chunk) { return lane * chunk + j; }
// the LDS word of coefficient x of the tile
TE_HD uint32_t lds_word(uint32_t x, uint32_t chunk) { return (x / chunk) * (kRecWords * chunk + kLanePad) + (x % chunk) * kRecWords; }
TE_HD uint32_t lds_data_words(uint32_t chunk) { return kLanes * (kRecWords * chunk + kLanePad); }
TE_HD uint32_t lds_scan_words() { return kLanes * kScanLimbs; }
TE_HD size_t lds_bytes_apply(uint32_t chunk) { return (size_t)(lds_data_words(chunk) + lds_scan_words()) * 4u; }
// entry e of the powers of polynomial `poly` at level l (word offset behind the regions)
TE_HD uint64_t pow_word(const plan& P, uint64_t poly, uint32_t l, uint32_t e) {
  return (((P.points == 1u ? 0 : poly) * P.levels + l) * kPowEntries + e) * kPowWords;
}

}  // namespace te_poly
