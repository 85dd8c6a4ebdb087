// scan_plan.hpp -- the plan of te_msm_field_scan* (kernels in scan.hip.hpp): prefix sums and prefix products of
// `count` vectors of n records over p, each from a seed.  The levels of the recursion, what a block's tile is, every global, scratch and
// LDS index a lane forms, where the sum path reduces, the size of the device's scratch buffer and the launch geometry.  HIP-free:
// points.hip, the kernels and the host shim (tests/csrc/scancheck.cpp) take their numbers from here, and the bounds replay and the
// interval test of tests/test_scan_host.py walk exactly these functions.
//
// Write o for + or * mod p.  A block of 256 lanes owns a tile of T = 256 chunk consecutive elements of ONE vector (the last tile of a
// vector may be partly filled; no tile spans two vectors; padding is the identity of o).
//   totals  tile b of level l computes t_b = a_(bT) o .. o a_(bT + T - 1)  ->  record b of the level's totals
//   carry   c_b = e o t_0 o .. o t_(b-1): the EXCLUSIVE scan of the totals from the seed e -- the same problem on tiles = ceil(n / T)
//           records: level l + 1.  The recursion ends at the level with one tile; its carry is the seed, and its total combined with the
//           seed is the vector's total.
//   apply   tile b of level l takes c_b = record b of level l + 1's exclusive scan and writes the inclusive or exclusive values.
// Level 0 reads a (under SHARED_A: record `vec` of a for every element) and writes out (which may be a); level l >= 1 lives in region l - 1
// of the device's scratch buffer: count x n_l records, n_l = tiles of level l - 1, its exclusive scan written over its elements.  Region
// levels - 1 holds one record a vector: the totals, in the caller's form.  Behind the regions: one record a vector, the seeds.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include "plan_arith.hpp"      // TE_HD

namespace te_scan {

constexpr uint64_t kMaxN = 1ull << 30;             // TE_MSM_SCAN_MAX_N
constexpr uint32_t kLanes = 256u;
constexpr uint32_t kChunkMin = 1u, kChunkMax = 16u, kChunkDefault = 8u;        // elements of a lane (TE_MSM_SCAN_CHUNK: measured)
constexpr uint32_t kMaxLevels = 4u;                // chunk 1: 2^30 -> 2^22 -> 2^14 -> 2^6 -> 1
constexpr uint32_t kRecWords = 8u;                 // a record in LDS: 8 words
constexpr uint32_t kLanePad = 4u;                  // words between the chunks of two lanes: lane pitch 8 chunk + 4, an odd number of 16-byte words
constexpr uint32_t kScanLimbs = 9u;                // a lane's value in the scan area: 9 limbs (an odd pitch over the 64 banks)
constexpr uint32_t kLog = 8u;                      // steps of the tree and of the scan over 256 lanes
enum { kSum = 0, kProduct = 1 };                   // TE_MSM_SCAN_SUM, TE_MSM_SCAN_PRODUCT
// what a record holds where a launch reads or writes it.  kInternal is the form of the scratch regions, the seeds and the LDS tile:
//   sum      the canonical words of the value (a seed: its 256 bits as given); nothing is decoded, and both caller's forms are the same code
//   product  the canonical words of v R mod p, R = 2^261 -- read back as limbs they ARE the Montgomery form of fp.hpp: no decoding product
enum { kInternal = 0, kCanonical = 1, kMontgomery = 2 };

// ---- where the sum path reduces (one product with R mod p: class N below R -> below value x 0.79 / 438.8 + p) ----------------------------
// The kernels ask these functions, and the interval test replays the bounds from what they answer.  2^256 = 13.72 p, R = 2^261 = 438.8 p;
// a value must stay below R wherever it is stored as 9 limbs or enters a product (class N with a top limb below 2^29).
//   a lane's own total   chunk <= 16 records below 13.72 p: below 219.5 p.  REDUCED: below 1.40 p
//   tree / scan steps    8 steps sum at most 256 lanes' totals: below 256 x 1.40 p = 358.4 p.  not reduced
//   + the carry          a scratch record below p, or a seed below 13.72 p: below 372.1 p.  the totals kernel writes it (scan_out reduces);
//   the lane's prefix    REDUCED in the apply kernel: below 1.67 p -- the walk then adds chunk records: below 221.2 p, and every output is
//                        reduced (below 1.40 p) and made canonical by one conditional subtraction
TE_HD bool sum_reduces_lane_total() { return true; }
TE_HD bool sum_reduces_step(uint32_t) { return false; }
TE_HD bool sum_reduces_prefix() { return true; }

struct level {
  uint64_t n, tiles;          // elements and tiles of one vector at this level
  uint64_t src, dst;          // record offsets in the scratch buffer of the level's elements (level 0: a itself) and of its totals
};
struct plan {
  uint32_t chunk, T, levels;
  uint64_t n, count;
  level lv[kMaxLevels];
  uint64_t seeds;             // record offset of the seeds: one a vector
  uint64_t records;           // records of all regions and the seeds
  uint64_t scratch_bytes;
};

TE_HD uint32_t clamp_chunk(long v) { return v >= (long)kChunkMin && v <= (long)kChunkMax ? (uint32_t)v : kChunkDefault; }
// the chunk of a call: kChunkDefault, or what TE_MSM_SCAN_CHUNK names (kChunkMin .. kChunkMax: tools/scan_cost.py measures the candidates
// with it, and the tests reach a deep recursion at small sizes)
inline uint32_t chunk_in_force() {
  const char* e = getenv("TE_MSM_SCAN_CHUNK");
  return clamp_chunk(e ? atol(e) : 0);
}
// the chunk a call of vectors of n elements runs at: the chunk in force, but no more than one tile needs to cover n
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
TE_HD bool make_plan(uint64_t n, uint64_t count, uint32_t chunk, plan& P) {
  if (n == 0 || n > kMaxN || chunk < kChunkMin || chunk > kChunkMax || count == 0 || count > (UINT64_MAX >> 5) / n) return false;
  P.chunk = chunk; P.T = kLanes * chunk; P.n = n; P.count = count;
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
  P.seeds = at;
  P.records = at + count;
  P.scratch_bytes = P.records * 32u;
  return true;
}

// ---- indices -------------------------------------------------------------------------------------------------------------------
// block -> vector and tile
struct tile { uint64_t vec, b, base, fill; };      // base: record offset of the tile's first element; fill: elements it holds (1 .. T)
TE_HD tile tile_of(const level& v, uint32_t T, uint64_t block) {
  tile t;
  t.vec = block / v.tiles; t.b = block % v.tiles;
  t.base = t.vec * v.n + t.b * T;
  const uint64_t rest = v.n - t.b * T;
  t.fill = rest < T ? rest : T;
  return t;
}
// where tile t's total goes, and where its carry comes from (relative to the level's totals / carries): record (vec, b).  At the last
// level tiles = 1 and this is the vector's number: its seed, and its total
TE_HD uint64_t total_of(const level& v, const tile& t) { return t.vec * v.tiles + t.b; }
// the record a block loads for element x of its tile: the element itself, or -- SHARED_A, level 0 -- the vector's one record
TE_HD uint64_t load_of(const tile& t, uint32_t x, bool shared) { return shared ? t.vec : t.base + x; }
// element x of a tile as the block loads and stores it: lane + 256 j (every load of a wave covers consecutive records)
TE_HD uint32_t wide_x(uint32_t lane, uint32_t j) { return lane + kLanes * j; }
// ... and as a lane owns it in the apply kernel: chunk consecutive elements
TE_HD uint32_t own_x(uint32_t lane, uint32_t j, uint32_t chunk) { return lane * chunk + j; }
// the LDS word of element x of the tile
TE_HD uint32_t lds_word(uint32_t x, uint32_t chunk) { return (x / chunk) * (kRecWords * chunk + kLanePad) + (x % chunk) * kRecWords; }
TE_HD uint32_t lds_data_words(uint32_t chunk) { return kLanes * (kRecWords * chunk + kLanePad); }
TE_HD uint32_t lds_scan_words() { return kLanes * kScanLimbs; }
TE_HD size_t lds_bytes_apply(uint32_t chunk) { return (size_t)(lds_data_words(chunk) + lds_scan_words()) * 4u; }

}  // namespace te_scan
