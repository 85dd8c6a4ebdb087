// spmv_plan.hpp -- the plan of te_msm_bind_matrix / te_msm_spmv* (kernels in spmv.hip.hpp): products of a sparse
// matrix over p, bound once in CSR form, with `count` vectors.  What a bind lays down on a device, what a block's tile is, every global,
// scratch and LDS index a lane forms, the size of the call's scratch buffer and the launch geometry.  HIP-free: points.hip, the kernels
// and the host shim (tests/csrc/spmvcheck.cpp) take their numbers from here, and the bounds replay of tests/test_spmv_host.py walks
// exactly these functions.
//
// ONE SIDE of a bound matrix (the matrix itself, or its transpose as a CSR matrix of its own) is one device allocation:
//   vals  nnz records of 32 bytes: v R mod p, canonical words (R = 2^261 of fp.hpp: mont_mul(v R, x) = v x, x never enters that form)
//   ptr   rows + 1 offsets of 64 bits: row r holds the entries ptr[r] .. ptr[r + 1] - 1
//   col   nnz column indices of 32 bits
//   row   nnz row ids of 32 bits: the row of every entry (the layout the tile kernel reads: a tile needs no table of its own)
// A TILE is T = 256 chunk consecutive ENTRIES of the stream, cut by position and never by row: tiles = ceil(nnz / T), whatever the rows.
//   k_spmv_tile  grid count x tiles.  Rows that begin and end inside a tile are summed and written there.  The run of a row that began
//                before the tile goes to fragment 0 of the tile, the run of a row that goes on past it (and began inside) to fragment 1:
//                two canonical records a tile and vector in the scratch buffer, written as 0 when the tile has no such run.
//   k_spmv_rows  grid count x max(tiles, ceil(rows / 256)).  Block b writes 0 for the empty rows among rows 256 b .. 256 b + 255, and --
//                when tile b's last row began inside it and goes on past it -- sums that row: fragment 1 of tile b and fragment 0 of
//                every tile up to the one the row ends in, lanes striding over the tiles, a tree through LDS.
// Every record of out is written exactly once: a row with entries by the one block that closes it, an empty row by k_spmv_rows.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "plan_arith.hpp"      // TE_HD

namespace te_spmv {

constexpr uint64_t kMaxDim = 1ull << 31;           // rows and cols of a bound matrix
constexpr uint64_t kMaxNnz = 1ull << 40;           // entries of a bound matrix (40 bytes each and side)
constexpr uint32_t kLanes = 256u;
constexpr uint32_t kChunkMin = 1u, kChunkMax = 16u, kChunkDefault = 4u;        // entries of a lane (TE_MSM_SPMV_CHUNK: measured)
constexpr uint32_t kLimbs = 9u;                    // a product in LDS: 9 limbs
constexpr uint32_t kHead = 0u, kTail = 1u, kFrags = 2u;      // the fragments of a tile
constexpr uint32_t kScanSteps = 8u, kScanReduce = 3u;        // the scan over the lanes reduces behind step kScanReduce (its fourth)
constexpr uint32_t kRowFold = 32u;                 // k_spmv_rows: fragments a lane adds between two reductions

TE_HD uint32_t clamp_chunk(long v) { return v >= (long)kChunkMin && v <= (long)kChunkMax ? (uint32_t)v : kChunkDefault; }
// the chunk of a call: kChunkDefault, or what TE_MSM_SPMV_CHUNK names (kChunkMin .. kChunkMax: tools/spmv_cost.py measures the candidates
// with it, and the tests reach many tiles at a few hundred entries)
inline uint32_t chunk_in_force() {
  const char* e = getenv("TE_MSM_SPMV_CHUNK");
  return clamp_chunk(e ? atol(e) : 0);
}

// ---- what a bind lays down -----------------------------------------------------------------------------------------------------
struct layout { uint64_t vals, ptr, col, row, bytes; };       // byte offsets of the four arrays of one side, and its size
TE_HD layout layout_of(uint64_t rows, uint64_t nnz) {
  layout l;
  l.vals = 0; l.ptr = 32u * nnz; l.col = l.ptr + 8u * (rows + 1u); l.row = l.col + 4u * nnz; l.bytes = l.row + 4u * nnz;
  return l;
}
// row[e] = the row of entry e (row_ptr: checked, monotone from 0)
inline void fill_rows(const uint64_t* row_ptr, uint64_t rows, uint32_t* row) {
  for (uint64_t r = 0; r < rows; r++)
    for (uint64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) row[e] = (uint32_t)r;
}
// the transpose as a CSR matrix of cols rows: a STABLE counting sort by column -- the entries of a column keep the order of their rows,
// and of their positions inside a row (a repeated column).  t_ptr: cols + 1 offsets; t_col: the row every entry came from; t_vals:
// its 32-byte record
inline void transpose(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const uint8_t* vals, uint64_t* t_ptr, uint32_t* t_col,
                      uint8_t* t_vals) {
  const uint64_t nnz = row_ptr[rows];
  for (uint64_t c = 0; c <= cols; c++) t_ptr[c] = 0;
  for (uint64_t e = 0; e < nnz; e++) t_ptr[(uint64_t)col_idx[e] + 1u]++;
  for (uint64_t c = 0; c < cols; c++) t_ptr[c + 1] += t_ptr[c];
  uint64_t* next = (uint64_t*)malloc((size_t)(cols ? cols : 1u) * sizeof(uint64_t));
  memcpy(next, t_ptr, (size_t)cols * sizeof(uint64_t));
  for (uint64_t r = 0; r < rows; r++)
    for (uint64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) {
      const uint64_t at = next[col_idx[e]]++;
      t_col[at] = (uint32_t)r;
      memcpy(t_vals + at * 32u, vals + e * 32u, 32);
    }
  free(next);
}

// ---- what a call runs ----------------------------------------------------------------------------------------------------------
struct plan {
  uint32_t chunk, T;
  uint64_t rows, cols, nnz, count;     // of the side the call multiplies by: out is count x rows, x is count x cols
  uint64_t tiles;                      // ceil(nnz / T)
  uint64_t row_blocks;                 // ceil(rows / 256)
  uint64_t per;                        // blocks of k_spmv_rows a vector: max(tiles, row_blocks)
  uint64_t frag_records;               // count x tiles x 2
  uint64_t scratch_bytes;
};
// false: a size is outside what a call may ask, a byte count does not fit 64 bits, or the grid of a launch would not fit
TE_HD bool make_plan(uint64_t rows, uint64_t cols, uint64_t nnz, uint64_t count, uint32_t chunk, plan& P) {
  if (rows == 0 || rows > kMaxDim || cols == 0 || cols > kMaxDim || nnz > kMaxNnz || chunk < kChunkMin || chunk > kChunkMax || count == 0) return false;
  if (count > (UINT64_MAX >> 5) / rows || count > (UINT64_MAX >> 5) / cols) return false;
  P.chunk = chunk; P.T = kLanes * chunk; P.rows = rows; P.cols = cols; P.nnz = nnz; P.count = count;
  P.tiles = (nnz + P.T - 1u) / P.T;
  P.row_blocks = (rows + kLanes - 1u) / kLanes;
  P.per = P.tiles > P.row_blocks ? P.tiles : P.row_blocks;
  if (count > 0x7fffffffull / P.per) return false;                  // blocks of one launch
  P.frag_records = count * P.tiles * kFrags;
  P.scratch_bytes = P.frag_records * 32u;
  return true;
}

// ---- indices -------------------------------------------------------------------------------------------------------------------
// block of k_spmv_tile -> vector and tile
struct tile { uint64_t vec, t, base; uint32_t fill; };            // base: the tile's first entry; fill: entries it holds (1 .. T)
TE_HD tile tile_of(const plan& P, uint64_t block) {
  tile t;
  t.vec = block / P.tiles; t.t = block % P.tiles;
  t.base = t.t * P.T;
  const uint64_t rest = P.nnz - t.base;
  t.fill = rest < P.T ? (uint32_t)rest : P.T;
  return t;
}
// block of k_spmv_rows -> vector and its number inside the vector
struct row_block { uint64_t vec, b; };
TE_HD row_block row_block_of(const plan& P, uint64_t block) { row_block r; r.vec = block / P.per; r.b = block % P.per; return r; }
// entry x of a tile as the block loads it: lane + 256 j (every load of a wave covers consecutive records)
TE_HD uint32_t wide_x(uint32_t lane, uint32_t j) { return lane + kLanes * j; }
// ... and as a lane owns it behind the barrier: chunk consecutive entries
TE_HD uint32_t own_x(uint32_t lane, uint32_t j, uint32_t chunk) { return lane * chunk + j; }
// the LDS word of the product of entry x: a lane's chunk products lie together, at an odd pitch from lane to lane
TE_HD uint32_t lane_pitch(uint32_t chunk) { return (kLimbs * chunk) | 1u; }
TE_HD uint32_t lds_word(uint32_t x, uint32_t chunk) { return (x / chunk) * lane_pitch(chunk) + (x % chunk) * kLimbs; }
TE_HD uint32_t lds_data_words(uint32_t chunk) { return kLanes * lane_pitch(chunk); }
// the scan area lies over the start of the products, behind a barrier of its own: 9 limbs a lane
TE_HD uint32_t scan_word(uint32_t lane) { return lane * kLimbs; }
TE_HD uint32_t lds_scan_words() { return kLanes * kLimbs; }
TE_HD size_t lds_bytes(uint32_t chunk) { return (size_t)lds_data_words(chunk) * 4u; }
// records: element c of vector v of x, row r of vector v of out, fragment `which` of tile t of vector v
TE_HD uint64_t x_of(const plan& P, uint64_t vec, uint32_t c) { return vec * P.cols + c; }
TE_HD uint64_t out_of(const plan& P, uint64_t vec, uint64_t r) { return vec * P.rows + r; }
TE_HD uint64_t frag_of(const plan& P, uint64_t vec, uint64_t t, uint32_t which) { return (vec * P.tiles + t) * kFrags + which; }
// the tile that holds entry e
TE_HD uint64_t tile_holding(const plan& P, uint64_t e) { return e / P.T; }

}  // namespace te_spmv
