// spmv.hip.hpp -- products of a bound sparse matrix over p with `count` vectors (te_msm_bind_matrix, te_msm_spmv*; include/te_msm.h
// "sparse matrices"):  out[k rows + r] = sum_e vals[e] x[k cols + col[e]] mod p  over the entries e of row r --
// the Az, Bz, Cz every R1CS prover starts with.  spmv_plan.hpp says what a bind lays down, what a tile is and forms every index; this
// file is the arithmetic of one lane in each phase of a block, and the two kernels.
//
// Like poly.hip.hpp, the per-lane functions are TE_HD and the kernels sit under __HIPCC__: tests/csrc/spmvcheck.cpp runs a block on the
// CPU as plain loops over its lanes, one loop per phase (a loop boundary is the block's barrier).
//
// THE PRODUCT IS LINEAR in x.  The values are held in the Montgomery form of fp.hpp (v R mod p as canonical words, one product with R^2
// or R^2 / A for every entry at bind time, on the host), and mont_mul(v R, x) = v x: x and the sums never enter that form, and the
// same code serves canonical vectors and MONTGOMERY ones (x A in, (sum v x) A out).
// TWO KERNELS, 256 lanes a block.
//   k_spmv_tile  a block owns one tile of T = 256 chunk consecutive ENTRIES of one vector (chunk is a run-time argument).  Lane l takes the
//                entries l + 256 j: value, column and the gathered x[col] (every load of a wave of values and indices covers consecutive
//                records), one product each, 9 limbs into LDS.  Behind the barrier lane l owns the chunk CONSECUTIVE entries from l chunk
//                and walks them with their row ids (spmv_walk): a run that begins and ends inside the lane is a whole row and is stored; the
//                lane keeps its first run (head) when a boundary lies inside it, and its last (tail).  A segmented Hillis-Steele scan over
//                the lanes' tails, 8 steps through LDS (the scan area lies over the products, behind a barrier), flag = "the tail does not
//                go on from the lane before", leaves in every lane the sum of the run that is open at its last entry.  A lane with a
//                boundary inside closes its head with the lane before's value; a lane whose tail ends at its last entry closes it.
//                spmv_close says where a closed run goes: out, or -- the tile's first run when its row began before the tile, its last
//                when the row goes on -- fragment 0 / 1 of the tile.  Lane 0 writes the fragments the tile does not use as 0.
//   k_spmv_rows  block b of a vector: lane l writes row 256 b + l as 0 when it is empty; and when tile b's last row began inside it and
//                goes on, the lanes stride over the tiles up to the row's last, add their fragments 0 (and fragment 1 of tile b), and a
//                tree through LDS leaves the row's sum in lane 0.
// No atomics, and every out record has one writer: the result is deterministic.
// LIMBS AND VALUES of everything stored (R = 2^261 = 438.8 p, 2^256 = 13.72 p; mont_mul(a, b) <= a b / R + p, exact for a class N operand
//   and limbs below 2^31 of the other).
//   vals: canonical words, below p.  x: any 256-bit record, below 13.72 p.  A product t = v R x / R + p < 13.72 p p / 438.8 p + p < 1.04 p,
//   class N: what the LDS tile holds.  A lane's walk adds at most 16 of them, normalising each sum: head and tail are class N below 16.5 p.
//   The scan adds the value of the lane 2^s before at step s: four steps take 16.5 p to below 264 p (< R: class N with a top limb below
//   2^29), spmv_reduce -- one product with R mod p = 0.79 p -- leaves below 264 x 0.79 / 438.8 p + p < 1.48 p, and the four steps behind
//   it below 23.7 p.  The scan area holds class N values below 132 p (a lane's own register up to 264 p).  A closed head is head + the lane before's value < 16.5 p + 23.7 p =
//   40.2 p, a closed tail below 23.7 p: spmv_out reduces once more (below 1.08 p) and subtracts p once (fo_words takes below 2 p).
//   Without the reduction the 8 steps reach 256 x 16.5 p = 4224 p: past R from the sixth step on, where a product with R mod p no longer
//   comes out below 2 p.  Fragments: canonical words.  k_spmv_rows adds kRowFold = 32 of them to a value below 1.08 p (33.1 p), reduces, and
//   reduces behind every step of its tree (2.2 p -> 1.01 p).
// Every global index is spmv_plan.hpp's x_of / out_of / frag_of or an entry below the tile's `fill`; every LDS index its lds_word /
// scan_word.  All offsets are 64 bits wide.
#pragma once
#include <string.h>
#include "field_ops.hip.hpp"
#include "spmv_plan.hpp"

namespace te {

TE_HD fel<9> spmv_product(const uint32_t (&v)[8], const uint32_t (&x)[8]) { return fe_mul(fp_from_words32(v), fp_from_words32(x)); }
TE_HD fel<9> spmv_add(const fel<9>& a, const fel<9>& b) { return fe_norm(fe_add(a, b)); }
// class N below R -> class N below value x 0.79 / 438.8 + p
TE_HD fel<9> spmv_reduce(const fel<9>& a) { return fe_mul(a, fe_one<9>()); }
// class N below R -> canonical words
TE_HD void spmv_out(const fel<9>& a, uint32_t (&w)[8]) { fo_words<9, 8>(spmv_reduce(a), w); }
TE_HD void spmv_lds_put(uint32_t* lds, uint32_t word, const fel<9>& v) {
#pragma unroll
  for (int k = 0; k < 9; k++) lds[word + k] = v.v[k];
}
TE_HD fel<9> spmv_lds_get(const uint32_t* lds, uint32_t word) {
  fel<9> r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = lds[word + k];
  return r;
}

// ---- the edges of a tile: its first and last row, and whether they reach past it (row: the row ids of the whole stream) ----------
struct spmv_edges { uint32_t r_first, r_last; bool began_before, goes_on; };
TE_HD spmv_edges spmv_edges_of(const uint32_t* row, uint64_t nnz, uint64_t base, uint32_t fill) {
  spmv_edges e;
  e.r_first = row[base]; e.r_last = row[base + fill - 1u];
  e.began_before = base > 0u && row[base - 1u] == e.r_first;
  e.goes_on = base + fill < nnz && row[base + fill] == e.r_last;
  return e;
}
// where a closed run of row r goes: the rows of a stream are contiguous, so a run of the tile's first row is its first run, and one of
// its last row its last
enum { SPMV_TO_OUT = 0, SPMV_TO_HEAD = 1, SPMV_TO_TAIL = 2 };
TE_HD int spmv_close(const spmv_edges& e, uint32_t r) {
  if (r == e.r_first && e.began_before) return SPMV_TO_HEAD;
  if (r == e.r_last && e.goes_on) return SPMV_TO_TAIL;
  return SPMV_TO_OUT;
}
TE_HD bool spmv_head_used(const spmv_edges& e) { return e.began_before; }
TE_HD bool spmv_tail_used(const spmv_edges& e) { return e.goes_on && !(e.began_before && e.r_first == e.r_last); }

// ---- a lane behind the barrier: its chunk consecutive entries ------------------------------------------------------------------------
struct spmv_lane {
  fel<9> head, tail;             // the sum of its first run (when `inner`) and of its last
  uint32_t r_first, r_last;
  bool any, inner;               // it holds entries; a row boundary lies inside it
  bool prev_same;                // its first run goes on from the lane before
  bool ends;                     // its last run ends at its last entry
};
// row: the row ids of the TILE (row[x], x < fill; row[-1] is read for lane > 0 only).  whole(r, sum): a run that begins and ends inside
// the lane -- a whole row
template <typename Whole> TE_HD spmv_lane spmv_walk(const uint32_t* lds, const uint32_t* row, uint32_t lane, uint32_t chunk, uint32_t fill, Whole&& whole) {
  spmv_lane L;
  L.head = fe_zero<9>(); L.tail = fe_zero<9>();
  L.r_first = L.r_last = 0u; L.inner = false; L.prev_same = false; L.ends = true;
  const uint32_t first = te_spmv::own_x(lane, 0, chunk);
  L.any = first < fill;
  if (!L.any) return L;
  const uint32_t n = fill - first < chunk ? fill - first : chunk;
  uint32_t r = row[first];
  L.r_first = r;
  fel<9> acc = fe_zero<9>();
#pragma unroll 1
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t rj = row[first + j];
    if (rj != r) {
      if (!L.inner) { L.head = acc; L.inner = true; }
      else whole(r, acc);
      acc = fe_zero<9>();
      r = rj;
    }
    acc = spmv_add(acc, spmv_lds_get(lds, te_spmv::lds_word(first + j, chunk)));
  }
  L.tail = acc; L.r_last = r;
  L.prev_same = lane > 0u && row[first - 1u] == L.r_first;
  L.ends = first + n >= fill || row[first + n] != L.r_last;
  return L;
}
// the flag a lane enters the scan with: its tail does not go on from the lane before
TE_HD uint32_t spmv_flag(const spmv_lane& L) { return !L.any || L.inner || !L.prev_same ? 1u : 0u; }
// step s of the segmented scan: lane l takes lane l - 2^s in unless a boundary lies between them
TE_HD void spmv_scan_step(const uint32_t* scan, const uint32_t* flags, uint32_t lane, uint32_t s, fel<9>& v, uint32_t& f) {
  if (lane < (1u << s)) return;
  const uint32_t from = lane - (1u << s);
  if (!f) v = spmv_add(v, spmv_lds_get(scan, te_spmv::scan_word(from)));
  f |= flags[from];
}
TE_HD bool spmv_scan_reduces(uint32_t s) { return s == te_spmv::kScanReduce; }

// ---- k_spmv_rows: the row that tile b leaves open, if it began there -----------------------------------------------------------------
struct spmv_span { bool open; uint32_t r; uint64_t last; };          // last: the tile the row ends in
TE_HD spmv_span spmv_span_of(const te_spmv::plan& P, const uint32_t* row, const uint64_t* ptr, uint64_t t) {
  spmv_span s; s.open = false; s.r = 0; s.last = t;
  if (t >= P.tiles) return s;
  const uint64_t base = t * P.T, rest = P.nnz - base, fill = rest < P.T ? rest : P.T;
  const uint32_t r = row[base + fill - 1u];
  if (base + fill >= P.nnz || row[base + fill] != r || ptr[r] < base) return s;
  s.open = true; s.r = r; s.last = te_spmv::tile_holding(P, ptr[r + 1u] - 1u);
  return s;
}
// step s of the tree: lane l takes lane l + 2^s in when l is a multiple of 2^(s+1)
TE_HD bool spmv_tree_takes(uint32_t lane, uint32_t s) { return (lane & ((2u << s) - 1u)) == 0u; }

// ---- what the calls check on the host before anything runs (points.hip; the shim of the CPU tests calls the same functions) ----------
enum { SPMV_OK = 0, SPMV_BAD_DIMS, SPMV_BAD_FLAGS, SPMV_BAD_PTR, SPMV_BAD_INDEX, SPMV_NULL, SPMV_NO_TRANSPOSE, SPMV_IN_PLACE, SPMV_TOO_LARGE };
// te_msm_bind_matrix; *bad: the lowest position of a column index that is not below cols (SPMV_BAD_INDEX)
inline int spmv_check_bind(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const uint8_t* vals, int flags, int64_t* bad) {
  if (rows == 0 || rows > te_spmv::kMaxDim || cols == 0 || cols > te_spmv::kMaxDim) return SPMV_BAD_DIMS;
  if (flags & ~(TE_MSM_MATRIX_MONTGOMERY | TE_MSM_MATRIX_TRANSPOSE)) return SPMV_BAD_FLAGS;
  if (!row_ptr) return SPMV_NULL;
  if (row_ptr[0] != 0) return SPMV_BAD_PTR;
  for (uint64_t r = 0; r < rows; r++) if (row_ptr[r + 1] < row_ptr[r]) return SPMV_BAD_PTR;
  const uint64_t nnz = row_ptr[rows];
  if (nnz > te_spmv::kMaxNnz) return SPMV_TOO_LARGE;
  if (nnz > 0 && (!col_idx || !vals)) return SPMV_NULL;
  for (uint64_t e = 0; e < nnz; e++) if (col_idx[e] >= cols) { *bad = (int64_t)e; return SPMV_BAD_INDEX; }
  return SPMV_OK;
}
// te_msm_spmv*: rows x cols as BOUND; has_t: the bind kept the transpose
inline int spmv_check_call(bool has_t, uint64_t rows, uint64_t cols, const void* x, uint64_t count, int flags, const void* out) {
  if (flags & ~(TE_MSM_SPMV_MONTGOMERY | TE_MSM_SPMV_TRANSPOSE)) return SPMV_BAD_FLAGS;
  if ((flags & TE_MSM_SPMV_TRANSPOSE) && !has_t) return SPMV_NO_TRANSPOSE;
  if (count == 0) return SPMV_OK;
  if (!x || !out) return SPMV_NULL;
  if (x == out) return SPMV_IN_PLACE;
  if (count > (UINT64_MAX >> 5) / rows || count > (UINT64_MAX >> 5) / cols) return SPMV_TOO_LARGE;
  return SPMV_OK;
}
// the record of a value as a side holds it: v R mod p, canonical (mont: the caller's record holds v 2^256 mod p)
inline void spmv_value(const uint8_t* rec, bool mont, uint8_t* out) {
  uint32_t w[8], o[8];
  memcpy(w, rec, 32);
  fo_words<9, 8>(mont ? fo_decode<9, true>(w) : fo_decode<9, false>(w), o);
  memcpy(out, o, 32);
}

#if defined(__HIPCC__)
// one side of a bound matrix on a device (te_spmv::layout)
struct spmv_side { const uint4* vals; const uint64_t* ptr; const uint32_t* col; const uint32_t* row; };

// grid = count x tiles; frag: the call's scratch buffer.  x and out are not __restrict__ (the call refuses out == x, no more).  Dynamic
// LDS: te_spmv::lds_bytes(P.chunk)
__global__ __launch_bounds__(256) void k_spmv_tile(spmv_side m, te_spmv::plan P, const uint4* x, uint4* out, uint4* frag) {
  extern __shared__ uint32_t spmv_lds[];
  __shared__ uint32_t flags[te_spmv::kLanes];
  uint32_t* const lds = spmv_lds;
  const uint32_t lane = threadIdx.x, chunk = P.chunk;
  const te_spmv::tile t = te_spmv::tile_of(P, blockIdx.x);
#pragma unroll 1
  for (uint32_t j = 0; j < chunk; j++) {
    const uint32_t e = te_spmv::wide_x(lane, j);
    if (e >= t.fill) continue;
    uint32_t v[8], xw[8];
    fo_load<2>(m.vals, (size_t)(t.base + e) * 2, v);
    fo_load<2>(x, (size_t)te_spmv::x_of(P, t.vec, m.col[t.base + e]) * 2, xw);
    spmv_lds_put(lds, te_spmv::lds_word(e, chunk), spmv_product(v, xw));
  }
  const spmv_edges edges = spmv_edges_of(m.row, P.nnz, t.base, t.fill);
  auto put = [&](uint32_t r, const fel<9>& sum) {
    uint32_t w[8];
    spmv_out(sum, w);
    const int to = spmv_close(edges, r);
    if (to == SPMV_TO_OUT) fo_store<2>(out, (size_t)te_spmv::out_of(P, t.vec, r) * 2, w);
    else fo_store<2>(frag, (size_t)te_spmv::frag_of(P, t.vec, t.t, to == SPMV_TO_HEAD ? te_spmv::kHead : te_spmv::kTail) * 2, w);
  };
  __syncthreads();
  const spmv_lane L = spmv_walk(lds, m.row + t.base, lane, chunk, t.fill, put);
  fel<9> v = L.tail;
  uint32_t f = spmv_flag(L);
  __syncthreads();                                                   // every lane has read its products: the scan area lies over them
#pragma unroll 1
  for (uint32_t s = 0; s < te_spmv::kScanSteps; s++) {
    spmv_lds_put(lds, te_spmv::scan_word(lane), v);
    flags[lane] = f;
    __syncthreads();
    spmv_scan_step(lds, flags, lane, s, v, f);
    if (spmv_scan_reduces(s)) v = spmv_reduce(v);
    __syncthreads();
  }
  spmv_lds_put(lds, te_spmv::scan_word(lane), v);
  __syncthreads();
  if (L.inner) put(L.r_first, L.prev_same ? spmv_add(L.head, spmv_lds_get(lds, te_spmv::scan_word(lane - 1u))) : L.head);
  if (L.any && L.ends) put(L.r_last, v);
  if (lane == 0u) {
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    if (!spmv_head_used(edges)) { const size_t at = (size_t)te_spmv::frag_of(P, t.vec, t.t, te_spmv::kHead) * 2; frag[at] = zero; frag[at + 1] = zero; }
    if (!spmv_tail_used(edges)) { const size_t at = (size_t)te_spmv::frag_of(P, t.vec, t.t, te_spmv::kTail) * 2; frag[at] = zero; frag[at + 1] = zero; }
  }
}

// grid = count x P.per
__global__ __launch_bounds__(256) void k_spmv_rows(spmv_side m, te_spmv::plan P, uint4* out, const uint4* __restrict__ frag) {
  __shared__ uint32_t tree[te_spmv::kLanes * te_spmv::kLimbs];
  const uint32_t lane = threadIdx.x;
  const te_spmv::row_block rb = te_spmv::row_block_of(P, blockIdx.x);
  const uint64_t r = rb.b * te_spmv::kLanes + lane;
  if (r < P.rows && m.ptr[r] == m.ptr[r + 1u]) {
    const size_t at = (size_t)te_spmv::out_of(P, rb.vec, r) * 2;
    out[at] = make_uint4(0u, 0u, 0u, 0u); out[at + 1] = make_uint4(0u, 0u, 0u, 0u);
  }
  const spmv_span sp = spmv_span_of(P, m.row, m.ptr, rb.b);
  if (!sp.open) return;                                              // (the same for every lane of the block)
  fel<9> acc = fe_zero<9>();
  uint32_t w[8];
  if (lane == 0u) { fo_load<2>(frag, (size_t)te_spmv::frag_of(P, rb.vec, rb.b, te_spmv::kTail) * 2, w); acc = fp_from_words32(w); }
  uint32_t since = 1u;
#pragma unroll 1
  for (uint64_t u = rb.b + 1u + lane; u <= sp.last; u += te_spmv::kLanes) {
    fo_load<2>(frag, (size_t)te_spmv::frag_of(P, rb.vec, u, te_spmv::kHead) * 2, w);
    acc = spmv_add(acc, fp_from_words32(w));
    if (++since == te_spmv::kRowFold) { acc = spmv_reduce(acc); since = 0u; }
  }
  acc = spmv_reduce(acc);
#pragma unroll 1
  for (uint32_t s = 0; s < te_spmv::kScanSteps; s++) {
    spmv_lds_put(tree, te_spmv::scan_word(lane), acc);
    __syncthreads();
    if (spmv_tree_takes(lane, s)) acc = spmv_reduce(spmv_add(acc, spmv_lds_get(tree, te_spmv::scan_word(lane + (1u << s)))));
    __syncthreads();
  }
  if (lane == 0u) {
    spmv_out(acc, w);
    fo_store<2>(out, (size_t)te_spmv::out_of(P, rb.vec, sp.r) * 2, w);
  }
}
#endif

}  // namespace te
