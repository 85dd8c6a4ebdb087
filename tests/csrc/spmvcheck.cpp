// spmvcheck.cpp -- TEST SHIM: compiles the product's sparse matrix-vector product (csrc/spmv.hip.hpp, csrc/spmv_plan.hpp) for the host, so
// that the exact per-lane code of k_spmv_tile and k_spmv_rows runs on the CPU box (tests/test_spmv_host.py, tests/csrc/san_spmv.cpp).
// Not part of the product; not a fallback.  Expected values come from tests/spmv_cases.py (Python integers), never from here.  It holds
//   spmv_emulate    te_msm_bind_matrix and te_msm_spmv's steps: the same argument checks, value conversion, row ids, transpose and plan as
//                   points.hip, then both launches, a block as plain loops over its 256 lanes -- one loop per phase, a loop boundary being
//                   the block's barrier.  Every global, scratch and LDS index is checked against what the plan says is allocated (-100 on
//                   a violation), and every out record must be written exactly once (-101 otherwise, except under a mistake).
//   spmv_sides      what a bind lays down: the row ids, and the transpose as CSR arrays (with the deliberate mistakes 5 and 6).
//   spmv_replay     the indices alone, no arithmetic and no matrix: every tile's entries and fragments, the extreme x and out records,
//                   every LDS word of a tile inside the block's and owned once, for nnz up to 2^33 and rows up to 2^31.
// `mistake` (0 in every real check) turns the emulation into a deliberately wrong variant, which the tests must catch:
//   1 a head fragment added to the row after the one it belongs to     2 empty rows left unwritten
//   3 the scan without its segment flags                              4 the reduction inside the scan removed
//   5 the transpose by an unstable counting sort (filled from the back)   6 ... with its offsets off by one
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/spmv.hip.hpp"

using namespace te;

namespace {
enum { M_HEAD_ROW = 1, M_EMPTY = 2, M_NO_FLAGS = 3, M_NO_REDUCE = 4, M_UNSTABLE = 5, M_OFF_BY_ONE = 6 };
constexpr int E_BOUNDS = -100, E_WRITES = -101;

void rd(const uint8_t* p, uint64_t i, uint32_t (&w)[8]) { memcpy(w, p + i * 32, 32); }
void wr(uint8_t* p, uint64_t i, const uint32_t (&w)[8]) { memcpy(p + i * 32, w, 32); }

// one side as a bind lays it down (host memory)
struct side_t {
  uint64_t rows = 0, nnz = 0;
  std::vector<uint8_t> vals; std::vector<uint64_t> ptr; std::vector<uint32_t> col, row;
};
void transpose_mistaken(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const uint8_t* vals, int mistake, uint64_t* t_ptr, uint32_t* t_col,
                        uint8_t* t_vals) {
  const uint64_t nnz = row_ptr[rows];
  if (mistake != M_UNSTABLE && mistake != M_OFF_BY_ONE) { te_spmv::transpose(rows, cols, row_ptr, col_idx, vals, t_ptr, t_col, t_vals); return; }
  std::vector<uint64_t> cnt(cols + 1, 0);
  for (uint64_t e = 0; e < nnz; e++) cnt[(uint64_t)col_idx[e] + 1u]++;
  for (uint64_t c = 0; c < cols; c++) cnt[c + 1] += cnt[c];
  for (uint64_t c = 0; c <= cols; c++) t_ptr[c] = cnt[c];
  if (mistake == M_UNSTABLE) {                                       // every column filled from its end: the rows of a column come out descending
    for (uint64_t r = 0; r < rows; r++)
      for (uint64_t e = row_ptr[r]; e < row_ptr[r + 1]; e++) {
        const uint64_t at = --cnt[(uint64_t)col_idx[e] + 1u];
        t_col[at] = (uint32_t)r;
        memcpy(t_vals + at * 32, vals + e * 32, 32);
      }
    return;
  }
  te_spmv::transpose(rows, cols, row_ptr, col_idx, vals, t_ptr, t_col, t_vals);
  for (uint64_t c = 1; c < cols; c++) t_ptr[c] = cnt[c] + (cnt[c] < nnz ? 1u : 0u);      // column c begins one entry late
}

// one launch of k_spmv_tile; false: an index left its allocation
bool tile_launch(const side_t& S, const te_spmv::plan& P, const uint8_t* x, uint8_t* out, std::vector<uint8_t>& frag, std::vector<uint32_t>& writes, int mistake) {
  const uint32_t chunk = P.chunk, data_words = te_spmv::lds_data_words(chunk);
  std::vector<uint32_t> lds(data_words), flags(te_spmv::kLanes), f(te_spmv::kLanes);
  std::vector<spmv_lane> L(te_spmv::kLanes);
  std::vector<fel<9>> v(te_spmv::kLanes);
  const uint64_t blocks = P.count * P.tiles;
  bool ok = true;
  for (uint64_t block = 0; block < blocks; block++) {
    const te_spmv::tile t = te_spmv::tile_of(P, block);
    if (t.vec >= P.count || t.base + t.fill > P.nnz || t.fill < 1u) return false;
    for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++)
      for (uint32_t j = 0; j < chunk; j++) {
        const uint32_t e = te_spmv::wide_x(lane, j);
        if (e >= t.fill) continue;
        const uint32_t c = S.col[t.base + e];
        if (c >= P.cols || te_spmv::x_of(P, t.vec, c) >= P.count * P.cols || te_spmv::lds_word(e, chunk) + 9u > data_words) return false;
        uint32_t vw[8], xw[8];
        rd(S.vals.data(), t.base + e, vw);
        rd(x, te_spmv::x_of(P, t.vec, c), xw);
        spmv_lds_put(lds.data(), te_spmv::lds_word(e, chunk), spmv_product(vw, xw));
      }
    const spmv_edges edges = spmv_edges_of(S.row.data(), P.nnz, t.base, t.fill);
    auto put = [&](uint32_t r, const fel<9>& sum) {
      uint32_t w[8];
      spmv_out(sum, w);
      const int to = spmv_close(edges, r);
      if (to == SPMV_TO_OUT) {
        if (r >= P.rows) { ok = false; return; }
        wr(out, te_spmv::out_of(P, t.vec, r), w);
        writes[te_spmv::out_of(P, t.vec, r)]++;
      } else {
        const uint64_t at = te_spmv::frag_of(P, t.vec, t.t, to == SPMV_TO_HEAD ? te_spmv::kHead : te_spmv::kTail);
        if (at >= P.frag_records) { ok = false; return; }
        wr(frag.data(), at, w);
      }
    };
    for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) {
      L[lane] = spmv_walk(lds.data(), S.row.data() + t.base, lane, chunk, t.fill, put);
      v[lane] = L[lane].tail;
      f[lane] = mistake == M_NO_FLAGS ? 0u : spmv_flag(L[lane]);
    }
    for (uint32_t s = 0; s < te_spmv::kScanSteps; s++) {
      for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) {
        if (te_spmv::scan_word(lane) + 9u > data_words) return false;
        spmv_lds_put(lds.data(), te_spmv::scan_word(lane), v[lane]);
        flags[lane] = f[lane];
      }
      for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) {
        spmv_scan_step(lds.data(), flags.data(), lane, s, v[lane], f[lane]);
        if (spmv_scan_reduces(s) && mistake != M_NO_REDUCE) v[lane] = spmv_reduce(v[lane]);
      }
    }
    for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) spmv_lds_put(lds.data(), te_spmv::scan_word(lane), v[lane]);
    for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) {
      if (L[lane].inner) put(L[lane].r_first, L[lane].prev_same ? spmv_add(L[lane].head, spmv_lds_get(lds.data(), te_spmv::scan_word(lane - 1u))) : L[lane].head);
      if (L[lane].any && L[lane].ends) put(L[lane].r_last, v[lane]);
    }
    const uint32_t zero[8] = {};
    if (!spmv_head_used(edges)) wr(frag.data(), te_spmv::frag_of(P, t.vec, t.t, te_spmv::kHead), zero);
    if (!spmv_tail_used(edges)) wr(frag.data(), te_spmv::frag_of(P, t.vec, t.t, te_spmv::kTail), zero);
    if (!ok) return false;
  }
  return true;
}

// one launch of k_spmv_rows
bool rows_launch(const side_t& S, const te_spmv::plan& P, uint8_t* out, const std::vector<uint8_t>& frag, std::vector<uint32_t>& writes, int mistake) {
  std::vector<uint32_t> tree(te_spmv::kLanes * te_spmv::kLimbs);
  std::vector<fel<9>> acc(te_spmv::kLanes);
  const uint64_t blocks = P.count * P.per;
  for (uint64_t block = 0; block < blocks; block++) {
    const te_spmv::row_block rb = te_spmv::row_block_of(P, block);
    if (rb.vec >= P.count) return false;
    for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) {
      const uint64_t r = rb.b * te_spmv::kLanes + lane;
      if (r < P.rows && S.ptr[r] == S.ptr[r + 1u] && mistake != M_EMPTY) {
        const uint32_t zero[8] = {};
        wr(out, te_spmv::out_of(P, rb.vec, r), zero);
        writes[te_spmv::out_of(P, rb.vec, r)]++;
      }
    }
    const spmv_span sp = spmv_span_of(P, S.row.data(), S.ptr.data(), rb.b);
    if (!sp.open) continue;
    if (sp.last >= P.tiles || sp.r >= P.rows) return false;
    for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) {
      uint32_t w[8];
      acc[lane] = fe_zero<9>();
      if (lane == 0u) { rd(frag.data(), te_spmv::frag_of(P, rb.vec, rb.b, te_spmv::kTail), w); acc[lane] = fp_from_words32(w); }
      uint32_t since = 1u;
      const uint64_t shift = mistake == M_HEAD_ROW && sp.last + 1u < P.tiles ? 1u : 0u;      // the head fragments one tile on: the next row's among them
      for (uint64_t u = rb.b + 1u + shift + lane; u <= sp.last + shift; u += te_spmv::kLanes) {
        if (te_spmv::frag_of(P, rb.vec, u, te_spmv::kHead) >= P.frag_records) return false;
        rd(frag.data(), te_spmv::frag_of(P, rb.vec, u, te_spmv::kHead), w);
        acc[lane] = spmv_add(acc[lane], fp_from_words32(w));
        if (++since == te_spmv::kRowFold) { acc[lane] = spmv_reduce(acc[lane]); since = 0u; }
      }
      acc[lane] = spmv_reduce(acc[lane]);
    }
    for (uint32_t s = 0; s < te_spmv::kScanSteps; s++) {
      for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) spmv_lds_put(tree.data(), te_spmv::scan_word(lane), acc[lane]);
      for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) {
        if (!spmv_tree_takes(lane, s)) continue;
        if (lane + (1u << s) >= te_spmv::kLanes) return false;
        acc[lane] = spmv_reduce(spmv_add(acc[lane], spmv_lds_get(tree.data(), te_spmv::scan_word(lane + (1u << s)))));
      }
    }
    uint32_t w[8];
    spmv_out(acc[0], w);
    wr(out, te_spmv::out_of(P, rb.vec, sp.r), w);
    writes[te_spmv::out_of(P, rb.vec, sp.r)]++;
  }
  return true;
}

void build_side(uint64_t rows, const uint64_t* ptr, const uint32_t* col, const uint8_t* vals, uint64_t nnz, side_t& S) {
  S.rows = rows; S.nnz = nnz;
  S.ptr.assign(ptr, ptr + rows + 1);
  S.col.assign(col, col + nnz);
  S.vals.assign(vals, vals + nnz * 32);
  S.row.resize(nnz);
  te_spmv::fill_rows(S.ptr.data(), rows, S.row.data());
}
}  // namespace

extern "C" {

// te_msm_bind_matrix + te_msm_spmv with the product's block code: 0, -1 (refused, out untouched; *reason = why: spmv.hip.hpp's SPMV_*;
// *bad = the lowest bad column position), -100 (an index left its allocation), -101 (an out record not written exactly once).
// chunk: 0 for the default.  x == out is passed through as it is (the call refuses it)
int spmv_emulate(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const uint8_t* vals, int mflags, const uint8_t* x, uint64_t count, int flags,
                 uint32_t chunk, int mistake, uint8_t* out, int* reason, int64_t* bad) {
  int64_t pos = -1;
  int why = spmv_check_bind(rows, cols, row_ptr, col_idx, vals, mflags, &pos);
  if (bad) *bad = pos;
  if (why == SPMV_OK) why = spmv_check_call((mflags & TE_MSM_MATRIX_TRANSPOSE) != 0, rows, cols, x, count, flags, out);
  if (reason) *reason = why;
  if (why != SPMV_OK) return -1;
  if (count == 0) return 0;
  const uint64_t nnz = row_ptr[rows];
  const bool mont = (mflags & TE_MSM_MATRIX_MONTGOMERY) != 0, tr = (flags & TE_MSM_SPMV_TRANSPOSE) != 0;
  std::vector<uint8_t> conv((size_t)nnz * 32);
  for (uint64_t e = 0; e < nnz; e++) spmv_value(vals + e * 32, mont, conv.data() + e * 32);
  side_t S;
  if (tr) {
    std::vector<uint64_t> t_ptr(cols + 1);
    std::vector<uint32_t> t_col(nnz);
    std::vector<uint8_t> t_vals((size_t)nnz * 32);
    transpose_mistaken(rows, cols, row_ptr, col_idx, conv.data(), mistake, t_ptr.data(), t_col.data(), t_vals.data());
    build_side(cols, t_ptr.data(), t_col.data(), t_vals.data(), nnz, S);
  } else {
    build_side(rows, row_ptr, col_idx, conv.data(), nnz, S);
  }
  te_spmv::plan P;
  if (!te_spmv::make_plan(tr ? cols : rows, tr ? rows : cols, nnz, count, te_spmv::clamp_chunk((long)chunk), P)) { if (reason) *reason = SPMV_TOO_LARGE; return -1; }
  std::vector<uint8_t> frag((size_t)P.frag_records * 32, 0xEE);      // (the call does not rely on what its scratch held)
  std::vector<uint32_t> writes((size_t)(P.count * P.rows), 0);
  if (P.tiles > 0 && !tile_launch(S, P, x, out, frag, writes, mistake)) return E_BOUNDS;
  if (!rows_launch(S, P, out, frag, writes, mistake)) return E_BOUNDS;
  if (!mistake)
    for (uint32_t w : writes) if (w != 1u) return E_WRITES;
  return 0;
}

// what a bind lays down beside the values: row[nnz] of the matrix, and its transpose (t_ptr[cols + 1], t_col[nnz], t_row[nnz], t_vals)
// -- the values are copied as they are, so that a test sees where every entry went
int spmv_sides(uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const uint8_t* vals, int mistake, uint32_t* row, uint64_t* t_ptr,
               uint32_t* t_col, uint32_t* t_row, uint8_t* t_vals) {
  int64_t pos = -1;
  if (spmv_check_bind(rows, cols, row_ptr, col_idx, vals, 0, &pos) != SPMV_OK) return -1;
  te_spmv::fill_rows(row_ptr, rows, row);
  transpose_mistaken(rows, cols, row_ptr, col_idx, vals, mistake, t_ptr, t_col, t_vals);
  te_spmv::fill_rows(t_ptr, cols, t_row);
  return 0;
}

// every index of the plan of a call, by arithmetic alone: 0 with *checked = how many, or -100
int spmv_replay(uint64_t rows, uint64_t cols, uint64_t nnz, uint64_t count, uint32_t chunk, uint64_t* checked) {
  te_spmv::plan P;
  *checked = 0;
  if (!te_spmv::make_plan(rows, cols, nnz, count, chunk, P)) return E_BOUNDS;
  const uint32_t data_words = te_spmv::lds_data_words(chunk);
  if (te_spmv::lds_bytes(chunk) + 4u * te_spmv::kLanes > 160u * 1024u || te_spmv::lds_scan_words() > data_words) return E_BOUNDS;
  std::vector<uint8_t> hit(data_words, 0);
  for (uint32_t lane = 0; lane < te_spmv::kLanes; lane++) {
    if (te_spmv::scan_word(lane) + 9u > te_spmv::lds_scan_words()) return E_BOUNDS;
    for (uint32_t j = 0; j < chunk; j++) {
      const uint32_t wx = te_spmv::wide_x(lane, j), ox = te_spmv::own_x(lane, j, chunk);
      if (wx >= P.T || ox >= P.T || te_spmv::lds_word(wx, chunk) + 9u > data_words) return E_BOUNDS;
      const uint32_t at = te_spmv::lds_word(ox, chunk);
      for (uint32_t k = 0; k < 9u; k++) { if (at + k >= data_words || hit[at + k]) return E_BOUNDS; hit[at + k] = 1; }
      *checked += 2;
    }
  }
  const te_spmv::layout lay = te_spmv::layout_of(rows, nnz);
  if (lay.ptr != 32u * nnz || lay.col != lay.ptr + 8u * (rows + 1u) || lay.row != lay.col + 4u * nnz || lay.bytes != lay.row + 4u * nnz || (lay.ptr & 7u) || (lay.col & 3u)) return E_BOUNDS;
  if (P.tiles != (nnz + P.T - 1u) / P.T || P.per < P.tiles || P.per * te_spmv::kLanes < rows || count * P.per >> 31) return E_BOUNDS;
  if (P.frag_records != count * P.tiles * 2u || P.scratch_bytes != P.frag_records * 32u) return E_BOUNDS;
  const uint64_t vecs[2] = {0, count - 1u};
  for (uint64_t vec : vecs) {
    uint64_t next = 0;                                               // the tiles cover the stream in order, once
    for (uint64_t tb = 0; tb < P.tiles; tb++) {
      const te_spmv::tile t = te_spmv::tile_of(P, vec * P.tiles + tb);
      if (t.vec != vec || t.t != tb || t.base != next || t.fill < 1u || t.fill > P.T || t.base + t.fill > nnz) return E_BOUNDS;
      next = t.base + t.fill;
      const uint64_t h = te_spmv::frag_of(P, vec, tb, te_spmv::kHead), tl = te_spmv::frag_of(P, vec, tb, te_spmv::kTail);
      if (tl != h + 1u || tl >= P.frag_records || h != (vec * P.tiles + tb) * 2u) return E_BOUNDS;
      *checked += 3;
    }
    if (next != nnz) return E_BOUNDS;
    if (nnz && te_spmv::tile_holding(P, nnz - 1u) != P.tiles - 1u) return E_BOUNDS;
    if (te_spmv::x_of(P, vec, (uint32_t)(cols - 1u)) != vec * cols + cols - 1u || te_spmv::x_of(P, vec, (uint32_t)(cols - 1u)) >= count * cols) return E_BOUNDS;
    if (te_spmv::out_of(P, vec, rows - 1u) != vec * rows + rows - 1u || te_spmv::out_of(P, vec, rows - 1u) >= count * rows) return E_BOUNDS;
    const te_spmv::row_block lastb = te_spmv::row_block_of(P, vec * P.per + P.per - 1u);
    if (lastb.vec != vec || lastb.b != P.per - 1u) return E_BOUNDS;
    *checked += 4;
  }
  return 0;
}

// the plan as numbers: out[0] T, [1] tiles, [2] row blocks, [3] blocks of k_spmv_rows a vector, [4] fragment records, [5] scratch bytes,
// [6] LDS bytes of the tile kernel, [7] the default chunk, [8] the largest chunk, [9] the scan step that reduces, [10] fragments between two
// reductions of k_spmv_rows, [11] bytes of one side on a device, [12] scan steps (out[0] = 0 when make_plan refuses)
void spmv_plan_info(uint64_t rows, uint64_t cols, uint64_t nnz, uint64_t count, uint32_t chunk, uint64_t* out) {
  te_spmv::plan P;
  memset(out, 0, 16 * sizeof(uint64_t));
  out[7] = te_spmv::kChunkDefault; out[8] = te_spmv::kChunkMax; out[9] = te_spmv::kScanReduce; out[10] = te_spmv::kRowFold; out[12] = te_spmv::kScanSteps;
  if (!te_spmv::make_plan(rows, cols, nnz, count, chunk, P)) return;
  out[0] = P.T; out[1] = P.tiles; out[2] = P.row_blocks; out[3] = P.per; out[4] = P.frag_records; out[5] = P.scratch_bytes; out[6] = te_spmv::lds_bytes(chunk);
  out[11] = te_spmv::layout_of(rows, nnz).bytes;
}

}
