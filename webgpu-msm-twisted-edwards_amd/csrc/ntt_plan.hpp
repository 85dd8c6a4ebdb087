// ntt_plan.hpp -- the plan of a batched NTT over p (te_msm_ntt*; kernels in ntt.hip.hpp): which passes a size runs
// in, what a block's tile is in each of them, every global and LDS index a lane forms, the sizes of the tables and the launch geometry.
// HIP-free: points.hip, the kernels and the host shim (tests/csrc/nttcheck.cpp) all take their numbers from here, and the bounds replay
// of tests/test_ntt_host.py walks exactly these functions.
//
// n = 2^L is cut into P <= 3 digits, L = r_1 + .. + r_P:  input index i = sum i_k 2^(S_k) (S_k = r_(k+1) + .. + r_P: i_1 is the top digit),
// output index j = sum j_k 2^(Q_k) (Q_k = r_1 + .. + r_(k-1): j_1 is the bottom digit).  i j mod n leaves, for every pair l <= m,
// i_m j_l 2^(S_m + Q_l): l = m is the DFT of digit m (size 2^(r_m)), l < m is a twiddle.  Pass k transforms digit k of every line and
// then multiplies by all the twiddles of j_k at once:  w^(j_k 2^(Q_k) (i mod 2^(S_k))).
//   P = 1 (L <= 10): a tile is 2^(10 - L) whole transforms, read and written where they lie.
//   passes 1 .. P-1: lines of stride 2^(S_k); a tile takes 2^c, c = 10 - r_k, NEIGHBOURING lines (consecutive low positions), so every
//     run of a load or a store is 2^c consecutive records.  Written where it was read (a -> tmp, tmp -> tmp).
//   pass P (P > 1): lines are contiguous (runs of 2^(r_P) records); a tile takes the 2^c lines of consecutive j_1 -- the top digit of
//     where they lie, the BOTTOM digit of where they go -- and writes natural order: runs of 2^c records (tmp -> out).  This is the one
//     transposition of the four-step scheme; no bit-reversal pass exists (the bit reversal of a line is the LDS slot it is stored to).
//   r_k <= 8 when P > 1, so c >= 2: a run is at least 128 bytes.  P = 2 from 2^11, P = 3 from 2^17; 2^24 = 8 + 8 + 8.
// tmp: a buffer of the call's own for the transforms of one piece (piece_transforms: at most 2^24 records); the same memory is never
// read by one block and written by another inside a launch, so out may be a.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "plan_arith.hpp"      // TE_HD

namespace te_ntt {

constexpr uint32_t kMaxLogN = 24u;                 // TE_MSM_NTT_MAX_LOG_N
constexpr uint32_t kTileLog = 10u, kTile = 1u << kTileLog, kLanes = 256u;      // records of a tile, lanes of a block
constexpr uint32_t kElemsPerLane = kTile / kLanes, kBflyPerLane = kTile / 2u / kLanes;
constexpr uint32_t kMinRunLog = 2u, kMaxMultiLog = kTileLog - kMinRunLog;       // multi-pass: c >= 2, r <= 8
constexpr uint32_t kMaxPasses = 3u;
constexpr uint32_t kLimbs = 9u;                    // words of an LDS slot (an odd stride over the 64 banks)
constexpr uint32_t kLdsSlots = 1056u;              // the largest tile with its padding: r = c = 5, 32 lines of pitch 33
constexpr size_t kLdsBytes = (size_t)kLdsSlots * kLimbs * 4u;                   // 38016
// twiddles: w_n^e = Omega^(e 2^(24 - L)), Omega of order 2^24; Omega^E = hi[E >> 12] lo[E & 4095] (hi[j] = Omega^(4096 j))
constexpr uint32_t kRootLog = 24u, kSplitLog = 12u, kTabEntries = 1u << kSplitLog, kTabWords = 12u;   // an entry: 9 limbs in 48 bytes
constexpr size_t kTabBytes = (size_t)kTabEntries * kTabWords * 4u;              // one table; the twiddles are two (hi | lo), a shift two more
constexpr uint64_t kPieceRecords = 1ull << 24;     // records of the transforms one piece runs (and of tmp)

struct pass {
  uint32_t log_n, r, c, pitch;       // L; a line is 2^r records; a tile 2^c lines; LDS slots from one line to the next
  uint32_t first, last;              // the pass decodes what it loads / encodes what it stores (else: packed limbs below 2 p, 32 bytes)
  uint32_t twiddle, tw_shift;        // behind the butterflies: Omega^((rho lowpos) << tw_shift), lowpos = (g << c) + kappa
  uint32_t g_log, mid_log;           // tile = ((o << mid_log | mid) << g_log) | g
  uint32_t rows_fast_src, rows_fast_dst;   // record x of a tile is (rho = x mod 2^r, kappa = x >> r), else (kappa = x mod 2^c, rho = x >> c)
  uint64_t o_stride, g_src, g_dst, mid_src, mid_dst;   // record offsets of a tile's corner
  uint64_t row_src, col_src, row_dst, col_dst;         // ... and of (rho, kappa) inside it
};
struct plan {
  uint32_t log_n, passes;
  uint32_t r[kMaxPasses];
  pass p[kMaxPasses];
  uint64_t piece_transforms;         // transforms of one piece: max(1, 2^24 >> L)
  uint64_t tmp_records;              // records of tmp for a call of `count` transforms: tmp_records_for()
};

TE_HD uint32_t passes_for(uint32_t L) { return L <= kTileLog ? 1u : L <= 2u * kMaxMultiLog ? 2u : 3u; }

TE_HD plan make_plan(uint32_t L) {
  plan P;
  P.log_n = L; P.passes = passes_for(L);
  // balanced digits, the larger ones first
  uint32_t rest = L;
  for (uint32_t k = 0; k < kMaxPasses; k++) {
    const uint32_t left = P.passes > k ? P.passes - k : 1u;
    P.r[k] = k < P.passes ? (rest + left - 1u) / left : 0u;
    rest -= P.r[k];
  }
  P.piece_transforms = (kPieceRecords >> L) ? (kPieceRecords >> L) : 1ull;
  P.tmp_records = 0;
  uint32_t Q = 0;
  for (uint32_t k = 0; k < P.passes; k++) {
    pass& s = P.p[k];
    const uint32_t r = P.r[k], c = kTileLog - r, S = L - Q - r;
    s.log_n = L; s.r = r; s.c = c;
    s.first = k == 0u; s.last = k + 1u == P.passes;
    s.mid_log = 0; s.mid_src = s.mid_dst = 0;
    if (P.passes == 1u) {
      s.pitch = 1u << r; s.twiddle = 0; s.tw_shift = 0; s.g_log = 0;
      s.rows_fast_src = s.rows_fast_dst = 1;
      s.o_stride = kTile; s.g_src = s.g_dst = 0;
      s.row_src = s.row_dst = 1; s.col_src = s.col_dst = 1ull << r;
    } else if (!s.last) {
      s.pitch = (1u << r) + 1u; s.twiddle = 1; s.tw_shift = Q + kRootLog - L; s.g_log = S - c;
      s.rows_fast_src = s.rows_fast_dst = 0;
      s.o_stride = 1ull << (S + r); s.g_src = s.g_dst = 1ull << c;
      s.row_src = s.row_dst = 1ull << S; s.col_src = s.col_dst = 1;
    } else {
      const uint32_t r0 = P.r[0], S0 = L - r0;
      s.pitch = (1u << r) + 1u; s.twiddle = 0; s.tw_shift = 0; s.g_log = r0 - c;
      if (P.passes == 3u) { s.mid_log = P.r[1]; s.mid_src = 1ull << r; s.mid_dst = 1ull << r0; }
      s.rows_fast_src = 1; s.rows_fast_dst = 0;
      s.o_stride = 1ull << L; s.g_src = 1ull << (c + S0); s.g_dst = 1ull << c;
      s.row_src = 1; s.col_src = 1ull << S0; s.row_dst = 1ull << (L - r); s.col_dst = 1;
    }
    Q += r;
  }
  return P;
}
// records of tmp for a call of `count` transforms (0: one pass, no tmp)
TE_HD uint64_t tmp_records_for(const plan& P, uint64_t count) {
  if (P.passes == 1u) return 0;
  return (count < P.piece_transforms ? count : P.piece_transforms) << P.log_n;
}
// launch geometry of a pass over cnt transforms: its lines and its blocks (one tile each)
TE_HD uint64_t lines_of(const pass& s, uint64_t cnt) { return cnt << (s.log_n - s.r); }
TE_HD uint64_t tiles_of(const pass& s, uint64_t cnt) { const uint64_t l = lines_of(s, cnt); return (l + (1ull << s.c) - 1u) >> s.c; }

// ---- indices -------------------------------------------------------------------------------------------------------------------
// record x (< 2^10) of tile `tile` as the pass reads it (src) or writes it (dst): its place in the line (rho), its line in the tile
// (kappa), whether that line exists (the last tile of a one-pass launch may be partly filled) and the record offset in the buffer
struct elem { bool valid; uint32_t rho, kappa, lowpos; uint64_t pos; };
TE_HD elem elem_of(const pass& s, uint64_t tile, uint32_t x, uint64_t lines, bool dst) {
  elem e;
  const bool rows_fast = dst ? s.rows_fast_dst != 0u : s.rows_fast_src != 0u;
  if (rows_fast) { e.rho = x & ((1u << s.r) - 1u); e.kappa = x >> s.r; }
  else { e.kappa = x & ((1u << s.c) - 1u); e.rho = x >> s.c; }
  const uint64_t g = tile & ((1ull << s.g_log) - 1u), mid = (tile >> s.g_log) & ((1ull << s.mid_log) - 1u), o = tile >> (s.g_log + s.mid_log);
  e.valid = ((tile << s.c) | e.kappa) < lines;
  e.lowpos = ((uint32_t)g << s.c) + e.kappa;
  e.pos = o * s.o_stride + (dst ? mid * s.mid_dst + g * s.g_dst + e.rho * s.row_dst + e.kappa * s.col_dst
                                : mid * s.mid_src + g * s.g_src + e.rho * s.row_src + e.kappa * s.col_src);
  return e;
}
// r-bit reversal (r <= 10)
TE_HD uint32_t brev(uint32_t v, uint32_t r) {
  v = ((v >> 1) & 0x55555555u) | ((v & 0x55555555u) << 1);
  v = ((v >> 2) & 0x33333333u) | ((v & 0x33333333u) << 2);
  v = ((v >> 4) & 0x0f0f0f0fu) | ((v & 0x0f0f0f0fu) << 4);
  v = ((v >> 8) & 0x00ff00ffu) | ((v & 0x00ff00ffu) << 8);
  v = (v >> 16) | (v << 16);
  return r ? v >> (32u - r) : 0u;
}
// the LDS slot of place q of line kappa; a record is loaded into place brev(rho) and read back from place rho
TE_HD uint32_t slot_of(const pass& s, uint32_t kappa, uint32_t q) { return kappa * s.pitch + q; }
// butterfly b (< 512) of stage st (< r): slots u and u + 2^st, and the twiddle's index in the hi table: w_(2^(st+1))^k = hi[k << (11 - st)]
struct bfly { uint32_t u, v, tw; };
TE_HD bfly bfly_of(const pass& s, uint32_t st, uint32_t b) {
  const uint32_t kappa = b >> (s.r - 1u), q = b & ((1u << (s.r - 1u)) - 1u), k = q & ((1u << st) - 1u);
  bfly f;
  f.u = slot_of(s, kappa, ((q >> st) << (st + 1u)) + k);
  f.v = f.u + (1u << st);
  f.tw = k << (kSplitLog - 1u - st);
  return f;
}
// the twiddle behind the butterflies of a pass: an exponent of Omega below 2^24
TE_HD uint32_t twiddle_exp(const pass& s, const elem& e) { return (uint32_t)(((uint64_t)e.rho * e.lowpos) << s.tw_shift); }
// Omega^(-E): the same tables read at 2^24 - E
TE_HD uint32_t root_index(uint32_t E, bool inverse) { return inverse ? (0u - E) & ((1u << kRootLog) - 1u) : E; }

}  // namespace te_ntt
