// scan.hip.hpp -- prefix sums and prefix products over p (te_msm_field_scan*; include/te_msm.h "prefix sums and products", DESIGN.md
// section 25): out[i] = e o a_0 o .. o a_i (inclusive) or e o a_0 o .. o a_(i-1) (exclusive) and totals = e o a_0 o .. o a_(n-1), o being
// + or * mod p and e the vector's seed -- the grand product of a permutation argument, a running sum, the powers of one record.
// scan_plan.hpp says which levels a call runs, forms every index and says where the sum path reduces; this file is the arithmetic of one
// lane in each phase of a block, and the two kernels.
//
// Like poly.hip.hpp, the per-lane functions are TE_HD and the kernels sit under __HIPCC__: tests/csrc/scancheck.cpp runs a block on the
// CPU as plain loops over its lanes, one loop per phase (a loop boundary is the block's barrier).
//
// TWO KERNELS, a block of 256 lanes on a tile of T = 256 chunk elements (chunk is a run-time argument), each compiled for + and for *:
//   k_scan_totals  lane l combines the elements l + 256 j of its tile (every load of a wave covers 64 consecutive records), then 8
//                  tree steps through LDS combine the lanes: lane 0 holds the tile's total, takes the seed in at the last level (one tile
//                  a vector) and writes it.  Nothing else is read or written.
//   k_scan_apply   the tile goes through LDS: loaded as k_scan_totals loads it and stored as 8 words in the internal form; behind the
//                  barrier lane l owns the chunk CONSECUTIVE elements l chunk .. l chunk + chunk - 1.  It walks them once for its own total,
//                  8 Hillis-Steele steps make that inclusive over the lanes, and lane l takes lane l - 1's value and the tile's carry: the
//                  value in front of its first element.  It walks its chunk again and stores every inclusive or exclusive value over the
//                  element in LDS, in the form the launch writes.  Behind a last barrier the tile is stored as it was loaded.  A block reads
//                  its tile before its first barrier and writes behind its last, and totals and apply are separate launches: out may be a.
// FORMS (scan_plan.hpp kInternal / kCanonical / kMontgomery) are run-time arguments of a launch: level 0 reads and writes the caller's
//   form, the totals of the last level leave in the caller's form, everything in scratch and in LDS is internal.
//   THE SUM is linear: a A + b A = (a + b) A, so both caller's forms are one code path and nothing is decoded.  Internal = the value's words.
//   THE PRODUCT is not.  An element enters the Montgomery form of fp.hpp (fo_decode: one product with R^2, or R^2 / A for words that hold
//   a A), products run there, and an output leaves it (fo_encode: one product with 1 or A).  Internal = the canonical words of v R mod p:
//   read back as limbs (fp_from_words32) they are the Montgomery form, so levels >= 1, the carries and the second walk decode nothing.
//   PRODUCTS AN ELEMENT, product scan: totals 2 (decode, combine) + 9 / T; apply 4 (decode into LDS, own total, walk, encode) + 9 / chunk
//   (8 scan steps and the carry).  Sum scan: totals 1 / chunk (the lane's reduction); apply 1 (the output's reduction) + 2 / chunk.
//   Levels >= 1 cost 1 / T of that.  A zero factor is an ordinary value (mont_mul gives p for 0 x b; fo_words makes it 0): nothing inverts.
// LIMBS AND VALUES of everything stored (R = 2^261 = 438.8 p, 2^256 = 13.72 p; mont_mul(a, b) <= a b / R + p, exact for a class N operand
//   with a top limb below 2^29, that is a value below R, and one more of class N).
//   Product path.  LDS tile and scratch: canonical words (below p).  Decoded elements, lane totals, scan area, prefixes: product outputs,
//   class N below 13.72 p p / R + p < 1.04 p.  Every product takes two class N operands below 13.72 p.
//   Sum path.  LDS tile: the words as loaded, any 256-bit value (below 13.72 p) at level 0, canonical above.  A lane's total: at most 16
//   of them, normalised after each addition: class N below 219.5 p, REDUCED (scan_plan.hpp sum_reduces_lane_total) to below
//   219.5 x 0.79 / 438.8 p + p < 1.40 p.  The 8 steps of the tree / scan add at most 256 lanes' totals: the scan area holds class N values
//   below 358.4 p.  With the carry (a scratch record below p, or a raw seed below 13.72 p): below 372.1 p < R.  k_scan_totals reduces that
//   once for its output (below 1.67 p < 2 p: fo_words).  k_scan_apply reduces the lane's prefix (sum_reduces_prefix) to below 1.67 p, the
//   walk adds at most 16 elements: below 221.2 p, and every output is reduced to below 1.40 p before fo_words.  Scratch: canonical words.
//   Without the lane's reduction T = 4096 records of 2^256 - 1 reach 56 000 p = 2^268.8 and the top limb leaves its 32 bits.
// Every global index is scan_plan.hpp's tile_of / total_of / load_of, guarded by the tile's `fill`; every LDS index its lds_word.  All
// offsets are 64 bits wide.  No atomics: the same bytes every time.
#pragma once
#include <string.h>
#include "field_ops.hip.hpp"
#include "scan_plan.hpp"

namespace te {

template <int OP> TE_HD fel<9> scan_identity() { if constexpr (OP == te_scan::kSum) return fe_zero<9>(); else return fe_one<9>(); }
template <int OP> TE_HD fel<9> scan_combine(const fel<9>& a, const fel<9>& b) {
  if constexpr (OP == te_scan::kSum) return fe_norm(fe_add(a, b)); else return fe_mul(a, b);
}
// class N below R -> class N below value x 0.79 / 438.8 + p
TE_HD fel<9> scan_reduce(const fel<9>& a) { return fe_mul(a, fe_one<9>()); }
// the words of a record in `form` -> the value a lane combines
template <int OP> TE_HD fel<9> scan_in(const uint32_t (&w)[8], uint32_t form) {
  const fel<9> x = fp_from_words32(w);
  if constexpr (OP == te_scan::kProduct) {
    if (form != te_scan::kInternal) return fe_mul(x, form == te_scan::kMontgomery ? fp_R2_A() : fp_R2());
  }
  return x;
}
// a value a lane holds (sum: class N below R; product: a product output) -> the words of a record in `form`.  raw_internal (false in every
// real use) is the test shim's deliberate mistake: a product's output left in the internal form
template <int OP> TE_HD void scan_out(const fel<9>& h, uint32_t form, uint32_t (&w)[8], bool raw_internal = false) {
  if constexpr (OP == te_scan::kSum) fo_words<9, 8>(scan_reduce(h), w);
  else {
    if (form == te_scan::kInternal || raw_internal) { fo_words<9, 8>(h, w); return; }
    fel<9> k = fe_zero<9>(); k.v[0] = 1u;
    if (form == te_scan::kMontgomery) k = fo_A<9>();
    fo_words<9, 8>(fe_mul(h, k), w);
  }
}
// the words of a record in `form` -> what the LDS tile holds of it: internal words
template <int OP> TE_HD void scan_stage(const uint32_t (&w)[8], uint32_t form, uint32_t (&o)[8]) {
  if (OP == te_scan::kSum || form == te_scan::kInternal) {
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = w[k];
  } else fo_words<9, 8>(scan_in<OP>(w, form), o);
}
// ... and of an element past the tile's fill: the identity.  zero_pad (false in every real use): the shim's deliberate mistake
template <int OP> TE_HD void scan_pad(uint32_t (&o)[8], bool zero_pad = false) {
  if (OP == te_scan::kSum || zero_pad) {
#pragma unroll
    for (int k = 0; k < 8; k++) o[k] = 0u;
  } else fo_words<9, 8>(fe_one<9>(), o);
}
TE_HD void scan_area_put(uint32_t* scan, uint32_t lane, const fel<9>& v) {
#pragma unroll
  for (int k = 0; k < 9; k++) scan[lane * te_scan::kScanLimbs + k] = v.v[k];
}
TE_HD fel<9> scan_area_get(const uint32_t* scan, uint32_t lane) {
  fel<9> r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = scan[lane * te_scan::kScanLimbs + k];
  return r;
}
TE_HD void scan_lds_put(uint32_t* lds, uint32_t word, const uint32_t (&w)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) lds[word + k] = w[k];
}
TE_HD void scan_lds_get(const uint32_t* lds, uint32_t word, uint32_t (&w)[8]) {
#pragma unroll
  for (int k = 0; k < 8; k++) w[k] = lds[word + k];
}
// step s of the tree of k_scan_totals: lane l takes lane l + 2^s in when l is a multiple of 2^(s+1)
TE_HD bool scan_tree_takes(uint32_t lane, uint32_t s) { return (lane & ((2u << s) - 1u)) == 0u; }
// step s of the scan of k_scan_apply: lane l takes lane l - 2^s in when there is one
TE_HD bool scan_step_takes(uint32_t lane, uint32_t s) { return lane >= (1u << s); }

// ---- one lane in each phase (the kernels below and the shim's loops call exactly these) ------------------------------------------------
// totals, phase 1: element j of the lane's walk (x = lane + 256 j inside the fill) joins its value
template <int OP> TE_HD void scan_take(const uint32_t (&w)[8], uint32_t form, bool first, fel<9>& acc) {
  const fel<9> v = scan_in<OP>(w, form);
  acc = first ? v : scan_combine<OP>(acc, v);
}
// ... and what closes a lane's own total (the sum's reduction; reduce = false is the shim's deliberate mistake)
template <int OP> TE_HD void scan_close_total(fel<9>& acc, bool reduce = true) {
  if constexpr (OP == te_scan::kSum) { if (te_scan::sum_reduces_lane_total() && reduce) acc = scan_reduce(acc); }
}
template <int OP> TE_HD void scan_after_step(fel<9>& acc, uint32_t s) {
  if constexpr (OP == te_scan::kSum) { if (te_scan::sum_reduces_step(s)) acc = scan_reduce(acc); }
}
// apply: the value in front of the lane's first element, from the tile's carry (internal words) and the lane before's inclusive value
template <int OP> TE_HD fel<9> scan_prefix(const uint32_t (&cw)[8], bool has_before, const fel<9>& before) {
  fel<9> h = fp_from_words32(cw);
  if (has_before) h = scan_combine<OP>(h, before);
  if constexpr (OP == te_scan::kSum) { if (te_scan::sum_reduces_prefix()) h = scan_reduce(h); }
  return h;
}
// apply, the second walk: element w (internal words) -> o, the words the tile stores in its place; h moves past the element
template <int OP> TE_HD void scan_walk(const uint32_t (&w)[8], bool exclusive, uint32_t form_out, fel<9>& h, uint32_t (&o)[8], bool raw_internal = false) {
  const fel<9> v = fp_from_words32(w);
  if (exclusive) { scan_out<OP>(h, form_out, o, raw_internal); h = scan_combine<OP>(h, v); }
  else { h = scan_combine<OP>(h, v); scan_out<OP>(h, form_out, o, raw_internal); }
}

// ---- what a call computes on the host before it launches (points.hip; the shim of the CPU tests calls the same functions) ------------
struct scan_req { int op = 0; uint64_t n = 0, count = 0; bool mont = false, exclusive = false, shared = false; uint32_t chunk = te_scan::kChunkDefault; };
enum { SCAN_OK = 0, SCAN_BAD_OP, SCAN_BAD_N, SCAN_BAD_FLAGS, SCAN_NO_OUTPUT, SCAN_TOO_LARGE, SCAN_NULL, SCAN_ALIAS };
// what every te_msm_field_scan* call checks first: SCAN_OK with r filled, or why it is refused
inline int scan_check(int op, const void* a, uint64_t n, uint64_t count, int flags, const void* totals, const void* out, scan_req& r) {
  if (op != TE_MSM_SCAN_SUM && op != TE_MSM_SCAN_PRODUCT) return SCAN_BAD_OP;
  if (n == 0 || n > TE_MSM_SCAN_MAX_N) return SCAN_BAD_N;
  if (flags & ~(TE_MSM_SCAN_MONTGOMERY | TE_MSM_SCAN_EXCLUSIVE | TE_MSM_SCAN_SHARED_A)) return SCAN_BAD_FLAGS;
  if (!totals && !out) return SCAN_NO_OUTPUT;
  if (count > (UINT64_MAX >> 5) / n) return SCAN_TOO_LARGE;
  if (count > 0 && !a) return SCAN_NULL;
  if (count > 0 && (flags & TE_MSM_SCAN_SHARED_A) && out == a) return SCAN_ALIAS;
  r.op = op; r.n = n; r.count = count; r.mont = (flags & TE_MSM_SCAN_MONTGOMERY) != 0; r.exclusive = (flags & TE_MSM_SCAN_EXCLUSIVE) != 0;
  r.shared = (flags & TE_MSM_SCAN_SHARED_A) != 0;
  return SCAN_OK;
}
TE_HD uint32_t scan_caller_form(const scan_req& r) { return r.mont ? te_scan::kMontgomery : te_scan::kCanonical; }
// the seeds of a call in the internal form, one record a vector: init's (NULL: the identity).  A sum's seed is its 256 bits as given
inline void scan_seeds(const scan_req& r, const uint8_t* init, uint8_t* out) {
  for (uint64_t k = 0; k < r.count; k++) {
    uint32_t w[8] = {}, o[8];
    if (init) memcpy(w, init + (size_t)32 * k, 32);
    if (r.op == TE_MSM_SCAN_SUM) memcpy(o, w, 32);
    else if (!init) scan_pad<te_scan::kProduct>(o);
    else scan_stage<te_scan::kProduct>(w, scan_caller_form(r), o);
    memcpy(out + (size_t)32 * k, o, 32);
  }
}

#if defined(__HIPCC__)
// grid = count x tiles of the level; a: the level's elements in form_in (shared: one record a vector), totals: record (vec, b) of the
// next level; seeds: nullptr, or -- the last level -- the vectors' seeds, taken in by lane 0; form_out: what the totals are written in
template <int OP> __global__ __launch_bounds__(256) void k_scan_totals(const uint4* __restrict__ a, uint4* __restrict__ totals, const uint4* __restrict__ seeds, te_scan::level v,
                                                                       uint32_t chunk, uint32_t form_in, uint32_t form_out, uint32_t shared) {
  __shared__ uint32_t scan[te_scan::kLanes * te_scan::kScanLimbs];
  const uint32_t lane = threadIdx.x;
  const te_scan::tile t = te_scan::tile_of(v, te_scan::kLanes * chunk, blockIdx.x);
  fel<9> acc = scan_identity<OP>();
#pragma unroll 1
  for (uint32_t j = 0; j < chunk; j++) {
    const uint32_t x = te_scan::wide_x(lane, j);
    if (x >= t.fill) break;
    uint32_t w[8];
    fo_load<2>(a, (size_t)te_scan::load_of(t, x, shared != 0u) * 2, w);
    scan_take<OP>(w, form_in, j == 0u, acc);
  }
  scan_close_total<OP>(acc);
#pragma unroll 1
  for (uint32_t s = 0; s < te_scan::kLog; s++) {
    scan_area_put(scan, lane, acc);
    __syncthreads();
    if (scan_tree_takes(lane, s)) { acc = scan_combine<OP>(acc, scan_area_get(scan, lane + (1u << s))); scan_after_step<OP>(acc, s); }
    __syncthreads();
  }
  if (lane == 0u) {
    uint32_t w[8];
    if (seeds) {
      fo_load<2>(seeds, (size_t)te_scan::total_of(v, t) * 2, w);
      acc = scan_combine<OP>(fp_from_words32(w), acc);
    }
    scan_out<OP>(acc, form_out, w);
    fo_store<2>(totals, (size_t)te_scan::total_of(v, t) * 2, w);
  }
}
// the same grid; carries: record (vec, b) of the next level's exclusive scan, or the seeds at the last level; internal form.  a and out
// are not __restrict__: out may be a.  Dynamic LDS: te_scan::lds_bytes_apply(chunk)
template <int OP> __global__ __launch_bounds__(256) void k_scan_apply(const uint4* a, uint4* out, const uint4* carries, te_scan::level v, uint32_t chunk, uint32_t form_in,
                                                                      uint32_t form_out, uint32_t exclusive, uint32_t shared) {
  extern __shared__ uint32_t scan_lds[];
  uint32_t* const lds = scan_lds;
  uint32_t* const scan = scan_lds + te_scan::lds_data_words(chunk);
  const uint32_t lane = threadIdx.x;
  const te_scan::tile t = te_scan::tile_of(v, te_scan::kLanes * chunk, blockIdx.x);
#pragma unroll 1
  for (uint32_t j = 0; j < chunk; j++) {
    const uint32_t x = te_scan::wide_x(lane, j);
    uint32_t w[8], o[8];
    if (x < t.fill) {
      fo_load<2>(a, (size_t)te_scan::load_of(t, x, shared != 0u) * 2, w);
      scan_stage<OP>(w, form_in, o);
    } else scan_pad<OP>(o);
    scan_lds_put(lds, te_scan::lds_word(x, chunk), o);
  }
  uint32_t cw[8];
  fo_load<2>(carries, (size_t)te_scan::total_of(v, t) * 2, cw);
  __syncthreads();
  fel<9> acc = scan_identity<OP>();
#pragma unroll 1
  for (uint32_t j = 0; j < chunk; j++) {
    uint32_t w[8];
    scan_lds_get(lds, te_scan::lds_word(te_scan::own_x(lane, j, chunk), chunk), w);
    scan_take<OP>(w, te_scan::kInternal, j == 0u, acc);
  }
  scan_close_total<OP>(acc);
#pragma unroll 1
  for (uint32_t s = 0; s < te_scan::kLog; s++) {
    scan_area_put(scan, lane, acc);
    __syncthreads();
    if (scan_step_takes(lane, s)) { acc = scan_combine<OP>(scan_area_get(scan, lane - (1u << s)), acc); scan_after_step<OP>(acc, s); }
    __syncthreads();
  }
  scan_area_put(scan, lane, acc);
  __syncthreads();
  fel<9> h = scan_prefix<OP>(cw, lane != 0u, scan_area_get(scan, lane ? lane - 1u : 0u));
#pragma unroll 1
  for (uint32_t j = 0; j < chunk; j++) {
    const uint32_t at = te_scan::lds_word(te_scan::own_x(lane, j, chunk), chunk);
    uint32_t w[8], o[8];
    scan_lds_get(lds, at, w);
    scan_walk<OP>(w, exclusive != 0u, form_out, h, o);
    scan_lds_put(lds, at, o);
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t j = 0; j < chunk; j++) {
    const uint32_t x = te_scan::wide_x(lane, j);
    if (x >= t.fill) break;
    uint32_t w[8];
    scan_lds_get(lds, te_scan::lds_word(x, chunk), w);
    fo_store<2>(out, (size_t)(t.base + x) * 2, w);
  }
}
#endif

}  // namespace te
