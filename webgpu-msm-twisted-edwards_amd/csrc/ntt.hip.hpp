// ntt.hip.hpp -- batched number-theoretic transforms over p (te_msm_ntt*; include/te_msm.h "batched NTTs"): the
// radix-2 domains of arkworks / snarkVM over BLS12-377's scalar field, natural order in and out.  ntt_plan.hpp says which passes a size
// runs in and forms every index; this file is the arithmetic of one lane in each of a block's three phases, and the kernels.
//
// Like field_ops.hip.hpp, the per-lane functions are TE_HD and the kernels sit under __HIPCC__: tests/csrc/nttcheck.cpp runs a block
// on the CPU as plain loops over its lanes, one loop per phase (a loop boundary is the block's barrier).
//
// ONE KERNEL, k_ntt_pass: a block of 256 lanes owns a tile of 2^10 records = 2^c lines of 2^r.
//   in     a lane loads 4 records (16-byte loads, runs of the plan), turns the first pass's into the Montgomery form (one product: with R^2 or
//          R^2 / A, or -- forward with a shift -- with R^2 s^i from the call's shift tables, one product more) and stores the 9 limbs
//          to LDS at place brev(rho) of its line.  Slots are 9 words apart and lines 2^r + 1 slots (multi-pass): both odd over 64 banks.
//   stage  r decimation-in-time stages; a lane does 2 butterflies per stage: t = v w (ONE product; w = hi[k << (11 - stage)], or read
//          at the negated index for the inverse), u' = norm(u + t), v' = norm(u - t + 2 p).
//   out    a lane reads 4 records at place rho, multiplies by the pass's twiddle Omega^E = hi[E >> 12] lo[E & 4095] (two products) and
//          stores the packed limbs -- or, in the last pass, by the encoding constant (1, A, 1 / n, A / n; with a shift the table value
//          s^-i / n, one product more) and stores the canonical words.
// LIMBS AND VALUES of everything stored (LDS, tmp, tables).  Table entries, decoded inputs and twiddled outputs are product outputs: class
//   N, below 1.2 p.  A record in tmp is such an output packed into 8 words (below 2^254) and read back by fp_from_words32: class N.  A
//   butterfly takes u, v of class N below B and stores norm(u + t), norm(u - t + 2 p): class N again (fe_norm), below B + t and B + 2 p,
//   where t = v w / R + p < B / 405 + p (w < 1.1 p, R = 446 p), which is also what the offset form of 2 p asks of it (t < 2 p).  So
//   B grows by at most 2 p + B / 405 per stage from 1.2 p: below 23 p after the 10 stages a pass can have -- and below 52 p = 2^257.9
//   after 24, had no pass boundary reset it -- far inside class N's 2^261 and the product's "operands below ~20 p x 1.1 p".  Every
//   product takes a class N operand and another one.
// Every global index is ntt_plan.hpp's elem_of, guarded by its `valid`; every LDS index its slot_of / bfly_of.
#pragma once
#include <string.h>
#include "field_ops.hip.hpp"
#include "ntt_plan.hpp"

namespace te {

// W = 22^((p - 1) / 2^47): arkworks' TWO_ADIC_ROOT_OF_UNITY of this field, of order 2^47; the domain of size 2^L uses W^(2^(47 - L))
constexpr uint32_t NTT_W_W32[8] = {0xec2a895eu, 0x476ef4a4u, 0x63e3f04au, 0x9b506ee3u, 0xd1a8a12fu, 0x60c69477u, 0x0cb92cc1u, 0x11d4b7f6u};
constexpr uint32_t NTT_TWO_ADICITY = 47u;

struct ntt_consts { fel<9> dec, enc; };                            // the first pass's decoding constant, the last pass's encoding constant
// hi, lo: the twiddle tables of the device; sh_hi, sh_lo: the shift tables of the call (nullptr: no shift)
struct ntt_tabs { const uint32_t *hi, *lo, *sh_hi, *sh_lo; };

TE_HD fel<9> ntt_tab(const uint32_t* t, uint32_t i) {
  fel<9> r;
  const uint32_t* p = t + (size_t)te_ntt::kTabWords * i;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = p[k];
  return r;
}
TE_HD fel<9> ntt_two_level(const uint32_t* hi, const uint32_t* lo, uint32_t e) {
  return fe_mul(ntt_tab(hi, e >> te_ntt::kSplitLog), ntt_tab(lo, e & (te_ntt::kTabEntries - 1u)));
}
TE_HD void ntt_lds_put(uint32_t* lds, uint32_t slot, const fel<9>& v) {
#pragma unroll
  for (int k = 0; k < 9; k++) lds[slot * te_ntt::kLimbs + k] = v.v[k];
}
TE_HD fel<9> ntt_lds_get(const uint32_t* lds, uint32_t slot) {
  fel<9> r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = lds[slot * te_ntt::kLimbs + k];
  return r;
}
// class N below 2^256 -> its 8 words, as it is (fo_words without the subtraction)
TE_HD void ntt_pack(const fel<9>& c, uint32_t (&w)[8]) {
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int bit = 32 * j, i = bit / 29, s = bit % 29;
    uint32_t v = c.v[i] >> s;
    if (i + 1 < 9) v |= c.v[i + 1] << (29 - s);
    if (i + 2 < 9 && 58 - s < 32) v |= c.v[i + 2] << (58 - s);
    w[j] = v;
  }
}
// g^j, j < 4096 (g and the result in Montgomery form), times `pre` as a plain factor when with_pre: the entry j of a table
TE_HD fel<9> ntt_power(const fel<9>& g, uint32_t j, const fel<9>& pre, bool with_pre) {
  fel<9> acc = fe_one<9>();
#pragma unroll 1
  for (int b = (int)te_ntt::kSplitLog - 1; b >= 0; b--) {
    acc = fe_mul(acc, acc);
    if ((j >> b) & 1u) acc = fe_mul(acc, g);
  }
  return with_pre ? fe_mul(pre, acc) : acc;
}

// ---- one lane of k_ntt_pass -------------------------------------------------------------------------------------------------------
// in: the words of record e (src side) -> LDS.  A line that does not exist is stored as zeros
TE_HD void ntt_lane_in(const te_ntt::pass& ps, const te_ntt::elem& e, const uint32_t (&w)[8], const fel<9>& dec, const ntt_tabs& tb, bool shift_in, uint32_t* lds) {
  fel<9> v = e.valid ? fp_from_words32(w) : fe_zero<9>();
  if (ps.first) {
    fel<9> k = dec;
    if (shift_in) k = ntt_two_level(tb.sh_hi, tb.sh_lo, (uint32_t)(e.pos & ((1ull << ps.log_n) - 1u)));
    v = fe_mul(v, k);
  }
  ntt_lds_put(lds, te_ntt::slot_of(ps, e.kappa, te_ntt::brev(e.rho, ps.r)), v);
}
// stage: butterfly b of stage st
TE_HD void ntt_lane_stage(const te_ntt::pass& ps, uint32_t st, uint32_t b, bool inverse, const ntt_tabs& tb, uint32_t* lds) {
  const te_ntt::bfly f = te_ntt::bfly_of(ps, st, b);
  const fel<9> u = ntt_lds_get(lds, f.u), v = ntt_lds_get(lds, f.v);
  const fel<9> t = fe_mul(v, ntt_tab(tb.hi, inverse ? (te_ntt::kTabEntries - f.tw) & (te_ntt::kTabEntries - 1u) : f.tw));
  ntt_lds_put(lds, f.u, fe_norm(fe_add(u, t)));
  ntt_lds_put(lds, f.v, fe_norm(fe_sub<2>(u, t)));
}
// out: LDS -> the words of record e (dst side)
TE_HD void ntt_lane_out(const te_ntt::pass& ps, const te_ntt::elem& e, bool inverse, const fel<9>& enc, const ntt_tabs& tb, bool shift_out, const uint32_t* lds,
                        uint32_t (&w)[8]) {
  const fel<9> y = ntt_lds_get(lds, te_ntt::slot_of(ps, e.kappa, e.rho));
  if (!ps.last) {
    ntt_pack(fe_mul(y, ntt_two_level(tb.hi, tb.lo, te_ntt::root_index(te_ntt::twiddle_exp(ps, e), inverse))), w);
  } else {
    fel<9> k = enc;
    if (shift_out) k = ntt_two_level(tb.sh_hi, tb.sh_lo, (uint32_t)(e.pos & ((1ull << ps.log_n) - 1u)));
    fo_words<9, 8>(fe_mul(y, k), w);
  }
}

// ---- what a call computes on the host before it launches (points.hip; the shim of the CPU tests calls the same functions) ------------
struct ntt_req { uint32_t log_n = 0; bool inverse = false, mont = false, shifted = false; fel<9> s = {}; };      // s: the shift in Montgomery form
enum { NTT_OK = 0, NTT_BAD_LOG_N, NTT_BAD_FLAGS, NTT_TOO_LARGE, NTT_NULL, NTT_ZERO_SHIFT };
// what every te_msm_ntt* call checks first: NTT_OK with q filled, or why it is refused
inline int ntt_check(const void* a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, const void* out, ntt_req& q) {
  if (log_n > TE_MSM_NTT_MAX_LOG_N) return NTT_BAD_LOG_N;
  if (flags & ~(TE_MSM_NTT_INVERSE | TE_MSM_NTT_MONTGOMERY)) return NTT_BAD_FLAGS;
  if (count > (UINT64_MAX >> 6 >> log_n)) return NTT_TOO_LARGE;
  if (count > 0 && (!a || !out)) return NTT_NULL;
  q.log_n = log_n; q.inverse = (flags & TE_MSM_NTT_INVERSE) != 0; q.mont = (flags & TE_MSM_NTT_MONTGOMERY) != 0; q.shifted = shift != nullptr;
  if (shift) {
    uint32_t w[8];
    memcpy(w, shift, 32);
    q.s = q.mont ? fo_decode<9, true>(w) : fo_decode<9, false>(w);
    if (fo_is_zero(q.s)) return NTT_ZERO_SHIFT;
  }
  return NTT_OK;
}
// the constants of the first load and the last store: R^2 or R^2 / A; the integer 1 or A, times 1 / n for the inverse (one fe_inv)
inline ntt_consts ntt_consts_of(const ntt_req& q) {
  ntt_consts k;
  k.dec = q.mont ? fo_decode_const<9, true>() : fo_decode_const<9, false>();
  k.enc = fe_zero<9>(); k.enc.v[0] = 1u;
  if (q.mont) k.enc = fo_A<9>();
  if (q.inverse) {
    fel<9> nn = fe_one<9>();
    for (uint32_t i = 0; i < q.log_n; i++) nn = fo_residue(fe_norm(fe_add(nn, nn)));      // n in Montgomery form
    k.enc = fe_mul(fe_inv(nn, kInvExpTe), k.enc);
  }
  return k;
}
// W^(2^(47 - L)) in Montgomery form (L <= 47)
inline fel<9> ntt_root_of(uint32_t L) {
  uint32_t w[8];
  memcpy(w, NTT_W_W32, 32);
  fel<9> g = fo_decode<9, false>(w);
  for (uint32_t i = L; i < NTT_TWO_ADICITY; i++) g = fe_mul(g, g);
  return g;
}
// the generators of a table pair: lo holds g^j, hi (g^4096)^j
inline void ntt_table_gens(const fel<9>& g, fel<9>& hi, fel<9>& lo) {
  lo = hi = g;
  for (uint32_t i = 0; i < te_ntt::kSplitLog; i++) hi = fe_mul(hi, hi);
}
// ... of the twiddle tables (g = Omega), and of a call's shift tables (g = s, or 1 / s for the inverse: one fe_inv), whose hi table
// carries the decoding (forward) or encoding (inverse) constant as a plain factor
inline void ntt_twiddle_gens(fel<9>& hi, fel<9>& lo) { ntt_table_gens(ntt_root_of(te_ntt::kRootLog), hi, lo); }
inline void ntt_shift_gens(const ntt_req& q, fel<9>& hi, fel<9>& lo) { ntt_table_gens(q.inverse ? fe_inv(q.s, kInvExpTe) : q.s, hi, lo); }

#if defined(__HIPCC__)
// entry j of a table of 4096 powers of g (ntt_power)
__global__ __launch_bounds__(256) void k_ntt_table(fel<9> g, fel<9> pre, int with_pre, uint32_t* out) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= te_ntt::kTabEntries) return;
  const fel<9> v = ntt_power(g, j, pre, with_pre != 0);
  uint4* o = reinterpret_cast<uint4*>(out) + (size_t)3 * j;
  o[0] = make_uint4(v.v[0], v.v[1], v.v[2], v.v[3]);
  o[1] = make_uint4(v.v[4], v.v[5], v.v[6], v.v[7]);
  o[2] = make_uint4(v.v[8], 0u, 0u, 0u);
}
// grid = tiles_of(ps, transforms of the launch); src and dst are not __restrict__: a one-pass launch may have dst == src (a block reads
// its whole tile before the barrier and writes the same records behind it)
template <bool INVERSE, bool SHIFT> __global__ __launch_bounds__(256) void k_ntt_pass(const uint4* src, uint4* dst, te_ntt::pass ps, uint64_t lines, ntt_consts k, ntt_tabs tb) {
  __shared__ uint32_t lds[te_ntt::kLdsSlots * te_ntt::kLimbs];
  const uint64_t tile = blockIdx.x;
  constexpr bool SHIFT_IN = SHIFT && !INVERSE, SHIFT_OUT = SHIFT && INVERSE;
#pragma unroll 1
  for (uint32_t q = 0; q < te_ntt::kElemsPerLane; q++) {
    const te_ntt::elem e = te_ntt::elem_of(ps, tile, threadIdx.x + te_ntt::kLanes * q, lines, false);
    uint32_t w[8] = {};
    if (e.valid) fo_load<2>(src, (size_t)e.pos * 2, w);
    ntt_lane_in(ps, e, w, k.dec, tb, SHIFT_IN, lds);
  }
  __syncthreads();
#pragma unroll 1
  for (uint32_t st = 0; st < ps.r; st++) {
#pragma unroll 1
    for (uint32_t q = 0; q < te_ntt::kBflyPerLane; q++) ntt_lane_stage(ps, st, threadIdx.x + te_ntt::kLanes * q, INVERSE, tb, lds);
    __syncthreads();
  }
#pragma unroll 1
  for (uint32_t q = 0; q < te_ntt::kElemsPerLane; q++) {
    const te_ntt::elem e = te_ntt::elem_of(ps, tile, threadIdx.x + te_ntt::kLanes * q, lines, true);
    if (!e.valid) continue;
    uint32_t w[8];
    ntt_lane_out(ps, e, INVERSE, k.enc, tb, SHIFT_OUT, lds, w);
    fo_store<2>(dst, (size_t)e.pos * 2, w);
  }
}
#endif

}  // namespace te
