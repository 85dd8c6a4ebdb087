// group_add.hip.hpp -- batched group addition out[i] = A_i +- B_i and the sum of a point buffer (te_msm_add*, te_msm_sum*; include/te_msm.h
// "batched group addition and point-set sums").  The reference's bulkAddGroups / reduceGroups.
//
// Like scalar_mul.hip.hpp, the per-lane functions are TE_HD and the kernels sit under __HIPCC__: tests/csrc/groupaddcheck.cpp runs the
// exact code of the kernels on the CPU, the sum's block as plain loops over its 256 lanes (a barrier is where one loop ends).
//
// THE GROUP LAWS are check.hip.hpp's: ete_add (here with the negation of B folded in, ete_add_cneg) is complete on the whole
// Twisted-Edwards curve, cofactor part included; sw377_add is the complete Renes-Costello-Batina addition on y^2 = x^3 + 1 for inputs
// in G1.  One addition serves A = B, A = -B and the neutral element: no lane branches on its data.
// BLS12-377 INFINITY: these calls write the point at infinity as 96 zero bytes, so they read that record as (0 : 1 : 0) -- a select
// on the OR of the record's words, in front of the addition.
//
// AFFINE OUTPUT: k_group_add writes projective slots in the layout of sm_sizes and te_msm_mul's k_scalar_mul_affine (chains of eight,
// unchanged) turns them into canonical x || y.  A block-wide batch inversion -- one Fermat inversion per 2048 points, prefix and suffix
// product scans through LDS -- was built and measured against it at 2^20 pairs (profiles/group_add_cost.txt): it
// was not lower in every round on either curve and was removed.  One lane's inversion chain is a latency the whole block waits for,
// while the chains of eight run theirs on every lane of two waves a SIMD that overlap each other.
//
// SUM (k_group_sum): a bounded grid; lane g adds points g, g + stride, .. into a projective accumulator that starts at the neutral
// element, the block folds its 256 accumulators through LDS (128 slots: the upper half of the active lanes stores, the lower half
// adds) and writes one projective partial; the same kernel over the partials, one block, leaves one.  A partial is X | Y | Z (| T):
// its head is a projective slot of sm_sizes, which the host normalises with sm_affine_group (one point: the host's inversion is
// faster than a launch whose one lane runs the chain).
//
// Every address is an affine function of the thread id, bounded by m.
#pragma once
#include <type_traits>
#include "scalar_mul.hip.hpp"

namespace te {

#define GS_BLOCK 256u                                              // lanes of a block of the sum
#define GS_SH_SLOTS 128u                                           // accumulators the sum's fold holds in LDS

template <int CURVE> using ga_pt = std::conditional_t<CURVE == 1, sw377, ete>;
template <int CURVE> struct ga_sizes {
  static constexpr int N = sm_sizes<CURVE>::N, PW = sm_sizes<CURVE>::PW, JW = sm_sizes<CURVE>::JW;
  static constexpr int AW = CURVE == 1 ? 42 : 36;                  // words of an accumulator: X | Y | Z (| T)
  static constexpr int TW = CURVE == 1 ? 44 : 36;                  // words of a partial (AW, rounded up to 16 bytes)
};

template <int CURVE> TE_HD ga_pt<CURVE> ga_identity() {
  if constexpr (CURVE == 1) return sw377_identity(); else return ete_identity();
}
// wire words -> the point; BLS12-377: the all-zero record is the point at infinity
template <int CURVE> TE_HD ga_pt<CURVE> ga_decode(const uint32_t (&w)[ga_sizes<CURVE>::PW]) {
  if constexpr (CURVE == 1) {
    te377::fq X, Y, sx;
    c377_coords(w, X, Y, sx);
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 24; i++) any |= w[i];
    return sw377_select(any == 0u, sw377_identity(), sw377_of(X, Y));
  } else {
    fp X, Y;
    te_coords(w, X, Y);
    return ete_of(X, Y);
  }
}
// a + (neg ? -b : b): one complete addition, the negation under a select
template <int CURVE> TE_HD ga_pt<CURVE> ga_add(const ga_pt<CURVE>& a, const ga_pt<CURVE>& b, bool neg) {
  if constexpr (CURVE == 1) return sw377_add(a, sw377_cneg(b, neg)); else return ete_add_cneg(a, b, neg);
}
// accumulator words X | Y | Z (| T), and back
template <int CURVE> TE_HD void ga_words(const ga_pt<CURVE>& p, uint32_t* o) {
  constexpr int N = ga_sizes<CURVE>::N;
#pragma unroll
  for (int i = 0; i < N; i++) {
    o[i] = p.x.v[i]; o[N + i] = p.y.v[i]; o[2 * N + i] = p.z.v[i];
    if constexpr (CURVE != 1) o[3 * N + i] = p.t.v[i];
  }
}
template <int CURVE> TE_HD ga_pt<CURVE> ga_of_words(const uint32_t* w) {
  constexpr int N = ga_sizes<CURVE>::N;
  ga_pt<CURVE> p;
#pragma unroll
  for (int i = 0; i < N; i++) {
    p.x.v[i] = w[i]; p.y.v[i] = w[N + i]; p.z.v[i] = w[2 * N + i];
    if constexpr (CURVE != 1) p.t.v[i] = w[3 * N + i];
  }
  return p;
}

// ---- one lane of k_group_add: the words of A_i and B_i -> the projective slot of A_i +- B_i (JW words, the padding zero) ---------------
template <int CURVE> TE_HD void ga_pair(const uint32_t (&wa)[ga_sizes<CURVE>::PW], const uint32_t (&wb)[ga_sizes<CURVE>::PW], bool neg,
                                        uint32_t (&o)[ga_sizes<CURVE>::JW]) {
  constexpr int N = ga_sizes<CURVE>::N, JW = ga_sizes<CURVE>::JW;
  const ga_pt<CURVE> r = ga_add<CURVE>(ga_decode<CURVE>(wa), ga_decode<CURVE>(wb), neg);
#pragma unroll
  for (int i = 0; i < N; i++) { o[i] = r.x.v[i]; o[N + i] = r.y.v[i]; o[2 * N + i] = r.z.v[i]; }
#pragma unroll
  for (int i = 3 * N; i < JW; i++) o[i] = 0u;
}

// ---- the sum: one step of a lane's accumulation, and the fold through LDS (word-major rows of GS_SH_SLOTS) ---------------------------
// PARTIALS: w holds a partial (TW words) instead of a wire point (PW words)
template <int CURVE, bool PARTIALS> TE_HD ga_pt<CURVE> gs_step(const ga_pt<CURVE>& acc, const uint32_t (&w)[PARTIALS ? ga_sizes<CURVE>::TW : ga_sizes<CURVE>::PW]) {
  if constexpr (PARTIALS) return ga_add<CURVE>(acc, ga_of_words<CURVE>(w), false);
  else return ga_add<CURVE>(acc, ga_decode<CURVE>(w), false);
}
// one fold step over the lanes [0, 2 s): lanes [s, 2 s) store ...
template <int CURVE> TE_HD void gs_fold_store(uint32_t lane, uint32_t* sh, uint32_t s, const ga_pt<CURVE>& acc) {
  if (lane < s || lane >= 2u * s) return;
  uint32_t w[ga_sizes<CURVE>::AW];
  ga_words<CURVE>(acc, w);
#pragma unroll
  for (int i = 0; i < ga_sizes<CURVE>::AW; i++) sh[(uint32_t)i * GS_SH_SLOTS + (lane - s)] = w[i];
}
// ... and, behind a barrier, lanes [0, s) add (a second barrier before the next step's stores)
template <int CURVE> TE_HD void gs_fold_add(uint32_t lane, const uint32_t* sh, uint32_t s, ga_pt<CURVE>& acc) {
  if (lane >= s) return;
  uint32_t w[ga_sizes<CURVE>::AW];
#pragma unroll
  for (int i = 0; i < ga_sizes<CURVE>::AW; i++) w[i] = sh[(uint32_t)i * GS_SH_SLOTS + lane];
  acc = ga_add<CURVE>(acc, ga_of_words<CURVE>(w), false);
}

// ---- option "check_points" for these calls: check.hip.hpp's verdicts, with the all-zero BLS12-377 record passing both levels -----------
template <int CURVE> TE_HD bool ga_is_infinity_record(const uint32_t (&w)[ga_sizes<CURVE>::PW]) {
  if constexpr (CURVE != 1) return false;
  uint32_t any = 0;
#pragma unroll
  for (int i = 0; i < ga_sizes<CURVE>::PW; i++) any |= w[i];
  return any == 0u;
}
template <int CURVE> TE_HD int ga_check_form(const uint32_t (&w)[ga_sizes<CURVE>::PW]) {
  int reason;
  if constexpr (CURVE == 1) reason = check_form_377(w); else reason = check_form_te(w);
  return ga_is_infinity_record<CURVE>(w) ? 0 : reason;
}
template <int CURVE> TE_HD bool ga_in_subgroup(const uint32_t (&w)[ga_sizes<CURVE>::PW], const naf_t& k) {
  bool in;
  if constexpr (CURVE == 1) in = in_subgroup_377(w, k); else in = in_subgroup_te(w, k);
  return in || ga_is_infinity_record<CURVE>(w);
}

#if defined(__HIPCC__)
template <int Q4> __device__ __forceinline__ void ga_load_words(const uint4* __restrict__ src, size_t at, uint32_t (&w)[Q4 * 4]) {
#pragma unroll
  for (int j = 0; j < Q4; j++) { const uint4 v = src[at + j]; w[4 * j] = v.x; w[4 * j + 1] = v.y; w[4 * j + 2] = v.z; w[4 * j + 3] = v.w; }
}
// one lane per pair of a piece of m; SHARED_B: b holds one point.  Lane i < m reads 16-byte words [i PQ, i PQ + PQ) of a (and of b),
// writes words [i JQ, i JQ + JQ) of proj
template <int CURVE, bool SHARED_B> __global__ __launch_bounds__(256) void k_group_add(const uint4* __restrict__ a, const uint4* __restrict__ b, uint32_t m, int neg,
                                                                                       uint4* __restrict__ proj) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  constexpr int PQ = ga_sizes<CURVE>::PW / 4, JQ = ga_sizes<CURVE>::JW / 4;
  uint32_t wa[4 * PQ], wb[4 * PQ], o[4 * JQ];
  ga_load_words<PQ>(a, (size_t)i * PQ, wa);
  ga_load_words<PQ>(b, SHARED_B ? (size_t)0 : (size_t)i * PQ, wb);
  ga_pair<CURVE>(wa, wb, neg != 0, o);
#pragma unroll
  for (int j = 0; j < JQ; j++) proj[(size_t)i * JQ + j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
}
// grid <= the bound the host passes (TE_MSM_GROUP_SUM_GRID); count items (wire points, or PARTIALS) -> one partial per block
template <int CURVE, bool PARTIALS> __global__ __launch_bounds__(256) void k_group_sum(const uint4* __restrict__ src, uint32_t count, uint4* __restrict__ partials) {
  constexpr int SQ = (PARTIALS ? ga_sizes<CURVE>::TW : ga_sizes<CURVE>::PW) / 4, TQ = ga_sizes<CURVE>::TW / 4;
  __shared__ uint32_t sh[ga_sizes<CURVE>::AW * GS_SH_SLOTS];
  const uint32_t lane = threadIdx.x, stride = gridDim.x * blockDim.x;
  ga_pt<CURVE> acc = ga_identity<CURVE>();
#pragma unroll 1
  for (uint64_t i = blockIdx.x * blockDim.x + lane; i < count; i += stride) {
    uint32_t w[4 * SQ];
    ga_load_words<SQ>(src, (size_t)i * SQ, w);
    acc = gs_step<CURVE, PARTIALS>(acc, w);
  }
#pragma unroll 1
  for (uint32_t s = GS_SH_SLOTS; s >= 1u; s >>= 1) {
    gs_fold_store<CURVE>(lane, sh, s, acc);
    __syncthreads();
    gs_fold_add<CURVE>(lane, sh, s, acc);
    __syncthreads();
  }
  if (lane != 0u) return;
  uint32_t o[4 * TQ];
  ga_words<CURVE>(acc, o);
#pragma unroll
  for (int j = ga_sizes<CURVE>::AW; j < 4 * TQ; j++) o[j] = 0u;
#pragma unroll
  for (int j = 0; j < TQ; j++) partials[(size_t)blockIdx.x * TQ + j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
}
// option "check_points" of te_msm_add* / te_msm_sum*: k_check_form / k_check_subgroup with the BLS12-377 zero record passing
template <int CURVE> __global__ __launch_bounds__(256) void k_group_check_form(const uint4* __restrict__ pts, uint32_t n, unsigned long long* word) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int PQ = ga_sizes<CURVE>::PW / 4;
  uint32_t w[4 * PQ];
  ga_load_words<PQ>(pts, (size_t)i * PQ, w);
  const int reason = ga_check_form<CURVE>(w);
  if (reason) atomicMax(word, (unsigned long long)check_code(n, i, reason));
}
template <int CURVE> __global__ __launch_bounds__(256) void k_group_check_subgroup(const uint4* __restrict__ pts, uint32_t n, unsigned long long* word, naf_t k) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int PQ = ga_sizes<CURVE>::PW / 4;
  uint32_t w[4 * PQ];
  ga_load_words<PQ>(pts, (size_t)i * PQ, w);
  if (!ga_in_subgroup<CURVE>(w, k)) atomicMax(word, (unsigned long long)check_code(n, i, 3));
}
#endif

}  // namespace te
