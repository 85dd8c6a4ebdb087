// signstate.cpp -- TEST SHIM: the sign state of k_accumulate (csrc/curve.hpp ete_open / ete_uv_neg / ete_madd_raw and the SGN closings),
// compiled for the host so tests/test_sign_state_host.py can check the exact limb code the GPU runs against bigints, for both curves
// and every record kind the kernel is instantiated with.  segment() below is the kernel's arithmetic for one segment, statement by
// statement, without its loads and index strip: whoever edits the sign handling of k_accumulate (csrc/kernels.hip.hpp) edits it here.
// The 14-limb products run with every column sum checked against 2^64 (g_fq377_overflow).  Not part of the product; not a fallback.
#include <stdint.h>
#include <string.h>
#define TE377_CHECK_COLUMNS 1
#include "../../webgpu-msm-twisted-edwards_amd/csrc/curve.hpp"

int g_fq377_overflow = 0;

using namespace te;

// trace: what the test asks of every intermediate -- the largest limb (below the top one) of an operand that met a record field
// in a product, and the number of sign changes the segment paid
struct seg_trace { uint32_t max_uv_limb, max_t_limb, flips; };

template <int N> static void note(seg_trace* tr, const ete_uv_t<N>& uv) {
  if (!tr) return;
  for (int i = 0; i < N - 1; i++) {
    if (uv.u.v[i] > tr->max_uv_limb) tr->max_uv_limb = uv.u.v[i];
    if (uv.v.v[i] > tr->max_uv_limb) tr->max_uv_limb = uv.v.v[i];
    if (uv.t.v[i] > tr->max_t_limb) tr->max_t_limb = uv.t.v[i];
  }
}

// k_accumulate for one segment of cnt entries (records as loaded, sign bits beside them); onto: the bucket's earlier sum or null
template <int N, class P> static ete_t<N> segment(const P* recs, const int* neg, uint32_t cnt, const ete_t<N>* onto, seg_trace* tr) {
  ete_t<N> acc = onto ? *onto : ete_identity_t<N>();
  bool flipped = false;
  if (cnt) {
    uint32_t j0 = 0;
    if (!onto) {
      flipped = neg[0] != 0;
      const bool ends = cnt <= 2u;
      if (cnt >= 2u) { acc = ete_from_pair<true>(recs[0], pnt_cneg(recs[1], (neg[1] != 0) != (neg[0] != 0)), ends && flipped); j0 = 2; }
      else { acc = ete_from_pnt<true>(recs[0], flipped); j0 = 1; }
    }
    ete_uv_t<N> uv = ete_open<N>(acc);
    auto sign_to = [&](uint32_t j) {
      const bool s = neg[j] != 0;
      if (s != flipped) { ete_uv_neg<N>(uv); flipped = s; if (tr) tr->flips++; }
      note<N>(tr, uv);
    };
    if (j0 < cnt) {
      uint32_t j = j0;
      for (; j + 2u < cnt; j += 2u) {
        sign_to(j);
        uv = ete_open<N>(ete_madd_raw(uv, recs[j]));
        sign_to(j + 1u);
        uv = ete_open<N>(ete_madd_raw(uv, recs[j + 1u]));
      }
      const bool two = j + 1u < cnt;
      sign_to(j);
      acc = ete_madd_raw<true>(uv, recs[j], !two && flipped);
      if (two) {
        uv = ete_open<N>(acc);
        sign_to(j + 1u);
        acc = ete_madd_raw<true>(uv, recs[j + 1u], flipped);
      }
    }
  }
  return acc;
}

template <int N, class P> static void run_segment(const uint32_t* recs, const int* neg, uint32_t cnt, const uint32_t* onto, uint32_t* out, uint32_t* trace) {
  P r[64];
  if (cnt > 64u) cnt = 64u;
  for (uint32_t i = 0; i < cnt; i++) memcpy(&r[i], recs + i * (sizeof(P) / 4u), sizeof(P));
  ete_t<N> o;
  if (onto) memcpy(&o, onto, sizeof o);
  seg_trace tr = {0u, 0u, 0u};
  const ete_t<N> res = segment<N, P>(r, neg, cnt, onto ? &o : nullptr, &tr);
  memcpy(out, &res, sizeof res);
  if (trace) { trace[0] = tr.max_uv_limb; trace[1] = tr.max_t_limb; trace[2] = tr.flips; }
}

extern "C" {

// ---- Twisted-Edwards BLS12, 9 limbs: record = hm | hp | dt (27 words), accumulator = x | y | z | t (36 words)
void ss_record(const uint8_t xy_le[64], uint32_t out[27]) {
  uint32_t xw[8], yw[8];
  memcpy(xw, xy_le, 32); memcpy(yw, xy_le + 32, 32);
  const pnt r = pnt_from_affine_raw(fp_from_words32(xw), fp_from_words32(yw));
  memcpy(out, &r, 108);
}
// at most 64 entries; onto may be null; trace: 3 words or null
void ss_segment(const uint32_t* recs, const int* neg, uint32_t cnt, const uint32_t* onto, uint32_t out[36], uint32_t* trace) {
  run_segment<9, pnt>(recs, neg, cnt, onto, out, trace);
}
// the reference for the same entries: every record negated by pnt_cneg and added with ete_madd, as the kernel did before
void ss_segment_cneg(const uint32_t* recs, const int* neg, uint32_t cnt, const uint32_t* onto, uint32_t out[36]) {
  ete acc = ete_identity();
  if (onto) memcpy(&acc, onto, sizeof acc);
  for (uint32_t i = 0; i < cnt; i++) { pnt r; memcpy(&r, recs + 27u * i, 108); acc = ete_madd(acc, pnt_cneg(r, neg[i] != 0)); }
  memcpy(out, &acc, sizeof acc);
}
// the opened form u | v | z | t of an accumulator, negated `times` times
void ss_open_neg(const uint32_t acc[36], int times, uint32_t out[36]) {
  ete a; memcpy(&a, acc, sizeof a);
  ete_uv_t<9> uv = ete_open<9>(a);
  for (int i = 0; i < times; i++) ete_uv_neg<9>(uv);
  memcpy(out, &uv, sizeof uv);
}

// ---- BLS12-377 G1, 14 limbs: projective record hm | hp | dt | z (56 words), affine record hm | hp | dt (42 words),
// accumulator x | y | z | t (56 words)
int ss377_overflow_and_reset() { const int v = g_fq377_overflow; g_fq377_overflow = 0; return v; }
// [R, 2d R, s R^2, f R]: what maps the Edwards form back to y^2 = x^3 + 1
void ss377_constants(uint32_t out[4 * 14]) {
  using namespace te377;
  const fq c[4] = {fq_R1(), fq_K2D_MONT(), fq_S_R2(), fq_F_MONT()};
  memcpy(out, c, sizeof c);
}
void ss377_record(const uint8_t xy_le[96], uint32_t out[56]) {
  uint32_t xw[12], yw[12]; memcpy(xw, xy_le, 48); memcpy(yw, xy_le + 48, 48);
  const pnt_t<14> r = pnt_from_sw377(te377::fq_from_words32(xw), te377::fq_from_words32(yw));
  memcpy(out, &r, 224);
}
void ss377_segment(const uint32_t* recs, const int* neg, uint32_t cnt, const uint32_t* onto, uint32_t out[56], uint32_t* trace) {
  run_segment<14, pnt_t<14>>(recs, neg, cnt, onto, out, trace);
}
void ss377_segment_aff(const uint32_t* recs, const int* neg, uint32_t cnt, const uint32_t* onto, uint32_t out[56], uint32_t* trace) {
  run_segment<14, pnt_aff377>(recs, neg, cnt, onto, out, trace);
}
void ss377_open_neg(const uint32_t acc[56], int times, uint32_t out[56]) {
  ete_t<14> a; memcpy(&a, acc, sizeof a);
  ete_uv_t<14> uv = ete_open<14>(a);
  for (int i = 0; i < times; i++) ete_uv_neg<14>(uv);
  memcpy(out, &uv, sizeof uv);
}

}  // extern "C"
