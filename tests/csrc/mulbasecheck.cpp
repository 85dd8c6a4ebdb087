// mulbasecheck.cpp -- TEST SHIM: compiles the product's fixed-base batch scalar multiplication (csrc/mul_base.hip.hpp) for the host, so
// that the exact per-lane code of k_mul_base and k_mul_base_entries, and the host-side table scalars, are compared with the bigint models
// on the CPU box (tests/test_mul_base_host.py).  The table is read through an accessor that checks index < entries and counts every
// violation (mbc_out_of_table).  Not part of the product; not a fallback.
//
// mbc_set_variant(v != 0) switches ONE deliberate mistake into the shim (never into the product): the host test requires each to be
// caught.  The two other mistakes the test plants -- table scalars that are not reduced, the C of another W -- come in through the
// arguments (mbc_table_from_scalars takes the scalars, mbc_mul the words of C).
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/mul_base.hip.hpp"

using namespace te;

namespace {
enum {
  V_NONE = 0,
  V_ENTRY_OFF_BY_ONE = 1,   // the accessor reads entry index + 1
  V_SIGN_DROPPED = 2,       // the window's addition never subtracts
};
int g_variant = V_NONE;
uint64_t g_out_of_table = 0;

struct host_table {
  const uint32_t* t; uint32_t entries;
  void load(uint32_t index, uint32_t (&w)[MB_ENTRY_WORDS]) const {
    if (g_variant == V_ENTRY_OFF_BY_ONE) index = (index + 1u) % entries;
    if (index >= entries) { g_out_of_table++; index = 0; }                  // (the assertion: counted, the test requires 0)
    memcpy(w, t + (size_t)index * MB_SLOT_WORDS, MB_ENTRY_WORDS * 4);
  }
};

// mb_lane with the mistake V_SIGN_DROPPED: its window loop restated (mul_base.hip.hpp: "acc = mb_step_te(acc, w, neg);" /
// "acc = mb_step_377(acc, w, mag, neg);") with neg replaced by false
template <int CURVE> void lane_sign_dropped(uint32_t (&k)[8], const mb_geom& g, const host_table& tab, uint32_t* proj) {
  constexpr int N = sm_sizes<CURVE>::N;
  uint32_t K[9];
  mb_recode(k, g.C, K);
  fel<N> X, Y, Z;
  if constexpr (CURVE == 1) {
    sw377 acc = sw377_identity();
    for (int i = 0; i < g.M; i++) {
      bool neg;
      const uint32_t mag = mb_next_digit(K, g.W, g.H, neg);
      uint32_t w[MB_ENTRY_WORDS];
      tab.load(mb_index(g, i, mag), w);
      acc = mb_step_377(acc, w, mag, false);
    }
    X = acc.x; Y = acc.y; Z = acc.z;
  } else {
    ete acc = ete_identity();
    for (int i = 0; i < g.M; i++) {
      bool neg;
      const uint32_t mag = mb_next_digit(K, g.W, g.H, neg);
      uint32_t w[MB_ENTRY_WORDS];
      tab.load(mb_index(g, i, mag), w);
      acc = mb_step_te(acc, w, false);
    }
    X = acc.x; Y = acc.y; Z = acc.z;
  }
  for (int i = 0; i < N; i++) { proj[i] = X.v[i]; proj[N + i] = Y.v[i]; proj[2 * N + i] = Z.v[i]; }
}

template <int CURVE> void affine_pass(const std::vector<uint32_t>& proj, uint64_t n, uint8_t* out) {
  using Z = sm_sizes<CURVE>;
  std::vector<uint32_t> res((size_t)n * Z::PW);
  for (uint64_t lo = 0; lo < n; lo += SM_AFF_GROUP)
    sm_affine_group<CURVE>(&proj[lo * Z::JW], (uint32_t)std::min<uint64_t>(SM_AFF_GROUP, n - lo), &res[lo * Z::PW], CURVE == 1 ? kInvExp377 : kInvExpTe);
  memcpy(out, res.data(), (size_t)n * Z::PW * 4);
}

// the table as the engine builds it: k_scalar_mul over the point and the given scalars, k_scalar_mul_affine, k_mul_base_entries
template <int CURVE> void table_from_scalars(const uint8_t* point, const uint8_t* scalars32, uint32_t entries, uint8_t* out) {
  using Z = sm_sizes<CURVE>;
  std::vector<uint32_t> proj((size_t)entries * Z::JW);
  std::vector<uint8_t> aff((size_t)entries * Z::PW * 4);
  const naf_t kn = {};
  for (uint32_t e = 0; e < entries; e++) {
    uint32_t w[Z::PW], k[8];
    memcpy(w, point, Z::PW * 4);
    memcpy(k, scalars32 + (size_t)e * 32, 32);
    sm_point<CURVE, false>(w, k, kn, &proj[(size_t)e * Z::JW]);
  }
  affine_pass<CURVE>(proj, entries, aff.data());
  for (uint32_t e = 0; e < entries; e++) {
    uint32_t w[Z::PW], slot[MB_SLOT_WORDS];
    memcpy(w, &aff[(size_t)e * Z::PW * 4], Z::PW * 4);
    mb_entry<CURVE>(w, slot);
    memcpy(out + (size_t)e * MB_SLOT_WORDS * 4, slot, MB_SLOT_WORDS * 4);
  }
}

// The same table WITHOUT the scalar multiplications, for the wide windows the host test could not wait for: window i's base 2^(W i) P by
// doublings, its entries by repeated addition, then the same affine pass and mb_entry.  An entry is a function of its canonical affine
// point alone, so both routes give the same bytes (the host test compares them at W = 4 and 8).
template <int CURVE> void table_by_addition(const mb_geom& g, const uint8_t* point, uint8_t* out) {
  using Z = sm_sizes<CURVE>;
  constexpr int N = Z::N;
  std::vector<uint32_t> proj((size_t)g.entries * Z::JW);
  std::vector<uint8_t> aff((size_t)g.entries * Z::PW * 4);
  uint32_t w[Z::PW];
  memcpy(w, point, Z::PW * 4);
  auto put = [&](uint32_t e, const fel<N>& X, const fel<N>& Y, const fel<N>& Zc) {
    uint32_t* p = &proj[(size_t)e * Z::JW];
    for (int i = 0; i < N; i++) { p[i] = X.v[i]; p[N + i] = Y.v[i]; p[2 * N + i] = Zc.v[i]; }
  };
  if constexpr (CURVE == 1) {
    te377::fq X, Y, sx;
    c377_coords(w, X, Y, sx);
    sw377 base = sw377_of(X, Y);
    for (int i = 0; i < g.M; i++) {
      sw377 cur = sw377_identity();
      for (uint32_t j = 0; j <= g.H; j++) { put(mb_index(g, i, j), cur.x, cur.y, cur.z); cur = sw377_add(cur, base); }
      for (int s = 0; s < g.W; s++) base = sw377_dbl(base);
    }
  } else {
    fp X, Y;
    te_coords(w, X, Y);
    ete base = ete_of(X, Y);
    for (int i = 0; i < g.M; i++) {
      ete cur = ete_identity();
      for (uint32_t j = 0; j <= g.H; j++) { put(mb_index(g, i, j), cur.x, cur.y, cur.z); cur = ete_add<9>(cur, base); }
      for (int s = 0; s < g.W; s++) base = ete_add<9>(base, base);
    }
  }
  affine_pass<CURVE>(proj, g.entries, aff.data());
  for (uint32_t e = 0; e < g.entries; e++) {
    uint32_t a[Z::PW], slot[MB_SLOT_WORDS];
    memcpy(a, &aff[(size_t)e * Z::PW * 4], Z::PW * 4);
    mb_entry<CURVE>(a, slot);
    memcpy(out + (size_t)e * MB_SLOT_WORDS * 4, slot, MB_SLOT_WORDS * 4);
  }
}

template <int CURVE, int FORM> void mul(const mb_geom& g, const host_table& tab, const uint8_t* ks, uint64_t n, uint8_t* out) {
  using Z = sm_sizes<CURVE>;
  constexpr int SB = CURVE == 1 ? 48 : 32;
  std::vector<uint32_t> proj((size_t)n * Z::JW);
  for (uint64_t i = 0; i < n; i++) {
    uint32_t k[8];
    memcpy(k, ks + i * SB, 32);
    if (g_variant == V_SIGN_DROPPED && FORM == SCALAR_FORM_CANONICAL) lane_sign_dropped<CURVE>(k, g, tab, &proj[i * Z::JW]);
    else mb_lane<CURVE, FORM>(k, g, tab, &proj[i * Z::JW]);
  }
  affine_pass<CURVE>(proj, n, out);
}
}  // namespace

extern "C" {

void mbc_set_variant(int v) { g_variant = v; }
uint64_t mbc_out_of_table(void) { return g_out_of_table; }

// M, H, entries and the nine words of C for window bits W
void mbc_geometry(int W, int* M, uint32_t* H, uint32_t* entries, uint32_t* C9) {
  const mb_geom g = mb_geometry(W);
  *M = g.M; *H = g.H; *entries = g.entries;
  memcpy(C9, g.C, 36);
}
// the M signed digits of k (32 bytes) at window bits W, lowest window first
void mbc_digits(int W, const uint8_t* k32, int32_t* digits) {
  const mb_geom g = mb_geometry(W);
  uint32_t k[8], K[9];
  memcpy(k, k32, 32);
  mb_recode(k, g.C, K);
  for (int i = 0; i < g.M; i++) {
    bool neg;
    const uint32_t mag = mb_next_digit(K, g.W, g.H, neg);
    digits[i] = neg ? -(int32_t)mag : (int32_t)mag;
  }
}
// the scalars of the table's entries, 32 bytes each
void mbc_table_scalars(int curve, int W, uint8_t* out) {
  const mb_geom g = mb_geometry(W);
  std::vector<uint32_t> s((size_t)g.entries * 8);
  mb_table_scalars(curve, g, s.data());
  memcpy(out, s.data(), s.size() * 4);
}
// `entries` table slots (128 bytes each) of the point (wire format) from the given scalars (32 bytes each)
void mbc_table_from_scalars(int curve, const uint8_t* point, const uint8_t* scalars32, uint32_t entries, uint8_t* out) {
  if (curve == 1) table_from_scalars<1>(point, scalars32, entries, out);
  else table_from_scalars<0>(point, scalars32, entries, out);
}
// the whole table of window bits W by repeated addition (table_by_addition above)
void mbc_table_by_addition(int curve, int W, const uint8_t* point, uint8_t* out) {
  const mb_geom g = mb_geometry(W);
  if (curve == 1) table_by_addition<1>(g, point, out);
  else table_by_addition<0>(g, point, out);
}
// n scalar records (32 / 48 bytes; form: scalar_form.hpp's) over a table of window bits W -> n affine points.  C9: the words of C the
// lanes are given (NULL: the geometry's own).
void mbc_mul(int curve, int form, int W, const uint8_t* table, const uint32_t* C9, const uint8_t* ks, uint64_t n, uint8_t* out) {
  mb_geom g = mb_geometry(W);
  if (C9) memcpy(g.C, C9, 36);
  const host_table tab = {reinterpret_cast<const uint32_t*>(table), g.entries};
  if (curve == 1) { if (form) mul<1, SCALAR_FORM_377>(g, tab, ks, n, out); else mul<1, SCALAR_FORM_CANONICAL>(g, tab, ks, n, out); }
  else { if (form) mul<0, SCALAR_FORM_TE>(g, tab, ks, n, out); else mul<0, SCALAR_FORM_CANONICAL>(g, tab, ks, n, out); }
}

}
