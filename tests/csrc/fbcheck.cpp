// fbcheck.cpp -- TEST SHIM: the fixed-base windows' host-side arithmetic (csrc/fb_plan.hpp: plan geometry and digit walk; csrc/host_tail.hpp:
// fixed_base_with / fixed_base_to_affine), compiled for the host so tests/test_fixed_base_host.py can compare it with the bigint model
// oracle/fixed_base.py.  k_fb_digits (csrc/kernels.hip.hpp) extracts every digit twice, in its phases A and B, in text of its own: both
// extractions, the sum s = scalar + half in front of them and the two stores behind them are RESTATED below line for line, with the
// kernel's lines quoted -- whoever edits those lines of the kernel edits them here.  Not part of the product; not a fallback.
//
// fbc_set_variant(v != 0) switches ONE deliberate mistake into the shim (never into the product): the host test runs its checks under
// every variant and requires each to be caught.
#include <stdint.h>
#include <string.h>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/fb_plan.hpp"
#include "../../webgpu-msm-twisted-edwards_amd/csrc/host_tail.hpp"

enum {
  V_NONE = 0,
  V_NO_EXTRA_ROW = 1,     // the top window's hb = 0 entries stay in row 0
  V_SIGN_LOST = 2,        // neg is never set
  V_CODE_LO = 3,          // code lo instead of lo + 1
  V_HALF_NO_TOP = 4,      // half lacks the top window's bit
  V_U_DOWN_TO_2 = 5,      // the tail's U = sum r T_r stops at r = 2
  V_CAP_UNROUNDED = 6,    // cap is not rounded to a multiple of 8
};
static int g_variant = V_NONE;

static te_fb::geometry geometry_of(uint64_t n, int c) {
  te_fb::geometry g = te_fb::make_geometry(n, c);
  if (g_variant == V_HALF_NO_TOP) { const int bit = (g.W - 1) * c + c - 1; g.half[bit >> 5] &= ~(1u << (bit & 31)); }
  if (g_variant == V_CAP_UNROUNDED) { const uint64_t big = g.reg > n ? g.reg : n; g.cap = big + big / 16 + 4096 + 1; }
  return g;
}

// fixed_base_with<ScalarAcc> with the mistake V_U_DOWN_TO_2 (host_tail.hpp: "for (int r = rb - 1; r >= 1; r--)")
static void tail_u_down_to_2(const uint8_t* partials, int rows, int rb, int bucket_bits, uint8_t out[64]) {
  using namespace te_host;
  int dw[4];
  for (int k = 0; k < 4; k++) dw[k] = (bucket_bits + 3 - k) / 4;
  const Fe k2d = tail_k2d();
  auto row_of = [&](int r) { return partials + (size_t)r * TE_TAIL_ROW_BYTES; };
  auto present = [&](int r) { return !all_zero_bytes(row_of(r), TE_TAIL_ROW_BYTES); };
  Pt S = identity(), U = identity();
  for (int r = rb - 1; r >= 2; r--) {
    if (present(r)) S = padd(S, load_point(row_of(r)), k2d);
    U = padd(U, S, k2d);
  }
  ScalarAcc acc;
  acc.add_point(U);
  auto slot_sum = [&](int slot) { for (int r = 0; r < rows; r++) if (present(r)) acc.add_point(load_point(row_of(r) + (size_t)slot * TE_TAIL_POINT_BYTES)); };
  acc.dbl_n(dw[3]); slot_sum(4);
  acc.dbl_n(dw[2]); slot_sum(3);
  acc.dbl_n(dw[1]); slot_sum(2);
  acc.dbl_n(dw[0]); slot_sum(1);
  slot_sum(0);
  acc.to_affine(out);
}

// ---- k_fb_digits restated (one live thread, scalar i of the launch)
static const uint32_t K_LOBITS = 15u;                      // "#define TE_FB_LOBITS 15u"
// "uint64_t c = 0; for (int j = 0; j < 10; j++) { c += (uint64_t)raw[j] + a.half[j]; s[j] = (uint32_t)c; c >>= 32; }"
static void kernel_sum(const uint32_t raw[10], const uint32_t half[10], uint32_t s[10]) {
  uint64_t c = 0;
  for (int j = 0; j < 10; j++) { c += (uint64_t)raw[j] + half[j]; s[j] = (uint32_t)c; c >>= 32; }
}
// phase A, the body of "for (int w = 0; w < WMAX; w++)": DIGIT_CARRY where the kernel sets `bad`, DIGIT_ENTRY with the row whose counter
// it bumps ("rank[w] = atomicAdd(&cnt[row], 1u);"), DIGIT_NONE where it continues
static int kernel_phase_a(int C, const uint32_t s[10], int w, uint32_t aW, uint32_t arb, uint32_t& row_out) {
  const int bit = w * C;
  if (bit >= 320) return te_fb::DIGIT_NONE;                                    // "if (bit >= 320) continue;"
  const int word = bit >> 5, off = bit & 31;                                   // "const int word = bit >> 5, off = bit & 31;"
  uint32_t v = s[word] >> off;                                                 // "uint32_t v = s[word] >> off;"
  if (off + C > 32 && word + 1 < 10) v |= s[word + 1] << (32 - off);           // "if (off + C > 32 && word + 1 < 10) v |= s[word + 1] << (32 - off);"
  v &= (1u << C) - 1u;                                                         // "v &= (1u << C) - 1u;"
  if ((uint32_t)w >= aW) return v != 0u ? te_fb::DIGIT_CARRY : te_fb::DIGIT_NONE;   // "if ((uint32_t)w >= a.W) { bad |= live && v != 0u; continue; }"
  const int d = (int)v - (1 << (C - 1));                                       // "const int d = (int)v - (1 << (C - 1));"
  if (d == 0) return te_fb::DIGIT_NONE;                                        // "if (!live || d == 0) continue;"
  const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u, hb = b >> K_LOBITS;      // "const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u, hb = b >> TE_FB_LOBITS;"
  row_out = ((uint32_t)w + 1u == aW && hb == 0u) ? arb : hb;                   // "const uint32_t row = ((uint32_t)w + 1u == a.W && hb == 0u) ? a.rb : hb;"
  return te_fb::DIGIT_ENTRY;
}
// phase B, for a window phase A ranked: the row it writes to, the code and the sign of the remap word
// ("if (rank[w] == 0xffffffffu) continue;" stands in front of it: phase B runs for exactly the windows phase A gave a rank)
static void kernel_phase_b(int C, const uint32_t s[10], int w, uint32_t aW, uint32_t arb, uint32_t& row_out, uint32_t& lo_out, bool& neg_out) {
  const int bit = w * C, word = bit >> 5, off = bit & 31;                      // "const int bit = w * C, word = bit >> 5, off = bit & 31;"
  uint32_t v = s[word] >> off;                                                 // "uint32_t v = s[word] >> off;"
  if (off + C > 32 && word + 1 < 10) v |= s[word + 1] << (32 - off);           // "if (off + C > 32 && word + 1 < 10) v |= s[word + 1] << (32 - off);"
  v &= (1u << C) - 1u;                                                         // "v &= (1u << C) - 1u;"
  const int d = (int)v - (1 << (C - 1));                                       // "const int d = (int)v - (1 << (C - 1));"
  // "const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u, hb = b >> TE_FB_LOBITS, lo = b & ((1u << TE_FB_LOBITS) - 1u);"
  const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u, hb = b >> K_LOBITS, lo = b & ((1u << K_LOBITS) - 1u);
  row_out = ((uint32_t)w + 1u == aW && hb == 0u) ? arb : hb;                   // "const uint32_t row = ((uint32_t)w + 1u == a.W && hb == 0u) ? a.rb : hb;"
  lo_out = lo; neg_out = d < 0;                                                // "(d < 0 ? 0x80000000u : 0u)"
}

extern "C" {

void fbc_set_variant(int v) { g_variant = v; }

// out: W rb rows reg cap chunks chunk_len CH S P logS seg_len | half[10] | lds_bytes | bind refused | MSM refused | 0
void fbc_geometry(uint64_t n, int c, uint64_t n_table, uint64_t out[26]) {
  const te_fb::geometry g = geometry_of(n, c);
  const uint64_t v[12] = {(uint64_t)g.W, g.rb, g.rows, g.reg, g.cap, g.chunks, g.chunk_len, g.CH, g.S, g.P, g.logS, g.seg_len};
  memcpy(out, v, sizeof v);
  for (int j = 0; j < 10; j++) out[12 + j] = g.half[j];
  out[22] = g.lds_bytes;
  out[23] = te_fb::bind_refused(c, n_table) ? 1 : 0;
  out[24] = te_fb::msm_refused(g, n_table) ? 1 : 0;
  out[25] = 0;
}

// the walk of `count` 32-byte little-endian scalars, scalar i of the launch being thread i: for every window w < windows (the kernel's
// WMAX = (255 + c) / c + 1, at most 18) six words  kind | row | row again | lo | code | remap word.
// from_kernel = 0: te_fb::add_half and te_fb::digit (row twice the same); 1: the kernel's text restated above -- kind and row from phase A,
// row again, lo and the sign from phase B.  Code and remap word are what k_fb_digits stores:
//   "a.digits[(size_t)row * a.cap + pos] = (uint16_t)(lo + 1u);"
//   "a.remap[(size_t)row * a.cap + pos] = ((uint32_t)w * a.n_table + a.idx_base + i) | (d < 0 ? 0x80000000u : 0u);"
// returns the windows per scalar
int fbc_walk(int from_kernel, int c, const uint8_t* scalars_le, uint32_t count, uint32_t n_table, uint32_t idx_base, uint32_t* out) {
  const te_fb::geometry g = geometry_of(count, c);
  const int wmax = (255 + c) / c + 1;
  for (uint32_t i = 0; i < count; i++) {
    uint32_t raw[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, s[10];
    memcpy(raw, scalars_le + 32u * (size_t)i, 32);
    if (from_kernel) kernel_sum(raw, g.half, s); else te_fb::add_half(raw, g.half, s);
    for (int w = 0; w < wmax; w++) {
      te_fb::entry e = {0u, 0u, false};
      uint32_t row_b = 0u;
      int kind;
      if (from_kernel) {
        kind = kernel_phase_a(c, s, w, (uint32_t)g.W, g.rb, e.row);
        if (kind == te_fb::DIGIT_ENTRY) kernel_phase_b(c, s, w, (uint32_t)g.W, g.rb, row_b, e.lo, e.neg);
      } else {
        kind = te_fb::digit_c(c, s, w, (uint32_t)g.W, g.rb, e);
        row_b = e.row;
      }
      if (kind == te_fb::DIGIT_ENTRY) {
        if (g_variant == V_NO_EXTRA_ROW && e.row == g.rb) e.row = row_b = 0u;
        if (g_variant == V_SIGN_LOST) e.neg = false;
      }
      uint32_t* o = out + ((size_t)i * (size_t)wmax + (size_t)w) * 6u;
      o[0] = (uint32_t)kind; o[1] = e.row; o[2] = row_b; o[3] = e.lo;
      o[4] = (uint16_t)(e.lo + (g_variant == V_CODE_LO ? 0u : 1u));
      o[5] = ((uint32_t)w * n_table + idx_base + i) | (e.neg ? 0x80000000u : 0u);
    }
  }
  return wmax;
}

int fbc_have_ifma() {
#if defined(__x86_64__)
  return te_host::have_ifma() ? 1 : 0;
#else
  return 0;
#endif
}

// the host tail of `rows` rows of 720 bytes; form 0: fixed_base_with<ScalarAcc>, 1: fixed_base_with<IfmaAcc> (-1 without IFMA),
// 2: fixed_base_to_affine (the engine's choice)
int fbc_tail(int form, const uint8_t* partials, int rows, int rb, int bucket_bits, uint8_t out[64]) {
  if (g_variant == V_U_DOWN_TO_2) { tail_u_down_to_2(partials, rows, rb, bucket_bits, out); return 0; }
  if (form == 0) { te_host::fixed_base_with<te_host::ScalarAcc>(partials, rows, rb, bucket_bits, out); return 0; }
  if (form == 1) {
#if defined(__x86_64__)
    if (te_host::have_ifma()) { te_host::fixed_base_with<te_host::IfmaAcc>(partials, rows, rb, bucket_bits, out); return 0; }
#endif
    return -1;
  }
  te_host::fixed_base_to_affine(partials, rows, rb, bucket_bits, out);
  return 0;
}

}  // extern "C"
