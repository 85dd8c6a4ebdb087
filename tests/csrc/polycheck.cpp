// polycheck.cpp -- TEST SHIM: compiles the product's polynomial opening (csrc/poly.hip.hpp, csrc/poly_plan.hpp) for the host, so that the
// exact per-lane code of k_poly_sums and k_poly_apply runs on the CPU box (tests/test_poly_host.py, tests/csrc/san_poly.cpp).  Not part
// of the product; not a fallback.  Expected values come from tests/poly_cases.py (Python integers), never from here.  It holds
//   poly_emulate  te_msm_poly_divide's steps: the same argument check, plan and power table as points.hip, then every launch of the plan,
//                 a block as plain loops over its 256 lanes -- one loop per phase, a loop boundary being the block's barrier.  Every
//                 global, scratch and LDS index is checked against what the plan says is allocated (-100 on a violation).
//   poly_replay   the indices alone, no arithmetic and no allocation: every tile's first and last record, its sum and its carry inside
//                 their allocations, every LDS word of a tile inside the block's and owned once.
// `mistake` (0 in every real check) turns the emulation into a deliberately wrong variant, which the tests must catch:
//   1 the carry of tile b where b + 1 belongs           2 z^(T - 1) for z^T as the next level's point
//   3 a partly filled last tile run as a full one       4 the quotient not shifted by one (h_i written at i)
//   5 q[n - 1] left unwritten
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/poly.hip.hpp"

using namespace te;

namespace {
enum { M_CARRY = 1, M_POINT = 2, M_FULL_TILE = 3, M_UNSHIFTED = 4, M_LAST = 5 };
constexpr int E_BOUNDS = -100;

void rd(const uint8_t* p, uint64_t i, uint32_t (&w)[8]) { memcpy(w, p + i * 32, 32); }
void wr(uint8_t* p, uint64_t i, const uint32_t (&w)[8]) { memcpy(p + i * 32, w, 32); }

struct buffer { const uint8_t* rd; uint8_t* wr; uint64_t records; };
struct launch {
  te_poly::level v; uint32_t chunk; uint64_t count;
  const uint32_t* pw; uint64_t pow_stride, pow_words_left;          // the level's entries of polynomial 0, and the words from there to the table's end
  int mistake; bool level0;
};
bool pows_ok(const launch& L, uint64_t poly) { return poly * L.pow_stride + (uint64_t)te_poly::kPowEntries * te_poly::kPowWords <= L.pow_words_left; }
// the tile as the block sees it; M_FULL_TILE: a partly filled tile claims all T
te_poly::tile tile_for(const launch& L, uint64_t block) {
  te_poly::tile t = te_poly::tile_of(L.v, te_poly::kLanes * L.chunk, block);
  if (L.mistake == M_FULL_TILE && L.level0) t.fill = te_poly::kLanes * L.chunk;
  return t;
}
// a load of the emulation: M_FULL_TILE reads what lies behind the polynomial, and a 1 behind the buffer
bool load(const launch& L, const buffer& src, uint64_t at, uint32_t (&w)[8]) {
  if (at >= src.records) {
    if (L.mistake != M_FULL_TILE) return false;
    memset(w, 0, 32); w[0] = 1u;
    return true;
  }
  rd(src.rd, at, w);
  return true;
}

// one launch of k_poly_sums; false: an index left its allocation
bool sums_launch(const launch& L, const buffer& src, const buffer& dst) {
  std::vector<uint32_t> scan(te_poly::lds_scan_words());
  std::vector<fel<9>> acc(te_poly::kLanes);
  const uint64_t blocks = L.count * L.v.tiles;
  for (uint64_t block = 0; block < blocks; block++) {
    const te_poly::tile t = tile_for(L, block);
    if (!pows_ok(L, t.poly)) return false;
    const uint32_t* pows = L.pw + t.poly * L.pow_stride;
    const fel<9> z256 = poly_pow(pows, te_poly::kPowZ + te_poly::kPowLog);
    for (uint32_t lane = 0; lane < te_poly::kLanes; lane++) {
      acc[lane] = fe_zero<9>();
      for (uint32_t j = L.chunk; j-- > 0u;) {
        const uint32_t x = te_poly::wide_x(lane, j);
        if (x >= t.fill) continue;
        uint32_t w[8];
        if (!load(L, src, t.base + x, w)) return false;
        poly_step(w, z256, acc[lane]);
      }
    }
    for (uint32_t s = 0; s < te_poly::kPowLog; s++) {
      for (uint32_t lane = 0; lane < te_poly::kLanes; lane++) poly_scan_put(scan.data(), lane, acc[lane]);
      for (uint32_t lane = 0; lane < te_poly::kLanes; lane++) {
        if (!poly_tree_takes(lane, s)) continue;
        if (lane + (1u << s) >= te_poly::kLanes) return false;
        acc[lane] = poly_combine(acc[lane], poly_pow(pows, te_poly::kPowZ + s), poly_scan_get(scan.data(), lane + (1u << s)));
      }
    }
    uint32_t w[8];
    poly_out(acc[0], w);
    const uint64_t at = t.poly * L.v.tiles + t.b;
    if (at >= dst.records) return false;
    wr(dst.wr, at, w);
  }
  return true;
}

// one launch of k_poly_apply (carries.rd == nullptr: the last level)
bool apply_launch(const launch& L, const buffer& src, const buffer& dst, const buffer& carries) {
  const uint32_t chunk = L.chunk, data_words = te_poly::lds_data_words(chunk);
  std::vector<uint32_t> lds(data_words + te_poly::lds_scan_words());
  uint32_t* const scan = lds.data() + data_words;
  std::vector<fel<9>> acc(te_poly::kLanes), h(te_poly::kLanes);
  const uint64_t blocks = L.count * L.v.tiles;
  for (uint64_t block = 0; block < blocks; block++) {
    const te_poly::tile t = tile_for(L, block);
    if (!pows_ok(L, t.poly)) return false;
    const uint32_t* pows = L.pw + t.poly * L.pow_stride;
    uint32_t cw[8] = {};
    for (uint32_t lane = 0; lane < te_poly::kLanes; lane++) {
      for (uint32_t j = 0; j < chunk; j++) {
        const uint32_t x = te_poly::wide_x(lane, j);
        uint32_t w[8] = {};
        if (x < t.fill && !load(L, src, t.base + x, w)) return false;
        if (te_poly::lds_word(x, chunk) + 8u > data_words) return false;
        poly_lds_put(lds.data(), te_poly::lds_word(x, chunk), w);
      }
      if (carries.rd && lane == te_poly::kLanes - 1u) {
        uint64_t at = t.poly * L.v.tiles + t.b;
        if (L.mistake == M_CARRY && L.level0) at = t.poly * L.v.tiles + (t.b + 1u) % L.v.tiles;
        if (at >= carries.records) return false;
        rd(carries.rd, at, cw);
      }
    }
    const fel<9> z1 = poly_pow(pows, te_poly::kPowZ);
    for (uint32_t lane = 0; lane < te_poly::kLanes; lane++) {
      acc[lane] = fe_zero<9>();
      for (uint32_t j = chunk; j-- > 0u;) {
        const uint32_t at = te_poly::lds_word(te_poly::own_x(lane, j, chunk), chunk);
        if (at + 8u > data_words) return false;
        uint32_t w[8];
        poly_lds_get(lds.data(), at, w);
        poly_step(w, z1, acc[lane]);
      }
      if (lane == te_poly::kLanes - 1u) acc[lane] = poly_combine(acc[lane], poly_pow(pows, te_poly::kPowC), fp_from_words32(cw));
    }
    for (uint32_t s = 0; s < te_poly::kPowLog; s++) {
      for (uint32_t lane = 0; lane < te_poly::kLanes; lane++) poly_scan_put(scan, lane, acc[lane]);
      for (uint32_t lane = 0; lane < te_poly::kLanes; lane++)
        if (poly_scan_takes(lane, s)) acc[lane] = poly_combine(acc[lane], poly_pow(pows, te_poly::kPowC + s), poly_scan_get(scan, lane + (1u << s)));
    }
    for (uint32_t lane = 0; lane < te_poly::kLanes; lane++) poly_scan_put(scan, lane, acc[lane]);
    for (uint32_t lane = 0; lane < te_poly::kLanes; lane++) {
      h[lane] = lane == te_poly::kLanes - 1u ? fp_from_words32(cw) : poly_scan_get(scan, lane + 1u);
      for (uint32_t j = chunk; j-- > 0u;) {
        const uint32_t at = te_poly::lds_word(te_poly::own_x(lane, j, chunk), chunk);
        uint32_t w[8], o[8];
        poly_lds_get(lds.data(), at, w);
        if (L.mistake == M_UNSHIFTED && L.level0) { poly_step(w, z1, h[lane]); poly_out(h[lane], o); poly_lds_put(lds.data(), at, o); continue; }
        poly_out(h[lane], o);
        poly_lds_put(lds.data(), at, o);
        poly_step(w, z1, h[lane]);
      }
    }
    for (uint32_t lane = 0; lane < te_poly::kLanes; lane++)
      for (uint32_t j = 0; j < chunk; j++) {
        const uint32_t x = te_poly::wide_x(lane, j);
        if (x >= t.fill) continue;
        if (t.base + x >= dst.records) { if (L.mistake == M_FULL_TILE) continue; return false; }
        if (L.mistake == M_LAST && L.level0 && t.b * te_poly::kLanes * chunk + x == L.v.n - 1u) continue;
        uint32_t w[8];
        poly_lds_get(lds.data(), te_poly::lds_word(x, chunk), w);
        wr(dst.wr, t.base + x, w);
      }
  }
  return true;
}
}  // namespace

extern "C" {

// te_msm_poly_divide's steps with the product's block code: 0, -1 (refused, outputs untouched; *reason = why: poly.hip.hpp's POLY_*), -100
// (an index left its allocation).  q may be a; evals or q may be NULL.  chunk: 0 for the default
int poly_emulate(const uint8_t* a, uint64_t n, uint64_t count, const uint8_t* z, int flags, uint32_t chunk, int mistake, uint8_t* evals, uint8_t* q, int* reason) {
  poly_req r;
  const int why = poly_check(a, n, count, z, flags, evals, q, r);
  if (reason) *reason = why;
  if (why != POLY_OK) return -1;
  if (count == 0) return 0;
  r.chunk = te_poly::chunk_for(n, te_poly::clamp_chunk((long)chunk));
  te_poly::plan P;
  if (!te_poly::make_plan(n, count, r.chunk, r.shared, P)) { if (reason) *reason = POLY_TOO_LARGE; return -1; }
  std::vector<uint32_t> pows((size_t)P.pow_words);
  poly_pow_table(P, z, r.mont, pows.data());
  if (mistake == M_POINT && P.levels > 1u) {                         // levels >= 1 built from z^(T - 1)
    for (uint32_t k = 0; k < P.points; k++) {
      fel<9> z0 = poly_pow(&pows[te_poly::pow_word(P, k, 0, 0)], 0), zr = fe_one<9>();
      for (uint32_t i = 0; i + 1u < P.T; i++) zr = fe_mul(zr, z0);
      for (uint32_t l = 1; l < P.levels; l++) {
        fel<9> e[te_poly::kPowEntries];
        poly_level_pows(zr, P.chunk, e);
        for (uint32_t i = 0; i < te_poly::kPowEntries; i++) for (uint32_t j = 0; j < 9u; j++) pows[te_poly::pow_word(P, k, l, i) + j] = e[i].v[j];
        zr = e[te_poly::kPowC + te_poly::kPowLog];
      }
    }
  }
  std::vector<uint8_t> reg((size_t)P.records * 32);
  const uint64_t pow_stride = P.points == 1u ? 0 : te_poly::pow_word(P, 1, 0, 0);
  auto region = [&](uint64_t off, uint64_t records) { return buffer{reg.data() + off * 32, reg.data() + off * 32, records}; };
  auto launch_of = [&](uint32_t l) {
    launch L;
    L.v = P.lv[l]; L.chunk = P.chunk; L.count = count; L.pw = pows.data() + te_poly::pow_word(P, 0, l, 0); L.pow_stride = pow_stride;
    L.pow_words_left = P.pow_words - te_poly::pow_word(P, 0, l, 0); L.mistake = mistake; L.level0 = l == 0u;
    return L;
  };
  for (uint32_t l = 0; l < P.levels; l++) {
    const te_poly::level& v = P.lv[l];
    if (v.dst + count * v.tiles > P.records) return E_BOUNDS;
    const buffer src = l ? region(v.src, count * v.n) : buffer{a, nullptr, count * n};
    if (!sums_launch(launch_of(l), src, region(v.dst, count * v.tiles))) return E_BOUNDS;
  }
  std::vector<uint8_t> ev((size_t)count * 32);
  memcpy(ev.data(), reg.data() + P.lv[P.levels - 1].dst * 32, ev.size());
  if (q) {
    for (uint32_t l = P.levels; l-- > 0u;) {
      const te_poly::level& v = P.lv[l];
      const buffer src = l ? region(v.src, count * v.n) : buffer{a, nullptr, count * n};
      const buffer dst = l ? region(v.src, count * v.n) : buffer{nullptr, q, count * n};
      const buffer carries = l + 1u < P.levels ? region(v.dst, count * v.tiles) : buffer{nullptr, nullptr, 0};
      if (!apply_launch(launch_of(l), src, dst, carries)) return E_BOUNDS;
    }
  }
  if (evals) memcpy(evals, ev.data(), ev.size());
  return 0;
}

// every index of the plan for `count` polynomials of n at `chunk`, by arithmetic alone: 0 with *checked = how many, or -100
int poly_replay(uint64_t n, uint64_t count, uint32_t chunk, int shared, uint64_t* checked) {
  te_poly::plan P;
  *checked = 0;
  if (!te_poly::make_plan(n, count, chunk, shared != 0, P)) return E_BOUNDS;
  if (P.levels < 1u || P.levels > te_poly::kMaxLevels || P.lv[P.levels - 1].tiles != 1u || P.lv[0].n != n) return E_BOUNDS;
  const uint32_t data_words = te_poly::lds_data_words(chunk);
  if (te_poly::lds_bytes_apply(chunk) > 160u * 1024u) return E_BOUNDS;
  std::vector<uint8_t> hit(data_words, 0);
  for (uint32_t lane = 0; lane < te_poly::kLanes; lane++)
    for (uint32_t j = 0; j < chunk; j++) {
      const uint32_t wx = te_poly::wide_x(lane, j), ox = te_poly::own_x(lane, j, chunk);
      if (wx >= P.T || ox >= P.T || te_poly::lds_word(wx, chunk) + 8u > data_words) return E_BOUNDS;
      const uint32_t at = te_poly::lds_word(ox, chunk);
      for (uint32_t k = 0; k < 8u; k++) { if (at + k >= data_words || hit[at + k]) return E_BOUNDS; hit[at + k] = 1; }
      *checked += 2;
    }
  uint64_t end = 0;
  for (uint32_t l = 0; l < P.levels; l++) {
    const te_poly::level& v = P.lv[l];
    if (l && (v.n != P.lv[l - 1].tiles || v.src != P.lv[l - 1].dst)) return E_BOUNDS;
    if (v.tiles != (v.n + P.T - 1) / P.T || v.dst != end || count * v.tiles >> 31) return E_BOUNDS;
    end = v.dst + count * v.tiles;
    if (end > P.records) return E_BOUNDS;
    const uint64_t src_records = count * v.n, blocks = count * v.tiles;
    uint64_t next = 0;                                               // the tiles cover the level's records in order, once
    for (uint64_t block = 0; block < blocks; block++) {
      const te_poly::tile t = te_poly::tile_of(v, P.T, block);
      if (t.poly >= count || t.b >= v.tiles || t.fill < 1u || t.fill > P.T || t.base != next || t.base + t.fill > src_records) return E_BOUNDS;
      if (t.b * P.T + t.fill > v.n) return E_BOUNDS;                 // a tile stays inside its polynomial
      next = t.base + t.fill;
      const uint64_t s = te_poly::sum_of(v, t);
      if (s < v.dst || s >= end || s - v.dst != block) return E_BOUNDS;
      if (te_poly::pow_word(P, t.poly, l, te_poly::kPowEntries - 1u) + te_poly::kPowWords > P.pow_words) return E_BOUNDS;
      *checked += 4;
    }
    if (next != src_records) return E_BOUNDS;
  }
  if (end != P.records || P.scratch_bytes != P.records * 32 + P.pow_words * 4) return E_BOUNDS;
  return 0;
}

// the chunk a call of polynomials of n coefficients runs at when `chunk` is in force
uint32_t poly_chunk_for(uint64_t n, uint32_t chunk) { return te_poly::chunk_for(n, chunk); }

// the plan as numbers: out[0] levels, [1] T, [2] records of scratch, [3] scratch bytes, [4] LDS bytes of the apply kernel, [5] the default
// chunk, [6] the largest chunk, then n and tiles of each level (0 when make_plan refuses: out[0] = 0)
void poly_plan_info(uint64_t n, uint64_t count, uint32_t chunk, int shared, uint64_t* out) {
  te_poly::plan P;
  memset(out, 0, 16 * sizeof(uint64_t));
  out[5] = te_poly::kChunkDefault; out[6] = te_poly::kChunkMax;
  if (!te_poly::make_plan(n, count, chunk, shared != 0, P)) return;
  out[0] = P.levels; out[1] = P.T; out[2] = P.records; out[3] = P.scratch_bytes; out[4] = te_poly::lds_bytes_apply(chunk);
  for (uint32_t l = 0; l < P.levels; l++) { out[7 + 2 * l] = P.lv[l].n; out[8 + 2 * l] = P.lv[l].tiles; }
}

}
