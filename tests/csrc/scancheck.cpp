// scancheck.cpp -- TEST SHIM: compiles the product's prefix sums and products (csrc/scan.hip.hpp, csrc/scan_plan.hpp) for the host, so that
// the exact per-lane code of k_scan_totals and k_scan_apply runs on the CPU box (tests/test_scan_host.py, tests/csrc/san_scan.cpp).  Not
// part of the product; not a fallback.  Expected values come from tests/scan_cases.py (Python integers), never from here.  It holds
//   scan_emulate  te_msm_field_scan's steps: the same argument check, plan and seeds as points.hip, then every launch of the plan, a block
//                 as plain loops over its 256 lanes -- one loop per phase, a loop boundary being the block's barrier.  Every global,
//                 scratch and LDS index is checked against what the plan says is allocated (-100 on a violation).
//   scan_replay   the indices alone, no arithmetic and no allocation: every tile's first and last record, its total and its carry inside
//                 their allocations, every LDS word of a tile inside the block's and owned once, every out record written exactly once.
//   scan_points   where the plan says the sum path reduces (the interval test replays the bounds from them).
// `mistake` (0 in every real check) turns the emulation into a deliberately wrong variant, which the tests must catch:
//   1 the carry of tile b + 1 where b belongs            2 the exclusive form not shifted
//   3 the seed dropped                                   4 the seed applied at every level
//   5 a partly filled tile of a product padded with 0    6 the sum without the reduction of a lane's total
//   7 a product written in the internal form, not the caller's
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/scan.hip.hpp"

using namespace te;

namespace {
enum { M_CARRY = 1, M_UNSHIFTED = 2, M_NO_SEED = 3, M_SEED_EVERYWHERE = 4, M_ZERO_PAD = 5, M_NO_REDUCE = 6, M_INTERNAL_OUT = 7 };
constexpr int E_BOUNDS = -100;

void rd(const uint8_t* p, uint64_t i, uint32_t (&w)[8]) { memcpy(w, p + i * 32, 32); }
void wr(uint8_t* p, uint64_t i, const uint32_t (&w)[8]) { memcpy(p + i * 32, w, 32); }

struct buffer { const uint8_t* rd; uint8_t* wr; uint64_t records; };
struct launch {
  te_scan::level v; uint32_t chunk; uint64_t count;
  uint32_t form_in, form_out; bool exclusive, shared, level0, last;
  int mistake;
};

// one launch of k_scan_totals (seeds.rd == nullptr: not the last level); false: an index left its allocation
template <int OP> bool totals_launch(const launch& L, const buffer& src, const buffer& dst, const buffer& seeds) {
  std::vector<uint32_t> scan(te_scan::lds_scan_words());
  std::vector<fel<9>> acc(te_scan::kLanes);
  const uint64_t blocks = L.count * L.v.tiles;
  for (uint64_t block = 0; block < blocks; block++) {
    const te_scan::tile t = te_scan::tile_of(L.v, te_scan::kLanes * L.chunk, block);
    for (uint32_t lane = 0; lane < te_scan::kLanes; lane++) {
      acc[lane] = L.mistake == M_ZERO_PAD ? fe_zero<9>() : scan_identity<OP>();      // (a lane past the fill holds the padding's value)
      for (uint32_t j = 0; j < L.chunk; j++) {
        const uint32_t x = te_scan::wide_x(lane, j);
        if (x >= t.fill) break;
        const uint64_t at = te_scan::load_of(t, x, L.shared);
        if (at >= src.records) return false;
        uint32_t w[8];
        rd(src.rd, at, w);
        scan_take<OP>(w, L.form_in, j == 0u, acc[lane]);
      }
      scan_close_total<OP>(acc[lane], L.mistake != M_NO_REDUCE);
    }
    for (uint32_t s = 0; s < te_scan::kLog; s++) {
      for (uint32_t lane = 0; lane < te_scan::kLanes; lane++) scan_area_put(scan.data(), lane, acc[lane]);
      for (uint32_t lane = 0; lane < te_scan::kLanes; lane++) {
        if (!scan_tree_takes(lane, s)) continue;
        if (lane + (1u << s) >= te_scan::kLanes) return false;
        acc[lane] = scan_combine<OP>(acc[lane], scan_area_get(scan.data(), lane + (1u << s)));
        scan_after_step<OP>(acc[lane], s);
      }
    }
    uint32_t w[8];
    const uint64_t at = te_scan::total_of(L.v, t);
    if (seeds.rd) {
      if (at >= seeds.records) return false;
      rd(seeds.rd, at, w);
      acc[0] = scan_combine<OP>(fp_from_words32(w), acc[0]);
    }
    scan_out<OP>(acc[0], L.form_out, w, L.mistake == M_INTERNAL_OUT && L.last);
    if (at >= dst.records) return false;
    wr(dst.wr, at, w);
  }
  return true;
}

// one launch of k_scan_apply; seeds: the call's (M_SEED_EVERYWHERE takes them in below the last level too)
template <int OP> bool apply_launch(const launch& L, const buffer& src, const buffer& dst, const buffer& carries, const buffer& seeds) {
  const uint32_t chunk = L.chunk, data_words = te_scan::lds_data_words(chunk);
  std::vector<uint32_t> lds(data_words + te_scan::lds_scan_words());
  uint32_t* const scan = lds.data() + data_words;
  std::vector<fel<9>> acc(te_scan::kLanes);
  const uint64_t blocks = L.count * L.v.tiles;
  for (uint64_t block = 0; block < blocks; block++) {
    const te_scan::tile t = te_scan::tile_of(L.v, te_scan::kLanes * chunk, block);
    for (uint32_t lane = 0; lane < te_scan::kLanes; lane++)
      for (uint32_t j = 0; j < chunk; j++) {
        const uint32_t x = te_scan::wide_x(lane, j);
        uint32_t w[8], o[8];
        if (x < t.fill) {
          const uint64_t at = te_scan::load_of(t, x, L.shared);
          if (at >= src.records) return false;
          rd(src.rd, at, w);
          scan_stage<OP>(w, L.form_in, o);
        } else scan_pad<OP>(o, L.mistake == M_ZERO_PAD);
        if (te_scan::lds_word(x, chunk) + 8u > data_words) return false;
        scan_lds_put(lds.data(), te_scan::lds_word(x, chunk), o);
      }
    uint32_t cw[8];
    uint64_t cat = te_scan::total_of(L.v, t);
    if (L.mistake == M_CARRY && L.level0) cat = t.vec * L.v.tiles + (t.b + 1u) % L.v.tiles;
    if (cat >= carries.records) return false;
    rd(carries.rd, cat, cw);
    if (L.mistake == M_SEED_EVERYWHERE && !L.last) {
      uint32_t sw[8];
      rd(seeds.rd, t.vec, sw);
      scan_out<OP>(scan_combine<OP>(fp_from_words32(sw), fp_from_words32(cw)), te_scan::kInternal, cw);
    }
    for (uint32_t lane = 0; lane < te_scan::kLanes; lane++) {
      acc[lane] = scan_identity<OP>();
      for (uint32_t j = 0; j < chunk; j++) {
        const uint32_t at = te_scan::lds_word(te_scan::own_x(lane, j, chunk), chunk);
        if (at + 8u > data_words) return false;
        uint32_t w[8];
        scan_lds_get(lds.data(), at, w);
        scan_take<OP>(w, te_scan::kInternal, j == 0u, acc[lane]);
      }
      scan_close_total<OP>(acc[lane], L.mistake != M_NO_REDUCE);
    }
    for (uint32_t s = 0; s < te_scan::kLog; s++) {
      for (uint32_t lane = 0; lane < te_scan::kLanes; lane++) scan_area_put(scan, lane, acc[lane]);
      for (uint32_t lane = 0; lane < te_scan::kLanes; lane++)
        if (scan_step_takes(lane, s)) { acc[lane] = scan_combine<OP>(scan_area_get(scan, lane - (1u << s)), acc[lane]); scan_after_step<OP>(acc[lane], s); }
    }
    for (uint32_t lane = 0; lane < te_scan::kLanes; lane++) scan_area_put(scan, lane, acc[lane]);
    const bool exclusive = L.exclusive && !(L.mistake == M_UNSHIFTED && L.level0);
    for (uint32_t lane = 0; lane < te_scan::kLanes; lane++) {
      fel<9> h = scan_prefix<OP>(cw, lane != 0u, scan_area_get(scan, lane ? lane - 1u : 0u));
      for (uint32_t j = 0; j < chunk; j++) {
        const uint32_t at = te_scan::lds_word(te_scan::own_x(lane, j, chunk), chunk);
        uint32_t w[8], o[8];
        scan_lds_get(lds.data(), at, w);
        scan_walk<OP>(w, exclusive, L.form_out, h, o, L.mistake == M_INTERNAL_OUT && L.level0);
        scan_lds_put(lds.data(), at, o);
      }
    }
    for (uint32_t lane = 0; lane < te_scan::kLanes; lane++)
      for (uint32_t j = 0; j < chunk; j++) {
        const uint32_t x = te_scan::wide_x(lane, j);
        if (x >= t.fill) break;
        if (t.base + x >= dst.records) return false;
        uint32_t w[8];
        scan_lds_get(lds.data(), te_scan::lds_word(x, chunk), w);
        wr(dst.wr, t.base + x, w);
      }
  }
  return true;
}

template <int OP> int emulate(const scan_req& r, const te_scan::plan& P, const uint8_t* a, const uint8_t* init, int mistake, uint8_t* totals, uint8_t* out) {
  const uint64_t count = r.count, n = r.n;
  std::vector<uint8_t> reg((size_t)P.records * 32);
  scan_seeds(r, mistake == M_NO_SEED ? nullptr : init, reg.data() + P.seeds * 32);
  const uint32_t caller = scan_caller_form(r);
  auto region = [&](uint64_t off, uint64_t records) { return buffer{reg.data() + off * 32, reg.data() + off * 32, records}; };
  const buffer seeds = region(P.seeds, count);
  auto launch_of = [&](uint32_t l) {
    launch L;
    L.v = P.lv[l]; L.chunk = P.chunk; L.count = count; L.mistake = mistake; L.level0 = l == 0u; L.last = l + 1u == P.levels;
    L.form_in = l ? (uint32_t)te_scan::kInternal : caller; L.shared = l == 0u && r.shared; L.exclusive = l || r.exclusive; L.form_out = te_scan::kInternal;
    return L;
  };
  const buffer src0 = buffer{a, nullptr, r.shared ? count : count * n};
  for (uint32_t l = 0; l < P.levels; l++) {
    const te_scan::level& v = P.lv[l];
    if (v.dst + count * v.tiles > P.seeds) return E_BOUNDS;
    launch L = launch_of(l);
    if (L.last && !totals) break;
    if (L.last) L.form_out = caller;
    if (!totals_launch<OP>(L, l ? region(v.src, count * v.n) : src0, region(v.dst, count * v.tiles), L.last ? seeds : buffer{nullptr, nullptr, 0})) return E_BOUNDS;
  }
  std::vector<uint8_t> tot((size_t)count * 32);
  if (totals) memcpy(tot.data(), reg.data() + P.lv[P.levels - 1].dst * 32, tot.size());
  if (out) {
    for (uint32_t l = P.levels; l-- > 0u;) {
      const te_scan::level& v = P.lv[l];
      launch L = launch_of(l);
      if (l == 0u) L.form_out = caller;
      const buffer dst = l ? region(v.src, count * v.n) : buffer{nullptr, out, count * n};
      if (!apply_launch<OP>(L, l ? region(v.src, count * v.n) : src0, dst, L.last ? seeds : region(v.dst, count * v.tiles), seeds)) return E_BOUNDS;
    }
  }
  if (totals) memcpy(totals, tot.data(), tot.size());
  return 0;
}
}  // namespace

extern "C" {

// te_msm_field_scan's steps with the product's block code: 0, -1 (refused, outputs untouched; *reason = why: scan.hip.hpp's SCAN_*), -100
// (an index left its allocation).  out may be a; totals or out may be NULL; init may be NULL.  chunk: 0 for the default
int scan_emulate(int op, const uint8_t* a, uint64_t n, uint64_t count, int flags, uint32_t chunk, int mistake, const uint8_t* init, uint8_t* totals, uint8_t* out, int* reason) {
  scan_req r;
  const int why = scan_check(op, a, n, count, flags, totals, out, r);
  if (reason) *reason = why;
  if (why != SCAN_OK) return -1;
  if (count == 0) return 0;
  r.chunk = te_scan::chunk_for(n, te_scan::clamp_chunk((long)chunk));
  te_scan::plan P;
  if (!te_scan::make_plan(n, count, r.chunk, P)) { if (reason) *reason = SCAN_TOO_LARGE; return -1; }
  return op == TE_MSM_SCAN_SUM ? emulate<te_scan::kSum>(r, P, a, init, mistake, totals, out) : emulate<te_scan::kProduct>(r, P, a, init, mistake, totals, out);
}

// every index of the plan for `count` vectors of n at `chunk`, by arithmetic alone: 0 with *checked = how many, or -100
int scan_replay(uint64_t n, uint64_t count, uint32_t chunk, int shared, uint64_t* checked) {
  te_scan::plan P;
  *checked = 0;
  if (!te_scan::make_plan(n, count, chunk, P)) return E_BOUNDS;
  if (P.levels < 1u || P.levels > te_scan::kMaxLevels || P.lv[P.levels - 1].tiles != 1u || P.lv[0].n != n) return E_BOUNDS;
  const uint32_t data_words = te_scan::lds_data_words(chunk);
  if (te_scan::lds_bytes_apply(chunk) > 160u * 1024u) return E_BOUNDS;
  std::vector<uint8_t> hit(data_words, 0);
  for (uint32_t lane = 0; lane < te_scan::kLanes; lane++)
    for (uint32_t j = 0; j < chunk; j++) {
      const uint32_t wx = te_scan::wide_x(lane, j), ox = te_scan::own_x(lane, j, chunk);
      if (wx >= P.T || ox >= P.T || te_scan::lds_word(wx, chunk) + 8u > data_words) return E_BOUNDS;
      const uint32_t at = te_scan::lds_word(ox, chunk);
      for (uint32_t k = 0; k < 8u; k++) { if (at + k >= data_words || hit[at + k]) return E_BOUNDS; hit[at + k] = 1; }
      *checked += 2;
    }
  for (uint32_t lane = 0; lane < te_scan::kLanes; lane++)
    for (uint32_t s = 0; s < te_scan::kLog; s++) {
      if (scan_tree_takes(lane, s) && lane + (1u << s) >= te_scan::kLanes) return E_BOUNDS;
      if (scan_step_takes(lane, s) && lane < (1u << s)) return E_BOUNDS;
      if ((lane + 1u) * te_scan::kScanLimbs > te_scan::lds_scan_words()) return E_BOUNDS;
    }
  uint64_t end = 0;
  for (uint32_t l = 0; l < P.levels; l++) {
    const te_scan::level& v = P.lv[l];
    if (l && (v.n != P.lv[l - 1].tiles || v.src != P.lv[l - 1].dst)) return E_BOUNDS;
    if (v.tiles != (v.n + P.T - 1) / P.T || v.dst != end || count * v.tiles >> 31) return E_BOUNDS;
    end = v.dst + count * v.tiles;
    if (end > P.seeds) return E_BOUNDS;
    const bool sh = shared && l == 0u;
    const uint64_t src_records = sh ? count : count * v.n, out_records = count * v.n, blocks = count * v.tiles;
    uint64_t next = 0;                                               // the tiles cover the level's records in order, once: every out record is written exactly once
    for (uint64_t block = 0; block < blocks; block++) {
      const te_scan::tile t = te_scan::tile_of(v, P.T, block);
      if (t.vec >= count || t.b >= v.tiles || t.fill < 1u || t.fill > P.T || t.base != next || t.base + t.fill > out_records) return E_BOUNDS;
      if (t.b * P.T + t.fill > v.n) return E_BOUNDS;                 // a tile stays inside its vector
      next = t.base + t.fill;
      if (te_scan::load_of(t, 0, sh) >= src_records || te_scan::load_of(t, (uint32_t)t.fill - 1u, sh) >= src_records) return E_BOUNDS;
      const uint64_t s = v.dst + te_scan::total_of(v, t);
      if (s < v.dst || s >= end || s - v.dst != block) return E_BOUNDS;
      if (l + 1u == P.levels && P.seeds + te_scan::total_of(v, t) >= P.records) return E_BOUNDS;     // its carry: the vector's seed
      *checked += 4;
    }
    if (next != out_records) return E_BOUNDS;
  }
  if (end != P.seeds || P.records != P.seeds + count || P.scratch_bytes != P.records * 32) return E_BOUNDS;
  return 0;
}

// the chunk a call of vectors of n elements runs at when `chunk` is in force
uint32_t scan_chunk_for(uint64_t n, uint32_t chunk) { return te_scan::chunk_for(n, chunk); }

// the plan as numbers: out[0] levels, [1] T, [2] records of scratch, [3] scratch bytes, [4] LDS bytes of the apply kernel, [5] the default
// chunk, [6] the largest chunk, then n and tiles of each level (0 when make_plan refuses: out[0] = 0)
void scan_plan_info(uint64_t n, uint64_t count, uint32_t chunk, uint64_t* out) {
  te_scan::plan P;
  memset(out, 0, 16 * sizeof(uint64_t));
  out[5] = te_scan::kChunkDefault; out[6] = te_scan::kChunkMax;
  if (!te_scan::make_plan(n, count, chunk, P)) return;
  out[0] = P.levels; out[1] = P.T; out[2] = P.records; out[3] = P.scratch_bytes; out[4] = te_scan::lds_bytes_apply(chunk);
  for (uint32_t l = 0; l < P.levels; l++) { out[7 + 2 * l] = P.lv[l].n; out[8 + 2 * l] = P.lv[l].tiles; }
}

// where the sum path reduces, as the plan says: out[0] a lane's total, out[1] the lane's prefix, out[2 + s] behind step s of the tree / scan
void scan_points(uint32_t* out) {
  out[0] = te_scan::sum_reduces_lane_total(); out[1] = te_scan::sum_reduces_prefix();
  for (uint32_t s = 0; s < te_scan::kLog; s++) out[2 + s] = te_scan::sum_reduces_step(s);
}

// the constants of the plan the header must agree with: out[0] SUM, [1] PRODUCT, [2] max n, [3] default chunk
void scan_constants(uint64_t* out) { out[0] = te_scan::kSum; out[1] = te_scan::kProduct; out[2] = te_scan::kMaxN; out[3] = te_scan::kChunkDefault; }

}
