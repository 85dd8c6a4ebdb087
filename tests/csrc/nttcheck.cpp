// nttcheck.cpp -- TEST SHIM: compiles the product's NTT (csrc/ntt.hip.hpp, csrc/ntt_plan.hpp) for the host, so that the exact per-lane
// code of k_ntt_pass and k_ntt_table runs on the CPU box (tests/test_ntt_host.py, tests/csrc/san_ntt.cpp; the GPU tests take ntt_ref as
// their reference).  Not part of the product; not a fallback.  It holds
//   ntt_ref      a textbook transform on the host build of fp.hpp: shift, decimation-in-frequency butterflies with twiddles walked by
//                repeated products from W^(2^(47 - L)), a bit-reversal permutation, scaling.  It knows nothing of the plan or the tables.
//   ntt_emulate  te_msm_ntt's steps: the same argument check, constants and table generators as points.hip, then every pass of the plan,
//                a block as plain loops over its 256 lanes -- one loop per phase, a loop boundary being the block's barrier.  Every
//                global and LDS index is checked against what the plan says is allocated (-100 on a violation).
//   ntt_replay   the indices alone, no arithmetic: every index of every pass inside its allocation, every record of a pass read exactly
//                once and written exactly once.
// `mistake` (0 in every real check) turns the emulation into a deliberately wrong variant, which the tests must catch:
//   1 the inverse root in the forward direction (and back)      2 1 / n missing                       3 output left bit-reversed
//   4 the shift applied behind the transform instead of in front  5 one twiddle index off by one at a pass boundary
//   6 the hi / lo split of the twiddle tables off by one (hi built from Omega^2048)
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/ntt.hip.hpp"

using namespace te;

namespace {
enum { M_ROOT = 1, M_SCALE = 2, M_BITREV = 3, M_SHIFT_AFTER = 4, M_TWIDDLE = 5, M_SPLIT = 6 };
constexpr int E_BOUNDS = -100;

void rd(const uint8_t* p, uint64_t i, uint32_t (&w)[8]) { memcpy(w, p + i * 32, 32); }
void wr(uint8_t* p, uint64_t i, const uint32_t (&w)[8]) { memcpy(p + i * 32, w, 32); }

// ---- the textbook transform ----------------------------------------------------------------------------------------------------
fel<9> red(const fel<9>& x) { return fo_residue(fe_norm(x)); }       // any sum or difference -> class N below 1.1 p
fel<9> inv(const fel<9>& x) { return fe_inv(x, kInvExpTe); }
void ref_one(const uint8_t* a, uint32_t L, bool inverse, bool mont, bool shifted, const fel<9>& s, uint8_t* out) {
  const uint64_t n = 1ull << L;
  std::vector<fel<9>> x(n);
  for (uint64_t i = 0; i < n; i++) { uint32_t w[8]; rd(a, i, w); x[i] = mont ? fo_decode<9, true>(w) : fo_decode<9, false>(w); }
  if (shifted && !inverse) { fel<9> pw = fe_one<9>(); for (uint64_t i = 0; i < n; i++) { x[i] = fe_mul(x[i], pw); pw = fe_mul(pw, s); } }
  fel<9> root = ntt_root_of(L);
  if (inverse) root = inv(root);
  for (uint64_t half = n >> 1; half >= 1; half >>= 1) {
    fel<9> step = root;                                              // root^(n / (2 half))
    for (uint64_t m = 2 * half; m < n; m <<= 1) step = fe_mul(step, step);
    for (uint64_t at = 0; at < n; at += 2 * half) {
      fel<9> w = fe_one<9>();
      for (uint64_t k = 0; k < half; k++) {
        const fel<9> u = x[at + k], v = x[at + k + half];
        x[at + k] = red(fe_add(u, v));
        x[at + k + half] = fe_mul(fe_norm(fe_sub<2>(u, v)), w);
        w = fe_mul(w, step);
      }
    }
  }
  std::vector<fel<9>> y(n);
  for (uint64_t i = 0; i < n; i++) { uint64_t r = 0; for (uint32_t b = 0; b < L; b++) r |= ((i >> b) & 1u) << (L - 1 - b); y[r] = x[i]; }
  if (inverse) {
    fel<9> nn = fe_one<9>();
    for (uint32_t i = 0; i < L; i++) nn = red(fe_add(nn, nn));
    fel<9> pw = inv(nn);
    const fel<9> si = shifted ? inv(s) : fe_one<9>();
    for (uint64_t i = 0; i < n; i++) { y[i] = fe_mul(y[i], pw); pw = fe_mul(pw, si); }
  }
  for (uint64_t i = 0; i < n; i++) {
    uint32_t w[8];
    if (mont) fo_encode<9, true>(y[i], w); else fo_encode<9, false>(y[i], w);
    wr(out, i, w);
  }
}

// ---- the emulated kernels --------------------------------------------------------------------------------------------------------
void table(const fel<9>& g, const fel<9>& pre, bool with_pre, uint32_t* out) {      // k_ntt_table, lane by lane
  for (uint32_t j = 0; j < te_ntt::kTabEntries; j++) {
    const fel<9> v = ntt_power(g, j, pre, with_pre);
    for (uint32_t k = 0; k < te_ntt::kTabWords; k++) out[(size_t)te_ntt::kTabWords * j + k] = k < 9 ? v.v[k] : 0u;
  }
}
struct buffer { const uint8_t* rd; uint8_t* wr; uint64_t records; };
// one launch of k_ntt_pass; false: an index left its allocation
bool pass_launch(const te_ntt::pass& ps, uint64_t transforms, const buffer& src, const buffer& dst, bool inverse, bool shifted, const ntt_consts& k, const ntt_tabs& tb,
                 int mistake) {
  std::vector<uint32_t> lds(te_ntt::kLdsSlots * te_ntt::kLimbs);
  const uint64_t tiles = te_ntt::tiles_of(ps, transforms), lines = te_ntt::lines_of(ps, transforms);
  const bool root_inverse = mistake == M_ROOT ? !inverse : inverse;
  bool shift_in = shifted && !inverse, shift_out = shifted && inverse;
  if (mistake == M_SHIFT_AFTER) std::swap(shift_in, shift_out);
  for (uint64_t tile = 0; tile < tiles; tile++) {
    for (uint32_t lane = 0; lane < te_ntt::kLanes; lane++)
      for (uint32_t q = 0; q < te_ntt::kElemsPerLane; q++) {
        te_ntt::elem e = te_ntt::elem_of(ps, tile, lane + te_ntt::kLanes * q, lines, false);
        uint32_t w[8] = {};
        if (e.valid) { if (e.pos >= src.records) return false; rd(src.rd, e.pos, w); }
        if (mistake == M_BITREV && ps.last) e.rho = te_ntt::brev(e.rho, ps.r);
        if (te_ntt::slot_of(ps, e.kappa, te_ntt::brev(e.rho, ps.r)) >= te_ntt::kLdsSlots) return false;
        ntt_lane_in(ps, e, w, k.dec, tb, shift_in, lds.data());
      }
    for (uint32_t st = 0; st < ps.r; st++)
      for (uint32_t lane = 0; lane < te_ntt::kLanes; lane++)
        for (uint32_t q = 0; q < te_ntt::kBflyPerLane; q++) {
          const te_ntt::bfly f = te_ntt::bfly_of(ps, st, lane + te_ntt::kLanes * q);
          if (f.v >= te_ntt::kLdsSlots || f.u >= f.v || f.tw >= te_ntt::kTabEntries) return false;
          ntt_lane_stage(ps, st, lane + te_ntt::kLanes * q, root_inverse, tb, lds.data());
        }
    for (uint32_t lane = 0; lane < te_ntt::kLanes; lane++)
      for (uint32_t q = 0; q < te_ntt::kElemsPerLane; q++) {
        te_ntt::elem e = te_ntt::elem_of(ps, tile, lane + te_ntt::kLanes * q, lines, true);
        if (!e.valid) continue;
        if (e.pos >= dst.records || te_ntt::slot_of(ps, e.kappa, e.rho) >= te_ntt::kLdsSlots) return false;
        if (mistake == M_TWIDDLE && tile == 0 && e.rho == 1u && e.kappa == 1u) e.lowpos += 1u;
        uint32_t w[8];
        ntt_lane_out(ps, e, root_inverse, k.enc, tb, shift_out, lds.data(), w);
        wr(dst.wr, e.pos, w);
      }
  }
  return true;
}

// ---- the indices alone -------------------------------------------------------------------------------------------------------------
bool replay_pass(const te_ntt::pass& ps, uint64_t transforms, uint64_t src_records, uint64_t dst_records, uint64_t* checked) {
  const uint64_t tiles = te_ntt::tiles_of(ps, transforms), lines = te_ntt::lines_of(ps, transforms), records = transforms << ps.log_n;
  std::vector<uint8_t> seen(records, 0);                             // bit 0: read, bit 1: written
  for (uint32_t st = 0; st < ps.r; st++) {                           // (a tile's butterflies do not depend on the tile)
    std::vector<uint8_t> hit(te_ntt::kLdsSlots, 0);
    for (uint32_t b = 0; b < te_ntt::kTile / 2u; b++) {
      const te_ntt::bfly f = te_ntt::bfly_of(ps, st, b);
      if (f.v >= te_ntt::kLdsSlots || f.u >= f.v || f.tw >= te_ntt::kTabEntries || hit[f.u] || hit[f.v]) return false;
      hit[f.u] = hit[f.v] = 1;                                       // no two lanes touch one slot between two barriers
      *checked += 3;
    }
  }
  for (uint64_t tile = 0; tile < tiles; tile++) {
    uint8_t slot_in[te_ntt::kLdsSlots] = {}, slot_out[te_ntt::kLdsSlots] = {};
    for (uint32_t x = 0; x < te_ntt::kTile; x++) {
      const te_ntt::elem e = te_ntt::elem_of(ps, tile, x, lines, false), o = te_ntt::elem_of(ps, tile, x, lines, true);
      const uint32_t si = te_ntt::slot_of(ps, e.kappa, te_ntt::brev(e.rho, ps.r)), so = te_ntt::slot_of(ps, o.kappa, o.rho);
      if (e.rho >> ps.r || e.kappa >> ps.c || si >= te_ntt::kLdsSlots || so >= te_ntt::kLdsSlots || slot_in[si]) return false;
      slot_in[si] = 1; slot_out[so] = 1;
      *checked += 2;
      if (e.valid) { if (e.pos >= src_records || e.pos >= records || (seen[e.pos] & 1)) return false; seen[e.pos] |= 1; *checked += 1; }
      if (o.valid) {
        if (o.pos >= dst_records || o.pos >= records || (seen[o.pos] & 2)) return false;
        seen[o.pos] |= 2; *checked += 1;
        if (ps.twiddle) {
          const uint64_t E = ((uint64_t)o.rho * o.lowpos) << ps.tw_shift;
          if (E >> te_ntt::kRootLog || te_ntt::twiddle_exp(ps, o) != E) return false;
          if ((te_ntt::root_index((uint32_t)E, true) >> te_ntt::kSplitLog) >= te_ntt::kTabEntries) return false;
          *checked += 1;
        }
        if ((o.pos & ((1ull << ps.log_n) - 1u)) >> te_ntt::kSplitLog >= te_ntt::kTabEntries) return false;      // the shift tables' hi index
      }
    }
    for (uint32_t s = 0; s < te_ntt::kLdsSlots; s++) if (slot_out[s] && !slot_in[s]) return false;              // what is read back was stored
  }
  for (uint64_t i = 0; i < records; i++) if (seen[i] != 3) return false;
  return true;
}
}  // namespace

extern "C" {

// te_msm_ntt's definition on host memory, by the textbook: 0, or -1 for what te_msm_ntt refuses (out untouched)
int ntt_ref(const uint8_t* a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, uint8_t* out) {
  ntt_req q;
  if (ntt_check(a, log_n, count, flags, shift, out, q) != NTT_OK) return -1;
  std::vector<uint8_t> res((size_t)32 << log_n);
  for (uint64_t t = 0; t < count; t++) {
    ref_one(a + ((t * 32) << log_n), log_n, q.inverse, q.mont, q.shifted, q.s, res.data());
    memcpy(out + ((t * 32) << log_n), res.data(), res.size());
  }
  return 0;
}

// te_msm_ntt's steps with the product's block code: 0, -1 (refused, out untouched; *reason = why: ntt.hip.hpp's NTT_*), -100 (an index
// left its allocation).  out may be a.  piece: transforms of one piece (0: the plan's), so that a test reaches the piece loop cheaply
int ntt_emulate(const uint8_t* a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, int mistake, uint64_t piece, uint8_t* out, int* reason) {
  ntt_req q;
  const int why = ntt_check(a, log_n, count, flags, shift, out, q);
  if (reason) *reason = why;
  if (why != NTT_OK) return -1;
  if (count == 0) return 0;
  te_ntt::plan P = te_ntt::make_plan(log_n);
  if (piece) P.piece_transforms = piece;
  ntt_consts k = ntt_consts_of(q);
  if (mistake == M_SCALE) { ntt_req fwd = q; fwd.inverse = false; k.enc = ntt_consts_of(fwd).enc; }
  const size_t T = (size_t)te_ntt::kTabEntries * te_ntt::kTabWords;
  static std::vector<uint32_t> device_tabs;                          // as on a device: built by the first call, kept
  std::vector<uint32_t> tabs(4 * T);
  fel<9> hi, lo;
  if (device_tabs.empty() || mistake == M_SPLIT) {
    ntt_twiddle_gens(hi, lo);
    if (mistake == M_SPLIT) { hi = lo; for (uint32_t i = 0; i + 1 < te_ntt::kSplitLog; i++) hi = fe_mul(hi, hi); }
    table(hi, hi, false, &tabs[0]);
    table(lo, lo, false, &tabs[T]);
    if (mistake != M_SPLIT) device_tabs.assign(tabs.begin(), tabs.begin() + 2 * T);
  } else {
    std::copy(device_tabs.begin(), device_tabs.end(), tabs.begin());
  }
  ntt_tabs tb = {&tabs[0], &tabs[T], nullptr, nullptr};
  if (q.shifted) {
    ntt_shift_gens(q, hi, lo);
    const bool enc_side = mistake == M_SHIFT_AFTER ? !q.inverse : q.inverse;
    table(hi, enc_side ? k.enc : k.dec, true, &tabs[2 * T]);
    table(lo, lo, false, &tabs[3 * T]);
    tb.sh_hi = &tabs[2 * T]; tb.sh_lo = &tabs[3 * T];
  }
  const uint64_t tmp_records = te_ntt::tmp_records_for(P, count);
  std::vector<uint8_t> tmp((size_t)tmp_records * 32);
  const uint64_t n = 1ull << log_n;
  for (uint64_t off = 0; off < count; off += P.piece_transforms) {
    const uint64_t m = std::min(P.piece_transforms, count - off);
    for (uint32_t p = 0; p < P.passes; p++) {
      const buffer in = {a + off * n * 32, nullptr, (count - off) * n}, mid = {tmp.data(), tmp.data(), tmp_records}, res = {nullptr, out + off * n * 32, (count - off) * n};
      if (!pass_launch(P.p[p], m, p == 0 ? in : mid, p + 1 == P.passes ? res : mid, q.inverse, q.shifted, k, tb, mistake)) return E_BOUNDS;
    }
  }
  return 0;
}

// every index of the plan for `count` transforms of 2^log_n: 0 with *checked = how many, or -100
int ntt_replay(uint32_t log_n, uint64_t count, uint64_t* checked) {
  const te_ntt::plan P = te_ntt::make_plan(log_n);
  *checked = 0;
  if (P.passes < 1 || P.passes > te_ntt::kMaxPasses || P.r[0] + P.r[1] + P.r[2] != log_n) return E_BOUNDS;
  const uint64_t tmp_records = te_ntt::tmp_records_for(P, count), n = 1ull << log_n;
  for (uint64_t off = 0; off < count; off += P.piece_transforms) {
    const uint64_t m = std::min(P.piece_transforms, count - off);
    for (uint32_t p = 0; p < P.passes; p++) {
      const te_ntt::pass& ps = P.p[p];
      if (ps.r + ps.c != te_ntt::kTileLog || (P.passes > 1 && ps.c < te_ntt::kMinRunLog) || ((1u << ps.c) - 1u) * ps.pitch + (1u << ps.r) > te_ntt::kLdsSlots) return E_BOUNDS;
      if (te_ntt::tiles_of(ps, m) >> 31) return E_BOUNDS;            // the grid of a launch
      if (!replay_pass(ps, m, p == 0 ? (count - off) * n : tmp_records, p + 1 == P.passes ? (count - off) * n : tmp_records, checked)) return E_BOUNDS;
    }
  }
  return 0;
}

// the plan as numbers: out[0] passes, [1..3] r, [4] transforms of a one-pass tile (0: multi-pass), [5] piece_transforms, [6] tmp records
// for `count`, [7] LDS bytes, [8] bytes of the twiddle tables
void ntt_plan_info(uint32_t log_n, uint64_t count, uint64_t* out) {
  const te_ntt::plan P = te_ntt::make_plan(log_n);
  out[0] = P.passes; out[1] = P.r[0]; out[2] = P.r[1]; out[3] = P.r[2];
  out[4] = P.passes == 1 ? 1ull << P.p[0].c : 0;
  out[5] = P.piece_transforms; out[6] = te_ntt::tmp_records_for(P, count); out[7] = te_ntt::kLdsBytes; out[8] = 2 * te_ntt::kTabBytes;
}

// where record x of tile `tile` of pass `pass` is written (count = 1): its offset in the output of the pass; *tiles = tiles of the pass
uint64_t ntt_tile_record(uint32_t log_n, uint32_t pass, uint64_t tile, uint32_t x, uint64_t* tiles) {
  const te_ntt::plan P = te_ntt::make_plan(log_n);
  const te_ntt::pass& ps = P.p[pass < P.passes ? pass : 0];
  *tiles = te_ntt::tiles_of(ps, 1);
  return te_ntt::elem_of(ps, tile, x, te_ntt::lines_of(ps, 1), true).pos;
}

// W and its order: words of W; *order_log = k with W^(2^k) = 1 and W^(2^(k-1)) = -1 (0 if neither within 64 squarings)
void ntt_root(uint8_t w_out[32], uint32_t* order_log) {
  memcpy(w_out, NTT_W_W32, 32);
  fel<9> g = ntt_root_of(NTT_TWO_ADICITY);
  *order_log = 0;
  uint32_t c[8], prev[8] = {};
  for (uint32_t k = 0; k <= 64; k++) {
    fo_encode<9, false>(g, c);
    uint32_t one[8] = {1u};
    if (!memcmp(c, one, 32)) {
      uint32_t m1[8]; memcpy(m1, P_W32, 32); m1[0] -= 1u;
      if (k > 0 && !memcmp(prev, m1, 32)) *order_log = k;
      return;
    }
    memcpy(prev, c, 32);
    g = fe_mul(g, g);
  }
}

}
