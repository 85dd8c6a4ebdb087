// fieldopscheck.cpp -- TEST SHIM: compiles the product's batched field arithmetic (csrc/field_ops.hip.hpp) for the host, so that the exact
// per-lane code of k_field_map, k_field_zero_scan, k_field_inv, k_field_pow and k_field_sqrt is compared with bigint models on the CPU
// box (tests/test_field_ops_host.py, tests/csrc/san_field.cpp).  A block of k_field_inv is emulated with plain loops over its lanes;
// its slab is plane-major as on the device.  Not part of the product; not a fallback.
//
// `mistake` (0 in every real check) turns the emulation into a deliberately wrong variant, which the tests must catch:
//   1  the backward walk of an inversion chain reads the prefix one slot off
//   2  a zero is not left out of an inversion chain
//   4  the larger square root
//   8  the exponent reduced mod p (one subtraction)
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/field_ops.hip.hpp"

using namespace te;

namespace {
enum { M_WALK = 1, M_ZERO = 2, M_LARGER = 4, M_REDUCE = 8 };
enum { OP_ADD = 0, OP_SUB, OP_MUL, OP_DOUBLE, OP_NEG, OP_SQUARE, OP_INV, OP_POW, OP_SQRT };
enum { F_SHARED = 1, F_MONT = 2, F_ZERO_OK = 4 };

template <int W> void rd(const uint8_t* p, uint64_t i, uint32_t (&w)[W]) { memcpy(w, p + i * W * 4, W * 4); }
template <int W> void wr(uint8_t* p, uint64_t i, const uint32_t (&w)[W]) { memcpy(p + i * W * 4, w, W * 4); }

// one launch of k_field_inv over m elements: blocks of 256 lanes, a lane's elements 256 apart in its block's tile
template <int N, bool MONT> void inv_launch(const uint8_t* a, uint32_t m, uint32_t group, int mistake, uint8_t* out) {
  constexpr int W = fo_sizes<N>::W, SQ = fo_sizes<N>::SQ;
  const uint32_t cap = m, blocks = (m + 256u * group - 1u) / (256u * group);
  std::vector<uint32_t> slab((size_t)SQ * cap * 4);
  const exp_t inv_exp = N == 9 ? kInvExpTe : kInvExp377;
  for (uint32_t blk = 0; blk < blocks; blk++)
    for (uint32_t lane = 0; lane < 256u; lane++) {
      const uint64_t first = (uint64_t)blk * 256u * group + lane;
      fel<N> run = fe_one<N>();
      for (uint32_t j = 0; j < group; j++) {
        const uint64_t e = first + (uint64_t)j * 256u;
        if (e >= m) break;
        uint32_t wa[W], s[4 * SQ];
        rd<W>(a, e, wa);
        fel<N> before;
        if (mistake & M_ZERO) { before = run; run = fe_mul(run, fo_decode<N, MONT>(wa)); }
        else fo_inv_forward<N, MONT>(wa, run, before);
        fo_slab_pack<N>(before, s);
        for (int q = 0; q < SQ; q++) memcpy(&slab[((size_t)q * cap + e) * 4], &s[4 * q], 16);
      }
      if (first >= m) continue;
      fel<N> inv = fe_inv(run, inv_exp);
      for (uint32_t j = group; j-- > 0u;) {
        const uint64_t e = first + (uint64_t)j * 256u;
        if (e >= m) continue;
        const uint64_t at = (mistake & M_WALK) && j > 0 ? e - 256u : e;
        uint32_t wa[W], s[4 * SQ], o[W];
        rd<W>(a, e, wa);
        for (int q = 0; q < SQ; q++) memcpy(&s[4 * q], &slab[((size_t)q * cap + at) * 4], 16);
        fo_inv_backward<N, MONT>(wa, fo_slab_unpack<N>(s), inv, o);
        wr<W>(out, e, o);
      }
    }
}

template <int N, bool MONT> int run(int op, const uint8_t* a, const uint8_t* b, uint64_t n, int flags, uint32_t group, int mistake, uint8_t* out, int64_t* bad, int* why) {
  constexpr int W = fo_sizes<N>::W;
  const bool shared = (flags & F_SHARED) != 0;
  *bad = -1; *why = 0;
  if (op == OP_INV) {
    if (!(flags & F_ZERO_OK))
      for (uint64_t i = 0; i < n; i++) {                           // k_field_zero_scan: the lowest index wins
        uint32_t wa[W];
        rd<W>(a, i, wa);
        if (fo_words_zero<N>(wa)) { *bad = (int64_t)i; *why = 1; return -6; }
      }
    inv_launch<N, MONT>(a, (uint32_t)n, group, mistake, out);
    return 0;
  }
  if (op == OP_SQRT) {
    std::vector<uint8_t> tmp((size_t)n * W * 4 + 1);
    for (uint64_t i = 0; i < n; i++) {
      uint32_t wa[W], o[W];
      rd<W>(a, i, wa);
      const int reason = fo_sqrt<N, MONT>(wa, N == 9 ? kRootExpTe : kRootExp377, o, (mistake & M_LARGER) != 0);
      wr<W>(tmp.data(), i, o);
      if (reason && *bad < 0) { *bad = (int64_t)i; *why = reason; }
    }
    if (*bad >= 0) return -6;
    memcpy(out, tmp.data(), (size_t)n * W * 4);
    return 0;
  }
  for (uint64_t i = 0; i < n; i++) {
    uint32_t wa[W], wb[W] = {}, o[W];
    rd<W>(a, i, wa);
    if (op == OP_POW) {
      uint32_t e[8];
      rd<8>(b, shared ? 0 : i, e);
      if ((mistake & M_REDUCE) && !words_lt<8>(e, P_W32)) {
        uint64_t br = 0;
        for (int k = 0; k < 8; k++) { const uint64_t s = (uint64_t)e[k] - P_W32[k] - br; br = (s >> 63) & 1u; e[k] = (uint32_t)s; }
      }
      if (shared) {
        fo_rec se = {};
        memcpy(se.w, e, 32);
        se.top = fo_exp_top(e);
        fo_pow_shared<N, MONT>(wa, se, o);
      } else {
        fo_pow<N, MONT>(wa, e, o);
      }
    } else {
      if (op == OP_ADD || op == OP_SUB || op == OP_MUL) rd<W>(b, shared ? 0 : i, wb);
      else memcpy(wb, wa, sizeof wb);                                // (double, square: b is a; neg reads a alone)
      switch (op) {
        case OP_ADD: case OP_DOUBLE: fo_map<N, FO_ADD, false>(wa, wb, o); break;
        case OP_SUB: fo_map<N, FO_SUB, false>(wa, wb, o); break;
        case OP_NEG: fo_map<N, FO_NEG, false>(wa, wb, o); break;
        default: fo_map<N, FO_MUL, MONT>(wa, wb, o); break;          // mul, square
      }
    }
    wr<W>(out, i, o);
  }
  return 0;
}
}  // namespace

extern "C" {

// te_msm_field_op's steps on host memory (arguments are not validated here): 0, or -6 with the lowest failing index and its reason and
// `out` untouched.  field 0: 32-byte elements mod p, 1: 48-byte elements mod q; flags: TE_MSM_FIELD_*; group: elements of an inversion chain
int fo_field_op(int field, int op, const uint8_t* a, const uint8_t* b, uint64_t n, int flags, uint32_t group, int mistake, uint8_t* out, int64_t* bad, int* why) {
  const bool mont = (flags & F_MONT) != 0;
  if (field == 1) return mont ? run<14, true>(op, a, b, n, flags, group, mistake, out, bad, why) : run<14, false>(op, a, b, n, flags, group, mistake, out, bad, why);
  return mont ? run<9, true>(op, a, b, n, flags, group, mistake, out, bad, why) : run<9, false>(op, a, b, n, flags, group, mistake, out, bad, why);
}

}
