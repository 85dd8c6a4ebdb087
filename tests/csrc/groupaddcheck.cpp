// groupaddcheck.cpp -- TEST SHIM: compiles the product's batched group addition and point-set sum (csrc/group_add.hip.hpp) for the host, so
// that the exact per-lane code of k_group_add and k_group_sum (and of the affine pass they share with te_msm_mul) is compared with the
// bigint models on the CPU box (tests/test_group_add_host.py, tests/sanitize/san_group_add.cpp).  A block of the sum is emulated with
// plain loops over its lanes, one loop per phase: a barrier is where one loop ends.  Not part of the product; not a fallback.
//
// `mistake` (0 in every real check) turns the emulation into a deliberately wrong variant, which the tests must catch:
//   4  B not negated under TE_MSM_ADD_SUBTRACT
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/group_add.hip.hpp"

using namespace te;

namespace {
enum { M_NO_NEGATE = 4 };

// k_scalar_mul_affine over m slots: chains of SM_AFF_GROUP
template <int CURVE> void affine_pass(const uint32_t* proj, uint32_t m, uint32_t* out) {
  using Z = ga_sizes<CURVE>;
  for (uint32_t lo = 0; lo < m; lo += SM_AFF_GROUP)
    sm_affine_group<CURVE>(proj + (size_t)lo * Z::JW, std::min<uint32_t>(SM_AFF_GROUP, m - lo), out + (size_t)lo * Z::PW, CURVE == 1 ? kInvExp377 : kInvExpTe);
}
// k_group_add over n pairs
template <int CURVE> void slots(const uint8_t* a, const uint8_t* b, uint64_t n, int flags, int mistake, uint32_t* proj) {
  using Z = ga_sizes<CURVE>;
  const bool neg = (flags & 1) && !(mistake & M_NO_NEGATE), shared = (flags & 2) != 0;
  for (uint64_t i = 0; i < n; i++) {
    uint32_t wa[Z::PW], wb[Z::PW], o[Z::JW];
    memcpy(wa, a + i * Z::PW * 4, Z::PW * 4);
    memcpy(wb, b + (shared ? 0 : i) * Z::PW * 4, Z::PW * 4);
    ga_pair<CURVE>(wa, wb, neg, o);
    memcpy(proj + i * Z::JW, o, sizeof o);
  }
}
template <int CURVE> void add(const uint8_t* a, const uint8_t* b, uint64_t n, int flags, int mistake, uint8_t* out) {
  using Z = ga_sizes<CURVE>;
  std::vector<uint32_t> proj((size_t)n * Z::JW + 1), res((size_t)n * Z::PW + 1);
  slots<CURVE>(a, b, n, flags, mistake, proj.data());
  affine_pass<CURVE>(proj.data(), (uint32_t)n, res.data());
  memcpy(out, res.data(), (size_t)n * Z::PW * 4);
}
// one launch of k_group_sum: count items -> `blocks` partials
template <int CURVE, bool PARTIALS> void sum_launch(const uint32_t* src, uint32_t count, uint32_t blocks, uint32_t* partials) {
  using Z = ga_sizes<CURVE>;
  constexpr int SW = PARTIALS ? Z::TW : Z::PW;
  std::vector<uint32_t> sh((size_t)Z::AW * GS_SH_SLOTS);
  std::vector<ga_pt<CURVE>> acc(GS_BLOCK);
  const uint32_t stride = blocks * GS_BLOCK;
  for (uint32_t blk = 0; blk < blocks; blk++) {
    for (uint32_t lane = 0; lane < GS_BLOCK; lane++) {
      acc[lane] = ga_identity<CURVE>();
      for (uint64_t i = blk * GS_BLOCK + lane; i < count; i += stride) {
        uint32_t w[SW];
        memcpy(w, src + i * SW, sizeof w);
        acc[lane] = gs_step<CURVE, PARTIALS>(acc[lane], w);
      }
    }
    for (uint32_t s = GS_SH_SLOTS; s >= 1u; s >>= 1) {
      for (uint32_t lane = 0; lane < GS_BLOCK; lane++) gs_fold_store<CURVE>(lane, sh.data(), s, acc[lane]);
      for (uint32_t lane = 0; lane < GS_BLOCK; lane++) gs_fold_add<CURVE>(lane, sh.data(), s, acc[lane]);
    }
    uint32_t o[Z::TW] = {};
    ga_words<CURVE>(acc[0], o);
    memcpy(partials + (size_t)blk * Z::TW, o, sizeof o);
  }
}
// te_msm_sum_device's steps: stage 1 over at most `grid` blocks, the same kernel over the partials, sm_affine_group over the one point
template <int CURVE> void sum(const uint8_t* pts, uint64_t n, uint32_t grid, uint8_t* out) {
  using Z = ga_sizes<CURVE>;
  if (n == 0) {                                                    // (the host's rule: no launch)
    memset(out, 0, Z::PW * 4);
    if (CURVE == 0) out[32] = 1;
    return;
  }
  const uint32_t blocks = std::min<uint32_t>(grid, (uint32_t)((n + GS_BLOCK - 1u) / GS_BLOCK));
  std::vector<uint32_t> src((size_t)n * Z::PW), stage1((size_t)blocks * Z::TW), last(Z::TW), res(Z::PW);
  memcpy(src.data(), pts, (size_t)n * Z::PW * 4);
  sum_launch<CURVE, false>(src.data(), (uint32_t)n, blocks, stage1.data());
  sum_launch<CURVE, true>(stage1.data(), blocks, 1u, last.data());
  affine_pass<CURVE>(last.data(), 1u, res.data());
  memcpy(out, res.data(), Z::PW * 4);
}
}  // namespace

extern "C" {

// curve 0: 64-byte points, curve 1: 96-byte points; flags: TE_MSM_ADD_*
void ga_add_points(int curve, const uint8_t* a, const uint8_t* b, uint64_t n, int flags, int mistake, uint8_t* out) {
  if (curve == 1) add<1>(a, b, n, flags, mistake, out); else add<0>(a, b, n, flags, mistake, out);
}
void ga_sum_points(int curve, const uint8_t* pts, uint64_t n, uint32_t grid, uint8_t* out) {
  if (curve == 1) sum<1>(pts, n, grid, out); else sum<0>(pts, n, grid, out);
}
// te_msm_add_x's steps on the Twisted-Edwards curve for one pair: recovery of both (from_x_te), then the addition; the first reason code
int ga_add_x_te(const uint8_t* ax32, const uint8_t* bx32, int flags, uint8_t* out64) {
  uint32_t xa[8], xb[8], pa[16], pb[16];
  memcpy(xa, ax32, 32); memcpy(xb, bx32, 32);
  const int ra = from_x_te(xa, pa, kRootExpTe, kNafTeOrder), rb = from_x_te(xb, pb, kRootExpTe, kNafTeOrder);
  if (ra || rb) return ra ? ra : rb;
  add<0>(reinterpret_cast<const uint8_t*>(pa), reinterpret_cast<const uint8_t*>(pb), 1, flags, 0, out64);
  return 0;
}
// the check verdicts of these calls for one point: form reason (0 = passes), and 1 when it passes the subgroup level
int ga_check(int curve, const uint8_t* p, int* in_subgroup) {
  if (curve == 1) {
    uint32_t w[24]; memcpy(w, p, 96);
    *in_subgroup = ga_in_subgroup<1>(w, kNaf377Order) ? 1 : 0;
    return ga_check_form<1>(w);
  }
  uint32_t w[16]; memcpy(w, p, 64);
  *in_subgroup = ga_in_subgroup<0>(w, kNafTeOrder) ? 1 : 0;
  return ga_check_form<0>(w);
}

}
