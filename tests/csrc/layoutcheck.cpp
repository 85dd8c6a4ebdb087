// layoutcheck.cpp -- TEST SHIM: the strided bind-time conversion (csrc/strided.hip.hpp's tile extent and pick, csrc/curve.hpp's
// pnt_from_sw377 / pnt_from_affine_raw / pnt_identity377) compiled for the host, block by block and lane by lane as
// k_prep_points377_strided / k_prep_points_strided run it, so tests/test_native_layout_host.py can compare the records with bigints and
// see every address the loader forms.  Not part of the product; not a fallback.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/curve.hpp"
#include "../../webgpu-msm-twisted-edwards_amd/csrc/strided.hip.hpp"

using namespace te;

namespace {
// strided_stage as the 256 threads of block blk run it; false = a load would leave [0, n * stride) or the tile
bool stage(std::vector<uint64_t>& tile, const uint8_t* src, uint32_t blk, uint32_t n, uint32_t stride, uint64_t* max_end) {
  const uint32_t words = strided_tile_words(blk, n, stride);
  const uint64_t first = strided_tile_first(blk, stride);
  for (uint32_t t = 0; t < TE_STRIDE_TILE; t++)
    for (uint32_t g = t; g < words; g += TE_STRIDE_TILE) {
      const uint64_t at = 8u * (first + g);
      if (at + 8u > (uint64_t)n * stride || g >= tile.size()) return false;
      if (at + 8u > *max_end) *max_end = at + 8u;
      memcpy(&tile[g], src + at, 8);
    }
  return true;
}
}  // namespace

extern "C" {

// n BLS12-377 records at `stride` -> n projective records hm | hp | dt | z (56 limb words each).  flag: the byte at offset 96, non-zero =
// infinity.  Returns the end of the highest byte loaded, or -1 when a load left the buffer.
int64_t lc_convert377(const uint8_t* src, uint32_t n, uint32_t stride, int mont, int flag, uint32_t* out) {
  std::vector<uint64_t> tile(TE_STRIDE_TILE * TE_STRIDE_MAX / 8u);
  uint64_t max_end = 0;
  for (uint32_t blk = 0; blk * TE_STRIDE_TILE < n; blk++) {
    if (!stage(tile, src, blk, n, stride, &max_end)) return -1;
    for (uint32_t t = 0; t < strided_tile_count(blk, n); t++) {
      uint32_t w[24], xw[12], yw[12];
      const uint32_t inf = strided_pick<24>(tile.data(), t, stride, w, flag != 0);
      for (int j = 0; j < 12; j++) { xw[j] = w[j]; yw[j] = w[12 + j]; }
      const fel<14> x = te377::fq_from_words32(xw), y = te377::fq_from_words32(yw);
      const pnt_t<14> conv = mont ? pnt_from_sw377<true>(x, y) : pnt_from_sw377<false>(x, y);
      const pnt_t<14> r = inf ? pnt_identity377() : conv;
      uint32_t* o = out + (size_t)(blk * TE_STRIDE_TILE + t) * 56;
      for (int j = 0; j < 14; j++) { o[j] = r.hm.v[j]; o[14 + j] = r.hp.v[j]; o[28 + j] = r.dt.v[j]; o[42 + j] = r.z.v[j]; }
    }
  }
  return (int64_t)max_end;
}

// n Twisted-Edwards records at `stride` -> n records hm | hp | dt (27 limb words each)
int64_t lc_convert_te(const uint8_t* src, uint32_t n, uint32_t stride, int mont, uint32_t* out) {
  std::vector<uint64_t> tile(TE_STRIDE_TILE * TE_STRIDE_MAX / 8u);
  uint64_t max_end = 0;
  for (uint32_t blk = 0; blk * TE_STRIDE_TILE < n; blk++) {
    if (!stage(tile, src, blk, n, stride, &max_end)) return -1;
    for (uint32_t t = 0; t < strided_tile_count(blk, n); t++) {
      uint32_t w[16], xw[8], yw[8];
      (void)strided_pick<16>(tile.data(), t, stride, w, false);
      for (int j = 0; j < 8; j++) { xw[j] = w[j]; yw[j] = w[8 + j]; }
      const pnt r = mont ? pnt_from_affine_raw<true>(fp_from_words32(xw), fp_from_words32(yw)) : pnt_from_affine_raw<false>(fp_from_words32(xw), fp_from_words32(yw));
      uint32_t* o = out + (size_t)(blk * TE_STRIDE_TILE + t) * 27;
      for (int j = 0; j < 9; j++) { o[j] = r.hm.v[j]; o[9 + j] = r.hp.v[j]; o[18 + j] = r.dt.v[j]; }
    }
  }
  return (int64_t)max_end;
}

}  // extern "C"
