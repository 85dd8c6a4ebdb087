// The two pieces of plan arithmetic that every launch sequence shares, whatever its "windows" are: the level-1 chunks of a row and the
// default segment length.  te_msm.hip (make_plan: rows = the windows of the sequence) and fb_plan.hpp (make_geometry: rows = the
// pseudo-windows of a fixed-base plan) both call them.  HIP-free: the host shims of the CPU tests compile it through fb_plan.hpp.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#ifndef TE_HD
#define TE_HD __host__ __device__ __forceinline__
#endif
#else
#ifndef TE_HD
#define TE_HD inline
#endif
#endif

namespace te_plan {

struct chunking {
  uint32_t asked;              // chunks per row asked for (before the rounding to whole tiles)
  uint32_t nst;                // padded row stride: n rounded up to 8 entries
  uint32_t chunk_len, CH;      // entries per chunk (whole 4096-entry tiles), chunks per row
};
// Level-1 chunks of `rows` rows of n entries each: scatter_blocks blocks of k_part_scatter over all rows (~4 blocks of 512 threads per
// CU), at most 256 chunks per row and at least one tile of min_chunk digits per chunk.  rows = 0: one chunk.
TE_HD chunking chunks_for(uint32_t rows, uint64_t n, uint32_t scatter_blocks, uint32_t min_chunk) {
  chunking k;
  uint32_t ch = rows > 0 ? scatter_blocks / rows : 1u;
  if (ch < 1) ch = 1;
  if (ch > 256) ch = 256;
  const uint32_t by_n = (uint32_t)((n + min_chunk - 1) / min_chunk);
  if (ch > by_n) ch = by_n ? by_n : 1;
  k.asked = ch;
  k.nst = (uint32_t)((n + 7) & ~(uint64_t)7);
  k.chunk_len = ((k.nst + ch - 1) / ch + 4095u) & ~4095u;
  k.CH = (k.nst + k.chunk_len - 1) / k.chunk_len;
  return k;
}

// Default segment length: twice the mean bucket size -- `entries` entries over `buckets` buckets -- as a power of two in [16, 64].
TE_HD uint32_t default_seg_len(uint64_t entries, uint64_t buckets) {
  const uint64_t a = (2 * entries + buckets - 1) / buckets;
  uint64_t s2 = 16;
  while (s2 < a && s2 < 64) s2 <<= 1;
  return (uint32_t)s2;
}

}  // namespace te_plan
