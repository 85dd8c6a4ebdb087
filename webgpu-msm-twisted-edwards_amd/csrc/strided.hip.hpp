// strided.hip.hpp -- input points at a record stride (options "point_stride" / "point_infinity_flag", include/te_msm.h): how the bind-time
// conversions (kernels.hip.hpp) and the point checks (check.hip.hpp) read a caller's records in place.  Point i starts at byte i * stride;
// x and y are its first 2 x 32 / 2 x 48 bytes; with the flag option the byte at offset 96 says "point at infinity"; nothing else of the
// record is interpreted.  The stride is a multiple of 8 and need not be one of 16 (arkworks' G1Affine: 104), so no 16-byte load is issued
// from the caller's buffer.
//
// Lanes reading their own record at a 104-byte stride would issue, per load instruction, 64 requests 104 bytes apart.  Instead a block of
// 256 threads reads the tile of its 256 records as ONE contiguous run of 8-byte words -- word g of the run by thread g mod 256, so every
// load instruction of a wave covers 512 consecutive bytes -- into LDS, and each lane picks its coordinates from there.  The tile is at most
// 256 x TE_STRIDE_MAX = 32 KB, which is why the stride is capped at 128: a larger record would need a smaller tile or dynamic LDS for
// padding no known prover has.  LDS reads of the pick: lane t reads 8-byte words at t * stride / 8; at stride 104 (13 words) consecutive
// lanes are 26 banks apart, a two-way conflict at worst -- a dozen reads per point in kernels that spend hundreds of field products on it.
//
// The arithmetic (tile extent, pick) is host-compilable: tests/csrc/layoutcheck.cpp runs it against the bigint model and replays its
// addresses.
#pragma once
#include <stdint.h>
#include <stddef.h>

#ifndef TE_HD
#if defined(__HIPCC__)
#define TE_HD __host__ __device__ __forceinline__
#else
#define TE_HD inline
#endif
#endif

namespace te {

#define TE_STRIDE_MAX 128u
#define TE_STRIDE_TILE 256u      // records of one block's tile = threads of the block

// the block's tile: records [blk * 256, min(n, blk * 256 + 256)) as 8-byte words [first, first + words) of the caller's buffer
TE_HD uint64_t strided_tile_first(uint32_t blk, uint32_t stride) { return (uint64_t)blk * TE_STRIDE_TILE * (stride / 8u); }
TE_HD uint32_t strided_tile_count(uint32_t blk, uint32_t n) { const uint32_t base = blk * TE_STRIDE_TILE; return n - base < TE_STRIDE_TILE ? n - base : TE_STRIDE_TILE; }
TE_HD uint32_t strided_tile_words(uint32_t blk, uint32_t n, uint32_t stride) { return strided_tile_count(blk, n) * (stride / 8u); }

// record t of the tile: its first PW 32-bit words (x || y); returns the flag byte (offset 4 PW = 96: BLS12-377 only) or 0 without the option
template <int PW> TE_HD uint32_t strided_pick(const uint64_t* tile, uint32_t t, uint32_t stride, uint32_t (&w)[PW], bool flag) {
  const uint64_t* r = tile + (size_t)t * (stride / 8u);
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int j = 0; j < PW / 2; j++) { const uint64_t v = r[j]; w[2 * j] = (uint32_t)v; w[2 * j + 1] = (uint32_t)(v >> 32); }
  return flag ? (uint32_t)(r[PW / 2] & 0xffu) : 0u;
}

#if defined(__HIPCC__)
// every thread of the 256-thread block; the tile is complete behind the barrier
__device__ __forceinline__ void strided_stage(uint64_t* __restrict__ tile, const uint64_t* __restrict__ src, uint32_t blk, uint32_t n, uint32_t stride) {
  const uint32_t words = strided_tile_words(blk, n, stride);
  const uint64_t* __restrict__ from = src + strided_tile_first(blk, stride);
  for (uint32_t g = threadIdx.x; g < words; g += TE_STRIDE_TILE) tile[g] = from[g];
  __syncthreads();
}
#endif

}  // namespace te
