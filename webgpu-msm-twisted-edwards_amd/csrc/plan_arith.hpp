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

// ---- the windows of a decomposition (options "window_bits", "signed_digits", "scalar_bits") ----------------------------------------
// c0: the window size the plan would choose without a declared width (option "window_bits", or the size chosen from n).  bits = b: the
// caller declared every scalar below 2^b (0: nothing declared -- the full-width rule: 253 bits for signed digits, whose windows reach
// bit 254, and all 256 bits of a record for unsigned ones).
//   W = ceil((b + g) / c0), g = 2 for signed digits and 0 for unsigned ones, and c = c0.
// (Shrinking c to the smallest size with that window count, max(4, ceil((b + g) / W)) -- as many accumulated entries, fewer buckets to
// reduce -- was measured (the narrow_shrunk column): 19 to 56 % slower than keeping c0 at n = 2^20 and never faster at 2^16
// (profiles/narrow_scalars_cost.txt).  A caller who wants it sets "window_bits".)
// Signed digits accept exactly s < 2^(cW) - half with half = sum_{w < W} 2^(cw + c - 1) < 2^(cW - 1) (1 + 2^(1 - c)) <= 2^(cW - 1) 9/8
// (c >= 4): c W >= b + 2 leaves 2^(cW) - half > 2^(cW - 2) 7/4 > 2^b, and c W = b + 1 does not (half > 2^(cW - 1) = 2^b).
struct windows { int c, W; };
TE_HD windows windows_for(int c0, int signed_digits, int bits) {
  const int x = (bits > 0 ? bits : signed_digits ? 253 : 256) + (signed_digits ? 2 : 0);
  windows r;
  r.W = (x + c0 - 1) / c0;
  r.c = c0;
  return r;
}

// ---- which scalar records the digit kernels load (kernels.hip.hpp: digits_block_narrow; digits_block spells the same clamp itself) ---
// A thread decomposes the pair of records i0 (even) and i0 + 1 of its MSM's n >= 1 records.  The loads are unconditional, so the indices
// are clamped into the slice: a pair that has no second record (odd n) or no record at all (the padding of the digit rows) reads the
// last record again and never a byte at or beyond n records.
struct record_pair { uint32_t ia, ib; };
TE_HD record_pair pair_records(uint32_t i0, uint32_t n) {
  record_pair r;
  r.ia = i0 < n - 1u ? i0 : n - 1u;
  r.ib = i0 + 1u < n - 1u ? i0 + 1u : n - 1u;
  return r;
}
// The loads of one pair as byte offsets from the first record of the MSM's slice.  Wide records (32 / 48 bytes): 16-byte loads, REC / 16
// per record.  16-byte records: one 16-byte load each.  8-byte records: both records in ONE 16-byte load where the slice starts on a
// 16-byte boundary (base16: i0 is even, so record i0 does too) and the second record exists -- else one 8-byte load each (the packed
// buffer of a batch call starts MSM m at record sum lens[j]: an odd offset is 8-byte aligned only).
struct pair_loads { uint64_t at[6]; uint32_t bytes[6]; int count; };
TE_HD pair_loads loads_of_pair(uint32_t rec, uint32_t i0, uint32_t n, bool base16) {
  pair_loads L; L.count = 0;
  const record_pair r = pair_records(i0, n);
  if (rec == 8u && base16 && i0 + 1u < n) { L.at[0] = 8ull * i0; L.bytes[0] = 16u; L.count = 1; return L; }
  const uint32_t unit = rec < 16u ? rec : 16u, per = rec / unit;
  for (uint32_t k = 0; k < per; k++) { L.at[L.count] = (uint64_t)rec * r.ia + 16u * k; L.bytes[L.count] = unit; L.count++; }
  for (uint32_t k = 0; k < per; k++) { L.at[L.count] = (uint64_t)rec * r.ib + 16u * k; L.bytes[L.count] = unit; L.count++; }
  return L;
}

}  // namespace te_plan
