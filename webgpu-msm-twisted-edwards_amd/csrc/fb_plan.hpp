// Fixed-base windows over a bound point set (option "bind_fixed_base" = c, kernels.hip.hpp "FIXED-BASE WINDOWS"): the arithmetic of
// the plan (te_msm.hip, make_plan_fb / enqueue_fixed_base call it) and the digit walk as a function.  HIP-free: tests/csrc/fbcheck.cpp
// compiles it for the CPU tests (tests/test_fixed_base_host.py), where it is compared with a model in Python integers.
// k_fb_digits keeps its own two extractions (phases A and B): calling digit() from the kernel cost every instantiation 6 to 11 VGPRs,
// 9 to 14 SGPRs and 1.3 to 1.5 % more instructions on gfx950.  The shim restates both extractions line for line and the host test
// holds each of them against digit() and the model, so the three texts cannot drift apart unnoticed.
//
// A scalar k < 2^(W c - 1) is walked in W = ceil(255 / c) signed windows: with half = sum_w 2^(c w + c - 1), window w of s = k + half
// holds d_w + 2^(c-1), d_w in [-2^(c-1), 2^(c-1)), and k = sum_w d_w 2^(c w); what s holds at bit W c and above is the final carry
// (a scalar the walk cannot represent).  A non-zero digit is an entry of bucket b = |d| - 1, cut into (hb | lo : 15 bits); entries of
// equal hb form a row, except the top window's entries with hb = 0, which go to the extra row rb.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "plan_arith.hpp"      // TE_HD; the chunks of a row and the default segment length, shared with make_plan

namespace te_fb {

constexpr uint32_t kLoBits = 15u;                // bucket bits of a row (kernels.hip.hpp, TE_FB_LOBITS)
constexpr int kMinBits = 16, kMaxBits = 21;      // option "bind_fixed_base"

TE_HD int windows_for(int c) { return (255 + c - 1) / c; }
TE_HD uint32_t regular_rows(int c) { return 1u << ((uint32_t)c - 1u - kLoBits); }

// ---- the plan of an MSM of n scalars with window bits c, as far as it is arithmetic
struct geometry {
  int W;                       // windows of the decomposition
  uint32_t rb, rows;           // regular rows (one per hb), rows = rb + 1 with the extra row
  uint64_t reg;                // entries of a regular row for well-spread digits: ceil((W - 1) n / rb)
  uint64_t cap;                // entries a row can hold = row stride of the digit / remap buffers
  uint32_t chunks;             // chunks per row asked for (before the rounding to whole tiles)
  uint32_t chunk_len, CH;      // entries per chunk (whole 4096-entry tiles), chunks per row
  uint32_t S, P, logS;         // buckets per level-1 partition, partitions per row
  uint32_t seg_len;            // default segment length: twice the mean bucket size of the ONE bucket set, a power of two in [16, 64]
  uint32_t half[10];           // sum_w 2^(c w + c - 1) over the W windows
  size_t lds_bytes;            // dynamic LDS of k_fb_digits: cnt[rows] | base[rows] | hist[rows][2][P]
};
// scatter_blocks, min_chunk: TE_SCATTER_BLOCKS and TE_SCATTER_MINCHUNK of te_msm.hip
TE_HD geometry make_geometry(uint64_t n, int c, uint32_t scatter_blocks = 1024u, uint32_t min_chunk = 4096u) {
  geometry g;
  g.W = windows_for(c);
  g.rb = regular_rows(c); g.rows = g.rb + 1u;
  // a regular row holds (W - 1) n / rb entries for well-spread digits, the extra row the top window's n: capacity for the larger of
  // the two plus a sixteenth (an overflow -- badly skewed scalars -- is detected on the device and falls back to the ordinary windows)
  g.reg = ((uint64_t)(g.W - 1) * n + g.rb - 1) / g.rb;
  const uint64_t big = g.reg > n ? g.reg : n;
  g.cap = (big + big / 16 + 4096 + 7) & ~(uint64_t)7;
  // chunks per row: make_plan's rule for rows of `cap` entries (cap is a multiple of 8: the row stride is cap itself)
  const te_plan::chunking k = te_plan::chunks_for(g.rows, g.cap, scatter_blocks, min_chunk);
  g.chunks = k.asked; g.chunk_len = k.chunk_len; g.CH = k.CH;
  g.S = 256u; g.P = (1u << kLoBits) / g.S; g.logS = 8u;
  g.seg_len = te_plan::default_seg_len((uint64_t)g.W * n, (uint64_t)g.rb << kLoBits);     // W n entries over the ONE bucket set
  for (int j = 0; j < 10; j++) g.half[j] = 0u;
  for (int w = 0; w < g.W; w++) { const int bit = w * c + c - 1; if (bit < 320) g.half[bit >> 5] |= 1u << (bit & 31); }
  g.lds_bytes = (size_t)(2u * g.rows + g.rows * 2u * g.P) * sizeof(uint32_t);
  return g;
}
// the two refusals "windows x points must stay below 2^31", as te_msm_bind_points (bases.hip) and enqueue_fixed_base (te_msm.hip) call them: of a
// bind, and of an MSM over the set
TE_HD bool bind_refused(int c, uint64_t n_table) { return (uint64_t)windows_for(c) * n_table >= (1ull << 31); }
TE_HD bool msm_refused(const geometry& g, uint64_t n_table) { return (uint64_t)g.rows * g.cap >= (1ull << 31) || (uint64_t)g.W * n_table >= (1ull << 31); }

// ---- the digit walk
// s = raw + half over ten 32-bit words (raw[8], raw[9] = 0 for a 256-bit scalar)
TE_HD void add_half(const uint32_t raw[10], const uint32_t half[10], uint32_t s[10]) {
  uint64_t c = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int j = 0; j < 10; j++) { c += (uint64_t)raw[j] + half[j]; s[j] = (uint32_t)c; c >>= 32; }
}
enum { DIGIT_NONE = 0, DIGIT_ENTRY = 1, DIGIT_CARRY = 2 };
struct entry { uint32_t row, lo; bool neg; };      // the entry's row, its code is lo + 1; neg: the digit is negative
// window w of s for window bits C: DIGIT_NONE (a zero digit, or no bits left: C w >= 320), DIGIT_ENTRY with e filled, or DIGIT_CARRY:
// w >= W and the bits are not zero (the final carry: the scalar is out of the walk's range)
template <int C> TE_HD int digit(const uint32_t s[10], int w, uint32_t W, uint32_t rb, entry& e) {
  const int bit = w * C;
  if (bit >= 320) return DIGIT_NONE;
  const int word = bit >> 5, off = bit & 31;
  uint32_t v = s[word] >> off;
  if (off + C > 32 && word + 1 < 10) v |= s[word + 1] << (32 - off);
  v &= (1u << C) - 1u;
  if ((uint32_t)w >= W) return v != 0u ? DIGIT_CARRY : DIGIT_NONE;
  const int d = (int)v - (1 << (C - 1));
  if (d == 0) return DIGIT_NONE;
  const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u, hb = b >> kLoBits;
  e.lo = b & ((1u << kLoBits) - 1u);
  e.row = ((uint32_t)w + 1u == W && hb == 0u) ? rb : hb;
  e.neg = d < 0;
  return DIGIT_ENTRY;
}
// the same for a run-time c in [kMinBits, kMaxBits] (host callers)
inline int digit_c(int c, const uint32_t s[10], int w, uint32_t W, uint32_t rb, entry& e) {
  switch (c) {
    case 16: return digit<16>(s, w, W, rb, e);
    case 17: return digit<17>(s, w, W, rb, e);
    case 18: return digit<18>(s, w, W, rb, e);
    case 19: return digit<19>(s, w, W, rb, e);
    case 20: return digit<20>(s, w, W, rb, e);
    default: return digit<21>(s, w, W, rb, e);
  }
}

}  // namespace te_fb
