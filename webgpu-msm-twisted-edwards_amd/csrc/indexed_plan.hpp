// MSMs over an indexed subset of a bound point set (te_msm_run_scalars_indexed*, include/te_msm.h): what the plan is made for, which
// form the sort's level-1 entries take, and how the m (index, scalar) pairs are cut into upload pieces and device slices.  Host code
// only (no HIP): tests/csrc/indexedplan.cpp compiles it for the CPU tests.
//
// The call is sum_{j < m} k_j P_{idx[j]} over a bound set of `count` records.  Entry j's scalar is record j of the call, so the digit
// pass, the sort and the schedule run over m entries and everything sized "from n" -- window bits, segment length, chunks, buffers --
// is sized from m, whatever the set holds.  The one thing that follows the SET is the entry form: a packed level-1 word gives the index
// 23 bits, and in this call the field holds a point index (below count), not a position (below m).
#pragma once

#include <cstddef>
#include <cstdint>

namespace te_indexed {

constexpr uint64_t kPackedIndexLimit = 1ull << 23;     // records a packed entry can address (kernels.hip.hpp, sort_geom::packed)

// What the engine's planner (te_msm.hip: make_plan calls this with plan_req::idx_count; a call that is not indexed is its own set,
// count = entries) takes for one launch sequence of `entries` pairs
struct call_plan {
  uint64_t plan_n;     // the "n" every size of the plan derives from: the entries of the sequence
  uint32_t packed;     // level-1 entries as one word: option "packed_sort" and count <= 2^23, whatever m is
};
inline call_plan plan_for(uint64_t entries, uint64_t count, int opt_packed) {
  return call_plan{entries, (opt_packed && count <= kPackedIndexLimit) ? 1u : 0u};
}

// pieces the scalars (or pairs) of one device are uploaded and processed in over a bound point set, indexed or not (te_msm.hip,
// scalar_pieces): option "scalar_chunks", else from m; never more pieces than pairs, never fewer than one
inline int pieces(uint64_t m, int opt_scalar_chunks) {
  int K = opt_scalar_chunks ? opt_scalar_chunks : (m >= (3ull << 18) ? 3 : m >= (1ull << 18) ? 2 : 1);
  if ((uint64_t)K > m) K = (int)m;
  return K < 1 ? 1 : K;
}
// first pair of piece i of K (i >= K: m): the pieces tile [0, m) and differ by at most one pair.  The one boundary rule of every
// host-buffer form (te_msm.hip, enqueue_host_pieces), host points included
inline uint64_t piece_lo(uint64_t m, int K, int i) {
  return i >= K ? m : (uint64_t)(((unsigned __int128)m * (unsigned)i) / (unsigned)K);
}

// devices a host-form call uses: as many as hold at least `shard_min` pairs each (option "host_shard_min"), at least one
inline size_t devices_for(uint64_t m, size_t n_dev, uint64_t shard_min) {
  if (shard_min < 1) shard_min = 1;
  uint64_t D = m / shard_min;
  if (D > n_dev) D = n_dev;
  return (size_t)(D < 1 ? 1 : D);
}
// first pair of device i's slice (i >= D: m): contiguous slices of floor(m / D) or ceil(m / D) pairs -- none empty while m >= D, none
// below shard_min when D came from devices_for
inline uint64_t slice_lo(uint64_t m, size_t D, size_t i) {
  return i >= D ? m : (uint64_t)(((unsigned __int128)m * i) / D);
}
// the largest slice: every slice's rows share the window bits planned for it
inline uint64_t slice_max(uint64_t m, size_t D) { return (m + D - 1) / D; }

}  // namespace te_indexed
