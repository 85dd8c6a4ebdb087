// Batched MSMs over prefixes of one bound point set (te_msm_run_scalars_batch[_device], include/te_msm.h): which MSMs share a launch
// sequence, and which device runs which MSM.  Host code only (no HIP): tests/csrc/batchplan.cpp compiles it for the CPU tests.
//
// A sequence is what te_msm_partial_device_batch runs: the windows of all its MSMs are decomposed, sorted, accumulated and reduced as
// the windows of ONE launch sequence, over a digit-row stride of the sequence's LARGEST length (shorter MSMs pad their rows with digit
// 0, which no later stage reads).  The planner
//   - splits the MSMs over the devices (host form, several devices): longest first, each to the device with the least sum of lengths so
//     far (ties: the lower device).  The loads then differ by at most one MSM's length;
//   - per device: an MSM longer than `small_max` runs alone (a whole-MSM sequence; the engine keeps several of them in flight on its
//     work sets).  The others are grouped by length class floor(log2 len) -- the largest length of a sequence is below twice its
//     smallest, so the padding of the digit pass stays below half of it -- and every class is cut into as few sequences as the
//     limits allow, of near-equal size, MSMs in input order;
//   - per sequence: at most `seq_cap` MSMs (the kernarg table of the ragged digit kernel), at most `seq_bytes` of scratch (digits,
//     sort buffers, buckets and the fold buffers: what the work set must hold, whatever `count` is), windows x stride below 2^31
//     and segments below 2^32 (the 32-bit indices of the sort and the schedule);
//   - MSMs of length 0 run nowhere: their result is the identity.
// Deterministic: the plan depends on the lengths, the device count, the limits and the cost model only.
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <numeric>
#include <vector>

namespace te_batch {

#define TE_BATCH_SEQ_MAX 64    // MSMs of one shared launch sequence (kernels.hip.hpp, ragged_tab)

struct limits {
  uint64_t small_max = 1ull << 15;      // MSMs up to this length share sequences (option "batch_small_max")
  uint32_t seq_cap = TE_BATCH_SEQ_MAX;  // MSMs per shared sequence
  uint64_t seq_bytes = 1ull << 30;      // scratch budget of one sequence
};

// What ONE MSM adds to a sequence whose largest length is n, under the engine's plan for n (bases.hip, batch_cost)
struct msm_cost {
  uint64_t bytes = 0;        // scratch bytes
  uint64_t windows = 1;      // windows of its decomposition
  uint64_t stride = 8;       // digit-row stride (n rounded up to 8)
  uint64_t segments = 1;     // upper bound of its work segments (buckets + entries / segment length, all windows)
};
using cost_fn = std::function<msm_cost(uint64_t n)>;

struct sequence {
  int device = 0;
  bool shared = false;                // a sequence of small MSMs (false: one MSM longer than small_max)
  uint64_t n_max = 0;                 // its largest length: the plan's n
  std::vector<uint32_t> msms;         // indices into the caller's list
};

struct plan {
  std::vector<sequence> seqs;         // large ones first (longest first), then the shared ones (longest class first)
  std::vector<uint32_t> empty;        // MSMs of length 0
  std::vector<uint64_t> device_load;  // sum of the lengths per device
};

inline int length_class(uint64_t len) { int c = 0; while (len >> (c + 1)) c++; return c; }

// device of every MSM (longest-processing-time first: balanced within one MSM's length)
inline std::vector<int> split_devices(const uint64_t* lens, uint32_t count, int n_dev, std::vector<uint64_t>* load_out = nullptr) {
  std::vector<int> dev(count, 0);
  std::vector<uint64_t> load((size_t)std::max(n_dev, 1), 0);
  std::vector<uint32_t> idx(count);
  std::iota(idx.begin(), idx.end(), 0u);
  std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
  for (uint32_t i : idx) {
    if (!lens[i]) continue;
    size_t best = 0;
    for (size_t d = 1; d < load.size(); d++) if (load[d] < load[best]) best = d;
    dev[i] = (int)best; load[best] += lens[i];
  }
  if (load_out) *load_out = load;
  return dev;
}

// most MSMs one shared sequence of largest length n may hold
inline uint32_t seq_capacity(uint64_t n, const limits& lim, const cost_fn& cost) {
  const msm_cost c = cost(n);
  uint64_t cap = std::max<uint32_t>(1u, std::min<uint32_t>(lim.seq_cap, TE_BATCH_SEQ_MAX));
  if (c.bytes) cap = std::min<uint64_t>(cap, std::max<uint64_t>(1, lim.seq_bytes / c.bytes));
  const uint64_t cells = c.windows * c.stride;
  if (cells) cap = std::min<uint64_t>(cap, std::max<uint64_t>(1, ((1ull << 31) - 1) / cells));
  if (c.segments) cap = std::min<uint64_t>(cap, std::max<uint64_t>(1, ((1ull << 32) - 2048) / c.segments));
  return (uint32_t)cap;
}

inline plan make_plan(const uint64_t* lens, uint32_t count, int n_dev, const limits& lim, const cost_fn& cost) {
  plan P;
  if (n_dev < 1) n_dev = 1;
  const std::vector<int> dev = split_devices(lens, count, n_dev, &P.device_load);
  std::vector<uint32_t> large;
  for (uint32_t i = 0; i < count; i++) {
    if (!lens[i]) P.empty.push_back(i);
    else if (lens[i] > lim.small_max) large.push_back(i);
  }
  std::stable_sort(large.begin(), large.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
  for (uint32_t i : large) { sequence s; s.device = dev[i]; s.shared = false; s.n_max = lens[i]; s.msms.push_back(i); P.seqs.push_back(std::move(s)); }
  for (int d = 0; d < n_dev; d++) {
    for (int cls = 63; cls >= 0; cls--) {
      std::vector<uint32_t> members;
      for (uint32_t i = 0; i < count; i++)
        if (lens[i] && lens[i] <= lim.small_max && dev[i] == d && length_class(lens[i]) == cls) members.push_back(i);
      if (members.empty()) continue;
      uint64_t n_cls = 0;
      for (uint32_t i : members) n_cls = std::max(n_cls, lens[i]);
      const uint32_t cap = seq_capacity(n_cls, lim, cost);          // (the class's largest length: every sequence of it fits)
      const size_t k = members.size(), nseq = (k + cap - 1) / cap;
      for (size_t s = 0; s < nseq; s++) {
        const size_t lo = s * k / nseq, hi = (s + 1) * k / nseq;    // near-equal parts, each <= cap
        sequence q; q.device = d; q.shared = true;
        for (size_t j = lo; j < hi; j++) { q.msms.push_back(members[j]); q.n_max = std::max(q.n_max, lens[members[j]]); }
        P.seqs.push_back(std::move(q));
      }
    }
  }
  return P;
}

}  // namespace te_batch
