// Host build of the batch planner (webgpu-msm-twisted-edwards_amd/csrc/batch_plan.hpp) for tests/test_msm_batch_host.py, with a cost
// model of the engine's shape: W windows, a digit-row stride of n rounded up to 8, `cell_bytes` per digit cell plus `fixed_bytes`
// (buckets and fold buffers) per MSM, W * (n / 16 + 2^12) segments.
#include <cstring>

#include "../../webgpu-msm-twisted-edwards_amd/csrc/batch_plan.hpp"

namespace {
te_batch::cost_fn model(uint32_t windows, uint64_t cell_bytes, uint64_t fixed_bytes) {
  return [=](uint64_t n) {
    te_batch::msm_cost c;
    c.windows = windows; c.stride = (n + 7) & ~7ull;
    c.bytes = c.windows * c.stride * cell_bytes + fixed_bytes;
    c.segments = c.windows * (n / 16 + 4096);
    return c;
  };
}
}  // namespace

extern "C" {
// Plans `count` MSMs.  Returns the number of sequences (or -1 when more than max_seqs); seq_size / seq_dev / seq_nmax / seq_shared receive
// one entry per sequence, members their MSM indices one after another; empty the MSMs of length 0 (n_empty of them); load the sum of
// lengths per device; msm_bytes the model's bytes of one MSM of each sequence's largest length.
int bp_plan(const uint64_t* lens, uint32_t count, int n_dev, uint64_t small_max, uint32_t seq_cap, uint64_t seq_bytes, uint32_t windows,
            uint64_t cell_bytes, uint64_t fixed_bytes, int max_seqs, uint32_t* seq_size, int32_t* seq_dev, uint64_t* seq_nmax, int32_t* seq_shared,
            uint64_t* msm_bytes, uint32_t* members, uint32_t* empty, uint32_t* n_empty, uint64_t* load) {
  te_batch::limits lim;
  lim.small_max = small_max; lim.seq_cap = seq_cap; lim.seq_bytes = seq_bytes;
  const te_batch::cost_fn cost = model(windows, cell_bytes, fixed_bytes);
  const te_batch::plan P = te_batch::make_plan(lens, count, n_dev, lim, cost);
  if ((int)P.seqs.size() > max_seqs) return -1;
  size_t at = 0;
  for (size_t s = 0; s < P.seqs.size(); s++) {
    const te_batch::sequence& q = P.seqs[s];
    seq_size[s] = (uint32_t)q.msms.size(); seq_dev[s] = q.device; seq_nmax[s] = q.n_max; seq_shared[s] = q.shared ? 1 : 0;
    msm_bytes[s] = cost(q.n_max).bytes;
    for (uint32_t m : q.msms) members[at++] = m;
  }
  *n_empty = (uint32_t)P.empty.size();
  for (size_t i = 0; i < P.empty.size(); i++) empty[i] = P.empty[i];
  for (size_t d = 0; d < P.device_load.size(); d++) load[d] = P.device_load[d];
  return (int)P.seqs.size();
}
int bp_length_class(uint64_t len) { return te_batch::length_class(len); }
int bp_seq_max(void) { return TE_BATCH_SEQ_MAX; }
}
