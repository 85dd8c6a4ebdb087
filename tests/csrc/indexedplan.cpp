// Host build of csrc/indexed_plan.hpp for tests/test_msm_indexed_host.py: what the plan of an indexed MSM is made for, the packed
// rule, the upload pieces and the device slices.
#include "../../webgpu-msm-twisted-edwards_amd/csrc/indexed_plan.hpp"

extern "C" {

// plan_n and packed for `entries` pairs over a set of `count` records
void ip_plan(uint64_t entries, uint64_t count, int opt_packed, uint64_t* plan_n, uint32_t* packed) {
  const te_indexed::call_plan p = te_indexed::plan_for(entries, count, opt_packed);
  *plan_n = p.plan_n; *packed = p.packed;
}
int ip_pieces(uint64_t m, int opt_scalar_chunks) { return te_indexed::pieces(m, opt_scalar_chunks); }
uint64_t ip_piece_lo(uint64_t m, int K, int i) { return te_indexed::piece_lo(m, K, i); }
uint64_t ip_devices_for(uint64_t m, uint64_t n_dev, uint64_t shard_min) { return te_indexed::devices_for(m, (size_t)n_dev, shard_min); }
uint64_t ip_slice_lo(uint64_t m, uint64_t D, uint64_t i) { return te_indexed::slice_lo(m, (size_t)D, (size_t)i); }
uint64_t ip_slice_max(uint64_t m, uint64_t D) { return te_indexed::slice_max(m, (size_t)D); }
uint64_t ip_packed_limit(void) { return te_indexed::kPackedIndexLimit; }

}
