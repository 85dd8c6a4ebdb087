// Host build of csrc/plan_arith.hpp for tests/test_narrow_scalars_host.py: the windows of a decomposition under a declared scalar
// width (te_plan::windows_for, the rule make_plan, te_msm_plan and the batch cost function share), and the loads the digit kernels
// issue for one pair of scalar records: te_plan::loads_of_pair, which digits_block_narrow calls.  For 32- / 48-byte records it is a
// RESTATEMENT: digits_block, whose instantiations keep their code, spells its own clamp and loads and does not call it.
#include "../../webgpu-msm-twisted-edwards_amd/csrc/plan_arith.hpp"

extern "C" {

void np_windows(int c0, int signed_digits, int bits, int* c, int* W) {
  const te_plan::windows w = te_plan::windows_for(c0, signed_digits, bits);
  *c = w.c; *W = w.W;
}

// the loads of the pair (i0, i0 + 1) of a slice of n records of `rec` bytes: byte offsets from the slice's first record and sizes; returns their count
int np_loads(uint32_t rec, uint32_t i0, uint32_t n, int base16, uint64_t at[6], uint32_t bytes[6]) {
  const te_plan::pair_loads L = te_plan::loads_of_pair(rec, i0, n, base16 != 0);
  for (int k = 0; k < L.count; k++) { at[k] = L.at[k]; bytes[k] = L.bytes[k]; }
  return L.count;
}

// the clamped records of the pair (digits_block's own min() pair)
void np_pair(uint32_t i0, uint32_t n, uint32_t* ia, uint32_t* ib) {
  const te_plan::record_pair r = te_plan::pair_records(i0, n);
  *ia = r.ia; *ib = r.ib;
}

}
