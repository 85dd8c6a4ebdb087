// devcheck.hip -- TEST SHIM: the gfx950 build of the operation table (devcheck_ops.hpp, one element per lane) and direct launches
// of the device-only code of csrc/kernels.hip.hpp -- the DPP team addition, the block-wide sum, the three fold kernels and the
// reduction tail -- on operands a test chooses.  Built with the HIPCC / ARCH / CXXFLAGS of csrc/Makefile (tests/devcheck.py), so
// what runs is the product's own code generation.  Every entry point takes device pointers, launches on the null stream,
// synchronises and returns the HIP error code (0 = success; -1 = the arguments would read or write outside the buffers, nothing
// was launched).  Lanes beyond the last element clamp their index and do not store; none returns before the DPP exchanges.
// Not part of the product; not a fallback.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <string.h>
#include <algorithm>
#include "../../webgpu-msm-twisted-edwards_amd/csrc/kernels.hip.hpp"
#include "devcheck_ops.hpp"

namespace {

int finish() {
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipDeviceSynchronize();
  return (int)e;
}

// ---- the table, one element per lane
#define X(name, fn, IW, OW)                                                                                                 \
  __global__ void __launch_bounds__(256) k_dc_##name(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n) { \
    const uint32_t gt = blockIdx.x * 256u + threadIdx.x, i = min(gt, n - 1u);                                               \
    uint32_t a[IW], r[OW];                                                                                                  \
    _Pragma("unroll") for (int j = 0; j < IW; j++) a[j] = in[(size_t)i * IW + j];                                           \
    fn(a, r);                                                                                                               \
    if (gt < n) { _Pragma("unroll") for (int j = 0; j < OW; j++) out[(size_t)i * OW + j] = r[j]; }                          \
  }
DC_OPS(X)
#undef X

// ---- ete_add_team: one quad per operand pair, lane q of the quad holds coordinate q of (X, Y, T, Z)
template <int N>
__global__ void __launch_bounds__(256) k_dc_add_team(const te::ete_t<N>* __restrict__ a, const te::ete_t<N>* __restrict__ b, te::ete_t<N>* __restrict__ out, uint32_t n) {
  const uint32_t gt = blockIdx.x * 256u + threadIdx.x, g = gt >> 2, q = gt & 3u, i = min(g, n - 1u), w = te::team_word<N>(q);
  const te::fel<N> m1 = te::load_coord<N>(te::words<N>(a + i) + w), m2 = te::load_coord<N>(te::words<N>(b + i) + w);
  const te::fel<N> r = te::ete_add_team<N>(m1, m2, q);
  if (g < n) te::store_coord<N>(te::words<N>(out + i) + w, r);
}
template <int N> int add_team(const void* a, const void* b, void* out, uint32_t n) {
  if (n == 0) return 0;
  using E = te::ete_t<N>;
  hipLaunchKernelGGL(k_dc_add_team<N>, dim3((4u * n + 255u) / 256u), dim3(256), 0, 0, static_cast<const E*>(a), static_cast<const E*>(b), static_cast<E*>(out), n);
  return finish();
}

// ---- block_sum_points: block j sums the cnt points src[first], src[first + stride], ... into out[j]
constexpr uint32_t DC_SUM_JOBS = 32;
struct sum_list { uint32_t first[DC_SUM_JOBS], stride[DC_SUM_JOBS], cnt[DC_SUM_JOBS]; };
template <int N, bool COHERENT>
__global__ void __launch_bounds__(256) k_dc_block_sum(const te::ete_t<N>* __restrict__ src, sum_list jobs, te::ete_t<N>* __restrict__ out) {
  __shared__ uint32_t lds[64 * te::geo<N>::PW];
  const uint32_t j = blockIdx.x;
  const te::fel<N> r = te::block_sum_points<N, COHERENT>(src + jobs.first[j], jobs.stride[j], jobs.cnt[j], lds);
  if ((threadIdx.x >> 2) == 0) te::store_coord<N>(te::words<N>(out + j) + te::team_word<N>(threadIdx.x & 3u), r);
}
template <int N> int block_sum(int coherent, const void* src, uint64_t src_points, const uint32_t* first, const uint32_t* stride, const uint32_t* cnt, uint32_t njobs, void* out) {
  if (njobs == 0) return 0;
  if (njobs > DC_SUM_JOBS) return -1;
  sum_list jobs; memset(&jobs, 0, sizeof jobs);
  for (uint32_t j = 0; j < njobs; j++) {
    if (cnt[j] == 0 || stride[j] == 0 || (uint64_t)first[j] + (uint64_t)(cnt[j] - 1u) * stride[j] >= src_points) return -1;
    jobs.first[j] = first[j]; jobs.stride[j] = stride[j]; jobs.cnt[j] = cnt[j];
  }
  using E = te::ete_t<N>;
  if (coherent) hipLaunchKernelGGL((k_dc_block_sum<N, true>), dim3(njobs), dim3(256), 0, 0, static_cast<const E*>(src), jobs, static_cast<E*>(out));
  else hipLaunchKernelGGL((k_dc_block_sum<N, false>), dim3(njobs), dim3(256), 0, 0, static_cast<const E*>(src), jobs, static_cast<E*>(out));
  return finish();
}

// ---- the fold kernels, launched as reduce_t of te_msm.hip launches them.  form 0: k_sum_groups<N, false> (a thread per output),
// 1: k_sum_groups<N, true> (a pair), 2: k_sum_groups_team<N> (a quad)
template <int N> int sum_groups(int form, const void* in, uint64_t in_points, void* out, uint64_t out_points, uint32_t n_out, uint32_t K, uint32_t inner,
                                uint32_t in_per_window, uint32_t out_per_window, uint32_t nw) {
  if (form < 0 || form > 2 || (K != 2u && K != 4u && K != 8u) || inner == 0 || n_out == 0 || nw == 0) return -1;
  // output o reads  ((o / inner) * K + t) * inner + o % inner,  t < K
  const uint64_t in_span = ((uint64_t)(n_out - 1u) / inner + 1u) * K * inner;
  if (in_span > in_per_window || (uint64_t)(nw - 1u) * in_per_window + in_span > in_points) return -1;
  if (n_out > out_per_window || (uint64_t)(nw - 1u) * out_per_window + n_out > out_points) return -1;
  using E = te::ete_t<N>;
  te::sum_jobs_t<N> js; memset(&js, 0, sizeof js);
  te::sum_job_t<N>& j = js.j[0];
  j.in = static_cast<const E*>(in); j.out = static_cast<E*>(out); j.K = K; j.n_out = n_out; j.inner = inner;
  j.in_per_window = in_per_window; j.out_per_window = out_per_window;
  const uint32_t most = n_out * nw;
  if (form == 0) {
    uint32_t blocks = (most + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((te::k_sum_groups<N, false>), dim3(blocks, 1), dim3(256), 0, 0, js, nw);
  } else if (form == 1) {
    uint32_t blocks = (2 * most + 255) / 256; if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL((te::k_sum_groups<N, true>), dim3(blocks, 1), dim3(256), 0, 0, js, nw);
  } else {
    uint32_t blocks = (most * 4 + 255) / 256; if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(te::k_sum_groups_team<N>, dim3(blocks, 1), dim3(256), 0, 0, js, nw);
  }
  return finish();
}

// ---- k_reduce_tail with reduce_t's shapes: grid (4, nw), 1024 threads, (max(H, L) + 16) points of dynamic LDS; rows of window k
// at rows + 5 k, no flag words
template <int N> int reduce_tail(const void* xin, uint64_t x_points, const void* yin, uint64_t y_points, uint32_t rx, uint32_t ry,
                                 uint32_t x_per_window, uint32_t y_per_window, const uint32_t* w, void* rows, uint64_t row_points, uint32_t nw) {
  if (nw == 0 || rx < 1 || rx > 4 || ry < 1 || ry > 4 || w[0] > 4 || w[1] > 4 || w[2] > 4 || w[3] > 4) return -1;
  using E = te::ete_t<N>;
  const uint32_t L = 1u << (w[0] + w[1]), H = 1u << (w[2] + w[3]);
  if ((uint64_t)H * rx > x_per_window || (uint64_t)(nw - 1u) * x_per_window + (uint64_t)H * rx > x_points) return -1;
  if ((uint64_t)L * ry > y_per_window || (uint64_t)(nw - 1u) * y_per_window + (uint64_t)L * ry > y_points) return -1;
  if (5ull * nw > row_points) return -1;
  const size_t lds_bytes = (size_t)(std::max(H, L) + 16u) * sizeof(E);
  if (lds_bytes > 64 * 1024) return -1;
  if (lds_bytes > 48 * 1024) {
    const hipError_t er = hipFuncSetAttribute(reinterpret_cast<const void*>(te::k_reduce_tail<N>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    if (er != hipSuccess) return (int)er;
  }
  te::tail_params_t<N> tp; memset(&tp, 0, sizeof tp);
  tp.xin = static_cast<const E*>(xin); tp.yin = static_cast<const E*>(yin); tp.rx = rx; tp.ry = ry;
  tp.x_per_window = x_per_window; tp.y_per_window = y_per_window;
  for (int k = 0; k < 4; k++) tp.w[k] = w[k];
  tp.rows = static_cast<E*>(rows); tp.row_stride = 5u; tp.win_per_msm = nw; tp.msm_stride = 5u * nw;
  tp.flag_src = nullptr; tp.flag_dst = nullptr; tp.flag_words = 0;
  hipLaunchKernelGGL(te::k_reduce_tail<N>, dim3(4, nw), dim3(1024), lds_bytes, 0, tp);
  return finish();
}

}  // namespace

extern "C" {

#define X(name, fn, IW, OW)                                                                             \
  int dc_##name(const uint32_t* in, uint32_t* out, uint32_t n) {                                        \
    if (n == 0) return 0;                                                                               \
    hipLaunchKernelGGL(k_dc_##name, dim3((n + 255u) / 256u), dim3(256), 0, 0, in, out, n);              \
    return finish();                                                                                    \
  }
DC_OPS(X)
#undef X
#define X(name, fn, IW, OW) #name ":" #IW ":" #OW ";"
const char* dc_table() { return DC_OPS(X); }
#undef X

// points are ete_t<N>: x | y | z | t, N words each
int dc_add_team_9(const void* a, const void* b, void* out, uint32_t n) { return add_team<9>(a, b, out, n); }
int dc_add_team_14(const void* a, const void* b, void* out, uint32_t n) { return add_team<14>(a, b, out, n); }
// first / stride / cnt: HOST arrays of njobs <= 32 entries; src holds src_points points
int dc_block_sum_9(int coherent, const void* src, uint64_t src_points, const uint32_t* first, const uint32_t* stride, const uint32_t* cnt, uint32_t njobs, void* out) {
  return block_sum<9>(coherent, src, src_points, first, stride, cnt, njobs, out);
}
int dc_block_sum_14(int coherent, const void* src, uint64_t src_points, const uint32_t* first, const uint32_t* stride, const uint32_t* cnt, uint32_t njobs, void* out) {
  return block_sum<14>(coherent, src, src_points, first, stride, cnt, njobs, out);
}
int dc_sum_groups_9(int form, const void* in, uint64_t in_points, void* out, uint64_t out_points, uint32_t n_out, uint32_t K, uint32_t inner,
                    uint32_t in_per_window, uint32_t out_per_window, uint32_t nw) {
  return sum_groups<9>(form, in, in_points, out, out_points, n_out, K, inner, in_per_window, out_per_window, nw);
}
int dc_sum_groups_14(int form, const void* in, uint64_t in_points, void* out, uint64_t out_points, uint32_t n_out, uint32_t K, uint32_t inner,
                     uint32_t in_per_window, uint32_t out_per_window, uint32_t nw) {
  return sum_groups<14>(form, in, in_points, out, out_points, n_out, K, inner, in_per_window, out_per_window, nw);
}
// w: HOST array of the four digit widths
int dc_reduce_tail_9(const void* xin, uint64_t x_points, const void* yin, uint64_t y_points, uint32_t rx, uint32_t ry, uint32_t x_per_window,
                     uint32_t y_per_window, const uint32_t* w, void* rows, uint64_t row_points, uint32_t nw) {
  return reduce_tail<9>(xin, x_points, yin, y_points, rx, ry, x_per_window, y_per_window, w, rows, row_points, nw);
}
int dc_reduce_tail_14(const void* xin, uint64_t x_points, const void* yin, uint64_t y_points, uint32_t rx, uint32_t ry, uint32_t x_per_window,
                      uint32_t y_per_window, const uint32_t* w, void* rows, uint64_t row_points, uint32_t nw) {
  return reduce_tail<14>(xin, x_points, yin, y_points, rx, ry, x_per_window, y_per_window, w, rows, row_points, nw);
}

}  // extern "C"
