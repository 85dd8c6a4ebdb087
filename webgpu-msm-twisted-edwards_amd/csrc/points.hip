// points.hip -- what the library does with points beside MSMs: validation (option "check_points", te_msm_check_points*), x-only
// points (te_msm_points_from_x*, te_msm_bind_points_x, te_msm_run_x), batch scalar multiplication (te_msm_mul*) and its fixed-base form
// over one bound point (te_msm_bind_base, te_msm_mul_base*), batched group addition and point-set sums (te_msm_add*, te_msm_sum*), and
// batched arithmetic in the two base fields (te_msm_field_op*), batched NTTs over p (te_msm_ntt*) and polynomial openings
// (te_msm_poly_divide*), bound sparse matrices and their products (te_msm_bind_matrix, te_msm_spmv*), prefix sums and products
// (te_msm_field_scan*).  The one unit that includes the kernels of check.hip.hpp, from_x.hip.hpp, scalar_mul.hip.hpp, mul_base.hip.hpp,
// group_add.hip.hpp, field_ops.hip.hpp, ntt.hip.hpp, poly.hip.hpp, spmv.hip.hpp and scan.hip.hpp.
#include "engine.hpp"
#include "check.hip.hpp"
#include "from_x.hip.hpp"
#include "scalar_mul.hip.hpp"
#include "mul_base.hip.hpp"
#include "group_add.hip.hpp"
#include "field_ops.hip.hpp"
#include "ntt.hip.hpp"
#include "poly.hip.hpp"
#include "spmv.hip.hpp"
#include "scan.hip.hpp"

using namespace te_eng;

namespace te_eng {

namespace {
// A kernel's template parameters from run-time values, as te_msm.hip's with_scalar_form: f(std::integral_constant<int, CURVE>{}) with the
// kernels' CURVE (0 Twisted-Edwards BLS12, 1 BLS12-377 G1) of a TE_MSM_CURVE_* value, f(std::true_type / std::false_type{}) of a flag.
// The per-curve constant of a launch comes by the same parameter: order_naf_of / root_exp_of / inv_exp_of<CURVE>().
template <typename F> void with_curve(int curve, F&& f) {
  if (curve == TE_MSM_CURVE_BLS12_377_G1) f(std::integral_constant<int, 1>{});
  else f(std::integral_constant<int, 0>{});
}
template <typename F> void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}
// ... and the 16-byte words of one scalar record (k_scalar_mul's and k_mul_base's SQ) of its bytes: 2, or 3 for BLS12-377's own 48-byte
// record.  The Twisted-Edwards curve has 32-byte records only: its kernels exist for SQ = 2 alone
template <int CURVE, typename F> void with_scalar_quads(size_t sb, F&& f) {
  if constexpr (CURVE == 1) {
    if (sb != 32) { f(std::integral_constant<int, 3>{}); return; }
  }
  f(std::integral_constant<int, 2>{});
}

// ---- input-point validation (option "check_points", te_msm_check_points*; kernels in check.hip.hpp) ----------------------------
// Runs on device devs[di] in front of whatever the call does with the points, and waits for its verdict: a point that fails must
// stop the call before an MSM result exists.  Device-resident points are checked where they lie (one launch per check); host points
// cross PCIe in pieces of kCheckPiece through the device's own buffer -- the same bytes the MSM uploads again afterwards: checking is
// opt-in and priced in the header.  The report word takes the lowest failing index of a launch (check_code); pieces run in order,
// so the first piece that reports holds the lowest index of the whole buffer.
constexpr uint64_t kCheckPiece = 1ull << 18;

// The check lane of a device (its stream, report word and pinned host word: check_points_on, recover_on, in_pieces, ...), held while
// this lives: chk_mu locked, the device made current, the three created on first use.  chk_mu is a plain mutex: whoever holds a lane
// calls nothing that takes one.  rc: 0, or the HIP error (noted) that left it unusable.
struct check_lane {
  gpu_t& d;
  std::lock_guard<std::mutex> lk;
  const int rc;
  check_lane(te_ctx* ctx, gpu_t& dev) : d(dev), lk(*dev.chk_mu), rc(open(ctx, dev)) {}
  hipStream_t stream() const { return d.chk_stream; }
  // the report word on the host: 0, or TE_MSM_EPOINT and the lowest failing index among the m points it covers (check_decode)
  int verdict(te_ctx* ctx, uint64_t m, int64_t* bad, int* reason) {
    HIP_TRY(ctx, hipMemcpyAsync(d.chk_host, d.chk_word, sizeof(unsigned long long), hipMemcpyDeviceToHost, d.chk_stream));
    HIP_TRY(ctx, hipStreamSynchronize(d.chk_stream));
    if (!*d.chk_host) return 0;
    te::check_decode(*d.chk_host, m, bad, reason);
    return TE_MSM_EPOINT;
  }
  // one check over m points, whatever the kernels (check_points_on's, group_check_on's): the word cleared, form(grid, block) launched,
  // subgroup(grid, block) behind it when level >= 2, and the verdict waited for
  template <typename Form, typename Subgroup> int check(te_ctx* ctx, uint32_t m, int level, int64_t* bad, int* reason, Form&& form, Subgroup&& subgroup) {
    HIP_TRY(ctx, hipMemsetAsync(d.chk_word, 0, sizeof(unsigned long long), d.chk_stream));
    const dim3 grid((m + 255u) / 256u), block(256);
    form(grid, block);
    if (level >= 2) subgroup(grid, block);
    HIP_TRY(ctx, hipGetLastError());
    return verdict(ctx, m, bad, reason);
  }
 private:
  static int open(te_ctx* ctx, gpu_t& d) {
    HIP_TRY(ctx, hipSetDevice(d.device));
    if (!d.chk_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&d.chk_stream, hipStreamNonBlocking));
    if (!d.chk_word) HIP_TRY(ctx, hipMalloc(&d.chk_word, sizeof(unsigned long long)));
    if (!d.chk_host) HIP_TRY(ctx, hipHostMalloc(&d.chk_host, sizeof(unsigned long long), hipHostMallocDefault));
    return 0;
  }
};

// check_points_on's check of one piece: m points at `at` (device memory), packed or -- lay.stride -- records at a stride
template <int CURVE, bool MONT> int check_piece(te_ctx* ctx, check_lane& lane, const uint8_t* at, uint32_t m, int level, point_layout lay, int64_t* bad, int* reason) {
  hipStream_t st = lane.stream();
  unsigned long long* word = lane.d.chk_word;
  if (lay.stride) {
    const uint64_t* p8 = reinterpret_cast<const uint64_t*>(at);
    const uint32_t sd = lay.stride, fl = lay.flag ? 1u : 0u;
    return lane.check(ctx, m, level, bad, reason,
                      [&](dim3 grid, dim3 block) { hipLaunchKernelGGL((te::k_check_form_strided<CURVE, MONT>), grid, block, 0, st, p8, sd, fl, m, word); },
                      [&](dim3 grid, dim3 block) { hipLaunchKernelGGL((te::k_check_subgroup_strided<CURVE, MONT>), grid, block, 0, st, p8, sd, fl, m, word, te::order_naf_of<CURVE>()); });
  }
  const uint4* p4 = reinterpret_cast<const uint4*>(at);
  return lane.check(ctx, m, level, bad, reason,
                    [&](dim3 grid, dim3 block) { hipLaunchKernelGGL((te::k_check_form<CURVE, MONT>), grid, block, 0, st, p4, m, word); },
                    [&](dim3 grid, dim3 block) { hipLaunchKernelGGL((te::k_check_subgroup<CURVE, MONT>), grid, block, 0, st, p4, m, word, te::order_naf_of<CURVE>()); });
}

// te_msm_run_x and te_msm_mul* read canonical scalars only: with option "scalars_montgomery" set they are refused (a silent canonical
// reading would be a wrong answer)
const char* const kNoMontgomeryScalars = "option \"scalars_montgomery\" is set: te_msm_run_x and te_msm_mul* take canonical scalars only";
int check_standalone(te_ctx* ctx, const void* src, bool src_is_host, uint64_t n, int level, int64_t* first_bad, int* reason) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  int64_t bad = -1; int why = 0;
  if (first_bad) *first_bad = -1;
  if (reason) *reason = 0;
  if (level != 1 && level != 2) return set_err(ctx, TE_MSM_EINVAL, "te_msm_check_points: level must be 1 or 2");
  if (int rc = check_n(ctx, n)) return rc;
  if (n > 0 && !src) return set_err(ctx, TE_MSM_EINVAL, "null point buffer");
  const int di = !src_is_host && n > 0 && ctx->devs.size() > 1
                     ? owner_of(ctx, "te_msm_check_points_device: the points must be resident on a device of the context", {src}) : 0;
  if (di < 0) return di;
  const point_layout lay = layout_now(ctx);
  if (int rc = check_layout(ctx, lay, src, src_is_host)) return rc;
  const int rc = check_points_on(ctx, (size_t)di, src, src_is_host, n, ctx->opt_curve, level, &bad, &why, ctx->opt_points_montgomery != 0, lay);
  if (rc != TE_MSM_EPOINT) return rc;
  return note_bad(ctx, kBadPoint, bad, why, first_bad, reason);
}

// ---- x-only points (te_msm_points_from_x[_device], te_msm_bind_points_x, te_msm_run_x; kernels in from_x.hip.hpp) ----------------
// Recovery runs on device devs[di] into a buffer of the call's own, and the call waits for the verdict: on a failure nothing reaches
// the caller's output and no MSM runs.  Host x-coordinates cross PCIe in pieces of kCheckPiece through a staging buffer, on the
// check stream of the device (one stream: a piece's copy waits for the previous piece's kernel); every piece reports into one word
// over the whole buffer, so the lowest failing index wins without a wait per piece.  The temporary buffers are freed before the call
// returns (dev_tmp): nothing is cached, nothing counts in "device_bytes".

inline size_t x_bytes_of(int curve) { return curve == TE_MSM_CURVE_BLS12_377_G1 ? TE_MSM_X_BYTES_BLS12_377 : TE_MSM_X_BYTES; }

// n x-coordinates at src (host, or memory of devs[di]) -> n points in d_pts (memory of devs[di]); then, when dst is given and every x
// passed, the points are copied to dst (host or device memory) before the lock is released
int recover_on(te_ctx* ctx, size_t di, const void* src, bool src_is_host, uint64_t n, void* d_pts, void* dst, bool dst_is_host,
               int64_t* bad, int* reason) {
  *bad = -1; *reason = 0;
  if (n == 0) return 0;
  gpu_t& d = ctx->devs[di];
  const int curve = ctx->opt_curve;
  const size_t xb = x_bytes_of(curve), pb = sizes_of(curve).point_in;
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  const uint64_t piece = src_is_host ? std::min(n, kCheckPiece) : n;
  dev_tmp stage;
  if (src_is_host) { if (int rc = tmp_alloc(ctx, d, stage, piece * xb)) return rc; }
  hipStream_t st = lane.stream();
  HIP_TRY(ctx, hipMemsetAsync(d.chk_word, 0, sizeof(unsigned long long), st));
  for (uint64_t off = 0; off < n; off += piece) {
    const uint32_t m = (uint32_t)std::min(piece, n - off);
    const uint8_t* at = static_cast<const uint8_t*>(src) + off * xb;
    if (src_is_host) { HIP_TRY(ctx, hipMemcpyAsync(stage.p, at, (size_t)m * xb, hipMemcpyHostToDevice, st)); at = static_cast<const uint8_t*>(stage.p); }
    const uint4* x4 = reinterpret_cast<const uint4*>(at);
    uint4* o4 = reinterpret_cast<uint4*>(static_cast<uint8_t*>(d_pts) + off * pb);
    const dim3 grid((m + 255u) / 256u), block(256);
    with_curve(curve, [&](auto c) {
      constexpr int C = decltype(c)::value;
      hipLaunchKernelGGL(te::k_points_from_x<C>, grid, block, 0, st, x4, m, o4, d.chk_word, n, off, te::root_exp_of<C>(), te::order_naf_of<C>());
    });
    HIP_TRY(ctx, hipGetLastError());
  }
  if (int rc = lane.verdict(ctx, n, bad, reason)) return rc;
  if (dst) {
    HIP_TRY(ctx, hipMemcpyAsync(dst, d_pts, n * pb, dst_is_host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
  }
  return 0;
}
// host x -> points of the first device in t (allocated here): 0, TE_MSM_EPOINT (noted) or a device error
int recover_host_to_first(te_ctx* ctx, const uint8_t* x_le, uint64_t n, dev_tmp& t) {
  if (int rc = tmp_alloc(ctx, ctx->devs[0], t, n * sizes_of(ctx->opt_curve).point_in)) return rc;
  int64_t bad = -1; int why = 0;
  const int rc = recover_on(ctx, 0, x_le, true, n, t.p, nullptr, false, &bad, &why);
  if (rc == TE_MSM_EPOINT) return note_bad(ctx, kBadX, bad, why);
  return rc;
}
int from_x_args(te_ctx* ctx, const void* x, uint64_t n, const void* out) {
  if (int rc = check_n(ctx, n)) return rc;
  if (n > 0 && (!x || !out)) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  return 0;
}
// te_msm_points_from_x (buffers on the host: recovery on the first device) and te_msm_points_from_x_device (on the device that holds them)
int points_from_x_common(te_ctx* ctx, const void* x, bool on_host, uint64_t n, void* out, int64_t* first_bad, int* reason) {
  if (!ctx) return TE_MSM_EINVAL;
  if (first_bad) *first_bad = -1;
  if (reason) *reason = 0;
  if (int rc = from_x_args(ctx, x, n, out)) return rc;
  if (n == 0) return 0;
  const int di = on_host ? 0 : owner_of(ctx, "te_msm_points_from_x_device: x and the output must be resident on one device of the context", {x, out});
  if (di < 0) return di;
  dev_tmp pts;
  if (int rc = tmp_alloc(ctx, ctx->devs[(size_t)di], pts, n * sizes_of(ctx->opt_curve).point_in)) return rc;
  int64_t bad = -1; int why = 0;
  const int rc = recover_on(ctx, (size_t)di, x, on_host, n, pts.p, out, on_host, &bad, &why);
  if (rc != TE_MSM_EPOINT) return rc;
  return note_bad(ctx, kBadX, bad, why, first_bad, reason);
}

// ---- batch scalar multiplication (te_msm_mul[_device], te_msm_mul_x; kernels in scalar_mul.hip.hpp) ------------------------------
// Host buffers: contiguous slices over the context's devices, as te_msm_run's point slices (slice_plan, below).  Every slice is staged
// whole on its device -- points (or x), scalars and results -- checked (recovery, option "check_points"), multiplied, and copied out only
// when no slice reported a bad point: on a failure `out` is untouched.  The chain writes projective results of a piece of kMulPiece
// points into a buffer of the call's own; the affine pass turns them into the wire format (in_pieces).  Every temporary is freed before
// the call returns (dev_tmp).
constexpr uint64_t kMulPiece = 1ull << 18;
// te_msm_mul* as te_msm_run_x: canonical scalars only -- refused under the option instead of a silent canonical reading
int mul_refused(te_ctx* ctx) { return ctx->opt_scalars_montgomery ? set_err(ctx, TE_MSM_EINVAL, kNoMontgomeryScalars) : 0; }

inline te::naf_t shared_naf_of(const uint8_t* k32, int curve) {
  uint32_t k[8];
  memcpy(k, k32, 32);
  return te::sm_shared_naf(k, curve);
}
inline size_t proj_bytes_of(int curve) { return 4u * (curve == TE_MSM_CURVE_BLS12_377_G1 ? te::sm_sizes<1>::JW : te::sm_sizes<0>::JW); }
// The piece loop of te_msm_mul*, te_msm_mul_base* and te_msm_add*: n results at d_out (memory of devs[di]) in pieces of at most
// piece_max, on the device's check lane -- taken here: no caller holds it.  chain(off, m, proj, stream) enqueues the kernel that writes
// the m projective results of the piece at off into proj, a buffer of the call's own; the affine pass (k_scalar_mul_affine, chains of
// eight) behind it turns them into the wire format at d_out + off.  One synchronise at the end: returns when the results are there.
template <typename Chain> int in_pieces(te_ctx* ctx, size_t di, uint64_t n, uint64_t piece_max, void* d_out, Chain&& chain) {
  if (n == 0) return 0;
  gpu_t& d = ctx->devs[di];
  const int curve = ctx->opt_curve;
  const size_t pb = sizes_of(curve).point_in;
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  const uint64_t piece = std::min(n, piece_max);
  dev_tmp proj;
  if (int rc = tmp_alloc(ctx, d, proj, piece * proj_bytes_of(curve))) return rc;
  hipStream_t st = lane.stream();
  for (uint64_t off = 0; off < n; off += piece) {
    const uint32_t m = (uint32_t)std::min(piece, n - off);
    uint32_t* o32 = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(d_out) + off * pb);
    const dim3 agrid((m + 256u * SM_AFF_GROUP - 1u) / (256u * SM_AFF_GROUP)), block(256);
    chain(off, m, static_cast<uint4*>(proj.p), st);
    with_curve(curve, [&](auto c) {
      constexpr int C = decltype(c)::value;
      hipLaunchKernelGGL(te::k_scalar_mul_affine<C>, agrid, block, 0, st, static_cast<const uint32_t*>(proj.p), m, o32, te::inv_exp_of<C>());
    });
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}
// n points and scalars (memory of devs[di]) -> n affine results at d_out (memory of devs[di]); returns when they are there.
// sb: bytes of one scalar record -- the call's (scalar_bytes_now), or the curve's own for the records te_msm_bind_base makes itself
int mul_on(te_ctx* ctx, size_t di, const void* d_pts, const void* d_sc, uint64_t n, bool shared, const te::naf_t& kn, void* d_out, size_t sb) {
  const int curve = ctx->opt_curve;
  const size_t pb = sizes_of(curve).point_in;
  return in_pieces(ctx, di, n, kMulPiece, d_out, [&](uint64_t off, uint32_t m, uint4* j4, hipStream_t st) {
    const uint4* p4 = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(d_pts) + off * pb);
    const uint4* s4 = shared ? nullptr : reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(d_sc) + off * sb);
    const dim3 grid((m + 255u) / 256u), block(256);
    with_curve(curve, [&](auto c) {
      constexpr int C = decltype(c)::value;
      if (shared) hipLaunchKernelGGL((te::k_scalar_mul<C, true>), grid, block, 0, st, p4, s4, m, j4, kn);     // (reads no record: the NAF)
      else with_scalar_quads<C>(sb, [&](auto q) { hipLaunchKernelGGL((te::k_scalar_mul<C, false, decltype(q)::value>), grid, block, 0, st, p4, s4, m, j4, kn); });
    });
  });
}
int mul_args(te_ctx* ctx, const void* pts, const void* sc, uint64_t n, const void* out) {
  if (int rc = check_n(ctx, n)) return rc;
  if (int rc = check_mul_scalar_record(ctx)) return rc;
  if (n > 0 && (!pts || !sc || !out)) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  return 0;
}

// ---- what the host forms of te_msm_mul*, te_msm_mul_base*, te_msm_add* and te_msm_sum* share ----------------------------------------
// Contiguous slices over the context's devices, one host thread per device (on_devices).  Every slice is staged whole on its device,
// worked on there, and copied out only when no slice reported a bad point: stage, then scan, then copy out.

// the slices of n > 0 items: D = min(devices, n) of them, slice i holds count(i) items from lo(i) on (the last ones may hold none)
struct slice_plan {
  uint64_t n; size_t D; uint64_t per;
  slice_plan(const te_ctx* ctx, uint64_t n_) : n(n_), D((size_t)std::min<uint64_t>(ctx->devs.size(), n_)), per((n_ + D - 1) / D) {}
  uint64_t lo(size_t i) const { return std::min<uint64_t>(n, per * i); }
  uint64_t count(size_t i) const { return std::min<uint64_t>(n, lo(i) + per) - lo(i); }
};
// every slice's result (count(i) points of pb bytes at res(i), memory of devs[i]) -> out + lo(i) * pb
template <typename Where> int copy_slices_out(te_ctx* ctx, const slice_plan& sp, size_t pb, uint8_t* out, Where&& res) {
  return te_sched::on_devices(*ctx, sp.D, [&](size_t i) -> int {
    if (sp.count(i) == 0) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->devs[i].device));
    HIP_TRY(ctx, hipMemcpy(out + sp.lo(i) * pb, res(i), sp.count(i) * pb, hipMemcpyDeviceToHost));
    return 0;
  });
}
// the verdict over the operands of a call (te_msm_add*: a = 0, b = 1; every other call: 0): the lowest failing index, a before b at
// equal index
struct pair_verdict {
  int64_t bad = -1; int why = 0, operand = 0; bad_kind kind = kBadPoint;
  void take(int64_t i, int reason, int op, bad_kind k) {
    if (i < 0 || (bad >= 0 && (bad < i || (bad == i && operand <= op)))) return;
    bad = i; why = reason; operand = op; kind = k;
  }
};
int note_pair(te_ctx* ctx, const pair_verdict& v, int64_t base) {
  const int rc = note_bad(ctx, v.kind, base + v.bad, v.why);
  ctx->bad_point_operand = v.operand;
  return rc;
}
// slices (each with a pair_verdict v) in order: the first that reports holds the lowest index of the call.  0: none reported
template <typename Slice> int note_slices(te_ctx* ctx, const slice_plan& sp, const std::vector<Slice>& sl) {
  for (size_t i = 0; i < sp.D; i++)
    if (sl[i].v.bad >= 0) return note_pair(ctx, sl[i].v, (int64_t)sp.lo(i));
  return 0;
}
// operand op of a slice onto devs[di]: m points in t (allocated here) of m host points at src (a copy), or -- x_only -- of m host
// x-coordinates (recovery; an x without a point goes to v as kBadX and the call goes on: 0)
int stage_operand(te_ctx* ctx, size_t di, const uint8_t* src, bool x_only, uint64_t m, dev_tmp& t, int op, pair_verdict& v) {
  const size_t pb = sizes_of(ctx->opt_curve).point_in;
  if (int rc = tmp_alloc(ctx, ctx->devs[di], t, m * pb)) return rc;
  if (!x_only) {
    HIP_TRY(ctx, hipMemcpy(t.p, src, m * pb, hipMemcpyHostToDevice));
    return 0;
  }
  int64_t bad = -1; int why = 0;
  const int rc = recover_on(ctx, di, src, true, m, t.p, nullptr, false, &bad, &why);
  if (rc != TE_MSM_EPOINT) return rc;
  v.take(bad, why, op, kBadX);
  return 0;
}

// te_msm_mul (x_only = false) and te_msm_mul_x (true): host buffers, sliced over the devices
int mul_host(te_ctx* ctx, const uint8_t* src, bool x_only, const uint8_t* scalars_le, uint64_t n, bool shared, uint8_t* out) {
  if (int rc = mul_args(ctx, src, scalars_le, n, out)) return rc;
  if (n == 0) return 0;
  const int curve = ctx->opt_curve, level = ctx->opt_check_points;
  const size_t pb = sizes_of(curve).point_in, sb = scalar_bytes_now(ctx), ib = x_only ? x_bytes_of(curve) : pb;
  const te::naf_t kn = shared ? shared_naf_of(scalars_le, curve) : te::naf_t{};
  const slice_plan sp(ctx, n);
  struct slice_t { dev_tmp pts, sc, res; pair_verdict v; };
  std::vector<slice_t> sl(sp.D);
  auto stage = [&](size_t i) -> int {                             // upload, recover, check, multiply: everything but the copy out
    const uint64_t lo = sp.lo(i), m = sp.count(i);
    if (m == 0) return 0;
    gpu_t& d = ctx->devs[i];
    slice_t& s = sl[i];
    if (int rc = tmp_alloc(ctx, d, s.res, m * pb)) return rc;
    if (!shared) {
      if (int rc = tmp_alloc(ctx, d, s.sc, m * sb)) return rc;
      HIP_TRY(ctx, hipMemcpy(s.sc.p, scalars_le + lo * sb, m * sb, hipMemcpyHostToDevice));
    }
    if (int rc = stage_operand(ctx, i, src + lo * ib, x_only, m, s.pts, 0, s.v)) return rc;
    if (s.v.bad >= 0) return 0;                                   // (a bad x is reported before a failed check of a recovered point)
    if (level) {
      int64_t bad = -1; int why = 0;
      const int rc = check_points_on(ctx, i, s.pts.p, false, m, curve, level, &bad, &why);
      if (rc == TE_MSM_EPOINT) { s.v.take(bad, why, 0, kBadPoint); return 0; }
      if (rc) return rc;
    }
    return mul_on(ctx, i, s.pts.p, s.sc.p, m, shared, kn, s.res.p, sb);
  };
  if (int rc = te_sched::on_devices(*ctx, sp.D, stage)) return rc;
  if (int rc = note_slices(ctx, sp, sl)) return rc;
  return copy_slices_out(ctx, sp, pb, out, [&](size_t i) { return sl[i].res.p; });
}

// ---- fixed-base batch scalar multiplication (te_msm_bind_base, te_msm_mul_base[_device]; kernels in mul_base.hip.hpp) ---------------
// The bind makes the table's scalars j 2^(W i) mod (4 L | r) on the host and runs te_msm_mul's own chain (mul_on) over the point
// replicated, on every device; k_mul_base_entries turns the affine results into entries.  A call is mul_on's piece loop (in_pieces) with
// k_mul_base as the chain: pieces of kMulPiece scalars.  The table is the only memory that outlives a call.
const char* const kBadBase = "not a bound point of this context (released, or bound to another context)";
const char* const kBaseCurve = "the point was bound under another curve than the one selected now (option \"curve\")";
int check_base(te_ctx* ctx, const te_base* b) {
  if (!b || std::find(ctx->mul_bases.begin(), ctx->mul_bases.end(), b) == ctx->mul_bases.end()) return set_err(ctx, TE_MSM_EINVAL, kBadBase);
  if (b->curve != ctx->opt_curve) return set_err(ctx, TE_MSM_EINVAL, kBaseCurve);
  return 0;
}
// the table of b on device devs[i]: pts / sc hold the point replicated and the scalar records of its entries (host memory)
int base_table_on(te_ctx* ctx, te_base* b, size_t i, const uint8_t* pts, const uint8_t* sc, const te::mb_geom& g) {
  gpu_t& d = ctx->devs[i];
  const size_t pb = sizes_of(b->curve).point_in, sb = sizes_of(b->curve).scalar_in;
  HIP_TRY(ctx, hipSetDevice(d.device));
  HIP_TRY(ctx, hipMalloc((void**)&b->tab[i], b->bytes()));                 // (freed by the caller on failure: free_mul_base)
  dev_tmp d_pts, d_sc, d_aff;
  if (int rc = tmp_alloc(ctx, d, d_pts, g.entries * pb)) return rc;
  if (int rc = tmp_alloc(ctx, d, d_sc, g.entries * sb)) return rc;
  if (int rc = tmp_alloc(ctx, d, d_aff, g.entries * pb)) return rc;
  HIP_TRY(ctx, hipMemcpy(d_pts.p, pts, g.entries * pb, hipMemcpyHostToDevice));
  HIP_TRY(ctx, hipMemcpy(d_sc.p, sc, g.entries * sb, hipMemcpyHostToDevice));
  if (int rc = mul_on(ctx, i, d_pts.p, d_sc.p, g.entries, false, te::naf_t{}, d_aff.p, sb)) return rc;
  check_lane lane(ctx, d);                                                  // (only now: mul_on takes the lane itself)
  if (lane.rc) return lane.rc;
  const dim3 grid((g.entries + 255u) / 256u), block(256);
  const uint4* a4 = static_cast<const uint4*>(d_aff.p);
  uint4* t4 = reinterpret_cast<uint4*>(b->tab[i]);
  with_curve(b->curve, [&](auto c) { hipLaunchKernelGGL(te::k_mul_base_entries<decltype(c)::value>, grid, block, 0, lane.stream(), a4, g.entries, t4); });
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(lane.stream()));
  return 0;
}
// n scalar records of sb bytes (memory of devs[di]; mont: Montgomery residues) -> n affine results at d_out (memory of devs[di]); returns when they are there
int mul_base_on(te_ctx* ctx, size_t di, const te_base* b, const void* d_sc, uint64_t n, bool mont, void* d_out, size_t sb) {
  const te::mb_geom g = te::mb_geometry(b->W);
  const uint4* t4 = reinterpret_cast<const uint4*>(b->tab[di]);
  return in_pieces(ctx, di, n, kMulPiece, d_out, [&](uint64_t off, uint32_t m, uint4* j4, hipStream_t st) {
    const uint4* s4 = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(d_sc) + off * sb);
    const dim3 grid((m + 255u) / 256u), block(256);
    with_curve(b->curve, [&](auto c) {
      with_flag(mont, [&](auto mt) {                                // the records' form: canonical, or the Montgomery residues of the curve's scalar field
        constexpr int C = decltype(c)::value, FORM = !decltype(mt)::value ? te::SCALAR_FORM_CANONICAL : C == 1 ? te::SCALAR_FORM_377 : te::SCALAR_FORM_TE;
        with_scalar_quads<C>(sb, [&](auto q) { hipLaunchKernelGGL((te::k_mul_base<C, FORM, decltype(q)::value>), grid, block, 0, st, t4, s4, m, j4, g); });
      });
    });
  });
}
// what every te_msm_mul_base* call checks first; *go = false: nothing to do (n = 0)
int mul_base_args(te_ctx* ctx, const te_base* b, const void* sc, uint64_t n, const void* out, bool* go) {
  *go = false;
  if (int rc = check_base(ctx, b)) return rc;
  if (int rc = check_n(ctx, n)) return rc;
  if (int rc = check_mul_scalar_record(ctx)) return rc;
  if (n > 0 && (!sc || !out)) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  *go = n > 0;
  return 0;
}
// te_msm_mul_base: host scalars sliced over the devices, as mul_host
int mul_base_host(te_ctx* ctx, const te_base* b, const uint8_t* scalars_le, uint64_t n, uint8_t* out) {
  const bool mont = ctx->opt_scalars_montgomery != 0;
  const size_t pb = sizes_of(b->curve).point_in, sb = scalar_bytes_now(ctx);
  const slice_plan sp(ctx, n);
  struct slice_t { dev_tmp sc, res; };
  std::vector<slice_t> sl(sp.D);
  auto stage = [&](size_t i) -> int {                             // upload and multiply: everything but the copy out
    const uint64_t m = sp.count(i);
    if (m == 0) return 0;
    gpu_t& d = ctx->devs[i];
    if (int rc = tmp_alloc(ctx, d, sl[i].sc, m * sb)) return rc;
    if (int rc = tmp_alloc(ctx, d, sl[i].res, m * pb)) return rc;
    HIP_TRY(ctx, hipMemcpy(sl[i].sc.p, scalars_le + sp.lo(i) * sb, m * sb, hipMemcpyHostToDevice));
    return mul_base_on(ctx, i, b, sl[i].sc.p, m, mont, sl[i].res.p, sb);
  };
  if (int rc = te_sched::on_devices(*ctx, sp.D, stage)) return rc;
  return copy_slices_out(ctx, sp, pb, out, [&](size_t i) { return sl[i].res.p; });
}

// ---- batched group addition and point-set sums (te_msm_add*, te_msm_sum*; kernels in group_add.hip.hpp) ------------------------------
// An addition is mul_on's piece loop (in_pieces) with k_group_add as the chain, in pieces of kAddPiece pairs, te_msm_mul's affine pass
// (k_scalar_mul_affine, unchanged) behind each -- the whole call in one piece up to 2^21 pairs: an addition is
// two launches of a few hundred microseconds, and pieces of kMulPiece would quadruple them at 2^20 for nothing but a smaller buffer.  A
// piece's additions have read a and b before its affine pass writes out, and later pieces lie behind it: d_out may be d_a or d_b.  The
// sum needs the points once: stage 1 over a bounded grid, the same kernel over its partials, one projective point back to the host,
// normalised there.
constexpr uint64_t kAddPiece = TE_MSM_GROUP_ADD_PIECE;
constexpr uint32_t kSumGrid = TE_MSM_GROUP_SUM_GRID;

// option "check_points" for these calls: n packed points in the memory of devs[di], one launch per level; the all-zero BLS12-377 record passes
int group_check_on(te_ctx* ctx, size_t di, const void* d_pts, uint64_t n, int level, int64_t* bad, int* reason) {
  *bad = -1; *reason = 0;
  if (n == 0 || !level) return 0;
  gpu_t& d = ctx->devs[di];
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  hipStream_t st = lane.stream();
  const uint32_t m = (uint32_t)n;
  const uint4* p4 = static_cast<const uint4*>(d_pts);
  int rc = 0;
  with_curve(ctx->opt_curve, [&](auto c) {
    constexpr int C = decltype(c)::value;
    rc = lane.check(ctx, m, level, bad, reason,
                    [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(te::k_group_check_form<C>, grid, block, 0, st, p4, m, d.chk_word); },
                    [&](dim3 grid, dim3 block) { hipLaunchKernelGGL(te::k_group_check_subgroup<C>, grid, block, 0, st, p4, m, d.chk_word, te::order_naf_of<C>()); });
  });
  return rc;
}

// one step (recovery, or a check level) over both operands in the memory of devs[di]: 0 with v filled in when a point failed
int check_pair_on(te_ctx* ctx, size_t di, const void* d_a, const void* d_b, uint64_t n, uint64_t nb, pair_verdict& v) {
  int64_t bad = -1; int why = 0;
  int rc = group_check_on(ctx, di, d_a, n, ctx->opt_check_points, &bad, &why);
  if (rc == TE_MSM_EPOINT) v.take(bad, why, 0, kBadPoint); else if (rc) return rc;
  if (!d_b) return 0;
  rc = group_check_on(ctx, di, d_b, nb, ctx->opt_check_points, &bad, &why);
  if (rc == TE_MSM_EPOINT) v.take(bad, why, 1, kBadPoint); else if (rc) return rc;
  return 0;
}

// n pairs (memory of devs[di]; shared: d_b holds one point) -> n affine results at d_out, which may be d_a or d_b; returns when they are there
int add_on(te_ctx* ctx, size_t di, const void* d_a, const void* d_b, uint64_t n, int flags, void* d_out) {
  const int curve = ctx->opt_curve;
  const bool shared = (flags & TE_MSM_ADD_SHARED_B) != 0;
  const int neg = (flags & TE_MSM_ADD_SUBTRACT) ? 1 : 0;
  const size_t pb = sizes_of(curve).point_in;
  return in_pieces(ctx, di, n, kAddPiece, d_out, [&](uint64_t off, uint32_t m, uint4* j4, hipStream_t st) {
    const uint4* a4 = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(d_a) + off * pb);
    const uint4* b4 = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(d_b) + (shared ? 0 : off * pb));
    const dim3 grid((m + 255u) / 256u), block(256);
    with_curve(curve, [&](auto c) {
      with_flag(shared, [&](auto sh) { hipLaunchKernelGGL((te::k_group_add<decltype(c)::value, decltype(sh)::value>), grid, block, 0, st, a4, b4, m, neg, j4); });
    });
  });
}
inline size_t partial_bytes_of(int curve) { return 4u * (curve == TE_MSM_CURVE_BLS12_377_G1 ? te::ga_sizes<1>::TW : te::ga_sizes<0>::TW); }
// count items at d_src (wire points, or -- partials -- projective partials) in the memory of devs[di] -> ONE partial in host memory
// (h_part: partial_bytes_of).  One temporary holds the stage-1 partials and, behind them, the last one.
int sum_fold_on(te_ctx* ctx, size_t di, const void* d_src, uint64_t count, bool partials, uint8_t* h_part) {
  gpu_t& d = ctx->devs[di];
  const size_t tb = partial_bytes_of(ctx->opt_curve);
  const uint32_t m = (uint32_t)count, blocks = std::min<uint32_t>(kSumGrid, (m + GS_BLOCK - 1u) / GS_BLOCK);
  dev_tmp tmp;
  if (int rc = tmp_alloc(ctx, d, tmp, (size_t)(blocks + 1u) * tb)) return rc;
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  hipStream_t st = lane.stream();
  const uint4 *s4 = static_cast<const uint4*>(d_src), *t4c = static_cast<const uint4*>(tmp.p);
  uint4 *t4 = static_cast<uint4*>(tmp.p), *o4 = reinterpret_cast<uint4*>(static_cast<uint8_t*>(tmp.p) + (size_t)blocks * tb);
  const dim3 block(GS_BLOCK);
  with_curve(ctx->opt_curve, [&](auto c) {
    constexpr int C = decltype(c)::value;
    with_flag(partials, [&](auto p) { hipLaunchKernelGGL((te::k_group_sum<C, decltype(p)::value>), dim3(blocks), block, 0, st, s4, m, t4); });
    hipLaunchKernelGGL((te::k_group_sum<C, true>), dim3(1), block, 0, st, t4c, blocks, o4);
  });
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipMemcpyAsync(h_part, o4, tb, hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}
// the partial (its head is a projective slot) -> canonical x || y: sm_affine_group's code, run by the host for this one point
void sum_finish(int curve, const uint8_t* h_part, uint8_t* out) {
  uint32_t w[te::ga_sizes<1>::TW], o[te::sm_sizes<1>::PW];
  memcpy(w, h_part, partial_bytes_of(curve));
  with_curve(curve, [&](auto c) { te::sm_affine_group<decltype(c)::value>(w, 1u, o, te::inv_exp_of<decltype(c)::value>()); });
  memcpy(out, o, sizes_of(curve).point_in);
}

int add_args(te_ctx* ctx, const void* a, const void* b, uint64_t n, int flags, const void* out) {
  if (flags & ~(TE_MSM_ADD_SUBTRACT | TE_MSM_ADD_SHARED_B)) return set_err(ctx, TE_MSM_EINVAL, "te_msm_add*: unknown flag bits");
  if (int rc = check_n(ctx, n)) return rc;
  if (n > 0 && (!a || !b || !out)) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  return 0;
}
// te_msm_add (x_only = false) and te_msm_add_x (true): host buffers, sliced over the devices; the result of a slice lands in its copy of a
int add_host(te_ctx* ctx, const uint8_t* a, const uint8_t* b, bool x_only, uint64_t n, int flags, uint8_t* out) {
  if (int rc = add_args(ctx, a, b, n, flags, out)) return rc;
  if (n == 0) return 0;
  const int curve = ctx->opt_curve;
  const bool shared = (flags & TE_MSM_ADD_SHARED_B) != 0;
  const size_t pb = sizes_of(curve).point_in, ib = x_only ? x_bytes_of(curve) : pb;
  const slice_plan sp(ctx, n);
  struct slice_t { dev_tmp a, b; pair_verdict v; };
  std::vector<slice_t> sl(sp.D);
  auto stage = [&](size_t i) -> int {                             // upload, recover, check, add: everything but the copy out
    const uint64_t lo = sp.lo(i), m = sp.count(i);
    if (m == 0) return 0;
    slice_t& s = sl[i];
    const uint64_t mb = shared ? 1 : m;
    if (int rc = stage_operand(ctx, i, a + lo * ib, x_only, m, s.a, 0, s.v)) return rc;
    if (int rc = stage_operand(ctx, i, b + (shared ? 0 : lo * ib), x_only, mb, s.b, 1, s.v)) return rc;
    if (s.v.bad >= 0) return 0;                                   // (after both: b may hold the lower index)
    if (int rc = check_pair_on(ctx, i, s.a.p, s.b.p, m, mb, s.v)) return rc;
    if (s.v.bad >= 0) return 0;
    return add_on(ctx, i, s.a.p, s.b.p, m, flags, s.a.p);
  };
  if (int rc = te_sched::on_devices(*ctx, sp.D, stage)) return rc;
  if (int rc = note_slices(ctx, sp, sl)) return rc;
  return copy_slices_out(ctx, sp, pb, out, [&](size_t i) { return sl[i].a.p; });
}
// te_msm_sum (x_only = false) and te_msm_sum_x (true): every device folds its slice to one partial; the first device adds the partials
int sum_host(te_ctx* ctx, const uint8_t* src, bool x_only, uint64_t n, uint8_t* out) {
  if (!out) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  if (int rc = check_n(ctx, n)) return rc;
  const int curve = ctx->opt_curve;
  if (n == 0) { write_identity(curve, out); return 0; }
  if (!src) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  const size_t pb = sizes_of(curve).point_in, ib = x_only ? x_bytes_of(curve) : pb, tb = partial_bytes_of(curve);
  const slice_plan sp(ctx, n);
  const size_t D = sp.D;
  struct slice_t { dev_tmp pts; pair_verdict v; bool have = false; };
  std::vector<slice_t> sl(D);
  std::vector<uint8_t> parts(D * tb);
  auto stage = [&](size_t i) -> int {
    const uint64_t m = sp.count(i);
    if (m == 0) return 0;
    slice_t& s = sl[i];
    if (int rc = stage_operand(ctx, i, src + sp.lo(i) * ib, x_only, m, s.pts, 0, s.v)) return rc;
    if (s.v.bad >= 0) return 0;
    if (int rc = check_pair_on(ctx, i, s.pts.p, nullptr, m, 0, s.v)) return rc;
    if (s.v.bad >= 0) return 0;
    if (int rc = sum_fold_on(ctx, i, s.pts.p, m, false, &parts[i * tb])) return rc;
    s.have = true;
    return 0;
  };
  if (int rc = te_sched::on_devices(*ctx, D, stage)) return rc;
  if (int rc = note_slices(ctx, sp, sl)) return rc;
  if (D > 1) {                                                    // the D partial results are added on the first device
    size_t have = 0;                                              // (D <= n: every slice holds points; counted all the same)
    for (size_t i = 0; i < D; i++)
      if (sl[i].have) { if (have != i) memcpy(&parts[have * tb], &parts[i * tb], tb); have++; }
    dev_tmp all;
    if (int rc = tmp_alloc(ctx, ctx->devs[0], all, have * tb)) return rc;
    HIP_TRY(ctx, hipMemcpy(all.p, parts.data(), have * tb, hipMemcpyHostToDevice));
    if (int rc = sum_fold_on(ctx, 0, all.p, have, true, parts.data())) return rc;
  }
  sum_finish(curve, parts.data(), out);
  return 0;
}
// ---- batched field arithmetic (te_msm_field_op*; kernels in field_ops.hip.hpp) ------------------------------------------------------
// One launch over the n elements on the device's check lane, except: a strict inversion runs k_field_zero_scan in front and waits for
// its verdict; an inversion runs in pieces of kFieldInvPiece elements that share one slab; a square root of the device form writes into
// a temporary of the call's own and is copied to d_out when no element was reported.  A failure is the check lane's report word
// (check_code / check_decode): reason 1 zero, 2 not a square.  SHARED_B: the one record (or exponent) is a kernel argument, read to
// the host first -- no lane reads b, so d_out == d_b needs no care there.
constexpr uint64_t kFieldInvPiece = 1ull << 20;
struct field_req { int field = 0, op = 0, flags = 0; te::fo_rec shared = {}; uint32_t group = FO_INV_GROUP_DEFAULT; };
inline size_t field_bytes_of(int field) { return field == TE_MSM_FIELD_Q377 ? 48 : 32; }
inline bool field_op_binary(int op) { return op == TE_MSM_FIELD_ADD || op == TE_MSM_FIELD_SUB || op == TE_MSM_FIELD_MUL || op == TE_MSM_FIELD_POW; }
// bytes of one record of b: an exponent is 32 bytes on both fields
inline size_t field_b_bytes_of(const field_req& q) { return q.op == TE_MSM_FIELD_POW ? 32 : field_bytes_of(q.field); }
// elements of one inversion chain: FO_INV_GROUP_DEFAULT (measured; read-only option "field_inv_group"), or what TE_MSM_FIELD_INV_GROUP
// names (1 .. FO_INV_GROUP_MAX: tools/field_ops_cost.py measures the candidates with it)
uint32_t field_inv_group() {
  const char* e = getenv("TE_MSM_FIELD_INV_GROUP");
  const long v = e ? atol(e) : 0;
  return v >= 1 && v <= (long)FO_INV_GROUP_MAX ? (uint32_t)v : FO_INV_GROUP_DEFAULT;
}
template <typename F> void with_limbs(int field, F&& f) {
  if (field == TE_MSM_FIELD_Q377) f(std::integral_constant<int, 14>{});
  else f(std::integral_constant<int, 9>{});
}
// k_field_map for add, sub, mul, double, neg, square: MONT is a template parameter of the products alone (field_ops.hip.hpp)
template <int N> void launch_field_map(const field_req& q, dim3 grid, hipStream_t st, const uint4* a, const uint4* b, uint32_t m, uint4* o) {
  const bool shared = (q.flags & TE_MSM_FIELD_SHARED_B) != 0, mont = (q.flags & TE_MSM_FIELD_MONTGOMERY) != 0;
  auto go = [&](auto op, auto mt, auto bs) {
    hipLaunchKernelGGL((te::k_field_map<N, decltype(op)::value, decltype(mt)::value, decltype(bs)::value>), grid, dim3(256), 0, st, a, b, q.shared, m, o);
  };
  using std::integral_constant;
  const integral_constant<int, te::FO_B_ARRAY> arr; const integral_constant<int, te::FO_B_SHARED> sh; const integral_constant<int, te::FO_B_IS_A> same;
  const integral_constant<int, te::FO_ADD> add; const integral_constant<int, te::FO_SUB> sub; const integral_constant<int, te::FO_MUL> mul; const integral_constant<int, te::FO_NEG> neg;
  const std::false_type plain; const std::true_type mg;
  switch (q.op) {
    case TE_MSM_FIELD_ADD: if (shared) go(add, plain, sh); else go(add, plain, arr); break;
    case TE_MSM_FIELD_DOUBLE: go(add, plain, same); break;
    case TE_MSM_FIELD_SUB: if (shared) go(sub, plain, sh); else go(sub, plain, arr); break;
    case TE_MSM_FIELD_NEG: go(neg, plain, same); break;
    case TE_MSM_FIELD_MUL:
      if (mont) { if (shared) go(mul, mg, sh); else go(mul, mg, arr); }
      else { if (shared) go(mul, plain, sh); else go(mul, plain, arr); }
      break;
    default: if (mont) go(mul, mg, same); else go(mul, plain, same); break;   // TE_MSM_FIELD_SQUARE
  }
}
// n elements a (and b) in the memory of devs[di] -> d_out, which may be d_a or d_b; returns when they are there.  TE_MSM_EFIELD: *bad /
// *why hold the lowest failing index and its reason, and d_out is as it was -- unless out_is_scratch (the host form's staged copy), which
// a failed square root leaves undefined
int field_on(te_ctx* ctx, size_t di, const field_req& q, const void* d_a, const void* d_b, uint64_t n, void* d_out, bool out_is_scratch, int64_t* bad, int* why) {
  *bad = -1; *why = 0;
  if (n == 0) return 0;
  gpu_t& d = ctx->devs[di];
  const size_t eb = field_bytes_of(q.field);
  const bool mont = (q.flags & TE_MSM_FIELD_MONTGOMERY) != 0, shared = (q.flags & TE_MSM_FIELD_SHARED_B) != 0;
  const uint32_t m = (uint32_t)n;
  dev_tmp tmp;                                                      // the slab of an inversion's piece, or a square root's results
  const uint64_t piece = std::min(n, kFieldInvPiece);
  if (q.op == TE_MSM_FIELD_INV) { if (int rc = tmp_alloc(ctx, d, tmp, piece * (q.field == TE_MSM_FIELD_Q377 ? 64 : 48))) return rc; }
  if (q.op == TE_MSM_FIELD_SQRT && !out_is_scratch) { if (int rc = tmp_alloc(ctx, d, tmp, n * eb)) return rc; }
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  hipStream_t st = lane.stream();
  const uint4 *a4 = static_cast<const uint4*>(d_a), *b4 = static_cast<const uint4*>(d_b);
  uint4* o4 = static_cast<uint4*>(d_out);
  const dim3 grid((m + 255u) / 256u), block(256);
  int rc = 0;
  with_limbs(q.field, [&](auto nl) {
    constexpr int N = decltype(nl)::value;
    with_flag(mont, [&](auto mt) {
      constexpr bool M = decltype(mt)::value;
      if (q.op == TE_MSM_FIELD_INV) {
        if (!(q.flags & TE_MSM_FIELD_ZERO_OK)) {
          rc = [&]() -> int {
            HIP_TRY(ctx, hipMemsetAsync(d.chk_word, 0, sizeof(unsigned long long), st));
            hipLaunchKernelGGL(te::k_field_zero_scan<N>, grid, block, 0, st, a4, m, d.chk_word, n, (uint64_t)0);
            HIP_TRY(ctx, hipGetLastError());
            return lane.verdict(ctx, n, bad, why);
          }();
          if (rc) return;
        }
        for (uint64_t off = 0; off < n; off += piece) {
          const uint32_t pm = (uint32_t)std::min(piece, n - off);
          const dim3 igrid((pm + 256u * q.group - 1u) / (256u * q.group));
          hipLaunchKernelGGL((te::k_field_inv<N, M>), igrid, block, 0, st, a4 + off * (eb / 16), pm, q.group, static_cast<uint4*>(tmp.p), (uint32_t)piece,
                             o4 + off * (eb / 16), N == 9 ? te::kInvExpTe : te::kInvExp377);
        }
      } else if (q.op == TE_MSM_FIELD_POW) {
        with_flag(shared, [&](auto sh) { hipLaunchKernelGGL((te::k_field_pow<N, M, decltype(sh)::value>), grid, block, 0, st, a4, b4, q.shared, m, o4); });
      } else if (q.op == TE_MSM_FIELD_SQRT) {
        uint4* r4 = out_is_scratch ? o4 : static_cast<uint4*>(tmp.p);
        rc = [&]() -> int {
          HIP_TRY(ctx, hipMemsetAsync(d.chk_word, 0, sizeof(unsigned long long), st));
          hipLaunchKernelGGL((te::k_field_sqrt<N, M>), grid, block, 0, st, a4, m, r4, d.chk_word, n, (uint64_t)0, N == 9 ? te::kRootExpTe : te::kRootExp377);
          HIP_TRY(ctx, hipGetLastError());
          if (int v = lane.verdict(ctx, n, bad, why)) return v;
          if (!out_is_scratch) HIP_TRY(ctx, hipMemcpyAsync(d_out, tmp.p, n * eb, hipMemcpyDeviceToDevice, st));
          return 0;
        }();
      } else {
        launch_field_map<N>(q, grid, st, a4, b4, m, o4);            // (reads the flag itself: only a product has two forms)
      }
    });
  });
  if (rc == TE_MSM_EPOINT) return TE_MSM_EFIELD;                    // (the lane's verdict: an element was reported)
  if (rc) return rc;
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}
// a failed element as the outcome of a call: remembered for get_option ("bad_field_index" / "bad_field_reason"), described in the error text
int note_bad_field(te_ctx* ctx, int64_t index, int reason) {
  ctx->bad_field_index = index; ctx->bad_field_reason = reason;
  char buf[160];
  snprintf(buf, sizeof buf, "field element %lld has no result (reason %d): %s", (long long)index, reason,
           reason == TE_MSM_FIELD_ZERO ? "the inverse of 0 (TE_MSM_FIELD_ZERO_OK writes 0 instead)" : "not a square");
  return set_err(ctx, TE_MSM_EFIELD, buf);
}
// what every te_msm_field_op* call checks first; q: the request, its shared record still empty
int field_args(te_ctx* ctx, int field, int op, const void* a, const void* b, uint64_t n, int flags, const void* out, field_req& q) {
  if (field != TE_MSM_FIELD_P && field != TE_MSM_FIELD_Q377) return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_op*: unknown field");
  if (op < TE_MSM_FIELD_ADD || op > TE_MSM_FIELD_SQRT) return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_op*: unknown op");
  if (flags & ~(TE_MSM_FIELD_SHARED_B | TE_MSM_FIELD_MONTGOMERY | TE_MSM_FIELD_ZERO_OK)) return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_op*: unknown flag bits");
  if ((flags & TE_MSM_FIELD_ZERO_OK) && op != TE_MSM_FIELD_INV) return set_err(ctx, TE_MSM_EINVAL, "TE_MSM_FIELD_ZERO_OK belongs to TE_MSM_FIELD_INV alone");
  if (!field_op_binary(op) && (b || (flags & TE_MSM_FIELD_SHARED_B))) return set_err(ctx, TE_MSM_EINVAL, "this op takes one operand: b must be NULL, without TE_MSM_FIELD_SHARED_B");
  if (int rc = check_n(ctx, n)) return rc;
  if (n > 0 && (!a || !out || (field_op_binary(op) && !b))) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  q.field = field; q.op = op; q.flags = flags; q.group = field_inv_group();
  return 0;
}
// the one record of b under SHARED_B (host memory) into the request
void field_take_shared(field_req& q, const uint8_t* rec) {
  memcpy(q.shared.w, rec, field_b_bytes_of(q));
  uint32_t e[8];
  memcpy(e, q.shared.w, 32);
  q.shared.top = te::fo_exp_top(e);
}
// te_msm_field_op: host buffers, sliced over the devices; the result of a slice lands in its copy of a
int field_host(te_ctx* ctx, field_req& q, const uint8_t* a, const uint8_t* b, uint64_t n, uint8_t* out) {
  const bool shared = (q.flags & TE_MSM_FIELD_SHARED_B) != 0, binary = field_op_binary(q.op);
  const size_t eb = field_bytes_of(q.field), bb = field_b_bytes_of(q);
  if (shared) field_take_shared(q, b);
  const slice_plan sp(ctx, n);
  struct slice_t { dev_tmp a, b; int64_t bad = -1; int why = 0; };
  std::vector<slice_t> sl(sp.D);
  auto stage = [&](size_t i) -> int {                             // upload and compute: everything but the copy out
    const uint64_t lo = sp.lo(i), m = sp.count(i);
    if (m == 0) return 0;
    slice_t& s = sl[i];
    if (int rc = tmp_alloc(ctx, ctx->devs[i], s.a, m * eb)) return rc;
    HIP_TRY(ctx, hipMemcpy(s.a.p, a + lo * eb, m * eb, hipMemcpyHostToDevice));
    if (binary && !shared) {
      if (int rc = tmp_alloc(ctx, ctx->devs[i], s.b, m * bb)) return rc;
      HIP_TRY(ctx, hipMemcpy(s.b.p, b + lo * bb, m * bb, hipMemcpyHostToDevice));
    }
    const int rc = field_on(ctx, i, q, s.a.p, s.b.p, m, s.a.p, true, &s.bad, &s.why);
    return rc == TE_MSM_EFIELD ? 0 : rc;
  };
  if (int rc = te_sched::on_devices(*ctx, sp.D, stage)) return rc;
  for (size_t i = 0; i < sp.D; i++)                               // slices in order: the first that reports holds the lowest index
    if (sl[i].bad >= 0) return note_bad_field(ctx, (int64_t)sp.lo(i) + sl[i].bad, sl[i].why);
  return copy_slices_out(ctx, sp, eb, out, [&](size_t i) { return sl[i].a.p; });
}

// ---- batched NTTs over p (te_msm_ntt*; kernels in ntt.hip.hpp, plan in ntt_plan.hpp) -------------------------------------------------
// `count` transforms on the device's check lane, in pieces of the plan's piece_transforms; a piece runs the plan's passes back to back:
// a -> out (one pass), or a -> tmp (-> tmp) -> out, tmp the device's scratch buffer (grown on use, held like the tables; the lane's mutex
// serialises its users).  The twiddle tables of the device are built by the
// first call (k_ntt_table from Omega = W^(2^23) and Omega^4096, computed here with the host build of the field) and stay until
// te_msm_trim / destroy; a call with a shift builds its two tables of powers of s (forward) or 1 / s (inverse) the same way, with
// the decoding / encoding constant folded into the hi table.  1 / s and 1 / n are one fe_inv each, here.
using te::ntt_req;
// entries of one table on st: g^j, times pre as a plain factor when with_pre (k_ntt_table)
void ntt_table_launch(hipStream_t st, const te::fel<9>& g, const te::fel<9>& pre, bool with_pre, uint32_t* out) {
  hipLaunchKernelGGL(te::k_ntt_table, dim3(te_ntt::kTabEntries / 256u), dim3(256), 0, st, g, pre, with_pre ? 1 : 0, out);
}
// the twiddle tables of d, built on st (the lane's stream, held by the caller)
int ntt_tables_on(te_ctx* ctx, gpu_t& d, hipStream_t st) {
  if (d.ntt_tab.p) return 0;
  if (int rc = make_room(ctx, d.ntt_tab, 2 * te_ntt::kTabBytes / sizeof(uint32_t))) return rc;
  te::fel<9> hi, lo;
  te::ntt_twiddle_gens(hi, lo);
  ntt_table_launch(st, hi, hi, false, d.ntt_tab.p);
  ntt_table_launch(st, lo, lo, false, d.ntt_tab.p + te_ntt::kTabEntries * te_ntt::kTabWords);
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
int ntt_on(te_ctx* ctx, size_t di, const ntt_req& q, const void* d_a, uint64_t count, void* d_out) {
  if (count == 0) return 0;
  gpu_t& d = ctx->devs[di];
  const te_ntt::plan P = te_ntt::make_plan(q.log_n);
  dev_tmp sh;
  if (q.shifted) { if (int rc = tmp_alloc(ctx, d, sh, 2 * te_ntt::kTabBytes)) return rc; }
  const te::ntt_consts k = te::ntt_consts_of(q);
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  hipStream_t st = lane.stream();
  if (int rc = ntt_tables_on(ctx, d, st)) return rc;
  // tmp is the device's own, grown on use and kept (allocating and freeing 32 MB a call cost more than the three passes over it)
  if (P.passes > 1) { if (int rc = make_room(ctx, d.ntt_tmp, (size_t)te_ntt::tmp_records_for(P, count) * 32)) return rc; }
  uint8_t* const tmp = d.ntt_tmp.p;
  te::ntt_tabs tb;
  tb.hi = d.ntt_tab.p; tb.lo = d.ntt_tab.p + te_ntt::kTabEntries * te_ntt::kTabWords;
  tb.sh_hi = tb.sh_lo = nullptr;
  if (q.shifted) {
    uint32_t* t = static_cast<uint32_t*>(sh.p);
    te::fel<9> hi, lo;
    te::ntt_shift_gens(q, hi, lo);
    ntt_table_launch(st, hi, q.inverse ? k.enc : k.dec, true, t);
    ntt_table_launch(st, lo, lo, false, t + te_ntt::kTabEntries * te_ntt::kTabWords);
    tb.sh_hi = t; tb.sh_lo = t + te_ntt::kTabEntries * te_ntt::kTabWords;
  }
  const size_t rec4 = (size_t)2 << q.log_n;                          // 16-byte words of one transform
  for (uint64_t off = 0; off < count; off += P.piece_transforms) {
    const uint64_t m = std::min(P.piece_transforms, count - off);
    const uint4* a4 = static_cast<const uint4*>(d_a) + off * rec4;
    uint4* o4 = static_cast<uint4*>(d_out) + off * rec4;
    for (uint32_t p = 0; p < P.passes; p++) {
      const te_ntt::pass& ps = P.p[p];
      const uint4* src = p == 0 ? a4 : reinterpret_cast<const uint4*>(tmp);
      uint4* dst = p + 1 == P.passes ? o4 : reinterpret_cast<uint4*>(tmp);
      const dim3 grid((uint32_t)te_ntt::tiles_of(ps, m)), block(te_ntt::kLanes);
      const uint64_t lines = te_ntt::lines_of(ps, m);
      with_flag(q.inverse, [&](auto inv) {
        with_flag(q.shifted, [&](auto shf) {
          hipLaunchKernelGGL((te::k_ntt_pass<decltype(inv)::value, decltype(shf)::value>), grid, block, 0, st, src, dst, ps, lines, k, tb);
        });
      });
    }
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}
// what every te_msm_ntt* call checks first (te::ntt_check); q: the request
int ntt_args(te_ctx* ctx, const void* a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, const void* out, ntt_req& q) {
  switch (te::ntt_check(a, log_n, count, flags, shift, out, q)) {
    case te::NTT_OK: return 0;
    case te::NTT_BAD_LOG_N: return set_err(ctx, TE_MSM_EINVAL, "te_msm_ntt*: log_n is above TE_MSM_NTT_MAX_LOG_N");
    case te::NTT_BAD_FLAGS: return set_err(ctx, TE_MSM_EINVAL, "te_msm_ntt*: unknown flag bits");
    case te::NTT_TOO_LARGE: return set_err(ctx, TE_MSM_EINVAL, "te_msm_ntt*: count x n x 32 does not fit 64 bits");
    case te::NTT_NULL: return set_err(ctx, TE_MSM_EINVAL, "null buffer");
    default: return set_err(ctx, TE_MSM_EINVAL, "te_msm_ntt*: the shift is 0 mod p");
  }
}
// te_msm_ntt: host buffers, whole transforms sliced over the devices; a slice is transformed in place in its staged copy
int ntt_host(te_ctx* ctx, const ntt_req& q, const uint8_t* a, uint64_t count, uint8_t* out) {
  const size_t tb = (size_t)32 << q.log_n;
  const slice_plan sp(ctx, count);
  struct slice_t { dev_tmp a; };
  std::vector<slice_t> sl(sp.D);
  auto stage = [&](size_t i) -> int {
    const uint64_t lo = sp.lo(i), m = sp.count(i);
    if (m == 0) return 0;
    if (int rc = tmp_alloc(ctx, ctx->devs[i], sl[i].a, m * tb)) return rc;
    HIP_TRY(ctx, hipMemcpy(sl[i].a.p, a + lo * tb, m * tb, hipMemcpyHostToDevice));
    return ntt_on(ctx, i, q, sl[i].a.p, m, sl[i].a.p);
  };
  if (int rc = te_sched::on_devices(*ctx, sp.D, stage)) return rc;
  return copy_slices_out(ctx, sp, tb, out, [&](size_t i) { return sl[i].a.p; });
}

// ---- polynomial openings (te_msm_poly_divide*; kernels in poly.hip.hpp, plan in poly_plan.hpp) ---------------------------------------
// `count` polynomials on the device's check lane: the powers of the points (computed here with the host build of the field: 25 products
// a point and level) go up behind the regions of the device's scratch buffer (grown on use, held like ntt_tmp; the lane's mutex
// serialises its users); k_poly_sums runs level by level upwards -- the one record a polynomial of the last region is a(z) -- and
// k_poly_apply level by level downwards, each level's quotient over its sums, the last launch a -> q.  No piece loop: the buffer is about
// count n / T records.
static_assert(TE_MSM_POLY_CHUNK == te_poly::kChunkDefault && TE_MSM_POLY_MAX_N == te_poly::kMaxN, "include/te_msm.h and poly_plan.hpp disagree");
using te::poly_req;
// z: the points on the host (count records, or one); evals: where the count evaluations go on the host once everything succeeded, or
// nullptr; d_q: nullptr evaluates only
int poly_on(te_ctx* ctx, size_t di, const poly_req& r, const void* d_a, uint64_t count, const uint8_t* z, uint8_t* evals, void* d_q) {
  if (count == 0) return 0;
  gpu_t& d = ctx->devs[di];
  te_poly::plan P;
  if (!te_poly::make_plan(r.n, count, r.chunk, r.shared, P)) return set_err(ctx, TE_MSM_EINVAL, "te_msm_poly_divide*: more tiles than one launch holds");
  std::vector<uint32_t> pows((size_t)P.pow_words);
  te::poly_pow_table(P, z, r.mont, pows.data());
  std::vector<uint8_t> ev(evals ? (size_t)count * 32 : 0);
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  hipStream_t st = lane.stream();
  if (int rc = make_room(ctx, d.poly_tmp, (size_t)P.scratch_bytes)) return rc;
  uint4* const reg = reinterpret_cast<uint4*>(d.poly_tmp.p);
  uint32_t* const d_pows = reinterpret_cast<uint32_t*>(d.poly_tmp.p + P.records * 32u);
  HIP_TRY(ctx, hipMemcpyAsync(d_pows, pows.data(), pows.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  const uint64_t pow_stride = P.points == 1u ? 0 : te_poly::pow_word(P, 1, 0, 0);
  const dim3 block(te_poly::kLanes);
  for (uint32_t l = 0; l < P.levels; l++) {
    const te_poly::level& v = P.lv[l];
    const uint4* src = l ? reg + v.src * 2 : static_cast<const uint4*>(d_a);
    hipLaunchKernelGGL(te::k_poly_sums, dim3((uint32_t)(count * v.tiles)), block, 0, st, src, reg + v.dst * 2, v, P.chunk, d_pows + te_poly::pow_word(P, 0, l, 0), pow_stride);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (evals) HIP_TRY(ctx, hipMemcpyAsync(ev.data(), reg + P.lv[P.levels - 1].dst * 2, ev.size(), hipMemcpyDeviceToHost, st));
  if (d_q) {
    const size_t lds = te_poly::lds_bytes_apply(P.chunk);
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&te::k_poly_apply), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (uint32_t l = P.levels; l-- > 0u;) {
      const te_poly::level& v = P.lv[l];
      const uint4* src = l ? reg + v.src * 2 : static_cast<const uint4*>(d_a);
      uint4* dst = l ? reg + v.src * 2 : static_cast<uint4*>(d_q);
      const uint4* carries = l + 1u < P.levels ? reg + v.dst * 2 : nullptr;
      hipLaunchKernelGGL(te::k_poly_apply, dim3((uint32_t)(count * v.tiles)), block, lds, st, src, dst, carries, v, P.chunk, d_pows + te_poly::pow_word(P, 0, l, 0), pow_stride);
    }
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (evals) memcpy(evals, ev.data(), ev.size());
  return 0;
}
// what every te_msm_poly_divide* call checks first (te::poly_check); r: the request
int poly_args(te_ctx* ctx, const void* a, uint64_t n, uint64_t count, const uint8_t* z, int flags, const void* evals, const void* q, poly_req& r) {
  switch (te::poly_check(a, n, count, z, flags, evals, q, r)) {
    case te::POLY_OK: r.chunk = te_poly::chunk_for(n, te_poly::chunk_in_force()); return 0;
    case te::POLY_BAD_N: return set_err(ctx, TE_MSM_EINVAL, "te_msm_poly_divide*: n must be in [1, TE_MSM_POLY_MAX_N]");
    case te::POLY_BAD_FLAGS: return set_err(ctx, TE_MSM_EINVAL, "te_msm_poly_divide*: unknown flag bits");
    case te::POLY_NO_OUTPUT: return set_err(ctx, TE_MSM_EINVAL, "te_msm_poly_divide*: evals and q are both NULL");
    case te::POLY_TOO_LARGE: return set_err(ctx, TE_MSM_EINVAL, "te_msm_poly_divide*: count x n x 32 does not fit 64 bits");
    default: return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  }
}
// te_msm_poly_divide: host buffers, whole polynomials sliced over the devices; a slice is divided in place in its staged copy, and the
// outputs are written once every slice succeeded
int poly_host(te_ctx* ctx, const poly_req& r, const uint8_t* a, uint64_t count, const uint8_t* z, uint8_t* evals, uint8_t* q) {
  const size_t pb = (size_t)r.n * 32;
  const slice_plan sp(ctx, count);
  struct slice_t { dev_tmp a; };
  std::vector<slice_t> sl(sp.D);
  std::vector<uint8_t> ev(evals ? (size_t)count * 32 : 0);
  auto stage = [&](size_t i) -> int {
    const uint64_t lo = sp.lo(i), m = sp.count(i);
    if (m == 0) return 0;
    if (int rc = tmp_alloc(ctx, ctx->devs[i], sl[i].a, m * pb)) return rc;
    HIP_TRY(ctx, hipMemcpy(sl[i].a.p, a + lo * pb, m * pb, hipMemcpyHostToDevice));
    return poly_on(ctx, i, r, sl[i].a.p, m, r.shared ? z : z + lo * 32, evals ? ev.data() + lo * 32 : nullptr, q ? sl[i].a.p : nullptr);
  };
  if (int rc = te_sched::on_devices(*ctx, sp.D, stage)) return rc;
  if (q) { if (int rc = copy_slices_out(ctx, sp, pb, q, [&](size_t i) { return sl[i].a.p; })) return rc; }
  if (evals) memcpy(evals, ev.data(), ev.size());
  return 0;
}

// ---- sparse matrices (te_msm_bind_matrix, te_msm_spmv*; kernels in spmv.hip.hpp, plan in spmv_plan.hpp) --------------------------------
// A bind converts the values on the host (one product an entry with the host build of the field), fills the row ids, builds the
// transpose when asked, and copies one allocation a side to every device.  A call runs on the device's check lane: k_spmv_tile over
// count x tiles blocks (none for a matrix without entries), k_spmv_rows behind it; the fragments live in the device's spmv_tmp, grown on
// use like poly_tmp.  No piece loop: x and out are the caller's.
static_assert(TE_MSM_SPMV_CHUNK == te_spmv::kChunkDefault, "include/te_msm.h and spmv_plan.hpp disagree");
const char* const kBadMatrix = "not a bound matrix of this context (released, or bound to another context)";
// one side as the host holds it before the upload: te_spmv::layout_of(rows, nnz) in one buffer
struct matrix_image {
  te_spmv::layout lay; std::vector<uint8_t> bytes;
  matrix_image(uint64_t rows, uint64_t nnz) : lay(te_spmv::layout_of(rows, nnz)), bytes((size_t)lay.bytes) {}
  uint8_t* vals() { return bytes.data() + lay.vals; }
  uint64_t* ptr() { return reinterpret_cast<uint64_t*>(bytes.data() + lay.ptr); }
  uint32_t* col() { return reinterpret_cast<uint32_t*>(bytes.data() + lay.col); }
  uint32_t* row() { return reinterpret_cast<uint32_t*>(bytes.data() + lay.row); }
};
int matrix_upload(te_ctx* ctx, size_t i, const matrix_image& img, uint8_t** where) {
  HIP_TRY(ctx, hipSetDevice(ctx->devs[i].device));
  HIP_TRY(ctx, hipMalloc((void**)where, img.bytes.size()));                 // (freed by the caller on failure: free_matrix)
  HIP_TRY(ctx, hipMemcpy(*where, img.bytes.data(), img.bytes.size(), hipMemcpyHostToDevice));
  return 0;
}
te::spmv_side side_at(const uint8_t* base, uint64_t rows, uint64_t nnz) {
  const te_spmv::layout l = te_spmv::layout_of(rows, nnz);
  return te::spmv_side{reinterpret_cast<const uint4*>(base + l.vals), reinterpret_cast<const uint64_t*>(base + l.ptr), reinterpret_cast<const uint32_t*>(base + l.col),
                       reinterpret_cast<const uint32_t*>(base + l.row)};
}
// `count` vectors at d_x (memory of devs[di]) -> d_out; tr: by the transpose.  Returns when d_out is complete
int spmv_on(te_ctx* ctx, size_t di, const te_matrix* M, bool tr, uint32_t chunk, const void* d_x, uint64_t count, void* d_out) {
  if (count == 0) return 0;
  gpu_t& d = ctx->devs[di];
  te_spmv::plan P;
  if (!te_spmv::make_plan(tr ? M->cols : M->rows, tr ? M->rows : M->cols, M->nnz, count, chunk, P))
    return set_err(ctx, TE_MSM_EINVAL, "te_msm_spmv*: count x rows x 32 does not fit 64 bits, or more blocks than one launch holds");
  const te::spmv_side side = side_at(tr ? M->side_t[di] : M->side[di], P.rows, P.nnz);
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  hipStream_t st = lane.stream();
  if (P.scratch_bytes) { if (int rc = make_room(ctx, d.spmv_tmp, (size_t)P.scratch_bytes)) return rc; }
  uint4* const frag = reinterpret_cast<uint4*>(d.spmv_tmp.p);
  const dim3 block(te_spmv::kLanes);
  if (P.tiles > 0) {
    const size_t lds = te_spmv::lds_bytes(P.chunk);
    HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&te::k_spmv_tile), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(te::k_spmv_tile, dim3((uint32_t)(count * P.tiles)), block, lds, st, side, P, static_cast<const uint4*>(d_x), static_cast<uint4*>(d_out), frag);
  }
  hipLaunchKernelGGL(te::k_spmv_rows, dim3((uint32_t)(count * P.per)), block, 0, st, side, P, static_cast<uint4*>(d_out), frag);
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}
// what every te_msm_spmv* call checks first (te::spmv_check_call); go: there is something to run
int spmv_args(te_ctx* ctx, const te_matrix* M, const void* x, uint64_t count, int flags, const void* out, bool* go) {
  *go = false;
  if (!M || std::find(ctx->matrices.begin(), ctx->matrices.end(), M) == ctx->matrices.end()) return set_err(ctx, TE_MSM_EINVAL, kBadMatrix);
  switch (te::spmv_check_call(M->with_t, M->rows, M->cols, x, count, flags, out)) {
    case te::SPMV_OK: *go = count > 0; return 0;
    case te::SPMV_BAD_FLAGS: return set_err(ctx, TE_MSM_EINVAL, "te_msm_spmv*: unknown flag bits");
    case te::SPMV_NO_TRANSPOSE: return set_err(ctx, TE_MSM_EINVAL, "te_msm_spmv*: the matrix was bound without TE_MSM_MATRIX_TRANSPOSE");
    case te::SPMV_IN_PLACE: return set_err(ctx, TE_MSM_EINVAL, "te_msm_spmv*: out must not be x (the product gathers from x)");
    case te::SPMV_TOO_LARGE: return set_err(ctx, TE_MSM_EINVAL, "te_msm_spmv*: count x rows x 32 does not fit 64 bits");
    default: return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  }
}
// te_msm_spmv: host buffers, whole vectors sliced over the devices; out is written once every slice succeeded
int spmv_host(te_ctx* ctx, const te_matrix* M, bool tr, uint32_t chunk, const uint8_t* x, uint64_t count, uint8_t* out) {
  const size_t xb = (size_t)(tr ? M->rows : M->cols) * 32, ob = (size_t)(tr ? M->cols : M->rows) * 32;
  const slice_plan sp(ctx, count);
  struct slice_t { dev_tmp x, out; };
  std::vector<slice_t> sl(sp.D);
  auto stage = [&](size_t i) -> int {
    const uint64_t lo = sp.lo(i), m = sp.count(i);
    if (m == 0) return 0;
    if (int rc = tmp_alloc(ctx, ctx->devs[i], sl[i].x, m * xb)) return rc;
    if (int rc = tmp_alloc(ctx, ctx->devs[i], sl[i].out, m * ob)) return rc;
    HIP_TRY(ctx, hipMemcpy(sl[i].x.p, x + lo * xb, m * xb, hipMemcpyHostToDevice));
    return spmv_on(ctx, i, M, tr, chunk, sl[i].x.p, m, sl[i].out.p);
  };
  if (int rc = te_sched::on_devices(*ctx, sp.D, stage)) return rc;
  return copy_slices_out(ctx, sp, ob, out, [&](size_t i) { return sl[i].out.p; });
}
// ---- prefix sums and products (te_msm_field_scan*; kernels in scan.hip.hpp, plan in scan_plan.hpp) ------------------------------------
// `count` vectors on the device's check lane: the seeds (put into the internal form here with the host build of the field: one product a
// vector) go up behind the regions of the device's scratch buffer (grown on use, held like poly_tmp; the lane's mutex serialises its
// users); k_scan_totals runs level by level upwards -- the one record a vector of the last region is the total, seed included -- and
// k_scan_apply level by level downwards, each level's exclusive scan over its elements, the last launch a -> out.  No piece loop: the
// buffer is about count n / T records.
static_assert(TE_MSM_SCAN_CHUNK == te_scan::kChunkDefault && TE_MSM_SCAN_MAX_N == te_scan::kMaxN && TE_MSM_SCAN_SUM == te_scan::kSum && TE_MSM_SCAN_PRODUCT == te_scan::kProduct,
              "include/te_msm.h and scan_plan.hpp disagree");
using te::scan_req;
template <int OP> int scan_launches(te_ctx* ctx, hipStream_t st, const scan_req& r, const te_scan::plan& P, uint4* reg, const void* d_a, bool want_totals, void* d_out) {
  const dim3 block(te_scan::kLanes);
  const uint4* const seeds = reg + P.seeds * 2;
  const uint32_t caller = te::scan_caller_form(r);
  for (uint32_t l = 0; l < P.levels; l++) {
    const te_scan::level& v = P.lv[l];
    const bool last = l + 1u == P.levels;
    if (last && !want_totals) break;
    const uint4* src = l ? reg + v.src * 2 : static_cast<const uint4*>(d_a);
    hipLaunchKernelGGL(te::k_scan_totals<OP>, dim3((uint32_t)(P.count * v.tiles)), block, 0, st, src, reg + v.dst * 2, last ? seeds : nullptr, v, P.chunk,
                       l ? (uint32_t)te_scan::kInternal : caller, last ? caller : (uint32_t)te_scan::kInternal, l == 0u && r.shared ? 1u : 0u);
  }
  HIP_TRY(ctx, hipGetLastError());
  if (!d_out) return 0;
  const size_t lds = te_scan::lds_bytes_apply(P.chunk);
  HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&te::k_scan_apply<OP>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  for (uint32_t l = P.levels; l-- > 0u;) {
    const te_scan::level& v = P.lv[l];
    const uint4* src = l ? reg + v.src * 2 : static_cast<const uint4*>(d_a);
    uint4* dst = l ? reg + v.src * 2 : static_cast<uint4*>(d_out);
    const uint4* carries = l + 1u < P.levels ? reg + v.dst * 2 : seeds;
    hipLaunchKernelGGL(te::k_scan_apply<OP>, dim3((uint32_t)(P.count * v.tiles)), block, lds, st, src, dst, carries, v, P.chunk, l ? (uint32_t)te_scan::kInternal : caller,
                       l ? (uint32_t)te_scan::kInternal : caller, l || r.exclusive ? 1u : 0u, l == 0u && r.shared ? 1u : 0u);
  }
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}
// init: the seeds on the host (count records) or nullptr; totals: where the count totals go on the host once everything succeeded, or
// nullptr; d_out: nullptr leaves the device's buffers alone
int scan_on(te_ctx* ctx, size_t di, const scan_req& q, const void* d_a, uint64_t count, const uint8_t* init, uint8_t* totals, void* d_out) {
  if (count == 0) return 0;
  gpu_t& d = ctx->devs[di];
  scan_req r = q;
  r.count = count;
  te_scan::plan P;
  if (!te_scan::make_plan(r.n, count, r.chunk, P)) return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_scan*: more tiles than one launch holds");
  std::vector<uint8_t> seeds((size_t)count * 32), tot(totals ? (size_t)count * 32 : 0);
  te::scan_seeds(r, init, seeds.data());
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  hipStream_t st = lane.stream();
  if (int rc = make_room(ctx, d.scan_tmp, (size_t)P.scratch_bytes)) return rc;
  uint4* const reg = reinterpret_cast<uint4*>(d.scan_tmp.p);
  HIP_TRY(ctx, hipMemcpyAsync(reg + P.seeds * 2, seeds.data(), seeds.size(), hipMemcpyHostToDevice, st));
  if (int rc = r.op == TE_MSM_SCAN_SUM ? scan_launches<te_scan::kSum>(ctx, st, r, P, reg, d_a, totals != nullptr, d_out)
                                       : scan_launches<te_scan::kProduct>(ctx, st, r, P, reg, d_a, totals != nullptr, d_out)) return rc;
  if (totals) HIP_TRY(ctx, hipMemcpyAsync(tot.data(), reg + P.lv[P.levels - 1].dst * 2, tot.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(ctx, hipStreamSynchronize(st));
  if (totals) memcpy(totals, tot.data(), tot.size());
  return 0;
}
// what every te_msm_field_scan* call checks first (te::scan_check); r: the request
int scan_args(te_ctx* ctx, int op, const void* a, uint64_t n, uint64_t count, int flags, const void* totals, const void* out, scan_req& r) {
  switch (te::scan_check(op, a, n, count, flags, totals, out, r)) {
    case te::SCAN_OK: r.chunk = te_scan::chunk_for(n, te_scan::chunk_in_force()); return 0;
    case te::SCAN_BAD_OP: return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_scan*: op must be TE_MSM_SCAN_SUM or TE_MSM_SCAN_PRODUCT");
    case te::SCAN_BAD_N: return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_scan*: n must be in [1, TE_MSM_SCAN_MAX_N]");
    case te::SCAN_BAD_FLAGS: return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_scan*: unknown flag bits");
    case te::SCAN_NO_OUTPUT: return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_scan*: totals and out are both NULL");
    case te::SCAN_TOO_LARGE: return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_scan*: count x n x 32 does not fit 64 bits");
    case te::SCAN_ALIAS: return set_err(ctx, TE_MSM_EINVAL, "te_msm_field_scan*: out may not be a under TE_MSM_SCAN_SHARED_A");
    default: return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  }
}
// te_msm_field_scan: host buffers, whole vectors sliced over the devices; a slice is scanned in place in its staged copy (SHARED_A: into a
// buffer of its own), and the outputs are written once every slice succeeded
int scan_host(te_ctx* ctx, const scan_req& r, const uint8_t* a, uint64_t count, const uint8_t* init, uint8_t* totals, uint8_t* out) {
  const size_t ob = (size_t)r.n * 32, ab = r.shared ? 32 : ob;
  const slice_plan sp(ctx, count);
  struct slice_t { dev_tmp a, out; };
  std::vector<slice_t> sl(sp.D);
  std::vector<uint8_t> tot(totals ? (size_t)count * 32 : 0);
  auto stage = [&](size_t i) -> int {
    const uint64_t lo = sp.lo(i), m = sp.count(i);
    if (m == 0) return 0;
    if (int rc = tmp_alloc(ctx, ctx->devs[i], sl[i].a, m * ab)) return rc;
    if (r.shared && out) { if (int rc = tmp_alloc(ctx, ctx->devs[i], sl[i].out, m * ob)) return rc; }
    HIP_TRY(ctx, hipMemcpy(sl[i].a.p, a + lo * ab, m * ab, hipMemcpyHostToDevice));
    return scan_on(ctx, i, r, sl[i].a.p, m, init ? init + lo * 32 : nullptr, totals ? tot.data() + lo * 32 : nullptr, !out ? nullptr : r.shared ? sl[i].out.p : sl[i].a.p);
  };
  if (int rc = te_sched::on_devices(*ctx, sp.D, stage)) return rc;
  if (out) { if (int rc = copy_slices_out(ctx, sp, ob, out, [&](size_t i) { return r.shared ? sl[i].out.p : sl[i].a.p; })) return rc; }
  if (totals) memcpy(totals, tot.data(), tot.size());
  return 0;
}
}  // namespace

void free_mul_base(te_ctx* ctx, te_base* b) {
  for (size_t i = 0; i < b->tab.size() && i < ctx->devs.size(); i++)
    if (b->tab[i]) { (void)hipSetDevice(ctx->devs[i].device); (void)hipFree(b->tab[i]); b->tab[i] = nullptr; }
}
void free_matrix(te_ctx* ctx, te_matrix* m) {
  for (std::vector<uint8_t*>* v : {&m->side, &m->side_t})
    for (size_t i = 0; i < v->size() && i < ctx->devs.size(); i++)
      if ((*v)[i]) { (void)hipSetDevice(ctx->devs[i].device); (void)hipFree((*v)[i]); (*v)[i] = nullptr; }
}

// mont: the coordinates are Montgomery residues (option "points_montgomery": te_msm_bind_points*, te_msm_check_points*); every per-call
// check of an MSM or a multiplication reads canonical coordinates
// lay: the records' stride and flag byte (te_msm_bind_points*, te_msm_check_points*): the strided kernels, pieces cut at record boundaries
point_layout layout_now(const te_ctx* ctx) { point_layout l; l.stride = (uint32_t)ctx->opt_point_stride; l.flag = ctx->opt_point_infinity_flag != 0; return l; }
// what a bind or a standalone check refuses before it reads a point: a stride below the pair size of the curve in force, the flag on the
// Twisted-Edwards curve ((0, 1) is an ordinary input there) or without room for its byte, a device buffer that is not 8-byte aligned
int check_layout(te_ctx* ctx, const point_layout& lay, const void* src, bool src_is_host) {
  const bool bls = ctx->opt_curve == TE_MSM_CURVE_BLS12_377_G1;
  if (lay.flag && !bls) return set_err(ctx, TE_MSM_EINVAL, "option \"point_infinity_flag\" is set: BLS12-377 G1 only (the Twisted-Edwards neutral element (0, 1) is an ordinary point)");
  if (lay.flag && lay.stride < 104) return set_err(ctx, TE_MSM_EINVAL, "option \"point_infinity_flag\" needs \"point_stride\" >= 104: the flag is the byte at offset 96");
  if (lay.stride && lay.stride < sizes_of(ctx->opt_curve).point_in) return set_err(ctx, TE_MSM_EINVAL, "option \"point_stride\" is below the size of x || y on this curve");
  if (lay.stride && !src_is_host && (reinterpret_cast<uintptr_t>(src) & 7u)) return set_err(ctx, TE_MSM_EINVAL, "with \"point_stride\" set, a device point buffer must be 8-byte aligned");
  return 0;
}
int check_points_on(te_ctx* ctx, size_t di, const void* src, bool src_is_host, uint64_t n, int curve, int level, int64_t* bad, int* reason, bool mont, point_layout lay) {
  *bad = -1; *reason = 0;
  if (n == 0) return 0;
  gpu_t& d = ctx->devs[di];
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  const size_t pb = lay.bytes(curve);
  const uint64_t piece = src_is_host ? std::min(n, kCheckPiece) : n;
  if (src_is_host) { if (int rc = make_room(ctx, d.chk_pts, piece * pb)) return rc; }
  hipStream_t st = lane.stream();
  for (uint64_t off = 0; off < n; off += piece) {
    const uint32_t m = (uint32_t)std::min(piece, n - off);
    const uint8_t* at = static_cast<const uint8_t*>(src) + off * pb;
    if (src_is_host) { HIP_TRY(ctx, hipMemcpyAsync(d.chk_pts, at, (size_t)m * pb, hipMemcpyHostToDevice, st)); at = d.chk_pts; }
    int64_t i = -1;
    int rc = 0;
    with_curve(curve, [&](auto c) {
      with_flag(mont, [&](auto mt) { rc = check_piece<decltype(c)::value, decltype(mt)::value>(ctx, lane, at, m, level, lay, &i, reason); });
    });
    if (rc == TE_MSM_EPOINT) *bad = (int64_t)off + i;
    if (rc) return rc;
  }
  return 0;
}
// A failed check (kBadPoint) or recovery (kBadX, x-only points) as the outcome of a call: the failure is remembered for get_option
// ("bad_point_index" / "bad_point_reason"), described in the error text and written to the caller's outputs where given.
int note_bad(te_ctx* ctx, bad_kind kind, int64_t index, int reason, int64_t* first_bad, int* reason_out) {
  ctx->bad_point_index = index; ctx->bad_point_reason = reason; ctx->bad_point_operand = 0;      // (te_msm_add* name operand b afterwards: note_pair)
  if (first_bad) *first_bad = index;
  if (reason_out) *reason_out = reason;
  char buf[256];
  if (kind == kBadPoint)
    snprintf(buf, sizeof buf, "input point %lld failed the check of option \"check_points\": %s", (long long)index,
             reason == TE_MSM_POINT_NONCANONICAL ? "non-canonical coordinate" : reason == TE_MSM_POINT_OFF_CURVE ? "not on the curve (or map undefined)" : "not in the prime-order subgroup");
  else
    snprintf(buf, sizeof buf, "x-coordinate %lld has no point (reason %d): %s", (long long)index, reason,
             reason == TE_MSM_POINT_NONCANONICAL ? "non-canonical (x >= modulus, or reserved flag bits set)"
             : reason == TE_MSM_POINT_OFF_CURVE ? "no point on the curve has this x (or the point at infinity / map undefined)"
                                                : "no point of the prime-order subgroup has this x");
  return set_err(ctx, TE_MSM_EPOINT, buf);
}
// option "check_points" in front of a call: 0 = go on, TE_MSM_EPOINT (noted) or a device error
int check_call(te_ctx* ctx, size_t di, const void* src, bool src_is_host, uint64_t n, bool mont, point_layout lay) {
  if (!ctx->opt_check_points) return 0;
  int64_t bad = -1; int reason = 0;
  const int rc = check_points_on(ctx, di, src, src_is_host, n, ctx->opt_curve, ctx->opt_check_points, &bad, &reason, mont, lay);
  if (rc == TE_MSM_EPOINT) return note_bad(ctx, kBadPoint, bad, reason);
  return rc;
}

int tmp_alloc(te_ctx* ctx, gpu_t& d, dev_tmp& t, size_t bytes) {
  HIP_TRY(ctx, hipSetDevice(d.device));
  HIP_TRY(ctx, hipMalloc(&t.p, bytes ? bytes : 16));
  t.dev = d.device;
  return 0;
}

}  // namespace te_eng

extern "C" {

int te_msm_check_points(te_ctx* ctx, const uint8_t* points_xy_le, uint64_t n, int level, int64_t* first_bad, int* reason) {
  return check_standalone(ctx, points_xy_le, true, n, level, first_bad, reason);
}
int te_msm_check_points_device(te_ctx* ctx, const void* d_points_xy_le, uint64_t n, int level, int64_t* first_bad, int* reason) {
  return check_standalone(ctx, d_points_xy_le, false, n, level, first_bad, reason);
}

int te_msm_points_from_x(te_ctx* ctx, const uint8_t* x_le, uint64_t n, uint8_t* out_points_xy_le, int64_t* first_bad, int* reason) {
  device_guard restore_callers_device;
  return points_from_x_common(ctx, x_le, true, n, out_points_xy_le, first_bad, reason);
}

int te_msm_points_from_x_device(te_ctx* ctx, const void* d_x_le, uint64_t n, void* d_out_points_xy_le, int64_t* first_bad, int* reason) {
  device_guard restore_callers_device;
  return points_from_x_common(ctx, d_x_le, false, n, d_out_points_xy_le, first_bad, reason);
}

int te_msm_bind_points_x(te_ctx* ctx, const uint8_t* x_le, uint64_t n, te_bases** out) {
  device_guard restore_callers_device;
  if (!ctx || !out) return TE_MSM_EINVAL;
  *out = nullptr;
  if (int rc = from_x_args(ctx, x_le, n, out)) return rc;
  if (n == 0) return bind_common(ctx, x_le, true, 0, out);
  dev_tmp pts;
  if (int rc = recover_host_to_first(ctx, x_le, n, pts)) return rc;
  return bind_common(ctx, pts.p, false, n, out);                 // as te_msm_bind_points_device (conversion on every device, check_points)
}

int te_msm_run_x(te_ctx* ctx, const uint8_t* x_le, const uint8_t* scalars_le, uint64_t n, uint8_t* out_xy_le) {
  device_guard restore_callers_device;
  if (!ctx || !out_xy_le) return TE_MSM_EINVAL;
  if (ctx->opt_scalars_montgomery) return set_err(ctx, TE_MSM_EINVAL, kNoMontgomeryScalars);
  if (int rc = check_scalar_record(ctx)) return rc;
  if (int rc = from_x_args(ctx, x_le, n, scalars_le)) return rc;
  if (n == 0) return run_common(ctx, x_le, scalars_le, true, 0, out_xy_le);
  dev_tmp pts, sc;
  if (int rc = recover_host_to_first(ctx, x_le, n, pts)) return rc;
  gpu_t& d = ctx->devs[0];
  const size_t sbytes = n * scalar_bytes_now(ctx);
  if (int rc = tmp_alloc(ctx, d, sc, sbytes)) return rc;
  {
    check_lane lane(ctx, d);
    if (lane.rc) return lane.rc;
    HIP_TRY(ctx, hipMemcpyAsync(sc.p, scalars_le, sbytes, hipMemcpyHostToDevice, lane.stream()));
    HIP_TRY(ctx, hipStreamSynchronize(lane.stream()));
  }
  return run_common(ctx, pts.p, sc.p, false, n, out_xy_le, SHARE_CONVERT);   // as te_msm_run_device (window shards, check_points, TE_MSM_ESCALAR)
}

int te_msm_mul(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, int shared_scalar, uint8_t* out_points_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  if (int rc = mul_refused(ctx)) return rc;
  return mul_host(ctx, points_xy_le, false, scalars_le, n, shared_scalar != 0, out_points_xy_le);
}

int te_msm_mul_x(te_ctx* ctx, const uint8_t* x_le, const uint8_t* scalars_le, uint64_t n, int shared_scalar, uint8_t* out_points_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  if (int rc = mul_refused(ctx)) return rc;
  return mul_host(ctx, x_le, true, scalars_le, n, shared_scalar != 0, out_points_xy_le);
}

int te_msm_mul_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n, int shared_scalar, void* d_out_points_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  if (int rc = mul_refused(ctx)) return rc;
  if (int rc = mul_args(ctx, d_points_xy_le, d_scalars_le, n, d_out_points_xy_le)) return rc;
  if (n == 0) return 0;
  const int owner = owner_of(ctx, "te_msm_mul_device: the points, the scalars and the output must be resident on one device of the context",
                             {d_points_xy_le, d_scalars_le, d_out_points_xy_le});
  if (owner < 0) return owner;
  gpu_t& d = ctx->devs[(size_t)owner];
  te::naf_t kn = {};
  if (shared_scalar) {                                            // the NAF is built here: the scalar's first 32 bytes come back
    uint8_t k[32];
    HIP_TRY(ctx, hipSetDevice(d.device));
    HIP_TRY(ctx, hipMemcpy(k, d_scalars_le, 32, hipMemcpyDeviceToHost));
    kn = shared_naf_of(k, ctx->opt_curve);
  }
  if (int rc = check_call(ctx, (size_t)owner, d_points_xy_le, false, n)) return rc;
  return mul_on(ctx, (size_t)owner, d_points_xy_le, d_scalars_le, n, shared_scalar != 0, kn, d_out_points_xy_le, scalar_bytes_now(ctx));
}

int te_msm_bind_base(te_ctx* ctx, const uint8_t* point_xy_le, te_base** out) {
  device_guard restore_callers_device;
  if (!ctx || !out) return TE_MSM_EINVAL;
  *out = nullptr;
  if (!point_xy_le) return set_err(ctx, TE_MSM_EINVAL, "null point");
  const int curve = ctx->opt_curve;
  if (ctx->opt_check_points) {                                      // (canonical coordinates: "points_montgomery" is not read here)
    int64_t bad = -1; int why = 0;
    const int rc = check_points_on(ctx, 0, point_xy_le, true, 1, curve, ctx->opt_check_points, &bad, &why);
    if (rc == TE_MSM_EPOINT) return note_bad(ctx, kBadPoint, 0, why);
    if (rc) return rc;
  }
  const te::mb_geom g = te::mb_geometry(ctx->opt_mul_base_window);
  const size_t pb = sizes_of(curve).point_in, sb = sizes_of(curve).scalar_in;     // (the table's scalars are records of the bind's own: the curve's, whatever "scalar_record_bytes" says)
  std::vector<uint32_t> words((size_t)g.entries * 8);
  te::mb_table_scalars(curve == TE_MSM_CURVE_BLS12_377_G1 ? 1 : 0, g, words.data());
  std::vector<uint8_t> sc((size_t)g.entries * sb, 0), pts((size_t)g.entries * pb);
  for (uint32_t e = 0; e < g.entries; e++) {
    memcpy(&sc[(size_t)e * sb], &words[(size_t)e * 8], 32);
    memcpy(&pts[(size_t)e * pb], point_xy_le, pb);
  }
  te_base* b = new te_base;
  b->ctx = ctx; b->curve = curve; b->W = g.W; b->M = g.M; b->per = g.H + 1u;
  const size_t nd = ctx->devs.size();
  b->tab.assign(nd, nullptr);
  const int rc = te_sched::on_devices(*ctx, nd, [&](size_t i) { return base_table_on(ctx, b, i, pts.data(), sc.data(), g); });
  if (rc) { free_mul_base(ctx, b); delete b; return rc; }
  ctx->mul_bases.push_back(b);
  *out = b;
  return 0;
}

int te_msm_release_base(te_ctx* ctx, te_base* base) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  const auto at = std::find(ctx->mul_bases.begin(), ctx->mul_bases.end(), base);
  if (!base || at == ctx->mul_bases.end()) return set_err(ctx, TE_MSM_EINVAL, kBadBase);
  free_mul_base(ctx, base);                                         // (every call over it has returned: they are synchronous)
  ctx->mul_bases.erase(at);
  delete base;
  return 0;
}

int te_msm_mul_base(te_ctx* ctx, te_base* base, const uint8_t* scalars_le, uint64_t n, uint8_t* out_points_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  bool go = false;
  if (int rc = mul_base_args(ctx, base, scalars_le, n, out_points_xy_le, &go)) return rc;
  return go ? mul_base_host(ctx, base, scalars_le, n, out_points_xy_le) : 0;
}

int te_msm_mul_base_device(te_ctx* ctx, te_base* base, const void* d_scalars_le, uint64_t n, void* d_out_points_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  bool go = false;
  if (int rc = mul_base_args(ctx, base, d_scalars_le, n, d_out_points_xy_le, &go)) return rc;
  if (!go) return 0;
  const int owner = owner_of(ctx, "te_msm_mul_base_device: the scalars and the output must be resident on one device of the context", {d_scalars_le, d_out_points_xy_le});
  if (owner < 0) return owner;
  return mul_base_on(ctx, (size_t)owner, base, d_scalars_le, n, ctx->opt_scalars_montgomery != 0, d_out_points_xy_le, scalar_bytes_now(ctx));
}

int te_msm_add(te_ctx* ctx, const uint8_t* a_xy_le, const uint8_t* b_xy_le, uint64_t n, int flags, uint8_t* out_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  return add_host(ctx, a_xy_le, b_xy_le, false, n, flags, out_xy_le);
}

int te_msm_add_x(te_ctx* ctx, const uint8_t* ax_le, const uint8_t* bx_le, uint64_t n, int flags, uint8_t* out_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  return add_host(ctx, ax_le, bx_le, true, n, flags, out_xy_le);
}

int te_msm_add_device(te_ctx* ctx, const void* d_a, const void* d_b, uint64_t n, int flags, void* d_out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  if (int rc = add_args(ctx, d_a, d_b, n, flags, d_out)) return rc;
  if (n == 0) return 0;
  const int owner = owner_of(ctx, "te_msm_add_device: both operands and the output must be resident on one device of the context", {d_a, d_b, d_out});
  if (owner < 0) return owner;
  pair_verdict v;
  if (int rc = check_pair_on(ctx, (size_t)owner, d_a, d_b, n, (flags & TE_MSM_ADD_SHARED_B) ? 1 : n, v)) return rc;
  if (v.bad >= 0) return note_pair(ctx, v, 0);
  return add_on(ctx, (size_t)owner, d_a, d_b, n, flags, d_out);
}

int te_msm_sum(te_ctx* ctx, const uint8_t* points_xy_le, uint64_t n, uint8_t* out_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  return sum_host(ctx, points_xy_le, false, n, out_xy_le);
}

int te_msm_sum_x(te_ctx* ctx, const uint8_t* x_le, uint64_t n, uint8_t* out_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  return sum_host(ctx, x_le, true, n, out_xy_le);
}

int te_msm_sum_device(te_ctx* ctx, const void* d_points_xy_le, uint64_t n, uint8_t* out_xy_le) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  if (!out_xy_le) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  if (int rc = check_n(ctx, n)) return rc;
  if (n == 0) { write_identity(ctx->opt_curve, out_xy_le); return 0; }
  if (!d_points_xy_le) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  const int owner = owner_of(ctx, "te_msm_sum_device: the points must be resident on a device of the context", {d_points_xy_le});
  if (owner < 0) return owner;
  pair_verdict v;
  if (int rc = check_pair_on(ctx, (size_t)owner, d_points_xy_le, nullptr, n, 0, v)) return rc;
  if (v.bad >= 0) return note_pair(ctx, v, 0);
  uint8_t part[4 * te::ga_sizes<1>::TW];
  if (int rc = sum_fold_on(ctx, (size_t)owner, d_points_xy_le, n, false, part)) return rc;
  sum_finish(ctx->opt_curve, part, out_xy_le);
  return 0;
}

int64_t te_msm_base_read(te_ctx* ctx, const te_base* base, int device_index, uint32_t window, uint32_t first, uint32_t count, void* dst, uint64_t cap,
                         int* entry_bytes) {
  device_guard restore_callers_device;
  if (!ctx || !dst) return TE_MSM_EINVAL;
  if (!base || std::find(ctx->mul_bases.begin(), ctx->mul_bases.end(), base) == ctx->mul_bases.end()) return set_err(ctx, TE_MSM_EINVAL, kBadBase);
  if (device_index < 0 || (size_t)device_index >= ctx->devs.size() || window >= (uint32_t)base->M || first > base->per || count > base->per - first)
    return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
  if (entry_bytes) *entry_bytes = 128;
  uint64_t bytes = (uint64_t)count * 128;
  if (bytes > cap) bytes = cap;
  if (!bytes) return 0;
  HIP_TRY(ctx, hipSetDevice(ctx->devs[(size_t)device_index].device));
  HIP_TRY(ctx, hipMemcpy(dst, base->tab[(size_t)device_index] + ((size_t)window * base->per + first) * 128, bytes, hipMemcpyDeviceToHost));
  return (int64_t)bytes;
}

int te_msm_field_op(te_ctx* ctx, int field, int op, const uint8_t* a, const uint8_t* b, uint64_t n, int flags, uint8_t* out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  field_req q;
  if (int rc = field_args(ctx, field, op, a, b, n, flags, out, q)) return rc;
  return n ? field_host(ctx, q, a, b, n, out) : 0;
}

int te_msm_field_op_device(te_ctx* ctx, int field, int op, const void* d_a, const void* d_b, uint64_t n, int flags, void* d_out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  field_req q;
  if (int rc = field_args(ctx, field, op, d_a, d_b, n, flags, d_out, q)) return rc;
  if (n == 0) return 0;
  const char* const where = "te_msm_field_op_device: the operands and the output must be resident on one device of the context";
  const int owner = d_b ? owner_of(ctx, where, {d_a, d_b, d_out}) : owner_of(ctx, where, {d_a, d_out});
  if (owner < 0) return owner;
  if (op == TE_MSM_FIELD_POW && field == TE_MSM_FIELD_Q377 && d_out == d_b && !(flags & TE_MSM_FIELD_SHARED_B))
    return set_err(ctx, TE_MSM_EINVAL, "TE_MSM_FIELD_POW on TE_MSM_FIELD_Q377: d_out may not be d_b (32-byte exponents, 48-byte results)");
  if (flags & TE_MSM_FIELD_SHARED_B) {                              // the one record comes back: it is a kernel argument
    uint8_t rec[48];
    HIP_TRY(ctx, hipSetDevice(ctx->devs[(size_t)owner].device));
    HIP_TRY(ctx, hipMemcpy(rec, d_b, field_b_bytes_of(q), hipMemcpyDeviceToHost));
    field_take_shared(q, rec);
  }
  int64_t bad = -1; int why = 0;
  const int rc = field_on(ctx, (size_t)owner, q, d_a, d_b, n, d_out, false, &bad, &why);
  return rc == TE_MSM_EFIELD ? note_bad_field(ctx, bad, why) : rc;
}

int te_msm_ntt(te_ctx* ctx, const uint8_t* a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, uint8_t* out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  ntt_req q;
  if (int rc = ntt_args(ctx, a, log_n, count, flags, shift, out, q)) return rc;
  return count ? ntt_host(ctx, q, a, count, out) : 0;
}

int te_msm_ntt_device(te_ctx* ctx, const void* d_a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, void* d_out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  ntt_req q;
  if (int rc = ntt_args(ctx, d_a, log_n, count, flags, shift, d_out, q)) return rc;
  if (count == 0) return 0;
  const int owner = owner_of(ctx, "te_msm_ntt_device: the input and the output must be resident on one device of the context", {d_a, d_out});
  if (owner < 0) return owner;
  return ntt_on(ctx, (size_t)owner, q, d_a, count, d_out);
}

int te_msm_poly_divide(te_ctx* ctx, const uint8_t* a, uint64_t n, uint64_t count, const uint8_t* z, int flags, uint8_t* evals, uint8_t* q) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  poly_req r;
  if (int rc = poly_args(ctx, a, n, count, z, flags, evals, q, r)) return rc;
  return count ? poly_host(ctx, r, a, count, z, evals, q) : 0;
}

int te_msm_poly_divide_device(te_ctx* ctx, const void* d_a, uint64_t n, uint64_t count, const uint8_t* z, int flags, uint8_t* evals, void* d_q) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  poly_req r;
  if (int rc = poly_args(ctx, d_a, n, count, z, flags, evals, d_q, r)) return rc;
  if (count == 0) return 0;
  const char* const where = "te_msm_poly_divide_device: the coefficients and the quotient must be resident on one device of the context";
  const int owner = d_q ? owner_of(ctx, where, {d_a, d_q}) : owner_of(ctx, where, {d_a});
  if (owner < 0) return owner;
  return poly_on(ctx, (size_t)owner, r, d_a, count, z, evals, d_q);
}

int te_msm_bind_matrix(te_ctx* ctx, uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const uint8_t* vals, int flags, te_matrix** out) {
  device_guard restore_callers_device;
  if (!ctx || !out) return TE_MSM_EINVAL;
  *out = nullptr;
  int64_t bad = -1;
  switch (te::spmv_check_bind(rows, cols, row_ptr, col_idx, vals, flags, &bad)) {
    case te::SPMV_OK: break;
    case te::SPMV_BAD_DIMS: return set_err(ctx, TE_MSM_EINVAL, "te_msm_bind_matrix: rows and cols must be in [1, 2^31]");
    case te::SPMV_BAD_FLAGS: return set_err(ctx, TE_MSM_EINVAL, "te_msm_bind_matrix: unknown flag bits");
    case te::SPMV_BAD_PTR: return set_err(ctx, TE_MSM_EINVAL, "te_msm_bind_matrix: row_ptr must start at 0 and never decrease");
    case te::SPMV_TOO_LARGE: return set_err(ctx, TE_MSM_EINVAL, "te_msm_bind_matrix: more than 2^40 entries");
    case te::SPMV_BAD_INDEX: {
      ctx->bad_index_position = bad;
      char buf[160];
      snprintf(buf, sizeof buf, "te_msm_bind_matrix: the column index at position %lld is not below cols", (long long)bad);
      return set_err(ctx, TE_MSM_EINVAL, buf);
    }
    default: return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  }
  const uint64_t nnz = row_ptr[rows];
  const bool mont = (flags & TE_MSM_MATRIX_MONTGOMERY) != 0, with_t = (flags & TE_MSM_MATRIX_TRANSPOSE) != 0;
  te_matrix* m = new te_matrix;
  m->ctx = ctx; m->rows = rows; m->cols = cols; m->nnz = nnz; m->with_t = with_t;
  const size_t nd = ctx->devs.size();
  m->side.assign(nd, nullptr);
  m->side_t.assign(with_t ? nd : 0, nullptr);
  int rc = 0;
  {
    matrix_image img(rows, nnz);
    for (uint64_t e = 0; e < nnz; e++) te::spmv_value(vals + e * 32, mont, img.vals() + e * 32);
    memcpy(img.ptr(), row_ptr, (size_t)(rows + 1) * sizeof(uint64_t));
    if (nnz) memcpy(img.col(), col_idx, (size_t)nnz * sizeof(uint32_t));
    te_spmv::fill_rows(row_ptr, rows, img.row());
    rc = te_sched::on_devices(*ctx, nd, [&](size_t i) { return matrix_upload(ctx, i, img, &m->side[i]); });
    if (!rc && with_t) {
      matrix_image tr(cols, nnz);
      te_spmv::transpose(rows, cols, row_ptr, col_idx, img.vals(), tr.ptr(), tr.col(), tr.vals());
      te_spmv::fill_rows(tr.ptr(), cols, tr.row());
      rc = te_sched::on_devices(*ctx, nd, [&](size_t i) { return matrix_upload(ctx, i, tr, &m->side_t[i]); });
    }
  }
  if (rc) { free_matrix(ctx, m); delete m; return rc; }
  ctx->matrices.push_back(m);
  *out = m;
  return 0;
}

int te_msm_release_matrix(te_ctx* ctx, te_matrix* matrix) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  const auto at = std::find(ctx->matrices.begin(), ctx->matrices.end(), matrix);
  if (!matrix || at == ctx->matrices.end()) return set_err(ctx, TE_MSM_EINVAL, kBadMatrix);
  free_matrix(ctx, matrix);                                         // (every call over it has returned: they are synchronous)
  ctx->matrices.erase(at);
  delete matrix;
  return 0;
}

int te_msm_matrix_shape(const te_matrix* matrix, uint64_t* rows, uint64_t* cols, uint64_t* nnz) {
  if (!matrix) return TE_MSM_EINVAL;
  if (rows) *rows = matrix->rows;
  if (cols) *cols = matrix->cols;
  if (nnz) *nnz = matrix->nnz;
  return 0;
}

int te_msm_spmv(te_ctx* ctx, te_matrix* matrix, const uint8_t* x, uint64_t count, int flags, uint8_t* out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  bool go = false;
  if (int rc = spmv_args(ctx, matrix, x, count, flags, out, &go)) return rc;
  return go ? spmv_host(ctx, matrix, (flags & TE_MSM_SPMV_TRANSPOSE) != 0, te_spmv::chunk_in_force(), x, count, out) : 0;
}

int te_msm_spmv_device(te_ctx* ctx, te_matrix* matrix, const void* d_x, uint64_t count, int flags, void* d_out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  bool go = false;
  if (int rc = spmv_args(ctx, matrix, d_x, count, flags, d_out, &go)) return rc;
  if (!go) return 0;
  const int owner = owner_of(ctx, "te_msm_spmv_device: the vectors and the output must be resident on one device of the context", {d_x, d_out});
  if (owner < 0) return owner;
  return spmv_on(ctx, (size_t)owner, matrix, (flags & TE_MSM_SPMV_TRANSPOSE) != 0, te_spmv::chunk_in_force(), d_x, count, d_out);
}

int te_msm_field_scan(te_ctx* ctx, int op, const uint8_t* a, uint64_t n, uint64_t count, int flags, const uint8_t* init, uint8_t* totals, uint8_t* out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  scan_req r;
  if (int rc = scan_args(ctx, op, a, n, count, flags, totals, out, r)) return rc;
  return count ? scan_host(ctx, r, a, count, init, totals, out) : 0;
}

int te_msm_field_scan_device(te_ctx* ctx, int op, const void* d_a, uint64_t n, uint64_t count, int flags, const uint8_t* init, uint8_t* totals, void* d_out) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  scan_req r;
  if (int rc = scan_args(ctx, op, d_a, n, count, flags, totals, d_out, r)) return rc;
  if (count == 0) return 0;
  const char* const where = "te_msm_field_scan_device: the vectors and the output must be resident on one device of the context";
  const int owner = d_out ? owner_of(ctx, where, {d_a, d_out}) : owner_of(ctx, where, {d_a});
  if (owner < 0) return owner;
  return scan_on(ctx, (size_t)owner, r, d_a, count, init, totals, d_out);
}

}  // extern "C"
