// run.hip -- a context's life (te_msm_init / te_msm_destroy), the lone calls te_msm_run / te_msm_run_device over one or several
// devices, and how the status and the rows of a finished MSM are settled.
#include "engine.hpp"
#include "host_tail.hpp"
#include "host_tail377.hpp"

using namespace te_eng;

static_assert(TE377_TAIL_ROW_BYTES == TE_MSM_PARTIAL_BYTES_BLS12_377, "row layout");

namespace te_eng {

namespace {
void note_entries(te_ctx* ctx, const workset_t& ws) { ctx->stat_entries = entries_of(ws); }

// Indexed MSMs (te_msm_run_scalars_indexed*): an index outside the bound set, seen by the device (te::index_args) -- the flag words of the
// work set are on the host.  -1: none; else the lowest bad position the set's launch sequences saw.
int64_t bad_index_of(const workset_t& ws) { return (ws.h_err[0] & 2u) ? (int64_t)(uint32_t)~ws.h_err[1] : -1; }
int note_bad_index(te_ctx* ctx, int64_t position) {
  ctx->bad_index_position = position;
  char buf[160];
  snprintf(buf, sizeof buf, "index at position %lld is not below te_msm_bases_count of the bound point set", (long long)position);
  return set_err(ctx, TE_MSM_EINVAL, buf);
}

// te_msm_run for a large MSM on one device: enqueue_host_pieces on a free work set, wait, host tail
int run_host_chunked(te_ctx* ctx, const uint8_t* src_points, const uint8_t* src_scalars, uint64_t n, int K, uint8_t out[64]) {
  gpu_t& d = ctx->devs[0];
  workset_t& ws = d.ws[0];
  const plan_t pf = make_plan(ctx, d, plan_whole(n));
  host_slice_req r; r.points = src_points; r.scalars = src_scalars; r.n = n; r.c = pf.c; r.K = K;
  if (int rc = enqueue_host_pieces(ctx, d, ws, r)) return rc;
  HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));
  if (int rc = settle_status(ctx, ws)) return rc;
  fold_rows(pf, ws.h_partials, out);
  return 0;
}

// te_msm_run_device on a context of D > 1 devices: WINDOW shards (device i computes windows i, i + D, ...), inputs resident
// on the first device.  Every device needs all n points and scalars; they travel as a scatter + all-gather over the
// point-to-point xGMI links instead of D - 1 full copies out of the first device's memory (SURVEY.md 8e "Inputs"):
//   phase 1  device i >= 1 pulls slice i (n / D points and their scalars) from the source           -- issued here, in turn: cheap,
//            and the "slice i has arrived" events must exist before any other device waits for them
//   phase 2  device i pulls slice 0 from the source and slice j from device j's staging area (j != i, j >= 1), behind the
//            event of phase 1 -- D - 1 different links into every device, 2 (D - 1) / D of the input out of the first
//            device instead of D - 1 times all of it
// Phase 2, the ~30 launches of the device's share and its read-back are enqueued by the device's own host thread: D enqueue
// sequences side by side instead of one after the other on the calling thread (0.35 ms of host time each).
// (One physical GPU named several times -- the only form a one-GPU box can run -- makes every copy a device-to-device copy.)
int run_device_window_shards(te_ctx* ctx, const void* src_points, const void* src_scalars, uint64_t n, uint8_t* out) {
  const size_t nd = ctx->devs.size();
  const plan_t p0 = make_plan(ctx, ctx->devs[0], plan_shard(n));
  const curve_sizes sz = sizes_of(p0.curve);
  const size_t sb = (size_t)p0.sc_bytes;
  std::vector<int> wsel;
  if (int rc = free_sets(ctx, nd, wsel)) return rc;
  const int src_dev = ctx->devs[0].device;
  const uint64_t per = (n + nd - 1) / nd;
  auto lo_of = [&](size_t j) { return std::min<uint64_t>(n, per * j); };
  const uint8_t* sp = static_cast<const uint8_t*>(src_points); const uint8_t* ss = static_cast<const uint8_t*>(src_scalars);
  // phase 1 (calling thread)
  for (size_t i = 1; i < nd; i++) {
    gpu_t& d = ctx->devs[i]; workset_t& ws = d.ws[wsel[i]];
    HIP_TRY(ctx, hipSetDevice(d.device));
    if (int rc = ensure_staging(ctx, ws, n * sz.point_in, n * sb)) return rc;
    if (int rc = wait_behind_previous(ctx, ws)) return rc;
    const uint64_t lo = lo_of(i), m = lo_of(i + 1) - lo;
    if (m) {
      HIP_TRY(ctx, hipMemcpyPeerAsync(static_cast<uint8_t*>(ws.d_in_points) + lo * sz.point_in, d.device, sp + lo * sz.point_in, src_dev, m * sz.point_in, ws.stream));
      HIP_TRY(ctx, hipMemcpyPeerAsync(static_cast<uint8_t*>(ws.d_in_scalars) + lo * sb, d.device, ss + lo * sb, src_dev, m * sb, ws.stream));
      ctx->stat_peer_copies += 2; ctx->stat_peer_bytes += (int64_t)(m * (sz.point_in + sb));
    }
    HIP_TRY(ctx, hipEventRecord(ws.ev_copy, ws.stream));
  }
  // phase 2 + the device's share, one host thread per device
  std::vector<int64_t> copies(nd, 0), bytes(nd, 0);
  auto share = [&](size_t i) -> int {
    gpu_t& d = ctx->devs[i]; workset_t& ws = d.ws[wsel[i]];
    HIP_TRY(ctx, hipSetDevice(d.device));
    const void *dp = src_points, *ds = src_scalars;
    if (i > 0) {
      for (size_t j = 0; j < nd; j++) {
        if (j == i) continue;
        const uint64_t lo = lo_of(j), m = lo_of(j + 1) - lo;
        if (!m) continue;
        const gpu_t& o = ctx->devs[j]; const workset_t& ows = o.ws[wsel[j]];
        const uint8_t* fp = j == 0 ? sp : static_cast<const uint8_t*>(ows.d_in_points);
        const uint8_t* fs = j == 0 ? ss : static_cast<const uint8_t*>(ows.d_in_scalars);
        if (j > 0) HIP_TRY(ctx, hipStreamWaitEvent(ws.stream, ows.ev_copy, 0));
        HIP_TRY(ctx, hipMemcpyPeerAsync(static_cast<uint8_t*>(ws.d_in_points) + lo * sz.point_in, d.device, fp + lo * sz.point_in, o.device, m * sz.point_in, ws.stream));
        HIP_TRY(ctx, hipMemcpyPeerAsync(static_cast<uint8_t*>(ws.d_in_scalars) + lo * sb, d.device, fs + lo * sb, o.device, m * sb, ws.stream));
        copies[i] += 2; bytes[i] += (int64_t)(m * (sz.point_in + sb));
      }
      dp = ws.d_in_points; ds = ws.d_in_scalars;
    }
    partial_req r; r.d_points = dp; r.d_scalars = ds; r.n = n; r.stream = ws.stream; r.scalar_bytes = p0.sc_bytes; r.scalar_bits = p0.sc_bits;
    if (int rc = enqueue_partial(ctx, d, ws, r)) return rc;
    return fetch_rows(ctx, ws, ws.stream);
  };
  const int rc = te_sched::on_devices(*ctx, nd, share);
  // a device whose staging area other devices read must not reuse it before they are done: every set's next MSM waits for
  // its own ev_done only, so the call ends with all of them complete (settle_window_shards) -- the copies are over by then
  for (size_t i = 0; i < nd; i++) { ctx->stat_peer_copies += copies[i]; ctx->stat_peer_bytes += bytes[i]; }
  return settle_window_shards(ctx, wsel, p0, rc, true, out);
}

thread_local std::string g_init_error;

void free_dev(gpu_t& d) {
  (void)hipSetDevice(d.device);
  for (auto& sl : d.slabs) {
    if (sl.d) { (void)hipFree(sl.d); sl.d = nullptr; }
    for (hipEvent_t& e : sl.ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (sl.conv_ev) { (void)hipEventDestroy(sl.conv_ev); sl.conv_ev = nullptr; }
  }
  d.slabs.clear();
  if (d.chk_stream) (void)hipStreamDestroy(d.chk_stream);
  d.chk_pts.release();
  d.ntt_tab.release();
  d.ntt_tmp.release();
  d.poly_tmp.release();
  d.scan_tmp.release();
  d.spmv_tmp.release();
  if (d.chk_word) (void)hipFree(d.chk_word);
  if (d.chk_host) (void)hipHostFree(d.chk_host);
  d.chk_stream = nullptr; d.chk_word = d.chk_host = nullptr;
  if (d.h_batch_rows) (void)hipHostFree(d.h_batch_rows);
  d.h_batch_rows = nullptr; d.h_batch_cap = 0;
  for (workset_t& ws : d.ws) {
    free_workset_buffers(ws);
    if (ws.h_err) (void)hipHostFree(ws.h_err);
    for (hipEvent_t e : ws.ring_ev) if (e) (void)hipEventDestroy(e);
    if (ws.ev_done) (void)hipEventDestroy(ws.ev_done);
    if (ws.ev_result) (void)hipEventDestroy(ws.ev_result);
    for (auto& ev : ws.ev) if (ev) (void)hipEventDestroy(ev);
    if (ws.ev_copy) (void)hipEventDestroy(ws.ev_copy);
    if (ws.ev_start) (void)hipEventDestroy(ws.ev_start);
    for (hipEvent_t e : ws.piece_events) (void)hipEventDestroy(e);
    if (ws.copy_stream) (void)hipStreamDestroy(ws.copy_stream);
    // a stream whose handle left the library stays alive (see "EXPORTED STREAMS ARE NEVER DESTROYED"); te_msm_destroy has synchronised it
    if (ws.stream) { if (d.streams_exported) park_stream(d.device, ws.stream); else (void)hipStreamDestroy(ws.stream); }
    ws.stream = nullptr; ws.copy_stream = nullptr;
  }
}
}  // namespace

// the host tail of the rows a plan produced (ordinary windows: Horner; fixed-base windows: one bucket set, no window doublings)
void fold_rows(const plan_t& p, const uint8_t* rows, uint8_t* out) {
  if (p.fb_rb) te_host::fixed_base_to_affine(rows, p.fb_rb + 1, p.fb_rb, (int)p.logB, out);
  else if (p.curve == TE_MSM_CURVE_BLS12_377_G1) te377_host::horner_to_affine(rows, p.c, (int)p.logB, p.W, out);
  else te_host::horner_to_affine(rows, p.c, (int)p.logB, p.W, out);
}
// the result of an empty MSM: the identity, (0, 1) on the Twisted-Edwards curve, infinity (all zero) on BLS12-377
void write_identity(int curve, uint8_t* out) {
  memset(out, 0, sizes_of(curve).result);
  if (curve == TE_MSM_CURVE_TE_BLS12) out[32] = 1;
}

// every job posted to the context's host threads has run (asynchronous submits touch work sets, options and the error
// string: calls that change or read those beside them wait first)
void drain_workers(te_ctx* ctx) { te_sched::drain_workers(*ctx); }

// the lowest-numbered work set of a device that no ticket owns (-1: none)
int free_workset_index(const gpu_t& d) { return te_sched::free_set_index(d, TE_MSM_WORKSETS); }

// a work set no ticket owns on each of the first D devices, for a lone call over several devices (tickets and lone calls may be mixed)
int free_sets(te_ctx* ctx, size_t D, std::vector<int>& wsel) {
  wsel.assign(D, 0);
  for (size_t i = 0; i < D; i++) { wsel[i] = free_workset_index(ctx->devs[i]); if (wsel[i] < 0) return set_err(ctx, TE_MSM_ESTATE, kAllSetsOwned); }
  return 0;
}
// the work set a lone call on one device runs on: the selected one, unless a submitted MSM still owns it -- then any free one; with
// every set owned by a ticket the call is refused
int lone_set(te_ctx* ctx, const gpu_t& d, int selected) {
  if (!te_sched::slot_ticket(d.ws[selected].slot)) return selected;
  const int wi = free_workset_index(d);
  return wi < 0 ? set_err(ctx, TE_MSM_ESTATE, kAllSetsOwned) : wi;
}

// the non-zero window digits the device counted for the MSM whose flag words are in the set's pinned block (word 1)
int64_t entries_of(const workset_t& ws) { uint64_t v; memcpy(&v, ws.h_err + Z_ENTRIES, sizeof v); return (int64_t)v; }

// The status of the MSM whose flag words are in the set's pinned block (ev_result has passed): its entries noted, an index outside
// the bound set reported (bit 1 of word 0: only the indexed first-level scatter sets it -- the fixed-base overflow is word 1 alone),
// else the final carry.  entries_of_failed = false (te_msm_finalize): a failed MSM leaves "entries_accumulated" as it was.
int settle_status(te_ctx* ctx, const workset_t& ws, bool entries_of_failed) {
  if (entries_of_failed || !*ws.h_err) note_entries(ctx, ws);
  if (const int64_t bad = bad_index_of(ws); bad >= 0) return note_bad_index(ctx, bad);
  if (*ws.h_err) return set_err(ctx, TE_MSM_ESCALAR, kFinalCarry);
  return 0;
}

// te_msm_run on a context of D > 1 devices: POINT sharding.  Points and scalars are cut into contiguous slices, one per
// device; one host thread per device stages its slice over that device's own PCIe link (pageable copies block the thread
// that issues them) and runs ALL windows on its n/D points (enqueue_host_pieces, itself in pieces for large slices); the D x W
// rows are linear in the bucket contents, so the host tail folds their sum (horner_to_affine_multi).  Every device pays the
// reduction of all W x B buckets -- which is why device-resident inputs (te_msm_run_device, one process per GPU) shard
// the WINDOWS instead -- but on this boundary the cost is the link: 1.85 of 2.47 ms at n = 2^20 on one device.  The window size
// follows the slice (all slices share it).  Reference: compute_msm uploads inside the call (cuzk/gpu.ts:33-46,
// submission.ts:73-78); multi-device is its README's future work (README.md:551).
// This is the form for the LONE call.  A caller with several MSMs to do keeps whole MSMs in flight instead, one per device
// (te_msm_submit / te_msm_submit_async below): no replicated bucket reduction, no row merge.
// bases: the MSM runs over a bound point set -- every device holds all records, so device i takes slice i of the SCALARS over its
// link and gathers from its own copy of the records at the slice's offset (src_points is not read).
// src_idx (with bases): an indexed subset of n (index, scalar) pairs -- device i takes slice i of BOTH arrays (indexed_plan.hpp: slices
// of near-equal size) and gathers from all of its records.
int run_host_sharded(te_ctx* ctx, const uint8_t* src_points, const uint8_t* src_scalars, uint64_t n, uint8_t* out, const te_bases* bases,
                     const uint32_t* src_idx) {
  const size_t nd = ctx->devs.size();
  uint64_t per_min = ctx->opt_host_shard_min > 0 ? (uint64_t)ctx->opt_host_shard_min : 1;
  size_t D = src_idx ? te_indexed::devices_for(n, nd, per_min) : (size_t)std::min<uint64_t>(nd, std::max<uint64_t>(1, n / per_min));
  const uint64_t per = (n + D - 1) / D;
  auto slice_lo = [&](size_t i) -> uint64_t { return src_idx ? te_indexed::slice_lo(n, D, i) : std::min<uint64_t>(n, per * i); };
  const plan_t p0 = make_plan(ctx, ctx->devs[0], plan_whole(per));     // geometry of every slice's rows (window bits from the slice size)
  const curve_sizes sz = sizes_of(p0.curve);
  const int K = bases ? scalar_pieces(ctx, per) : host_pieces(ctx, per);
  std::vector<int> wsel;
  if (int rc = free_sets(ctx, D, wsel)) return rc;
  auto slice = [&](size_t i) -> int {
    const uint64_t lo = slice_lo(i), hi = src_idx ? slice_lo(i + 1) : std::min<uint64_t>(n, lo + per);
    gpu_t& d = ctx->devs[i];
    if (hi == lo) return 0;
    workset_t& ws = d.ws[wsel[i]];
    host_slice_req r; r.scalars = src_scalars + lo * (size_t)p0.sc_bytes; r.n = hi - lo; r.c = p0.c; r.K = K; r.scalar_bytes = p0.sc_bytes; r.scalar_bits = p0.sc_bits;
    if (!bases) r.points = src_points + lo * sz.point_in;
    else if (!src_idx) { r.recs = bases->recs[i] + lo * bases->rec_bytes; r.rec_kind = bases->rec_kind; }
    else { r.recs = bases->recs[i]; r.rec_kind = bases->rec_kind; r.idx = src_idx + lo; r.idx_count = bases->n; r.idx_pos = lo; }
    if (int rc = enqueue_host_pieces(ctx, d, ws, r)) return rc;
    HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));
    return 0;
  };
  if (int rc = te_sched::on_devices(*ctx, D, slice)) return rc;
  std::vector<const uint8_t*> sets;
  int64_t entries = 0;
  if (src_idx) {                                            // an index outside the set, on any device: the lowest position of the call
    int64_t bad = -1;
    for (size_t i = 0; i < D; i++) { const int64_t b = bad_index_of(ctx->devs[i].ws[wsel[i]]); if (b >= 0 && (bad < 0 || b < bad)) bad = b; }
    if (bad >= 0) return note_bad_index(ctx, bad);
  }
  for (size_t i = 0; i < D; i++) {
    if (slice_lo(i) >= n) break;
    workset_t& ws = ctx->devs[i].ws[wsel[i]];
    if (*ws.h_err) return set_err(ctx, TE_MSM_ESCALAR, kFinalCarry);
    entries += entries_of(ws);
    sets.push_back(ws.h_partials);
  }
  ctx->stat_entries = entries;
  const int ns = (int)sets.size();
  if (ns <= 2) {                                            // one or two sets: summed on the fly inside the fold
    if (p0.curve == TE_MSM_CURVE_BLS12_377_G1) te377_host::horner_to_affine_multi(sets.data(), ns, p0.c, (int)p0.logB, p0.W, out);
    else te_host::horner_to_affine_multi(sets.data(), ns, p0.c, (int)p0.logB, p0.W, out);
    return 0;
  }
  // more: the sets' rows are summed window by window by the devices' host threads (5 x (sets - 1) additions per window,
  // ~0.2 us each: summed on the fly by the one thread that folds, eight sets cost ~100 us of a 0.7 ms call), then one fold
  // over the merged points.  Thread t merges windows t, t + D, ...: distinct elements of merged[] and present[].
  const bool bls = p0.curve == TE_MSM_CURVE_BLS12_377_G1;
  std::vector<te_host::Pt> m9(bls ? 0 : (size_t)p0.W * 5);
  std::vector<te377_host::Pt> m14(bls ? (size_t)p0.W * 5 : 0);
  std::vector<uint8_t> present((size_t)p0.W, 0);
  auto merge = [&](size_t t) -> int {
    for (int w = (int)t; w < p0.W; w += (int)D) {
      if (bls) te377_host::merge_window_rows(sets.data(), ns, w, m14.data(), present.data());
      else te_host::merge_window_rows(sets.data(), ns, w, m9.data(), present.data());
    }
    return 0;
  };
  (void)te_sched::on_devices(*ctx, D, merge);
  if (bls) te377_host::horner_to_affine_points(m14.data(), present.data(), p0.c, (int)p0.logB, p0.W, out);
  else te_host::horner_to_affine_points(m9.data(), present.data(), p0.c, (int)p0.logB, p0.W, out);
  return 0;
}

// The end of a lone call over window shards (wsel: each device's work set; rc: the status of their enqueues): every device's MSM
// complete, each device's windows merged into one set of rows, the entries summed and the final carry checked, then one fold.
// stage_ms: the first device's stage times are collected (option "profile").
int settle_window_shards(te_ctx* ctx, const std::vector<int>& wsel, const plan_t& p0, int rc, bool stage_ms, uint8_t* out) {
  const size_t row = sizes_of(p0.curve).row;
  std::vector<uint8_t> merged((size_t)p0.W * row, 0);
  int64_t entries = 0; bool carry = false;
  for (size_t i = 0; i < wsel.size(); i++) {
    gpu_t& d = ctx->devs[i];
    workset_t& ws = d.ws[wsel[i]];
    if (rc) { (void)hipSetDevice(d.device); (void)hipStreamSynchronize(ws.stream); continue; }      // leave nothing of a failed call in flight
    HIP_TRY(ctx, hipSetDevice(d.device));
    HIP_TRY(ctx, hipEventSynchronize(ws.ev_done));
    carry = carry || *ws.h_err != 0;
    entries += entries_of(ws);
    for (int w = d.w_first; w < p0.W; w += d.w_step) memcpy(&merged[(size_t)w * row], ws.h_partials + (size_t)w * row, row);
  }
  if (rc) return rc;
  ctx->stat_entries = entries;
  if (carry) return set_err(ctx, TE_MSM_ESCALAR, kFinalCarry);
  if (stage_ms) (void)collect_stage_ms(ctx, ctx->devs[0], ctx->devs[0].ws[wsel[0]]);
  fold_rows(p0, merged.data(), out);
  return 0;
}

int check_n(te_ctx* ctx, uint64_t n) { return n >= (1ull << 31) ? set_err(ctx, TE_MSM_EINVAL, "n must be < 2^31") : 0; }

// share: how a single-device call from device-resident points keeps its records (share_mode; x-only points: SHARE_CONVERT)
int run_common(te_ctx* ctx, const void* src_points, const void* src_scalars, bool src_is_host, uint64_t n, uint8_t out[64], share_mode share) {
  if (!ctx || !out) return TE_MSM_EINVAL;
  if (int rc = check_n(ctx, n)) return rc;
  if (int rc = check_scalar_record(ctx, src_is_host ? nullptr : src_scalars)) return rc;
  if (n == 0) { write_identity(ctx->opt_curve, out); return 0; }
  if (!src_points || !src_scalars) return set_err(ctx, TE_MSM_EINVAL, "null input buffer");
  // (device-resident inputs live on the first device: a multi-device call checks them there, before the scatter)
  if (int rc = check_call(ctx, 0, src_points, src_is_host, n)) return rc;
  const size_t nd = ctx->devs.size();
  // several devices: host buffers -> slices of the points, one upload thread per device; device-resident inputs -> window shards
  if (nd > 1) {
    if (src_is_host) return run_host_sharded(ctx, static_cast<const uint8_t*>(src_points), static_cast<const uint8_t*>(src_scalars), n, out);
    // (fewer windows than devices -- a narrow plan: a shard would be left without a window, so the call runs whole on the first
    // device, which holds the inputs, as a lone call over a fixed-base set does)
    if ((size_t)make_plan(ctx, ctx->devs[0], plan_shard(n)).W >= nd) return run_device_window_shards(ctx, src_points, src_scalars, n, out);
  }
  const bool whole = nd > 1;
  gpu_t& d = ctx->devs[0];
  if (src_is_host && !ctx->opt_profile && ctx->opt_workset == 0 && d.w_step == 1 && d.in_flight == 0) {
    // no tickets in flight, no stage timing requested: every work set is free for the pieces
    const int K = host_pieces(ctx, n);
    if (K > 1) return run_host_chunked(ctx, static_cast<const uint8_t*>(src_points), static_cast<const uint8_t*>(src_scalars), n, K, out);
  }
  const int wsel = lone_set(ctx, d, whole ? 0 : ctx->opt_workset);
  if (wsel < 0) return wsel;
  const plan_t p0 = make_plan(ctx, d, whole ? plan_whole(n) : plan_shard(n));
  const curve_sizes sz = sizes_of(p0.curve);
  const size_t sb = (size_t)p0.sc_bytes;
  workset_t& ws = d.ws[wsel];
  HIP_TRY(ctx, hipSetDevice(d.device));
  const void *dp = src_points, *ds = src_scalars;
  if (src_is_host) {
    if (int rc = ensure_staging(ctx, ws, n * sz.point_in, n * sb)) return rc;
    // scalars first; the points follow from inside enqueue_partial (pageable copies return when the data has left
    // the caller's buffer, so the scalar-only stages enqueued in between run while the points are still in flight)
    if (int rc = upload(ctx, ws, ws.d_in_scalars, static_cast<const uint8_t*>(src_scalars), n * sb, ws.stream)) return rc;
    dp = ws.d_in_points; ds = ws.d_in_scalars;
  }
  const std::function<int(hipStream_t)> upload_points = [&](hipStream_t side) -> int {
    // on the side stream, beside the scalar-only kernels on ws.stream; the conversion to records follows it there
    return upload(ctx, ws, ws.d_in_points, static_cast<const uint8_t*>(src_points), n * sz.point_in, side);
  };
  partial_req r; r.d_points = dp; r.d_scalars = ds; r.n = n; r.stream = ws.stream; r.whole = whole;
  if (src_is_host) r.upload_points = &upload_points; else r.share = share;
  if (int rc = enqueue_partial(ctx, d, ws, r)) return rc;
  if (int rc = fetch_rows(ctx, ws, ws.stream)) return rc;
  HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));          // (pinned sources included: the call ends after its uploads)
  release_shared_recs(d, ws);                               // the call is over: its record slab (if shared) may serve another point buffer
  if (int rc = settle_status(ctx, ws)) return rc;
  (void)collect_stage_ms(ctx, d, ws);                       // (of a call that succeeded: a failed lone call leaves the previous stage times)
  // a window-sharded single-device context (te_msm_set_window_shard) folds its own rows only: the others read as zero
  fold_rows(p0, ws.h_partials, out);
  return 0;
}

}  // namespace te_eng

extern "C" {

int te_msm_init(const int* device_ids, int n_dev, te_ctx** out) {
  device_guard restore_callers_device;
  if (!out || n_dev < 1 || n_dev > 64) { g_init_error = "te_msm_init: bad arguments"; return TE_MSM_EINVAL; }
  *out = nullptr;
  if (!te_host::tail_selftest() || !te377_host::tail_selftest()) { g_init_error = "te_msm_init: host tail constants self-test failed"; return TE_MSM_ESTATE; }
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count < 1) {
    g_init_error = std::string("te_msm_init: no usable HIP device (") + hipGetErrorString(e) + "); this library has no CPU fallback";
    return TE_MSM_EDEVICE;
  }
  te_ctx* ctx = new te_ctx();
  if (const char* e = getenv("TE_MSM_QUEUE_PROBE")) ctx->opt_queue_probe = e[0] != '0';  // option "queue_probe"
  if (const char* e = getenv("TE_MSM_PACKED")) ctx->opt_packed = e[0] != '0';            // option "packed_sort"
  if (const char* e = getenv("TE_MSM_HOST_STAGING")) ctx->opt_host_staging = e[0] != '0'; // option "host_staging"
  if (const char* e = getenv("TE_MSM_UPLOAD_THREADS")) { const int v = atoi(e); if (v >= 1 && v <= 16) ctx->opt_upload_threads = v; }   // option "upload_threads"
  if (const char* e = getenv("TE_MSM_FOLD_PAIRS")) ctx->opt_fold_pairs = e[0] != '0';    // option "fold_pairs"
  if (const char* e = getenv("TE_MSM_SHARE_RECORDS")) ctx->opt_share_records = e[0] == '0' ? 0 : e[0] == '2' ? 2 : 1;   // option "share_records"
  ctx->devs.resize(n_dev);
  for (int i = 0; i < n_dev; i++) {
    gpu_t& d = ctx->devs[i];
    d.device = device_ids ? device_ids[i] : i;
    d.w_first = i; d.w_step = n_dev;
    if (d.device < 0 || d.device >= count) { g_init_error = "te_msm_init: device id out of range"; delete ctx; return TE_MSM_EINVAL; }
    hipError_t er = hipSetDevice(d.device);
    if (er == hipSuccess) { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, d.device) == hipSuccess) d.wall_clock_khz = khz; }
    if (er == hipSuccess) er = allow_tail_lds();       // (te_msm.hip: the dynamic LDS of k_reduce_tail)
    if (er == hipSuccess && create_workset_streams(d) != 0) er = hipErrorOutOfMemory;
    for (workset_t& ws : d.ws) {       // the small fixed allocations of every work set; the big buffers come with the first MSM
      if (er == hipSuccess) er = hipEventCreateWithFlags(&ws.ev_copy, hipEventDisableTiming);
      if (er == hipSuccess) er = hipEventCreateWithFlags(&ws.ev_start, hipEventDisableTiming);
      if (er == hipSuccess) er = hipHostMalloc((void**)&ws.h_err, Z_ROWS * 4 + (size_t)TE_MAX_WINDOWS * TE_MAX_ROW_BYTES, hipHostMallocDefault);
      if (er == hipSuccess) ws.h_partials = reinterpret_cast<uint8_t*>(ws.h_err + Z_ROWS);
      if (er == hipSuccess) er = hipHostGetDevicePointer((void**)&ws.h_err_dev, ws.h_err, 0);
      if (er == hipSuccess) er = hipEventCreateWithFlags(&ws.ev_done, hipEventDisableTiming);
      if (er == hipSuccess) er = hipEventCreateWithFlags(&ws.ev_result, hipEventDisableTiming);
      for (auto& evn : ws.ev) if (er == hipSuccess) er = hipEventCreate(&evn);
      if (er == hipSuccess) *ws.h_err = 0;
    }
    if (er != hipSuccess) {
      g_init_error = std::string("te_msm_init: ") + hipGetErrorString(er);
      for (auto& dd : ctx->devs) free_dev(dd);
      delete ctx; return TE_MSM_EDEVICE;
    }
  }
  *out = ctx;
  return 0;
}

void te_msm_destroy(te_ctx* ctx) {
  device_guard restore_callers_device;
  if (!ctx) return;
  ctx->lanes.clear();                   // finishes the uploads of tickets that were never collected, joins the threads
  ctx->workers.clear();                 // joins the per-device host threads (idle between calls)
  ctx->stagers.clear();
  for (auto& d : ctx->devs) {
    (void)hipSetDevice(d.device);
    for (workset_t& ws : d.ws) {        // this context's streams only: other work of the process is none of its business
      if (ws.stream) (void)hipStreamSynchronize(ws.stream);
      if (ws.copy_stream) (void)hipStreamSynchronize(ws.copy_stream);
      if (ws.last_stream && ws.last_stream != ws.stream && ws.ev_done) (void)hipEventSynchronize(ws.ev_done);
    }
    free_dev(d);
  }
  for (te_bases* b : ctx->bases) {      // bound point sets the caller did not release
    for (size_t i = 0; i < b->recs.size() && i < ctx->devs.size(); i++)
      if (b->recs[i]) { (void)hipSetDevice(ctx->devs[i].device); (void)hipFree(b->recs[i]); }
    delete b;
  }
  for (te_base* b : ctx->mul_bases) { free_mul_base(ctx, b); delete b; }   // ... and the bound points of te_msm_bind_base
  for (te_matrix* m : ctx->matrices) { free_matrix(ctx, m); delete m; }    // ... and the matrices of te_msm_bind_matrix
  delete ctx;
}

// (a device's host thread may be writing ctx->err this very moment -- an asynchronous submit that fails: a copy taken under
// the lock, per calling thread; valid until that thread asks again)
const char* te_msm_last_error(const te_ctx* ctx) {
  if (!ctx) return g_init_error.c_str();
  thread_local std::string copy;
  { std::lock_guard<std::mutex> lk(const_cast<te_ctx*>(ctx)->err_mu); copy = ctx->err; }
  return copy.c_str();
}

int te_msm_run(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, uint8_t out_xy_le[64]) {
  device_guard restore_callers_device;
  return run_common(ctx, points_xy_le, scalars_le, true, n, out_xy_le);
}

int te_msm_run_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n, uint8_t out_xy_le[64]) {
  device_guard restore_callers_device;
  return run_common(ctx, d_points_xy_le, d_scalars_le, false, n, out_xy_le);
}

}  // extern "C"
