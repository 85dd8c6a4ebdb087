// abi.hip -- the rest of the C-ABI of libtemsm.so (include/te_msm.h): options, trim, the building blocks te_msm_partial_device*,
// host tails, stage times, synthetic inputs and debug reads.
#include "engine.hpp"
#include "host_tail.hpp"
#include "host_tail377.hpp"
#include "synth.hpp"

using namespace te_eng;

extern "C" {

int te_msm_probe_queues(te_ctx* ctx) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  drain_workers(ctx);
  int classes = 0;
  for (gpu_t& d : ctx->devs) {
    if (d.in_flight) return set_err(ctx, TE_MSM_ESTATE, "te_msm_probe_queues: collect the MSMs in flight first");
    HIP_TRY(ctx, hipSetDevice(d.device));
    spread_streams_over_queues(d);
    d.streams_final = true;
    int c = -1; for (const workset_t& ws : d.ws) c = std::max(c, ws.hw_queue_class);
    classes = std::max(classes, c + 1);
  }
  return classes;          // 0: the measurement was not accepted (its two passes disagreed): creation order kept
}

int te_msm_trim(te_ctx* ctx, int keep_worksets) {
  device_guard restore_callers_device;
  if (!ctx || keep_worksets < 0) return TE_MSM_EINVAL;
  drain_workers(ctx);
  int freed = 0;
  for (gpu_t& d : ctx->devs) {
    HIP_TRY(ctx, hipSetDevice(d.device));
    for (int i = keep_worksets; i < TE_MSM_WORKSETS; i++) {
      workset_t& ws = d.ws[i];
      if (te_sched::slot_ticket(ws.slot) || !(ws.d_recs || ws.d_in_points || ws.d_zero)) continue;       // owned by a ticket, or nothing to free
      if (ws.used) HIP_TRY(ctx, hipEventSynchronize(ws.ev_done));
      if (ws.copy_stream) HIP_TRY(ctx, hipStreamSynchronize(ws.copy_stream));
      free_workset_buffers(ws);
      freed++;
    }
    { std::lock_guard<std::mutex> lk(*d.chk_mu); d.ntt_tab.release(); d.ntt_tmp.release(); d.poly_tmp.release(); d.spmv_tmp.release(); d.scan_tmp.release(); }      // the NTT twiddle tables and scratch: made again by the next transform (none runs: it holds chk_mu)
    for (auto& sl : d.slabs) if (sl.users == 0 && sl.d) {                    // idle shared record slabs
      if (int rc = settle_slab(ctx, sl, nullptr, true)) return rc;
      for (workset_t& ws : d.ws) if (ws.recs_last == sl.d) ws.recs_last = nullptr;
      HIP_TRY(ctx, hipFree(sl.d)); sl.d = nullptr; sl.cap = 0; sl.src = nullptr; sl.converted = false;
    }
  }
  return freed;
}

int te_msm_set_option(te_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return TE_MSM_EINVAL;
  drain_workers(ctx);               // asynchronous submits read the options on the devices' host threads
  if (!strcmp(key, "window_bits")) { if (value != 0 && (value < 4 || value > 16)) return set_err(ctx, TE_MSM_EINVAL, "window_bits must be 0 or in [4,16]"); ctx->opt_window_bits = (int)value; return 0; }
  if (!strcmp(key, "sort_buckets")) { ctx->opt_sort = value ? 1 : 0; return 0; }
  if (!strcmp(key, "signed_digits")) { ctx->opt_signed = value ? 1 : 0; return 0; }
  if (!strcmp(key, "curve")) {
    if (value != TE_MSM_CURVE_TE_BLS12 && value != TE_MSM_CURVE_BLS12_377_G1) return set_err(ctx, TE_MSM_EINVAL, "unknown curve");
    ctx->opt_curve = (int)value; return 0;
  }
  if (!strcmp(key, "profile")) { ctx->opt_profile = value < 0 ? 0 : (value > 2 ? 2 : (int)value); ctx->have_stage_ms = false; return 0; }
  if (!strcmp(key, "prezero")) { ctx->opt_prezero = value ? 1 : 0; return 0; }
  if (!strcmp(key, "check_points")) { if (value < 0 || value > 2) return set_err(ctx, TE_MSM_EINVAL, "check_points must be 0, 1 or 2"); ctx->opt_check_points = (int)value; return 0; }
  if (!strcmp(key, "host_chunks")) { if (value < 0 || value > 64) return set_err(ctx, TE_MSM_EINVAL, "host_chunks out of range"); ctx->opt_host_chunks = (int)value; return 0; }
  if (!strcmp(key, "workset")) { if (value < 0 || value >= TE_MSM_WORKSETS) return set_err(ctx, TE_MSM_EINVAL, "workset out of range"); ctx->opt_workset = (int)value; return 0; }
  if (!strcmp(key, "segment_len")) { if (value < 0 || value > 1000000) return set_err(ctx, TE_MSM_EINVAL, "segment_len must be 0 (from n) or in [1, 1e6]"); ctx->opt_seg_len = (int)value; return 0; }
  if (!strcmp(key, "host_shard_min")) { if (value < 1 || value > (1ll << 30)) return set_err(ctx, TE_MSM_EINVAL, "host_shard_min out of range"); ctx->opt_host_shard_min = (int)value; return 0; }
  if (!strcmp(key, "queue_probe")) { ctx->opt_queue_probe = value ? 1 : 0; return 0; }
  if (!strcmp(key, "packed_sort")) { ctx->opt_packed = value ? 1 : 0; return 0; }
  if (!strcmp(key, "fold_pairs")) { ctx->opt_fold_pairs = value ? 1 : 0; return 0; }
  if (!strcmp(key, "stage_device_inputs")) { ctx->opt_stage_device_inputs = value ? 1 : 0; return 0; }
  if (!strcmp(key, "host_staging")) { ctx->opt_host_staging = value ? 1 : 0; return 0; }
  if (!strcmp(key, "upload_threads")) { if (value < 1 || value > 16) return set_err(ctx, TE_MSM_EINVAL, "upload_threads must be in [1, 16]"); ctx->opt_upload_threads = (int)value; return 0; }
  if (!strcmp(key, "bind_affine")) { ctx->opt_bind_affine = value ? 1 : 0; return 0; }
  if (!strcmp(key, "share_records")) { ctx->opt_share_records = value == 2 ? 2 : value ? 1 : 0; return 0; }
  if (!strcmp(key, "bind_fixed_base")) { if (value != 0 && (value < 16 || value > 21)) return set_err(ctx, TE_MSM_EINVAL, "bind_fixed_base must be 0 or in [16, 21]"); ctx->opt_bind_fixed_base = (int)value; return 0; }
  if (!strcmp(key, "scalar_chunks")) { if (value < 0 || value > 64) return set_err(ctx, TE_MSM_EINVAL, "scalar_chunks out of range"); ctx->opt_scalar_chunks = (int)value; return 0; }
  if (!strcmp(key, "scalars_montgomery")) { if (value != 0 && value != 1) return set_err(ctx, TE_MSM_EINVAL, "scalars_montgomery must be 0 or 1"); ctx->opt_scalars_montgomery = (int)value; return 0; }
  if (!strcmp(key, "points_montgomery")) { if (value != 0 && value != 1) return set_err(ctx, TE_MSM_EINVAL, "points_montgomery must be 0 or 1"); ctx->opt_points_montgomery = (int)value; return 0; }
  if (!strcmp(key, "point_stride")) {
    if (value != 0 && (value % 8 != 0 || value < 64 || value > (int64_t)kPointStrideMax)) return set_err(ctx, TE_MSM_EINVAL, "point_stride must be 0 or a multiple of 8 in [64, 128]");
    ctx->opt_point_stride = (int)value; return 0;
  }
  if (!strcmp(key, "point_infinity_flag")) { if (value != 0 && value != 1) return set_err(ctx, TE_MSM_EINVAL, "point_infinity_flag must be 0 or 1"); ctx->opt_point_infinity_flag = (int)value; return 0; }
  if (!strcmp(key, "scalar_record_bytes")) { if (value != 0 && value != 8 && value != 16 && value != 32 && value != 48) return set_err(ctx, TE_MSM_EINVAL, "scalar_record_bytes must be 0, 8, 16, 32 or 48");
    // (16 was never a record size: it stays refused, as a slip for 32 or 48 would be, until the caller has declared a width it can hold)
    if (value == 16 && !ctx->opt_scalar_bits) return set_err(ctx, TE_MSM_EINVAL, "scalar_record_bytes = 16 needs option \"scalar_bits\" set first (1..128)");
    ctx->opt_scalar_record_bytes = (int)value; return 0; }
  if (!strcmp(key, "scalar_bits")) { if (value < 0 || value > 256) return set_err(ctx, TE_MSM_EINVAL, "scalar_bits must be 0 or in [1, 256]"); ctx->opt_scalar_bits = (int)value; return 0; }
  if (!strcmp(key, "mul_base_window")) { if (value < 4 || value > 12) return set_err(ctx, TE_MSM_EINVAL, "mul_base_window must be in [4, 12]"); ctx->opt_mul_base_window = (int)value; return 0; }
  if (!strcmp(key, "batch_small_max")) { if (value < 0 || value > (1ll << 31)) return set_err(ctx, TE_MSM_EINVAL, "batch_small_max must be in [0, 2^31]"); ctx->opt_batch_small_max = value; return 0; }
  return set_err(ctx, TE_MSM_EINVAL, "unknown option");
}

int te_msm_get_option(te_ctx* ctx, const char* key, int64_t* value) {
  if (!ctx || !key || !value) return TE_MSM_EINVAL;
  if (!strcmp(key, "window_bits")) { *value = ctx->opt_window_bits; return 0; }
  if (!strcmp(key, "sort_buckets")) { *value = ctx->opt_sort; return 0; }
  if (!strcmp(key, "signed_digits")) { *value = ctx->opt_signed; return 0; }
  if (!strcmp(key, "curve")) { *value = ctx->opt_curve; return 0; }
  if (!strcmp(key, "profile")) { *value = ctx->opt_profile; return 0; }
  if (!strcmp(key, "num_devices")) { *value = (int64_t)ctx->devs.size(); return 0; }
  if (!strcmp(key, "peer_copies")) { *value = ctx->stat_peer_copies; return 0; }
  if (!strcmp(key, "peer_bytes")) { *value = ctx->stat_peer_bytes; return 0; }
  if (!strcmp(key, "entries_accumulated")) { *value = ctx->stat_entries; return 0; }
  if (!strcmp(key, "stage_device_inputs")) { *value = ctx->opt_stage_device_inputs; return 0; }
  if (!strcmp(key, "host_staging")) { *value = ctx->opt_host_staging; return 0; }
  if (!strcmp(key, "upload_threads")) { *value = ctx->opt_upload_threads; return 0; }
  if (!strcmp(key, "segment_len")) { *value = ctx->opt_seg_len; return 0; }
  if (!strcmp(key, "segment_len_used")) { drain_workers(ctx); const gpu_t& d0 = ctx->devs[0]; *value = d0.ws[d0.last_ws].used ? (int64_t)d0.ws[d0.last_ws].plan.seg_len : 0; return 0; }
  if (!strcmp(key, "workset")) { *value = ctx->opt_workset; return 0; }
  if (!strcmp(key, "prezero")) { *value = ctx->opt_prezero; return 0; }
  if (!strcmp(key, "check_points")) { *value = ctx->opt_check_points; return 0; }
  if (!strcmp(key, "bad_point_index")) { *value = ctx->bad_point_index; return 0; }
  if (!strcmp(key, "bad_point_reason")) { *value = ctx->bad_point_reason; return 0; }
  if (!strcmp(key, "bad_point_operand")) { *value = ctx->bad_point_operand; return 0; }
  if (!strcmp(key, "group_add_piece")) { *value = (int64_t)TE_MSM_GROUP_ADD_PIECE; return 0; }
  if (!strcmp(key, "group_sum_grid")) { *value = (int64_t)TE_MSM_GROUP_SUM_GRID; return 0; }
  if (!strcmp(key, "bad_field_index")) { *value = ctx->bad_field_index; return 0; }
  if (!strcmp(key, "bad_field_reason")) { *value = ctx->bad_field_reason; return 0; }
  if (!strcmp(key, "field_inv_group")) { *value = (int64_t)TE_MSM_FIELD_INV_GROUP; return 0; }
  if (!strcmp(key, "ntt_max_log_n")) { *value = (int64_t)TE_MSM_NTT_MAX_LOG_N; return 0; }
  if (!strcmp(key, "ntt_table_bytes")) {                               // twiddle tables the context holds, over its devices
    *value = 0;
    for (gpu_t& d : ctx->devs) { std::lock_guard<std::mutex> lk(*d.chk_mu); *value += d.ntt_tab.p ? (int64_t)d.ntt_tab.cap : 0; }
    return 0;
  }
  if (!strcmp(key, "ntt_scratch_bytes")) {                             // ... and the buffer between the passes of multi-pass transforms
    *value = 0;
    for (gpu_t& d : ctx->devs) { std::lock_guard<std::mutex> lk(*d.chk_mu); *value += d.ntt_tmp.p ? (int64_t)d.ntt_tmp.cap : 0; }
    return 0;
  }
  if (!strcmp(key, "poly_chunk")) { *value = (int64_t)te_poly::chunk_in_force(); return 0; }   // TE_MSM_POLY_CHUNK, or what the environment names
  if (!strcmp(key, "poly_scratch_bytes")) {                            // the sums, carries and powers of te_msm_poly_divide*
    *value = 0;
    for (gpu_t& d : ctx->devs) { std::lock_guard<std::mutex> lk(*d.chk_mu); *value += d.poly_tmp.p ? (int64_t)d.poly_tmp.cap : 0; }
    return 0;
  }
  if (!strcmp(key, "spmv_chunk")) { *value = (int64_t)te_spmv::chunk_in_force(); return 0; }   // TE_MSM_SPMV_CHUNK, or what the environment names
  if (!strcmp(key, "spmv_scratch_bytes")) {                            // the fragments of te_msm_spmv*
    *value = 0;
    for (gpu_t& d : ctx->devs) { std::lock_guard<std::mutex> lk(*d.chk_mu); *value += d.spmv_tmp.p ? (int64_t)d.spmv_tmp.cap : 0; }
    return 0;
  }
  if (!strcmp(key, "scan_chunk")) { *value = (int64_t)te_scan::chunk_in_force(); return 0; }   // TE_MSM_SCAN_CHUNK, or what the environment names
  if (!strcmp(key, "scan_scratch_bytes")) {                            // the totals, carries and seeds of te_msm_field_scan*
    *value = 0;
    for (gpu_t& d : ctx->devs) { std::lock_guard<std::mutex> lk(*d.chk_mu); *value += d.scan_tmp.p ? (int64_t)d.scan_tmp.cap : 0; }
    return 0;
  }
  if (!strcmp(key, "matrix_bytes")) {                                  // the bound matrices, over all devices
    int64_t t = 0;
    for (const te_matrix* m : ctx->matrices) for (const uint8_t* s : m->side) if (s) t += (int64_t)m->bytes();
    *value = t;
    return 0;
  }
  if (!strcmp(key, "bad_index_position")) { *value = ctx->bad_index_position; return 0; }
  if (!strcmp(key, "host_chunks")) { *value = ctx->opt_host_chunks; return 0; }
  if (!strcmp(key, "host_shard_min")) { *value = ctx->opt_host_shard_min; return 0; }
  if (!strcmp(key, "queue_probe")) { *value = ctx->opt_queue_probe; return 0; }
  if (!strcmp(key, "packed_sort")) { *value = ctx->opt_packed; return 0; }
  if (!strcmp(key, "fold_pairs")) { *value = ctx->opt_fold_pairs; return 0; }
  if (!strcmp(key, "streams_final")) { *value = ctx->devs[0].streams_final ? 1 : 0; return 0; }
  if (!strcmp(key, "bind_affine")) { *value = ctx->opt_bind_affine; return 0; }
  if (!strcmp(key, "share_records")) { *value = ctx->opt_share_records; return 0; }
  if (!strcmp(key, "record_conversions")) { *value = __atomic_load_n(&ctx->stat_record_conversions, __ATOMIC_RELAXED); return 0; }
  if (!strcmp(key, "record_slabs")) { int64_t t = 0; for (const gpu_t& d : ctx->devs) for (const auto& sl : d.slabs) if (sl.d) t++; *value = t; return 0; }
  if (!strcmp(key, "scalar_chunks")) { *value = ctx->opt_scalar_chunks; return 0; }
  if (!strcmp(key, "batch_small_max")) { *value = ctx->opt_batch_small_max; return 0; }
  if (!strcmp(key, "scalars_montgomery")) { *value = ctx->opt_scalars_montgomery; return 0; }
  if (!strcmp(key, "points_montgomery")) { *value = ctx->opt_points_montgomery; return 0; }
  if (!strcmp(key, "point_stride")) { *value = ctx->opt_point_stride; return 0; }
  if (!strcmp(key, "point_infinity_flag")) { *value = ctx->opt_point_infinity_flag; return 0; }
  if (!strcmp(key, "scalar_record_bytes")) { *value = ctx->opt_scalar_record_bytes; return 0; }
  if (!strcmp(key, "scalar_bits")) { *value = ctx->opt_scalar_bits; return 0; }
  if (!strcmp(key, "batch_sequences")) { *value = ctx->stat_batch_sequences; return 0; }
  if (!strcmp(key, "bind_fixed_base")) { *value = ctx->opt_bind_fixed_base; return 0; }
  if (!strcmp(key, "fixed_base_fallbacks")) { *value = ctx->stat_fb_fallbacks; return 0; }
  if (!strcmp(key, "bases_bound")) { *value = (int64_t)ctx->bases.size(); return 0; }
  if (!strcmp(key, "bases_bytes")) { int64_t t = 0; for (const te_bases* b : ctx->bases) for (const uint8_t* r : b->recs) if (r) t += (int64_t)(b->n * b->rec_bytes) * (b->fb_c ? b->fb_W : 1); *value = t; return 0; }
  if (!strcmp(key, "mul_base_window")) { *value = ctx->opt_mul_base_window; return 0; }
  if (!strcmp(key, "mul_bases_bound")) { *value = (int64_t)ctx->mul_bases.size(); return 0; }
  if (!strcmp(key, "mul_base_bytes")) { int64_t t = 0; for (const te_base* b : ctx->mul_bases) for (const uint8_t* r : b->tab) if (r) t += (int64_t)b->bytes(); *value = t; return 0; }
  if (!strcmp(key, "in_flight")) { int64_t t = 0; for (const gpu_t& d : ctx->devs) t += d.in_flight; *value = t; return 0; }
  if (!strcmp(key, "device_bytes")) {      drain_workers(ctx);      // device memory this context holds in work-set buffers (te_msm_trim gives it back)
    int64_t tot = 0;
    for (const gpu_t& d : ctx->devs) {
      for (const workset_t& ws : d.ws) workset_t::each_buffer(ws, [&](const auto& b) { tot += (int64_t)b.cap; });
      for (const auto& sl : d.slabs) if (sl.d) tot += (int64_t)sl.cap;
    }
    *value = tot; return 0;
  }
  return set_err(ctx, TE_MSM_EINVAL, "unknown option");
}

int te_msm_set_window_shard(te_ctx* ctx, int first, int step) {
  if (!ctx) return TE_MSM_EINVAL;
  if (ctx->devs.size() != 1) return set_err(ctx, TE_MSM_ESTATE, "window shards are set automatically for multi-device contexts");
  if (first < 0 || step < 1) return set_err(ctx, TE_MSM_EINVAL, "need first >= 0 and step >= 1");
  drain_workers(ctx);               // asynchronous enqueues read the shard on the device's host threads
  ctx->devs[0].w_first = first; ctx->devs[0].w_step = step;
  return 0;
}

int te_msm_plan(te_ctx* ctx, uint64_t n, int* window_bits, int* num_windows) {
  if (!ctx) return TE_MSM_EINVAL;
  const plan_t p = make_plan(ctx, ctx->devs[0], plan_shard(n ? n : 1));
  if (window_bits) *window_bits = p.c;
  if (num_windows) *num_windows = p.W;
  return 0;
}

static const char* const kPartialNoCheck =
    "option \"check_points\" is not supported by the te_msm_partial_device building blocks (they report nothing per point): "
    "check the points with te_msm_check_points_device, then set \"check_points\" to 0";
int te_msm_partial_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n, void* d_partials, void* stream) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  if (ctx->devs.size() != 1) return set_err(ctx, TE_MSM_ESTATE, "te_msm_partial_device needs a single-device context");
  if (ctx->opt_check_points) return set_err(ctx, TE_MSM_EINVAL, kPartialNoCheck);
  if (!d_points_xy_le || !d_scalars_le || !d_partials || n == 0 || n >= (1ull << 31)) return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
  if (int rc = check_scalar_record(ctx, d_scalars_le)) return rc;
  gpu_t& d = ctx->devs[0];
  workset_t& ws = d.ws[ctx->opt_workset];
  if (te_sched::slot_ticket(ws.slot)) return set_err(ctx, TE_MSM_ESTATE, "the selected work set holds a submitted MSM that has not been collected");
  HIP_TRY(ctx, hipSetDevice(d.device));
  partial_req r; r.d_points = d_points_xy_le; r.d_scalars = d_scalars_le; r.n = n; r.d_partials_out = d_partials; r.share = SHARE_CONVERT;
  r.stream = stream == TE_MSM_OWN_STREAM ? ws.stream : (hipStream_t)stream;
  return enqueue_partial(ctx, d, ws, r);
}

int te_msm_partial_device_batch(te_ctx* ctx, const void* const* d_points_xy_le, const void* const* d_scalars_le, uint64_t n, int count,
                                void* d_partials, void* stream) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  if (ctx->devs.size() != 1) return set_err(ctx, TE_MSM_ESTATE, "te_msm_partial_device_batch needs a single-device context");
  if (ctx->opt_check_points) return set_err(ctx, TE_MSM_EINVAL, kPartialNoCheck);
  if (!d_points_xy_le || !d_scalars_le || !d_partials || n == 0 || n >= (1ull << 31) || count < 1 || count > TE_MSM_MAX_BATCH)
    return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
  for (int m = 0; m < count; m++) if (!d_points_xy_le[m] || !d_scalars_le[m]) return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
  for (int m = 0; m < count; m++) if (int rc = check_scalar_record(ctx, d_scalars_le[m])) return rc;
  gpu_t& d = ctx->devs[0];
  workset_t& ws = d.ws[ctx->opt_workset];
  if (te_sched::slot_ticket(ws.slot)) return set_err(ctx, TE_MSM_ESTATE, "the selected work set holds a submitted MSM that has not been collected");
  HIP_TRY(ctx, hipSetDevice(d.device));
  partial_req r; r.n = n; r.d_partials_out = d_partials; r.share = SHARE_CONVERT; r.batch = count;
  r.stream = stream == TE_MSM_OWN_STREAM ? ws.stream : (hipStream_t)stream;
  // the pointer arrays are only read while the launches are enqueued
  if (count == 1) { r.d_points = d_points_xy_le[0]; r.d_scalars = d_scalars_le[0]; } else { r.d_points = d_points_xy_le; r.d_scalars = d_scalars_le; }
  return enqueue_partial(ctx, d, ws, r);
}

int te_msm_workset_stream(te_ctx* ctx, int workset, void** stream, int* hw_queue_class) {
  if (!ctx || workset < 0 || workset >= TE_MSM_WORKSETS || !stream) return TE_MSM_EINVAL;
  if (ctx->devs.size() != 1) return set_err(ctx, TE_MSM_ESTATE, "te_msm_workset_stream needs a single-device context");
  const workset_t& ws = ctx->devs[0].ws[workset];
  ctx->devs[0].streams_exported = true;       // the handle leaves the library: the device's streams are parked, not destroyed, from now on
  *stream = (void*)ws.stream;
  if (hw_queue_class) *hw_queue_class = ws.hw_queue_class;
  return 0;
}

int te_msm_partial_wait(te_ctx* ctx, int workset) {
  device_guard restore_callers_device;
  if (!ctx || workset < 0 || workset >= TE_MSM_WORKSETS) return TE_MSM_EINVAL;
  if (ctx->devs.size() != 1) return set_err(ctx, TE_MSM_ESTATE, "te_msm_partial_wait needs a single-device context");
  drain_workers(ctx);
  workset_t& ws = ctx->devs[0].ws[workset];
  if (!ws.used) return 0;
  HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));
  (void)collect_stage_ms(ctx, ctx->devs[0], ws);     // stage times of that launch sequence, when it was profiled (te_msm_stage_ms), whatever its status
  return settle_status(ctx, ws);
}

int te_msm_finalize(te_ctx* ctx, const uint8_t* partials, int window_bits, int num_windows, uint8_t out_xy_le[64]) {
  device_guard restore_callers_device;
  if (!ctx || !partials || !out_xy_le || window_bits < 2 || window_bits > 16 || num_windows < 1 || num_windows > 128) return TE_MSM_EINVAL;
  gpu_t& d = ctx->devs[0];
  workset_t& ws = d.ws[d.last_ws];
  int bucket_bits = ctx->opt_signed ? window_bits - 1 : window_bits;
  if (ws.used) {
    HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));
    if (int rc = settle_status(ctx, ws, false)) return rc;
    (void)collect_stage_ms(ctx, d, ws);
    // the rows were produced under ws.plan: its digit form decides, not an option changed since
    if (window_bits != ws.plan.c || num_windows != ws.plan.W)
      return set_err(ctx, TE_MSM_ESTATE, "te_msm_finalize: window_bits / num_windows differ from the plan of the last te_msm_partial_device call (use te_msm_finalize_host_ex for rows produced elsewhere)");
    bucket_bits = (int)ws.plan.logB;
    if (ws.plan.curve == TE_MSM_CURVE_BLS12_377_G1) { te377_host::horner_to_affine(partials, window_bits, bucket_bits, num_windows, out_xy_le); return 0; }
  } else if (ctx->opt_curve == TE_MSM_CURVE_BLS12_377_G1) {
    te377_host::horner_to_affine(partials, window_bits, bucket_bits, num_windows, out_xy_le); return 0;
  }
  te_host::horner_to_affine(partials, window_bits, bucket_bits, num_windows, out_xy_le);
  return 0;
}

int te_msm_host_tail_features(void) {
  int f = te_host::have_adx() ? 1 : 0;
#if defined(__x86_64__)
  if (te_host::have_ifma()) f |= 2;
#endif
  return f;
}

int te_msm_finalize_host(const uint8_t* partials, int window_bits, int num_windows, uint8_t out_xy_le[64]) {
  if (!partials || !out_xy_le || window_bits < 2 || window_bits > 16 || num_windows < 1 || num_windows > 128) return TE_MSM_EINVAL;
  return te_msm_finalize_host_ex(partials, window_bits, window_bits - 1, num_windows, out_xy_le);
}

int te_msm_finalize_host_ex(const uint8_t* partials, int window_bits, int bucket_bits, int num_windows, uint8_t out_xy_le[64]) {
  if (!partials || !out_xy_le || window_bits < 2 || window_bits > 16 || num_windows < 1 || num_windows > 128) return TE_MSM_EINVAL;
  if (bucket_bits != window_bits && bucket_bits != window_bits - 1) return TE_MSM_EINVAL;
  if (!te_host::tail_selftest()) return TE_MSM_ESTATE;
  te_host::horner_to_affine(partials, window_bits, bucket_bits, num_windows, out_xy_le);
  return 0;
}

int te_msm_finalize_gathered(const uint8_t* gathered, int world, int window_bits, int bucket_bits, int num_windows,
                             uint8_t out_xy_le[64]) {
  if (!gathered || world < 1 || num_windows < 1 || num_windows > 128) return TE_MSM_EINVAL;
  std::vector<uint8_t> merged((size_t)num_windows * TE_MSM_PARTIAL_BYTES);
  for (int w = 0; w < num_windows; w++)
    memcpy(&merged[(size_t)w * TE_MSM_PARTIAL_BYTES],
           gathered + ((size_t)(w % world) * num_windows + w) * TE_MSM_PARTIAL_BYTES, TE_MSM_PARTIAL_BYTES);
  return te_msm_finalize_host_ex(merged.data(), window_bits, bucket_bits, num_windows, out_xy_le);
}

int te_msm_finalize_host_curve(int curve, const uint8_t* partials, int window_bits, int bucket_bits, int num_windows, uint8_t* out_xy_le) {
  if (curve == TE_MSM_CURVE_TE_BLS12) return te_msm_finalize_host_ex(partials, window_bits, bucket_bits, num_windows, out_xy_le);
  if (curve != TE_MSM_CURVE_BLS12_377_G1) return TE_MSM_EINVAL;
  if (!partials || !out_xy_le || window_bits < 2 || window_bits > 16 || num_windows < 1 || num_windows > 128) return TE_MSM_EINVAL;
  if (bucket_bits != window_bits && bucket_bits != window_bits - 1) return TE_MSM_EINVAL;
  if (!te377_host::tail_selftest()) return TE_MSM_ESTATE;
  te377_host::horner_to_affine(partials, window_bits, bucket_bits, num_windows, out_xy_le);
  return 0;
}

int te_msm_finalize_gathered_curve(int curve, const uint8_t* gathered, int world, int window_bits, int bucket_bits, int num_windows,
                                   uint8_t* out_xy_le) {
  if (!gathered || world < 1 || num_windows < 1 || num_windows > 128) return TE_MSM_EINVAL;
  if (curve != TE_MSM_CURVE_TE_BLS12 && curve != TE_MSM_CURVE_BLS12_377_G1) return TE_MSM_EINVAL;
  const size_t row = sizes_of(curve).row;
  std::vector<uint8_t> merged((size_t)num_windows * row);
  for (int w = 0; w < num_windows; w++)
    memcpy(&merged[(size_t)w * row], gathered + ((size_t)(w % world) * num_windows + w) * row, row);
  return te_msm_finalize_host_curve(curve, merged.data(), window_bits, bucket_bits, num_windows, out_xy_le);
}

int te_msm_finalize_sum_curve(int curve, const uint8_t* const* row_sets, int sets, int window_bits, int bucket_bits, int num_windows, uint8_t* out_xy_le) {
  if (curve != TE_MSM_CURVE_TE_BLS12 && curve != TE_MSM_CURVE_BLS12_377_G1) return TE_MSM_EINVAL;
  if (!row_sets || sets < 1 || sets > 4096 || !out_xy_le || window_bits < 2 || window_bits > 16 || num_windows < 1 || num_windows > 128) return TE_MSM_EINVAL;
  if (bucket_bits != window_bits && bucket_bits != window_bits - 1) return TE_MSM_EINVAL;
  for (int i = 0; i < sets; i++) if (!row_sets[i]) return TE_MSM_EINVAL;
  // three or more sets: merged window by window first, then folded (the two-step form the multi-device te_msm_run spreads over
  // its host threads); one or two: summed on the fly
  std::vector<uint8_t> present((size_t)num_windows, 0);
  if (curve == TE_MSM_CURVE_BLS12_377_G1) {
    if (!te377_host::tail_selftest()) return TE_MSM_ESTATE;
    if (sets <= 2) { te377_host::horner_to_affine_multi(row_sets, sets, window_bits, bucket_bits, num_windows, out_xy_le); return 0; }
    std::vector<te377_host::Pt> m((size_t)num_windows * 5);
    for (int w = 0; w < num_windows; w++) te377_host::merge_window_rows(row_sets, sets, w, m.data(), present.data());
    te377_host::horner_to_affine_points(m.data(), present.data(), window_bits, bucket_bits, num_windows, out_xy_le);
  } else {
    if (!te_host::tail_selftest()) return TE_MSM_ESTATE;
    if (sets <= 2) { te_host::horner_to_affine_multi(row_sets, sets, window_bits, bucket_bits, num_windows, out_xy_le); return 0; }
    std::vector<te_host::Pt> m((size_t)num_windows * 5);
    for (int w = 0; w < num_windows; w++) te_host::merge_window_rows(row_sets, sets, w, m.data(), present.data());
    te_host::horner_to_affine_points(m.data(), present.data(), window_bits, bucket_bits, num_windows, out_xy_le);
  }
  return 0;
}

int te_msm_stage_ms(te_ctx* ctx, float* ms, const char** names, int max_stages) {
  if (!ctx || !ms) return TE_MSM_EINVAL;
  if (!ctx->have_stage_ms) return set_err(ctx, TE_MSM_ESTATE, "no profiled run yet (set option profile=1)");
  int k = 0;
  for (int i = 0; i < ST_COUNT + 2 && k < max_stages; i++) {
    if (ctx->stage_ms[i] < 0) continue;            // not measured at this profile level
    ms[k] = ctx->stage_ms[i]; if (names) names[k] = kStageNames[i]; k++;
  }
  return k;
}

int te_msm_synth_inputs(uint64_t seed, uint64_t n, int fixed_point, uint8_t* points_xy_le, uint8_t* scalars_le) {
  if (n >= (1ull << 31) || !te_host::tail_selftest()) return TE_MSM_EINVAL;
  if (scalars_le) te_host::synth_scalars(seed, n, scalars_le);
  if (points_xy_le) {
    if (fixed_point == 1) te_host::synth_points_fixed(n, points_xy_le);
    else if (fixed_point == 2) te_host::synth_points_random(seed, n, points_xy_le);
    else if (fixed_point == 0) te_host::synth_points(seed, n, points_xy_le);
    else return TE_MSM_EINVAL;
  }
  return 0;
}

int te_msm_synth_inputs_bls12_377(uint64_t seed, uint64_t n, uint8_t* points_xy_le, uint8_t* scalars_le) {
  if (n >= (1ull << 31) || !te377_host::tail_selftest()) return TE_MSM_EINVAL;
  if (scalars_le) te377_host::synth_scalars(seed, n, scalars_le);
  if (points_xy_le) te377_host::synth_points(seed, n, points_xy_le);
  return 0;
}

int64_t te_msm_debug_read(te_ctx* ctx, const char* stage, void* dst, uint64_t cap) {
  device_guard restore_callers_device;
  if (!ctx || !stage || !dst) return TE_MSM_EINVAL;
  drain_workers(ctx);
  gpu_t& d = ctx->devs[0];
  workset_t& ws = d.ws[d.last_ws];
  if (!ws.used) return set_err(ctx, TE_MSM_ESTATE, "no run yet");
  const plan_t& p = ws.plan; const uint64_t n = ws.n;
  const void* src = nullptr; uint64_t bytes = 0;
  if (ws.zero_clean_words && (!strcmp(stage, "bucket_count") || !strcmp(stage, "num_segments") || !strcmp(stage, "partials")))
    return set_err(ctx, TE_MSM_ESTATE, "this stage lives in the block that is cleared behind an MSM's read-back: set option prezero = 0 before the run to keep it");
  if (!strcmp(stage, "records")) {
    if (!ws.recs_last) return set_err(ctx, TE_MSM_ESTATE, "the last run gathered from a bound point set: the work set holds no records of its own");
    src = ws.recs_last; bytes = n * sizes_of(p.curve).rec;
  }
  else if (!strcmp(stage, "digits")) { src = ws.d_digits; bytes = (uint64_t)p.nw * p.nst * 2; }   // row stride nst = n rounded up to 8
  else if (!strcmp(stage, "bucket_count")) { src = ws.d_bucket_count; bytes = (uint64_t)p.nw * p.B * 4; }
  else if (!strcmp(stage, "bucket_start")) { src = ws.d_bucket_start; bytes = (uint64_t)p.nw * p.B * 4; }
  else if (!strcmp(stage, "sorted")) { src = ws.d_sorted; bytes = (uint64_t)p.nw * n * 4; }
  else if (!strcmp(stage, "num_segments")) { src = ws.d_num_seg; bytes = 4; }
  else if (!strcmp(stage, "seg_bucket")) { src = ws.d_seg_bucket; bytes = ((uint64_t)p.nw * p.B + (uint64_t)p.nw * (n / p.seg_len)) * 4; }
  else if (!strcmp(stage, "seg_len")) { src = ws.d_seg_lenv; bytes = ((uint64_t)p.nw * p.B + (uint64_t)p.nw * (n / p.seg_len)) * 4; }
  else if (!strcmp(stage, "order")) { src = ws.d_order; bytes = ((uint64_t)p.nw * p.B + (uint64_t)p.nw * (n / p.seg_len)) * 4; }
  else if (!strcmp(stage, "part_start")) { src = ws.d_part_start; bytes = (uint64_t)p.nw * p.P * 4; }
  else if (!strcmp(stage, "part_count")) { src = ws.d_part_count; bytes = (uint64_t)p.nw * p.P * 4; }
  else if (!strcmp(stage, "part_keys") && !p.packed) { src = ws.d_part_keys; bytes = (uint64_t)p.nw * p.nst * 2; }
  else if (!strcmp(stage, "part_idx") && !p.packed) { src = ws.d_part_idx; bytes = (uint64_t)p.nw * p.nst * 4; }
  else if (!strcmp(stage, "part_keys") || !strcmp(stage, "part_idx")) {
    // packed level-1 entries (index | bucket low bits << 23 | sign << 31): taken apart here into the two views of the general form
    const bool want_keys = stage[5] == 'k';
    const uint64_t words = (uint64_t)p.nw * p.nst;
    std::vector<uint32_t> pk(words);
    HIP_TRY(ctx, hipSetDevice(d.device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    HIP_TRY(ctx, hipMemcpy(pk.data(), ws.d_part_idx, words * 4, hipMemcpyDeviceToHost));
    uint64_t out_bytes = words * (want_keys ? 2 : 4);
    if (out_bytes > cap) out_bytes = cap;
    if (want_keys) { uint16_t* o = static_cast<uint16_t*>(dst); for (uint64_t i = 0; i < out_bytes / 2; i++) o[i] = (uint16_t)(((pk[i] >> 23) & 0xffu) | ((pk[i] >> 31) << 15)); }
    else { uint32_t* o = static_cast<uint32_t*>(dst); for (uint64_t i = 0; i < out_bytes / 4; i++) o[i] = pk[i] & 0x7fffffu; }
    return (int64_t)out_bytes;
  }
  else if (!strcmp(stage, "buckets")) { src = ws.d_buckets; bytes = (uint64_t)p.nw * p.B * sizes_of(p.curve).acc; }
  else if (!strcmp(stage, "partials")) { src = ws.d_partials; bytes = (uint64_t)p.W * sizes_of(p.curve).row; }
  else return set_err(ctx, TE_MSM_EINVAL, "unknown stage");
  if (bytes > cap) bytes = cap;
  HIP_TRY(ctx, hipSetDevice(d.device));
  HIP_TRY(ctx, hipDeviceSynchronize());
  HIP_TRY(ctx, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return (int64_t)bytes;
}

}  // extern "C"
