// bases.hip -- bound point sets (include/te_msm.h, "resident bases"): bind and release, MSMs from scalars alone, over an indexed
// subset, and in batches over prefixes of the set.
#include "engine.hpp"

using namespace te_eng;

namespace te_eng {

namespace {
// ---- resident bases (include/te_msm.h): points bound once, scalars per call ---------------------------------------------------
bool valid_bases(const te_ctx* ctx, const te_bases* b) { return b && std::find(ctx->bases.begin(), ctx->bases.end(), b) != ctx->bases.end(); }
const char* const kBadBases = "not a bound point set of this context (released, or bound to another context)";
const char* const kBasesCurve = "the point set was bound under another curve than the one selected now (option \"curve\")";
// a bound point set of this context, bound under the curve selected now
int check_bases(te_ctx* ctx, const te_bases* b) {
  if (!valid_bases(ctx, b)) return set_err(ctx, TE_MSM_EINVAL, kBadBases);
  if (b->curve != ctx->opt_curve) return set_err(ctx, TE_MSM_EINVAL, kBasesCurve);
  return 0;
}

void free_bases(te_ctx* ctx, te_bases* b) {
  for (size_t i = 0; i < b->recs.size() && i < ctx->devs.size(); i++)
    if (b->recs[i]) { (void)hipSetDevice(ctx->devs[i].device); (void)hipFree(b->recs[i]); b->recs[i] = nullptr; }
}

// A whole MSM over a fixed-base set from HOST scalars on work set `ws`: all scalars cross PCIe in one copy (the digits of every
// window address one bucket set: there are no pieces to accumulate onto), then the fixed-base launch sequence and its read-back.
// (Fixed-base sets exist on the Twisted-Edwards curve only, whose one scalar record is the curve's own: option "scalar_record_bytes"
// changes nothing here, and k_fb_digits reads 32-byte records.)
int enqueue_fixed_base_host(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases, const uint8_t* src_scalars, uint64_t n, bool wait_for_pinned,
                            int scalar_form = -1) {
  HIP_TRY(ctx, hipSetDevice(d.device));
  const size_t sb = sizes_of(bases->curve).scalar_in;
  if (int rc = ensure_staging(ctx, ws, 0, n * sb)) return rc;
  if (int rc = wait_behind_previous(ctx, ws)) return rc;
  if (!wait_for_pinned) {
    // an asynchronous ticket: the lane thread waits for the upload itself (lane_wait), no wait enters the work set's stream
    if (ws.used) HIP_TRY(ctx, hipEventSynchronize(ws.ev_done));
    if (int rc = need_copy_stream(ctx, ws)) return rc;
    if (int rc = upload(ctx, ws, ws.d_in_scalars, src_scalars, n * sb, ws.copy_stream)) return rc;
    if (int rc = lane_wait(ctx, ws, ws.ev_copy, true)) return rc;
  } else {
    if (int rc = upload(ctx, ws, ws.d_in_scalars, src_scalars, n * sb, ws.stream)) return rc;
    if (wait_for_pinned && !ctx->opt_host_staging && host_memory_is_pinned(src_scalars)) {
      HIP_TRY(ctx, hipEventRecord(ws.ev_copy, ws.stream));
      HIP_TRY(ctx, hipEventSynchronize(ws.ev_copy));
    }
  }
  if (int rc = enqueue_fixed_base(ctx, d, ws, bases, ws.d_in_scalars, n, 0, ws.stream, scalar_form)) return rc;
  return fetch_rows(ctx, ws, ws.stream);
}

// te_msm_run_scalars_device on a context of D > 1 devices: WINDOW shards (device i computes windows i, i + D, ...).  Every
// device needs all n scalars: the holder reads them in place, the others pull them over their peer link (32 bytes per point:
// a third of what run_device_window_shards moves, so one copy each instead of its scatter + all-gather); every device gathers
// from its own copy of the bound records.  One host thread per device enqueues its copy, its share and its read-back.
int run_bound_window_shards(te_ctx* ctx, const te_bases* bases, const void* d_scalars, uint64_t n, uint8_t* out) {
  const size_t nd = ctx->devs.size();
  const plan_t p0 = make_plan(ctx, ctx->devs[0], plan_shard(n));
  const int owner = owner_of(ctx, "te_msm_run_scalars_device: the scalars must be resident on a device of the context", {d_scalars});
  if (owner < 0) return owner;
  const int src_dev = ctx->devs[(size_t)owner].device;
  std::vector<int> wsel;
  if (int rc = free_sets(ctx, nd, wsel)) return rc;
  std::vector<peer_traffic> moved(nd);
  auto share = [&](size_t i) -> int {
    gpu_t& d = ctx->devs[i]; workset_t& ws = d.ws[wsel[i]];
    HIP_TRY(ctx, hipSetDevice(d.device));
    device_inputs in; in.scalars = d_scalars;
    if (must_pull(ctx, d, src_dev)) { if (int rc = pull_inputs(ctx, d, ws, src_dev, n, (size_t)p0.sc_bytes, in, moved[i])) return rc; }
    partial_req r; r.d_scalars = in.scalars; r.n = n; r.stream = ws.stream; r.bases = bases; r.scalar_bytes = p0.sc_bytes; r.scalar_bits = p0.sc_bits;
    if (int rc = enqueue_partial(ctx, d, ws, r)) return rc;
    return fetch_rows(ctx, ws, ws.stream);
  };
  const int rc = te_sched::on_devices(*ctx, nd, share);
  for (const peer_traffic& m : moved) note_peer_traffic(ctx, m);
  return settle_window_shards(ctx, wsel, p0, rc, false, out);
}

int run_scalars_common(te_ctx* ctx, te_bases* bases, const void* src, bool src_is_host, uint8_t* out) {
  if (!ctx || !out) return TE_MSM_EINVAL;
  if (int rc = check_bases(ctx, bases)) return rc;
  if (int rc = check_scalar_record(ctx, src_is_host ? nullptr : src)) return rc;
  const uint64_t n = bases->n;
  if (n == 0) { write_identity(ctx->opt_curve, out); return 0; }
  if (!src) return set_err(ctx, TE_MSM_EINVAL, "null scalar buffer");
  size_t di = 0;
  const bool multi = ctx->devs.size() > 1;
  const bool fb_set = bases->fb_c && !scalar_bits_now(ctx);      // (a declared width runs the ordinary windows over the set's table 0)
  if (multi) {
    if (!fb_set) {
      if (src_is_host) return run_host_sharded(ctx, nullptr, static_cast<const uint8_t*>(src), n, out, bases);
      // (fewer windows than devices -- a narrow plan: a shard would be left without a window, the call runs whole on the holder, below)
      if ((size_t)make_plan(ctx, ctx->devs[0], plan_shard(n)).W >= ctx->devs.size()) return run_bound_window_shards(ctx, bases, src, n, out);
    }
    // a fixed-base set has no windows or point slices to shard (one bucket set): the lone call runs on ONE device -- the holder of
    // device-resident scalars, else the first; MSMs in flight (tickets) are how several devices work on such a set
    if (!src_is_host) {
      const int owner = owner_of(ctx, "te_msm_run_scalars_device: the scalars must be resident on a device of the context", {src});
      if (owner < 0) return owner;
      di = (size_t)owner;
    }
  }
  gpu_t& d = ctx->devs[di];
  const int wsel = lone_set(ctx, d, ctx->devs.size() > 1 ? 0 : ctx->opt_workset);
  if (wsel < 0) return wsel;
  workset_t& ws = d.ws[wsel];
  HIP_TRY(ctx, hipSetDevice(d.device));
  const plan_t p0 = make_plan(ctx, d, plan_shard(n));
  const size_t sb = (size_t)p0.sc_bytes;
  const bool fb = fb_set && (multi || d.w_step == 1);      // (a window-sharded single-device context keeps the ordinary windows)
  if (fb) {
    if (src_is_host) { if (int rc = enqueue_fixed_base_host(ctx, d, ws, bases, static_cast<const uint8_t*>(src), n, true)) return rc; }
    else { if (int rc = enqueue_fixed_base(ctx, d, ws, bases, src, n, 0, ws.stream)) return rc; if (int rc = fetch_rows(ctx, ws, ws.stream)) return rc; }
  } else if (src_is_host && !ctx->opt_profile && d.w_step == 1) {
    // whole MSM, no stage timing: the scalars in pieces
    host_slice_req r; r.recs = bases->recs[di]; r.rec_kind = bases->rec_kind; r.scalars = static_cast<const uint8_t*>(src); r.n = n;
    r.c = p0.c; r.K = scalar_pieces(ctx, n);
    if (int rc = enqueue_host_pieces(ctx, d, ws, r)) return rc;
  } else {
    const void* ds = src;
    if (src_is_host) {
      if (int rc = ensure_staging(ctx, ws, 0, n * sb)) return rc;
      if (int rc = wait_behind_previous(ctx, ws)) return rc;
      if (int rc = upload(ctx, ws, ws.d_in_scalars, static_cast<const uint8_t*>(src), n * sb, ws.stream)) return rc;
      ds = ws.d_in_scalars;
    }
    partial_req r; r.d_scalars = ds; r.n = n; r.stream = ws.stream; r.bases = bases; r.whole = multi;
    if (int rc = enqueue_partial(ctx, d, ws, r)) return rc;
    if (int rc = fetch_rows(ctx, ws, ws.stream)) return rc;
  }
  HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));
  if (int rc = fixed_base_settle(ctx, d, ws, bases)) return rc;
  if (int rc = settle_status(ctx, ws)) return rc;
  (void)collect_stage_ms(ctx, d, ws);
  fold_rows(ws.plan, ws.h_partials, out);
  return 0;
}

// ---- MSMs over an indexed subset of a bound point set (include/te_msm.h) ------------------------------------------------------
// the arguments all four calls share; 0 = go on
int indexed_args(te_ctx* ctx, const te_bases* bases, const void* idx, const void* scalars, uint64_t m, bool device = false) {
  if (int rc = check_bases(ctx, bases)) return rc;
  if (int rc = check_n(ctx, m)) return rc;
  if (int rc = check_scalar_record(ctx, device ? scalars : nullptr)) return rc;
  if (ctx->devs.size() == 1 && ctx->devs[0].w_step != 1) return set_err(ctx, TE_MSM_EINVAL, "indexed MSMs are whole MSMs: reset the window shard first");
  if (m > 0 && (!idx || !scalars)) return set_err(ctx, TE_MSM_EINVAL, "null index or scalar buffer");
  if (m > 0 && bases->n == 0) { ctx->bad_index_position = 0; return set_err(ctx, TE_MSM_EINVAL, "the bound point set is empty: no index is below its count"); }
  return 0;
}
const char* const kIndexedResident = "indexed MSM: indices and scalars must be resident on one device of the context";

// The end of a lone indexed call on one work set: result awaited, bad index / final carry reported, rows folded.
int settle_indexed(te_ctx* ctx, gpu_t& d, workset_t& ws, uint8_t* out) {
  HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));
  if (int rc = settle_status(ctx, ws)) return rc;
  (void)collect_stage_ms(ctx, d, ws);
  fold_rows(ws.plan, ws.h_partials, out);
  return 0;
}

int run_indexed_common(te_ctx* ctx, te_bases* bases, const void* idx, const void* src, bool src_is_host, uint64_t m, uint8_t* out) {
  if (!ctx || !out) return TE_MSM_EINVAL;
  if (int rc = indexed_args(ctx, bases, idx, src, m, !src_is_host)) return rc;
  if (m == 0) { write_identity(ctx->opt_curve, out); return 0; }
  const bool multi = ctx->devs.size() > 1;
  if (src_is_host && multi) return run_host_sharded(ctx, nullptr, static_cast<const uint8_t*>(src), m, out, bases, static_cast<const uint32_t*>(idx));
  // device form: the whole MSM on the device that holds the pairs
  const int owner = src_is_host ? 0 : owner_of(ctx, kIndexedResident, {idx, src});
  if (owner < 0) return owner;
  gpu_t& d = ctx->devs[(size_t)owner];
  const int wsel = lone_set(ctx, d, multi ? 0 : ctx->opt_workset);
  if (wsel < 0) return wsel;
  workset_t& ws = d.ws[wsel];
  HIP_TRY(ctx, hipSetDevice(d.device));
  if (src_is_host) {
    host_slice_req r; r.recs = bases->recs[(size_t)owner]; r.rec_kind = bases->rec_kind; r.scalars = static_cast<const uint8_t*>(src); r.n = m;
    r.c = make_plan(ctx, d, plan_whole(m)).c; r.K = scalar_pieces(ctx, m);
    r.idx = static_cast<const uint32_t*>(idx); r.idx_count = bases->n;
    if (int rc = enqueue_host_pieces(ctx, d, ws, r)) return rc;
  } else {
    partial_req r; r.d_scalars = src; r.n = m; r.stream = ws.stream; r.whole = true; r.bases = bases; r.d_idx = static_cast<const uint32_t*>(idx);
    if (int rc = enqueue_partial(ctx, d, ws, r)) return rc;
    if (int rc = fetch_rows(ctx, ws, ws.stream)) return rc;
  }
  return settle_indexed(ctx, d, ws, out);
}

// ---- batched MSMs over prefixes of a bound point set (te_msm_run_scalars_batch[_device]) -------------------------------------------
// what one MSM adds to a ragged sequence whose largest length is n (ensure_buffers' sizes, per MSM; te_batch::make_plan's budget)
void batch_cost(const te_ctx* ctx, uint64_t n, te_batch::msm_cost& c) {
  const plan_t p = make_plan(ctx, ctx->devs[0], plan_whole(n));
  const curve_sizes sz = sizes_of(p.curve);
  c.windows = (uint64_t)p.W; c.stride = p.nst;
  const uint64_t cells = c.windows * c.stride, wb = c.windows * p.B, segs = wb + c.windows * (n / p.seg_len);
  c.segments = segs;
  // digits 2 + sorted 4 + level-1 index 4 (+ key 2) bytes a cell; buckets, two fold chains (1.5 x) and bucket tables; segment tables and
  // sums; the rows
  c.bytes = cells * (p.packed ? 10 : 12) + wb * (sz.acc * 5 / 2 + 28) + segs * (sz.acc + 20) + c.windows * sz.row;
}

int run_batch_common(te_ctx* ctx, te_bases* bases, int count, const uint64_t* lens, const void* src, bool src_is_host, uint8_t* out) {
  if (!ctx) return TE_MSM_EINVAL;
  drain_workers(ctx);
  if (int rc = check_bases(ctx, bases)) return rc;
  if (int rc = check_scalar_record(ctx, src_is_host ? nullptr : src)) return rc;
  // (the window shards of a multi-device context are the engine's own, for its lone calls: a batch runs whole MSMs on every device)
  if (ctx->devs.size() == 1 && ctx->devs[0].w_step != 1) return set_err(ctx, TE_MSM_EINVAL, "batched MSMs compute whole MSMs: reset the window shard first");
  if (count < 0) return set_err(ctx, TE_MSM_EINVAL, "count must be >= 0");
  if (count == 0) return 0;
  if (!lens || !out) return set_err(ctx, TE_MSM_EINVAL, "null lens or out");
  uint64_t total = 0;
  std::vector<uint64_t> off((size_t)count);
  for (int m = 0; m < count; m++) {
    if (lens[m] > bases->n) return set_err(ctx, TE_MSM_EINVAL, "an MSM of the batch is longer than the bound point set");
    off[(size_t)m] = total; total += lens[m];
  }
  if (total && !src) return set_err(ctx, TE_MSM_EINVAL, "null scalar buffer");
  const curve_sizes sz = sizes_of(ctx->opt_curve);
  const size_t sb = scalar_bytes_now(ctx);               // the packed buffer: off[m] in records of this size (the sequences' plans carry it: sc_bytes)
  const int owner = !src_is_host && total && ctx->devs.size() > 1
                        ? owner_of(ctx, "te_msm_run_scalars_batch_device: the scalars must be resident on a device of the context", {src}) : 0;
  if (owner < 0) return owner;
  const size_t holder = (size_t)owner;
  const size_t nd = src_is_host ? ctx->devs.size() : 1;
  te_batch::limits lim;
  lim.small_max = (uint64_t)ctx->opt_batch_small_max;
  const te_batch::plan P = te_batch::make_plan(lens, (uint32_t)count, (int)nd, lim, [ctx](uint64_t n) { te_batch::msm_cost c; batch_cost(ctx, n, c); return c; });
  ctx->stat_batch_sequences = (int64_t)P.seqs.size();
  // per device: its sequences with their launch plans
  std::vector<std::vector<batch_seq_run>> runs(nd);
  for (const te_batch::sequence& s : P.seqs) {
    batch_seq_run r; r.s = &s;
    const size_t di = src_is_host ? (size_t)s.device : holder;
    plan_req q = plan_whole(s.n_max); q.batch = (int)s.msms.size(); q.rec_kind = bases->rec_kind;
    r.p = make_plan(ctx, ctx->devs[di], q);
    runs[(size_t)s.device].push_back(r);
  }
  // the scalars on each device that runs sequences: device form -- in place; host form -- one device: the caller's packed buffer,
  // uploaded whole; several: each device's MSMs packed (input order) into a buffer of its own
  std::vector<dev_tmp> tmp(nd);
  std::vector<std::vector<uint64_t>> offs(nd);
  std::vector<const void*> dsc(nd, src);
  for (size_t i = 0; i < nd; i++) {
    if (runs[i].empty()) continue;
    if (!src_is_host) { offs[i] = off; continue; }
    gpu_t& d = ctx->devs[i];
    if (nd == 1) {
      offs[i] = off;
      if (int rc = tmp_alloc(ctx, d, tmp[i], total * sb)) return rc;
      HIP_TRY(ctx, hipMemcpy(tmp[i].p, src, total * sb, hipMemcpyHostToDevice));
    } else {
      offs[i].assign((size_t)count, 0);
      std::vector<uint32_t> mine;
      for (const batch_seq_run& r : runs[i]) mine.insert(mine.end(), r.s->msms.begin(), r.s->msms.end());
      std::sort(mine.begin(), mine.end());
      uint64_t here = 0;
      for (uint32_t m : mine) { offs[i][m] = here; here += lens[m]; }
      std::vector<uint8_t> pack((size_t)(here * sb));
      for (uint32_t m : mine) memcpy(&pack[(size_t)(offs[i][m] * sb)], static_cast<const uint8_t*>(src) + off[m] * sb, (size_t)(lens[m] * sb));
      if (int rc = tmp_alloc(ctx, d, tmp[i], pack.size())) return rc;
      HIP_TRY(ctx, hipMemcpy(tmp[i].p, pack.data(), pack.size(), hipMemcpyHostToDevice));
    }
    dsc[i] = tmp[i].p;
  }
  std::vector<char> carry(nd, 0);
  std::vector<int64_t> entries(nd, 0);
  auto on = [&](size_t i) -> int {
    if (runs[i].empty()) return 0;
    bool c = false;
    const int r = run_batch_on_device(ctx, src_is_host ? i : holder, bases, dsc[i], offs[i], lens, runs[i], &c, &entries[i]);
    carry[i] = c;
    return r;
  };
  if (int rc = te_sched::on_devices(*ctx, nd, on)) return rc;
  int64_t ent = 0; bool any_carry = false;
  for (size_t i = 0; i < nd; i++) { ent += entries[i]; any_carry = any_carry || carry[i]; }
  ctx->stat_entries = ent;
  if (any_carry) return set_err(ctx, TE_MSM_ESCALAR, kFinalCarry);
  // host tails: one fold per MSM with its sequence's plan, on up to 8 threads
  struct fold_job { const plan_t* p; const uint8_t* rows; uint32_t m; };
  std::vector<fold_job> jobs;
  for (size_t i = 0; i < nd; i++) {
    const gpu_t& d = ctx->devs[src_is_host ? i : holder];
    for (const batch_seq_run& r : runs[i]) {
      const size_t rb = (size_t)r.p.W * sizes_of(r.p.curve).row;
      for (size_t j = 0; j < r.s->msms.size(); j++) jobs.push_back({&r.p, d.h_batch_rows + r.rows_at + j * rb, r.s->msms[j]});
    }
  }
  std::vector<uint8_t> res((size_t)count * sz.result, 0);
  const size_t nthreads = std::min<size_t>(8, (jobs.size() + 7) / 8);
  auto fold_part = [&](size_t t) { for (size_t j = t; j < jobs.size(); j += nthreads) fold_rows(*jobs[j].p, jobs[j].rows, &res[(size_t)jobs[j].m * sz.result]); };
  if (nthreads <= 1) { if (!jobs.empty()) fold_part(0); }
  else {
    std::vector<std::thread> th;
    for (size_t t = 1; t < nthreads; t++) th.emplace_back(fold_part, t);
    fold_part(0);
    for (std::thread& t : th) t.join();
  }
  for (uint32_t m : P.empty) write_identity(ctx->opt_curve, &res[(size_t)m * sz.result]);
  memcpy(out, res.data(), res.size());
  return 0;
}
}  // namespace

// mont: option "points_montgomery" as te_msm_bind_points[_device] found it (te_msm_bind_points_x binds points it recovered itself: canonical)
int bind_common(te_ctx* ctx, const void* src, bool src_is_host, uint64_t n, te_bases** out, bool mont, point_layout lay) {
  if (!ctx || !out) return TE_MSM_EINVAL;
  *out = nullptr;
  if (int rc = check_n(ctx, n)) return rc;
  if (int rc = check_layout(ctx, lay, src, src_is_host)) return rc;
  if (n > 0 && !src) return set_err(ctx, TE_MSM_EINVAL, "null point buffer");
  drain_workers(ctx);
  const size_t nd = ctx->devs.size();
  int src_dev = -1;
  if (!src_is_host && n > 0) {
    const int owner = nd > 1 ? owner_of(ctx, "te_msm_bind_points_device: the points must be resident on a device of the context", {src}) : 0;
    if (owner < 0) return owner;
    src_dev = ctx->devs[(size_t)owner].device;
  }
  if (n > 0) {                                        // option "check_points": once, here (MSMs over the set never check again)
    size_t ci = 0;
    if (!src_is_host) while (ctx->devs[ci].device != src_dev) ci++;
    if (int rc = check_call(ctx, ci, src, src_is_host, n, mont, lay)) return rc;
  }
  te_bases* b = new te_bases();
  b->ctx = ctx; b->n = n; b->curve = ctx->opt_curve;
  b->rec_kind = (b->curve == TE_MSM_CURVE_BLS12_377_G1 && ctx->opt_bind_affine) ? 1 : 0;
  b->rec_bytes = rec_bytes_of(b->curve, b->rec_kind);
  if (ctx->opt_bind_fixed_base && b->curve == TE_MSM_CURVE_TE_BLS12 && n > 0) {
    b->fb_c = ctx->opt_bind_fixed_base; b->fb_W = fb_windows_for(b->fb_c);
    if (te_fb::bind_refused(b->fb_c, n)) { delete b; return set_err(ctx, TE_MSM_EINVAL, "bind_fixed_base: windows x points must stay below 2^31"); }
  }
  b->recs.assign(nd, nullptr);
  const int rc = n > 0 ? te_sched::on_devices(*ctx, nd, [=](size_t i) { return bind_on_device(ctx, b, i, src, src_is_host, src_dev, mont, lay); }) : 0;
  if (rc) { free_bases(ctx, b); delete b; return rc; }
  // a set bound from HOST memory announces tickets from host scalars: the lanes' first concurrent copies (15-30 ms once per process,
  // warm_upload_lanes) happen here, in the call that blocks anyway, not in the first te_msm_submit_scalars -- which the N-API addon
  // issues on the JavaScript thread (js/promise_protocol.hpp: enter)
  if (src_is_host && n > 0) warm_upload_lanes(ctx);
  ctx->bases.push_back(b);
  *out = b;
  return 0;
}

// The rows of a fixed-base MSM are on the host (ev_result passed).  A row of the pseudo-window buffers overflowed -- badly skewed
// scalars: all equal, a few distinct values -- : the MSM runs again with the ordinary windows over table 0 of the same set (the
// ordinary records), on the same work set; the caller then folds ws.plan's rows as usual.  0 = the rows in the pinned block are final.
int fixed_base_settle(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases) {
  if (!ws.plan.fb_rb || *ws.h_err || !ws.h_err[1]) return 0;
  ctx->stat_fb_fallbacks++;
  HIP_TRY(ctx, hipSetDevice(d.device));
  partial_req r; r.d_scalars = ws.fb_scalars; r.n = ws.fb_n; r.stream = ws.stream; r.whole = true; r.bases = bases;
  r.scalar_form = ws.plan.scalar_mont; r.scalar_bytes = ws.plan.sc_bytes; r.scalar_bits = 0;   // (a ticket: the form and size it was submitted with, whatever the options say at its collect)
  if (int rc = enqueue_partial(ctx, d, ws, r)) return rc;
  if (int rc = fetch_rows(ctx, ws, ws.stream)) return rc;
  HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));
  return 0;
}

}  // namespace te_eng

extern "C" {

int te_msm_bind_points(te_ctx* ctx, const uint8_t* points_xy_le, uint64_t n, te_bases** out) {
  device_guard restore_callers_device;
  return bind_common(ctx, points_xy_le, true, n, out, ctx && ctx->opt_points_montgomery, ctx ? layout_now(ctx) : point_layout{});
}

int te_msm_bind_points_device(te_ctx* ctx, const void* d_points_xy_le, uint64_t n, te_bases** out) {
  device_guard restore_callers_device;
  return bind_common(ctx, d_points_xy_le, false, n, out, ctx && ctx->opt_points_montgomery, ctx ? layout_now(ctx) : point_layout{});
}

uint64_t te_msm_bases_count(const te_bases* bases) { return bases ? bases->n : 0; }

int te_msm_release_points(te_ctx* ctx, te_bases* bases) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  if (!valid_bases(ctx, bases)) return set_err(ctx, TE_MSM_EINVAL, kBadBases);
  if (bases->in_flight > 0) return set_err(ctx, TE_MSM_ESTATE, "te_msm_release_points: a ticket over this point set is in flight: collect it first");
  drain_workers(ctx);
  for (gpu_t& d : ctx->devs) {            // lone calls are over when they return; the streams may still clear their zeroed blocks -- nothing reads the records
    (void)hipSetDevice(d.device);
    for (workset_t& ws : d.ws) if (ws.used && ws.ev_done) (void)hipEventSynchronize(ws.ev_done);
  }
  free_bases(ctx, bases);
  ctx->bases.erase(std::find(ctx->bases.begin(), ctx->bases.end(), bases));
  delete bases;
  return 0;
}

int te_msm_run_scalars(te_ctx* ctx, te_bases* bases, const uint8_t* scalars_le, uint8_t out_xy_le[64]) {
  device_guard restore_callers_device;
  return run_scalars_common(ctx, bases, scalars_le, true, out_xy_le);
}

int te_msm_run_scalars_device(te_ctx* ctx, te_bases* bases, const void* d_scalars_le, uint8_t out_xy_le[64]) {
  device_guard restore_callers_device;
  return run_scalars_common(ctx, bases, d_scalars_le, false, out_xy_le);
}

int te_msm_submit_scalars(te_ctx* ctx, te_bases* bases, const uint8_t* scalars_le, uint64_t* ticket) {
  device_guard restore_callers_device;
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (int rc = check_bases(ctx, bases)) return rc;
  if (int rc = check_scalar_record(ctx)) return rc;
  const uint64_t n = bases->n;
  if (!scalars_le || n == 0) return set_err(ctx, TE_MSM_EINVAL, "bad arguments (an empty point set has no tickets: te_msm_run_scalars returns the identity)");
  if (ctx->devs.size() == 1 && ctx->devs[0].w_step != 1) return set_err(ctx, TE_MSM_ESTATE, "te_msm_submit_scalars computes whole MSMs: reset the window shard first");
  std::optional<ticket_set> taken;
  if (int rc = take_free_workset(ctx, -1, false, taken)) return rc;
  const ticket_set& t = *taken;
  const plan_t pf = make_plan(ctx, t.d, plan_whole(n));
  // pieces shorten ONE MSM's way through the device (its upload hides under its own first pieces); with other tickets in flight on
  // the device the upload hides under THEIR device work, and one piece keeps the sort and the accumulation at full width
  host_slice_req r; r.recs = bases->recs[(size_t)t.di]; r.rec_kind = bases->rec_kind; r.scalars = scalars_le; r.n = n;
  r.c = pf.c; r.K = (ctx->opt_scalar_chunks || t.d.in_flight == 0) ? scalar_pieces(ctx, n) : 1;
  r.wait_for_pinned = false; r.scalar_form = pf.scalar_mont; r.scalar_bytes = pf.sc_bytes; r.scalar_bits = pf.sc_bits;
  te_sched::job_ref job = post_to_lane(ctx, t, [ctx, t, bases, r]() -> int {
    return bases->fb_c && !r.scalar_bits ? enqueue_fixed_base_host(ctx, t.d, t.ws, bases, r.scalars, r.n, false, r.scalar_form) : enqueue_host_pieces(ctx, t.d, t.ws, r);
  });
  hand_out_ticket(ctx, t, ticket, bases, std::move(job));
  return 0;
}

int te_msm_submit_scalars_device(te_ctx* ctx, te_bases* bases, const void* d_scalars_le, uint64_t* ticket) {
  device_guard restore_callers_device;
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (int rc = check_bases(ctx, bases)) return rc;
  if (int rc = check_scalar_record(ctx, d_scalars_le)) return rc;
  const uint64_t n = bases->n;
  if (!d_scalars_le || n == 0) return set_err(ctx, TE_MSM_EINVAL, "bad arguments (an empty point set has no tickets: te_msm_run_scalars_device returns the identity)");
  const bool multi = ctx->devs.size() > 1;
  const int owner = multi ? owner_of(ctx, "te_msm_submit_scalars_device: the scalars must be resident on a device of the context", {d_scalars_le}) : 0;
  if (owner < 0) return owner;
  std::optional<ticket_set> taken;
  if (int rc = take_free_workset(ctx, owner, true, taken)) return rc;
  const ticket_set& t = *taken;
  device_inputs in; in.scalars = d_scalars_le;
  if (int rc = pull_for_ticket(ctx, t, owner, n, scalar_bytes_now(ctx), in)) return rc;
  if (bases->fb_c && !scalar_bits_now(ctx) && (multi || t.d.w_step == 1)) { if (int rc = enqueue_fixed_base(ctx, t.d, t.ws, bases, in.scalars, n, 0, t.ws.stream)) return rc; }
  else {
    partial_req r; r.d_scalars = in.scalars; r.n = n; r.stream = t.ws.stream; r.whole = multi; r.bases = bases;
    if (int rc = enqueue_partial(ctx, t.d, t.ws, r)) return rc;
  }
  if (int rc = fetch_rows(ctx, t.ws, t.ws.stream)) return rc;
  hand_out_ticket(ctx, t, ticket, bases);
  return 0;
}

int te_msm_run_scalars_indexed(te_ctx* ctx, te_bases* bases, const uint32_t* idx, const uint8_t* scalars_le, uint64_t m, uint8_t* out_xy_le) {
  device_guard restore_callers_device;
  return run_indexed_common(ctx, bases, idx, scalars_le, true, m, out_xy_le);
}

int te_msm_run_scalars_indexed_device(te_ctx* ctx, te_bases* bases, const void* d_idx, const void* d_scalars_le, uint64_t m, uint8_t* out_xy_le) {
  device_guard restore_callers_device;
  return run_indexed_common(ctx, bases, d_idx, d_scalars_le, false, m, out_xy_le);
}

int te_msm_submit_scalars_indexed(te_ctx* ctx, te_bases* bases, const uint32_t* idx, const uint8_t* scalars_le, uint64_t m, uint64_t* ticket) {
  device_guard restore_callers_device;
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (int rc = indexed_args(ctx, bases, idx, scalars_le, m)) return rc;
  if (m == 0) return set_err(ctx, TE_MSM_EINVAL, "bad arguments (an empty index list has no tickets: te_msm_run_scalars_indexed returns the identity)");
  std::optional<ticket_set> taken;
  if (int rc = take_free_workset(ctx, -1, false, taken)) return rc;
  const ticket_set& t = *taken;
  const plan_t pf = make_plan(ctx, t.d, plan_whole(m));
  host_slice_req r; r.recs = bases->recs[(size_t)t.di]; r.rec_kind = bases->rec_kind; r.scalars = scalars_le; r.n = m;
  // (pieces: the rule of te_msm_submit_scalars -- with other tickets in flight the upload hides under their device work)
  r.c = pf.c; r.K = (ctx->opt_scalar_chunks || t.d.in_flight == 0) ? scalar_pieces(ctx, m) : 1;
  r.idx = idx; r.idx_count = bases->n;
  r.wait_for_pinned = false; r.scalar_form = pf.scalar_mont; r.scalar_bytes = pf.sc_bytes; r.scalar_bits = pf.sc_bits;
  te_sched::job_ref job = post_to_lane(ctx, t, [ctx, t, r]() -> int { return enqueue_host_pieces(ctx, t.d, t.ws, r); });
  hand_out_ticket(ctx, t, ticket, bases, std::move(job));
  return 0;
}

int te_msm_submit_scalars_indexed_device(te_ctx* ctx, te_bases* bases, const void* d_idx, const void* d_scalars_le, uint64_t m, uint64_t* ticket) {
  device_guard restore_callers_device;
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (int rc = indexed_args(ctx, bases, d_idx, d_scalars_le, m, true)) return rc;
  if (m == 0) return set_err(ctx, TE_MSM_EINVAL, "bad arguments (an empty index list has no tickets: te_msm_run_scalars_indexed_device returns the identity)");
  const int owner = owner_of(ctx, kIndexedResident, {d_idx, d_scalars_le});
  if (owner < 0) return owner;
  std::optional<ticket_set> taken;
  if (int rc = take_free_workset(ctx, owner, true, taken)) return rc;
  const ticket_set& t = *taken;
  device_inputs in; in.scalars = d_scalars_le; in.idx = static_cast<const uint32_t*>(d_idx);
  if (int rc = pull_for_ticket(ctx, t, owner, m, scalar_bytes_now(ctx), in)) return rc;
  partial_req r; r.d_scalars = in.scalars; r.n = m; r.stream = t.ws.stream; r.whole = true; r.bases = bases; r.d_idx = in.idx;
  if (int rc = enqueue_partial(ctx, t.d, t.ws, r)) return rc;
  if (int rc = fetch_rows(ctx, t.ws, t.ws.stream)) return rc;
  hand_out_ticket(ctx, t, ticket, bases);
  return 0;
}

int te_msm_run_scalars_batch(te_ctx* ctx, te_bases* bases, int count, const uint64_t* lens, const uint8_t* scalars_le, uint8_t* out) {
  device_guard restore_callers_device;
  return run_batch_common(ctx, bases, count, lens, scalars_le, true, out);
}

int te_msm_run_scalars_batch_device(te_ctx* ctx, te_bases* bases, int count, const uint64_t* lens, const void* d_scalars_le, uint8_t* out) {
  device_guard restore_callers_device;
  return run_batch_common(ctx, bases, count, lens, d_scalars_le, false, out);
}

int64_t te_msm_bases_read(te_ctx* ctx, const te_bases* bases, int device_index, uint64_t first, uint64_t count, void* dst, uint64_t cap, int* record_bytes) {
  device_guard restore_callers_device;
  if (!ctx || !dst) return TE_MSM_EINVAL;
  if (!valid_bases(ctx, bases)) return set_err(ctx, TE_MSM_EINVAL, kBadBases);
  const uint64_t total = bases->n * (uint64_t)(bases->fb_c ? bases->fb_W : 1);      // (a fixed-base set: table w at records [w n, (w + 1) n))
  if (device_index < 0 || (size_t)device_index >= ctx->devs.size() || first > total || count > total - first) return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
  if (record_bytes) *record_bytes = (int)bases->rec_bytes;
  uint64_t bytes = count * bases->rec_bytes;
  if (bytes > cap) bytes = cap;
  if (!bytes) return 0;
  HIP_TRY(ctx, hipSetDevice(ctx->devs[(size_t)device_index].device));
  HIP_TRY(ctx, hipMemcpy(dst, bases->recs[(size_t)device_index] + first * bases->rec_bytes, bytes, hipMemcpyDeviceToHost));
  return (int64_t)bytes;
}

}  // extern "C"
