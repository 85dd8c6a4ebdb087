// tickets.hip -- MSMs in flight: te_msm_submit*, te_msm_ticket_wait, te_msm_collect (the bookkeeping itself is host_sched.hpp's).
#include "engine.hpp"

using namespace te_eng;

namespace te_eng {

namespace {
// Tickets.  A ticket is a whole MSM in flight on ONE work set of ONE device of the context; its number is context-wide.
//   single-device context   the MSMs overlap on the device (own stream and buffers per work set)
//   D devices               a ticket goes to the device with the fewest in flight (ties: the device that holds the inputs, then
//                           round-robin): one whole MSM per device -- D PCIe links for host buffers, no replicated bucket
//                           reduction, no row merge -- the throughput form for a prover with several MSMs to do
//                           (ui/Benchmark.tsx:32 awaits an async call; nothing stops a caller from having several in flight;
//                           multi-device is the reference README's future work, README.md:551).  te_msm_run* stay the forms
//                           for the lone call (point slices / window shards over all devices).

// the device the next ticket goes to (index into ctx->devs); prefer: the device that holds the inputs, or -1
// (the bookkeeping itself is host_sched.hpp's: the same code runs under ThreadSanitizer in tests/csrc/sched_harness.cpp)
int pick_device(te_ctx* ctx, int prefer) { return te_sched::pick_device_of(*ctx, TE_MSM_WORKSETS, prefer); }
const char* const kAllInFlight = "every work set has an MSM in flight: collect one first";

// option "check_points" (level) on the points of a ticket, on device ci: 0 = go on; TE_MSM_EPOINT = the ticket's outcome, kept in the
// set for te_msm_collect (nothing is enqueued for the ticket); else a device error
int check_ticket(te_ctx* ctx, workset_t& ws, size_t ci, const void* src, bool src_is_host, uint64_t n, int curve, int level) {
  if (!level) return 0;
  ws.pt_rc = check_points_on(ctx, ci, src, src_is_host, n, curve, level, &ws.pt_index, &ws.pt_reason);
  const int rc = ws.pt_rc;
  if (rc != TE_MSM_EPOINT) ws.pt_rc = 0;
  return rc;
}

// check_ticket on the thread that submits, and what its answer means for the call: false = the points passed, go on; true = the call
// is over with *rc -- 0 with the ticket handed out (TE_MSM_EPOINT is the ticket's outcome: te_msm_collect reports it), or a device error
bool ticket_ends_at_check(te_ctx* ctx, const ticket_set& t, size_t ci, const void* src, bool src_is_host, uint64_t n, uint64_t* ticket, int* rc) {
  *rc = check_ticket(ctx, t.ws, ci, src, src_is_host, n, ctx->opt_curve, ctx->opt_check_points);
  if (*rc != TE_MSM_EPOINT) return *rc != 0;
  hand_out_ticket(ctx, t, ticket);
  *rc = 0;
  return true;
}
workset_t* workset_of_ticket(te_ctx* ctx, uint64_t ticket, gpu_t** dev = nullptr) {
  int di = -1;
  workset_t* ws = te_sched::find_ticket(*ctx, ticket, &di);
  if (ws && dev) *dev = &ctx->devs[(size_t)di];
  return ws;
}
// index into ctx->devs of the device whose memory holds p (device-resident inputs of a ticket), -1 if none of the context's
int device_index_of_pointer(te_ctx* ctx, const void* p) {
  hipPointerAttribute_t at; memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return -1; }
  if (at.type != hipMemoryTypeDevice) return -1;
  for (size_t i = 0; i < ctx->devs.size(); i++) if (ctx->devs[i].device == at.device) return (int)i;
  return -1;
}

const char* const kNoTicket = "no such ticket in flight (already collected, or never handed out)";

int submit_host(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, uint64_t* ticket, bool async) {
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (!points_xy_le || !scalars_le || n == 0 || n >= (1ull << 31)) return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
  if (int rc = check_scalar_record(ctx)) return rc;
  if (ctx->devs.size() == 1 && ctx->devs[0].w_step != 1) return set_err(ctx, TE_MSM_ESTATE, "te_msm_submit computes whole MSMs: reset the window shard first");
  std::optional<ticket_set> taken;
  if (int rc = take_free_workset(ctx, -1, false, taken)) return rc;
  const ticket_set& t = *taken;
  const plan_t pf = make_plan(ctx, t.d, plan_whole(n));
  host_slice_req r; r.points = points_xy_le; r.scalars = scalars_le; r.n = n;
  r.c = pf.c; r.K = host_pieces(ctx, n);                     // the plan's window bits and pieces are fixed here
  if (!async) {
    if (int rc; ticket_ends_at_check(ctx, t, (size_t)t.di, points_xy_le, true, n, ticket, &rc)) return rc;
    if (int rc = enqueue_host_pieces(ctx, t.d, t.ws, r)) return rc;
    hand_out_ticket(ctx, t, ticket);
    return 0;
  }
  const int level = ctx->opt_check_points, curve = ctx->opt_curve;
  r.wait_for_pinned = false; r.scalar_form = pf.scalar_mont; r.scalar_bytes = pf.sc_bytes; r.scalar_bits = pf.sc_bits;
  te_sched::job_ref job = post_to_lane(ctx, t, [ctx, t, r, level, curve]() -> int {
    // on the lane: te_msm_collect finds TE_MSM_EPOINT as the job's status
    if (const int rc = check_ticket(ctx, t.ws, (size_t)t.di, r.points, true, r.n, curve, level)) return rc;
    return enqueue_host_pieces(ctx, t.d, t.ws, r);
  });
  hand_out_ticket(ctx, t, ticket, nullptr, std::move(job));
  return 0;
}
// the enqueue of an asynchronous ticket has run (any thread); its status
int await_job(workset_t& ws) { return te_sched::await_job(ws); }
void retire_ticket(te_ctx* ctx, gpu_t& d, workset_t& ws) {
  if (ws.bound) { ws.bound->in_flight--; ws.bound = nullptr; }       // the ticket gathered from a bound point set: it may be released now
  release_shared_recs(d, ws);                                        // the ticket's MSM is over: its record slab may serve another point buffer
  te_sched::retire(*ctx, (int)(&d - ctx->devs.data()), ws);
}
}  // namespace

// The work set of a new ticket: on the device pick_device chooses (made current), the lowest-numbered free work set (each has its
// own stream: the MSMs overlap on the device).  Not ticket % sets: with fewer MSMs in flight than sets only as many sets as needed are
// ever touched -- no buffer allocation in the middle of a run, and a smaller footprint in the Infinity Cache.
// probe: the lazy hardware-queue measurement (16 ms, once per device) -- device-resident tickets only: a host-buffer ticket is bound
// by its upload, not by how the work sets' streams share the hardware queues
int take_free_workset(te_ctx* ctx, int prefer, bool probe, std::optional<ticket_set>& t) {
  const int di = pick_device(ctx, prefer);
  if (di < 0) return set_err(ctx, TE_MSM_ESTATE, kAllInFlight);
  gpu_t& d = ctx->devs[(size_t)di];
  HIP_TRY(ctx, hipSetDevice(d.device));
  if (d.in_flight >= TE_MSM_WORKSETS) return set_err(ctx, TE_MSM_ESTATE, kAllInFlight);
  if (probe && !d.queues_probed && ctx->opt_queue_probe && d.in_flight == 0) spread_streams_over_queues(d);      // once per device, with nothing of it in flight
  // the work sets' streams can still be re-dealt by a later te_msm_submit_device as long as the measurement is on and has not run
  d.streams_final = d.queues_probed || !ctx->opt_queue_probe;
  const int wi = free_workset_index(d);
  if (wi < 0) return set_err(ctx, TE_MSM_ESTATE, kAllInFlight);
  t.emplace(ticket_set{di, d, d.ws[wi]});
  return 0;
}

// the status of a ticket's job on an upload lane; the error text of a failure is kept in the set for te_msm_collect (TE_MSM_EPOINT
// is reported from the set's pt_index / pt_reason)
int lane_status(te_ctx* ctx, workset_t& ws, int rc) {
  if (rc && rc != TE_MSM_EPOINT) { std::lock_guard<std::mutex> lk(ctx->err_mu); ws.job_err = ctx->err; }
  return rc;
}
// bound: the point set the ticket gathers from (te_msm_submit_scalars*) -- it cannot be released before the collect (retire_ticket)
void hand_out_ticket(te_ctx* ctx, const ticket_set& t, uint64_t* ticket, te_bases* bound, te_sched::job_ref job) {
  if (bound) { t.ws.bound = bound; bound->in_flight++; }
  te_sched::hand_out(*ctx, t.di, t.ws, ticket, std::move(job));      // te_msm_ticket_wait looks the ticket up from other threads
}

// index into ctx->devs of the device whose memory holds every one of ptrs; else TE_MSM_EINVAL with the caller's message
int owner_of(te_ctx* ctx, const char* msg, std::initializer_list<const void*> ptrs) {
  int owner = -1;
  for (const void* p : ptrs) {
    const int o = device_index_of_pointer(ctx, p);
    if (o < 0 || (owner >= 0 && o != owner)) return set_err(ctx, TE_MSM_EINVAL, msg);
    owner = o;
  }
  return owner;
}
// The device-resident inputs of a ticket (on device `owner` of the context), where its launch sequence reads them: in place, or -- the
// ticket went to another device -- pulled into its set's staging area and counted.  pulled: which of the two.
int pull_for_ticket(te_ctx* ctx, const ticket_set& t, int owner, uint64_t n, size_t scalar_bytes, device_inputs& in, bool* pulled) {
  const int src_dev = ctx->devs[(size_t)owner].device;
  const bool pull = must_pull(ctx, t.d, src_dev);
  if (pulled) *pulled = pull;
  if (!pull) return 0;
  peer_traffic moved;
  if (int rc = pull_inputs(ctx, t.d, t.ws, src_dev, n, scalar_bytes, in, moved)) return rc;
  note_peer_traffic(ctx, moved);
  return 0;
}

// The first times SEVERAL host threads copy to one device at the same moment, the ROCm runtime brings further copy (SDMA)
// engines online -- each time a pause of ~7 ms for every thread that is copying to that device (they are released together;
// profiles/r05_point_shard_rehearsal.txt, r05_point_shard_sdma_experiment.txt: ~5 such pauses for eight threads, one for four,
// once per process).  With upload lanes that would fall into the first few asynchronous tickets of a process; instead the lanes
// of every device of the context copy 2 MB each in lockstep, twice, before the first asynchronous ticket is taken (15-30 ms the
// first time in a process, ~1 ms for a later context).
void warm_upload_lanes(te_ctx* ctx) {
  static std::mutex mu; static uint64_t warmed = 0;           // per process and HIP device (ids < 64)
  const int L = ctx->opt_upload_threads;
  std::vector<size_t> todo;                                   // the context's devices whose lanes have not copied in lockstep yet: all of them at once
  {
    std::lock_guard<std::mutex> lk(mu);
    for (size_t di = 0; di < ctx->devs.size(); di++) {
      const int dev = ctx->devs[di].device;
      if (dev < 64 && ((warmed >> dev) & 1u)) continue;
      if (dev < 64) warmed |= 1ull << dev;
      todo.push_back(di);
    }
  }
  if (L < 2 || todo.empty()) return;
  struct gate_t { std::mutex m; std::condition_variable cv; int waiting = 0, round = 0, parties = 0; } gate;
  gate.parties = L * (int)todo.size();
  auto arrive = [&gate]() {
    std::unique_lock<std::mutex> lk(gate.m);
    const int r = gate.round;
    if (++gate.waiting == gate.parties) { gate.waiting = 0; gate.round++; gate.cv.notify_all(); }
    else gate.cv.wait(lk, [&] { return gate.round != r; });
  };
  constexpr size_t SZ = 2u << 20;
  std::vector<te_sched::job_ref> jobs;
  std::vector<te_sched::worker_t*> who;
  for (size_t di : todo) {
    const int dev = ctx->devs[di].device;
    for (int l = 0; l < L; l++) {
      te_sched::worker_t& w = te_sched::next_lane_of(*ctx, di, L);
      who.push_back(&w);
      jobs.push_back(w.post([dev, &arrive]() -> int {
        hipStream_t st = nullptr; void* dbuf = nullptr;
        std::vector<uint8_t> h(SZ, 1);
        const bool ok = hipSetDevice(dev) == hipSuccess && hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess && hipMalloc(&dbuf, SZ) == hipSuccess;
        for (int r = 0; r < 2; r++) {
          arrive();                                           // every lane reaches the gate, whatever happened to its allocations
          if (ok) { (void)hipMemcpyAsync(dbuf, h.data(), SZ, hipMemcpyHostToDevice, st); (void)hipStreamSynchronize(st); }
        }
        if (dbuf) (void)hipFree(dbuf);
        if (st) (void)hipStreamDestroy(st);
        (void)hipGetLastError();
        return 0;
      }));
    }
  }
  for (size_t i = 0; i < jobs.size(); i++) (void)who[i]->wait(jobs[i]);
}

}  // namespace te_eng

extern "C" {

int te_msm_submit_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n, uint64_t* ticket) {
  device_guard restore_callers_device;
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (!d_points_xy_le || !d_scalars_le || n == 0 || n >= (1ull << 31)) return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
  if (int rc = check_scalar_record(ctx, d_scalars_le)) return rc;
  const bool multi = ctx->devs.size() > 1;
  // several devices: the inputs may live on any of them; the ticket goes to the least loaded one and pulls them over xGMI
  const int owner = multi ? owner_of(ctx, "te_msm_submit_device: points and scalars must be resident on one device of the context", {d_points_xy_le, d_scalars_le}) : 0;
  if (owner < 0) return owner;
  std::optional<ticket_set> taken;
  if (int rc = take_free_workset(ctx, owner, true, taken)) return rc;
  const ticket_set& t = *taken;
  // checked where the inputs lie
  if (int rc; ticket_ends_at_check(ctx, t, (size_t)owner, d_points_xy_le, false, n, ticket, &rc)) return rc;
  // The peer copies (if any), the ~10 launches of the MSM and its read-back, on the calling thread.  (Handing them to a host thread, as
  // te_msm_submit_async does with uploads, was measured: no gain at n = 2^16 .. 2^18, 3-7 % slower at 2^19 / 2^20 -- the submitting
  // thread is not what bounds small MSMs in flight; profiles/r05_enqueue_async_experiment.txt.)
  HIP_TRY(ctx, hipSetDevice(t.d.device));
  device_inputs in; in.scalars = d_scalars_le; in.points = d_points_xy_le;
  bool pull = false;
  if (int rc = pull_for_ticket(ctx, t, owner, n, scalar_bytes_now(ctx), in, &pull)) return rc;
  // a single-device context keeps its window shard (te_msm_set_window_shard); on several devices a ticket is a whole MSM
  partial_req r; r.d_points = in.points; r.d_scalars = in.scalars; r.n = n; r.stream = t.ws.stream; r.whole = multi; r.share = pull ? SHARE_NONE : SHARE_RUN;
  if (int rc = enqueue_partial(ctx, t.d, t.ws, r)) return rc;
  if (int rc = fetch_rows(ctx, t.ws, t.ws.stream)) return rc;
  hand_out_ticket(ctx, t, ticket);
  return 0;
}

int te_msm_submit(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, uint64_t* ticket) {
  device_guard restore_callers_device;
  return submit_host(ctx, points_xy_le, scalars_le, n, ticket, false);
}

int te_msm_submit_async(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, uint64_t* ticket) {
  device_guard restore_callers_device;
  return submit_host(ctx, points_xy_le, scalars_le, n, ticket, true);
}

int te_msm_ticket_wait(te_ctx* ctx, uint64_t ticket) {
  device_guard restore_callers_device;
  if (!ctx) return TE_MSM_EINVAL;
  workset_t* ws = workset_of_ticket(ctx, ticket);
  if (!ws) return set_err(ctx, TE_MSM_ESTATE, kNoTicket);
  if (const int rc = await_job(*ws)) return rc;      // te_msm_collect reports it (and frees the ticket)
  HIP_TRY(ctx, hipEventSynchronize(ws->ev_result));
  return 0;
}

int te_msm_ticket_device(te_ctx* ctx, uint64_t ticket, int* device_index, int* device_id) {
  if (!ctx) return TE_MSM_EINVAL;
  gpu_t* d = nullptr;
  if (!workset_of_ticket(ctx, ticket, &d)) return set_err(ctx, TE_MSM_ESTATE, kNoTicket);
  if (device_index) *device_index = (int)(d - ctx->devs.data());
  if (device_id) *device_id = d->device;
  return 0;
}

int te_msm_collect(te_ctx* ctx, uint64_t ticket, uint8_t out_xy_le[64]) {
  device_guard restore_callers_device;
  if (!ctx || !out_xy_le) return TE_MSM_EINVAL;
  gpu_t* dp = nullptr;
  workset_t* wsp = workset_of_ticket(ctx, ticket, &dp);
  if (!wsp) return set_err(ctx, TE_MSM_ESTATE, kNoTicket);
  workset_t& ws = *wsp; gpu_t& d = *dp;
  if (const int jrc = !ws.slot.job && ws.pt_rc == TE_MSM_EPOINT ? TE_MSM_EPOINT : await_job(ws)) {
    if (jrc == TE_MSM_EPOINT) {       // its points failed the check in te_msm_submit[_device] or on the lane of te_msm_submit_async: nothing was enqueued
      const int64_t bad = ws.pt_index; const int reason = ws.pt_reason;
      ws.pt_rc = 0;
      retire_ticket(ctx, d, ws);
      return note_bad(ctx, kBadPoint, bad, reason);
    }
    // the upload / enqueue failed on the device's host thread: the ticket is over, the set must not keep half an MSM
    (void)hipSetDevice(d.device);
    (void)hipStreamSynchronize(ws.stream); if (ws.copy_stream) (void)hipStreamSynchronize(ws.copy_stream);
    ws.zero_clean_words = 0;
    retire_ticket(ctx, d, ws);
    return set_err(ctx, jrc, ws.job_err.empty() ? "the asynchronous submit failed" : ws.job_err.c_str());
  }
  HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));   // on failure the ticket stays collectable
  if (ws.bound) { if (int rc = fixed_base_settle(ctx, d, ws, ws.bound)) return rc; }      // (a fixed-base ticket whose rows overflowed: run again with the ordinary windows)
  (void)collect_stage_ms(ctx, d, ws);                // (a ticket reports its stage times whatever its status)
  const int rc = settle_status(ctx, ws);
  retire_ticket(ctx, d, ws);                         // the MSM is over, with a result, a bad index or a scalar-range error
  if (rc) return rc;
  fold_rows(ws.plan, ws.h_partials, out_xy_le);
  return 0;
}

}  // extern "C"
