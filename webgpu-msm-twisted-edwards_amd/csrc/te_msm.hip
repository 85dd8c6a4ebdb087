// te_msm.hip -- context, stage orchestration and the C-ABI of libtemsm.so (include/te_msm.h).
//
// Host-side counterpart of compute_msm's orchestration (submission/submission.ts:73-413) and of the
// WebGPU wrapper it drives (implementation/cuzk/gpu.ts:14-229).  Differences that matter:
//   * the context is persistent -- device buffers, streams and kernels survive across calls (the
//     reference re-creates device, buffers and pipelines on every call, submission.ts:96-97,360);
//   * every stage of one MSM is enqueued on one HIP stream with no host synchronisation in between, like the
//     reference's single command-encoder submit (gpu.ts:118); several MSMs are kept in flight on separate
//     work sets / streams so that they overlap on the device;
//   * windows can be sharded over contexts / devices; the reference is single-device.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <deque>
#include <algorithm>
#include <functional>
#include <chrono>
#include <thread>
#include <mutex>
#include <condition_variable>
#include <memory>
#include <optional>
#include <type_traits>
#if defined(__x86_64__)
#include <immintrin.h>
#endif

#include "../../include/te_msm.h"
#include "host_tail.hpp"
#include "synth.hpp"
#include "kernels.hip.hpp"
#include "check.hip.hpp"
#include "from_x.hip.hpp"
#include "scalar_mul.hip.hpp"
#include "probe.hip.hpp"
#include "host_tail377.hpp"
#include "host_sched.hpp"
#include "batch_plan.hpp"
#include "indexed_plan.hpp"
#include "plan_arith.hpp"
#include "fb_plan.hpp"

namespace {

thread_local std::string g_init_error;

// in execution order: everything that needs only the scalars first, so that a host-buffer call can upload the points
// (2/3 of the bytes) while those stages already run
enum { ST_DIGITS = 0, ST_SCATTER, ST_BSORT, ST_ORDER, ST_PREP, ST_ACCUM, ST_TREE, ST_WEIGHTED, ST_COUNT };
// the last two entries are not event intervals: k_accumulate's own first-wave-in .. last-wave-out device clock in ms, and the
// mean shader clock over that span in GHz (not a time: te_msm_stage_ms reports it under its own name)
const char* const kStageNames[ST_COUNT + 2] = {"digits", "part_scatter", "bucket_sort", "order", "prep_points",
                                               "accumulate", "marginal_sums", "weighted_sum", "accumulate_on_device", "accumulate_core_clock_ghz"};

// per-curve sizes: wire format, device accumulator, record slot, partial row (5 points), result
struct curve_sizes { size_t point_in, scalar_in, acc, rec, row, result; };
inline curve_sizes sizes_of(int curve) {
  return curve == TE_MSM_CURVE_BLS12_377_G1 ? curve_sizes{96, 48, sizeof(te::ete_t<14>), sizeof(te::rec_slot<14>), TE377_TAIL_ROW_BYTES, 96}
                                            : curve_sizes{TE_MSM_POINT_BYTES, TE_MSM_SCALAR_BYTES, sizeof(te::ete), sizeof(te::rec_slot<9>), TE_MSM_PARTIAL_BYTES, 64};
}
// bytes of one record: the curve's own (converted per call), or -- rec_kind 1 -- the affine BLS12-377 record of a bound point set
inline size_t rec_bytes_of(int curve, int rec_kind) { return (curve == TE_MSM_CURVE_BLS12_377_G1 && rec_kind == 1) ? sizeof(te::rec_aff377) : sizes_of(curve).rec; }
static_assert(TE377_TAIL_ROW_BYTES == TE_MSM_PARTIAL_BYTES_BLS12_377 && sizeof(te::ete_t<14>) * 5 == TE377_TAIL_ROW_BYTES, "row layout");
constexpr size_t TE_MAX_ROW_BYTES = TE377_TAIL_ROW_BYTES;

struct plan_t {
  int curve = 0;                      // TE_MSM_CURVE_*
  int c = 0, W = 0, nw = 0;           // window bits, total windows, windows of this launch sequence (shard windows x batch)
  int nw1 = 0, batch = 1;             // windows of this shard per MSM; MSMs that share the launch sequence (te_msm_partial_device_batch)
  int w_first = 0, w_step = 1;        // the windows this launch sequence computes: w_first + k * w_step (the device's shard, or 0 / 1 = all: whole MSMs)
  uint32_t B = 0, logB = 0;           // buckets per window = 2^(c-1) (signed digits) or 2^c (unsigned)
  int signed_digits = 1;
  uint32_t dw[4] = {0, 0, 0, 0};      // bits of the four digits of a bucket index (dw[0] lowest)
  uint32_t CH = 0, chunk_len = 0, nst = 0;   // level-1 chunks per window (chunk_len multiple of 4096); padded row stride
  uint32_t seg_len = 64;
  uint32_t S = 0, logS = 0, P = 0;   // level-1 partition: S buckets each, P = B/S partitions per window
  uint32_t packed = 0;               // level-1 entries as one 32-bit word (index | key << 23 | sign << 31): n <= 2^23
  int rec_kind = 0;                  // records k_accumulate gathers: 0 = the curve's own, 1 = affine BLS12-377 (bound point sets)
  int scalar_mont = 0;               // the scalar records hold k 2^256 mod (the curve's scalar field): option "scalars_montgomery" as it was when the call started
  // fixed-base windows (bound point sets with a per-window table, kernels.hip.hpp k_fb_digits): fb_rb > 0 -- the "windows" of this
  // plan are fb_rb + 1 pseudo-windows (rows) of 2^15 buckets over ONE bucket set; fb_c / fb_W: window bits and windows of the real decomposition
  int fb_rb = 0, fb_c = 0, fb_W = 0;
};

// A grow-only device allocation and its one owner: the pointer and its capacity in bytes.  make_room() (below) grows it, release() gives it back.
template <typename T> struct dev_buf {
  T* p = nullptr; size_t cap = 0;
  operator T*() const { return p; }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// Everything one MSM in flight needs on the device.  A GPU owns TE_MSM_WORKSETS work sets with their own streams so that
// several MSMs overlap ON THE DEVICE: the launch gaps and the latency-bound reduction tail of one are filled by the wide kernels of the
// other (te_msm_submit_device alternates them; "workset" option for te_msm_partial_device callers).
struct workset_t {
  hipStream_t stream = nullptr, copy_stream = nullptr;   // copy_stream: host-buffer uploads beside the compute stream (created on first use)
  int hw_queue_class = -1;            // which of the measured hardware-queue classes `stream` is on (-1: not probed)
  hipEvent_t ev_copy = nullptr, ev_start = nullptr;
  dev_buf<uint8_t> d_recs;            // record slots of the plan's curve (te::rec_slot<N>)
  dev_buf<uint16_t> d_digits, d_part_keys;
  dev_buf<uint32_t> d_part_start, d_part_count, d_part_idx, d_seg_part_base;
  dev_buf<uint32_t> d_bucket_start, d_bucket_cursor, d_sorted;
  dev_buf<uint32_t> d_seg_base, d_seg_bucket, d_seg_lenv, d_order;
  dev_buf<uint32_t> d_split_list, d_chunk_list;
  dev_buf<uint8_t> d_seg_out, d_buckets, d_red[4];   // accumulators of the plan's curve (te::ete_t<N>); d_red: ping/pong of the two fold chains
  // ONE zeroed block per MSM (a single memset), words: [0] bit 0 final-carry flag, bit 1 an index of an indexed MSM lies outside the bound
  // set; [1] fixed-base windows: a row overflowed / indexed MSMs: ~(lowest bad position of the call), see te::index_args; [2..3] non-zero window digits as ONE 64-bit count (= entries
  // accumulated; W * n passes 2^32 inside the allowed range n < 2^31: round-5 advisor; [0..3] survive the pieces of a host-buffer MSM),
  // [4] number of segments, [5..7] split / giant
  // bucket counters, [Z_ROWS..) the partial rows of the MSM (so that flag and rows come back in ONE device-to-host copy),
  // [Z_HIST..) segment-length histogram (TE_HIST_COPIES copies), [Z_CURSOR..) reservation cursors of the schedule, [Z_END..) the level-1 histogram
  // counts1[window][chunk][partition], then bucket_count[window][bucket].  d_err .. d_bucket_count point into d_zero.
  dev_buf<uint32_t> d_zero; size_t zero_words = 0;
  size_t zero_clean_words = 0;        // words of d_zero known to be zero on the set's stream: the block is cleared AFTER an MSM's read-back
                                      // (finish_sequence), so that the next MSM on the set starts with its first kernel, not a fill
  uint32_t *d_err = nullptr, *d_num_seg = nullptr, *d_size_hist = nullptr, *d_size_cursor = nullptr, *d_counts1 = nullptr, *d_bucket_count = nullptr;
  uint32_t* d_part_ticket = nullptr;  // [window][partition]: pieces of a multi-piece partition counted so far (k_l2_local), behind bucket_count in the zeroed block
  uint8_t* d_partials = nullptr;      // = d_zero + Z_ROWS: TE_MAX_WINDOWS rows
  uint32_t* h_err = nullptr;          // pinned: mirror of d_zero[0 .. Z_ROWS + rows)
  uint8_t* h_partials = nullptr;      // = h_err + Z_ROWS
  uint32_t* h_err_dev = nullptr;      // the device-visible address of h_err: k_reduce_tail writes flag words and rows there itself
  bool rows_on_host = false;          // the last launch sequence did so: fetch_rows has nothing to copy
  hipEvent_t ev_done = nullptr;       // the set is free again (everything of its last MSM, the clearing of the zeroed block included)
  hipEvent_t ev_result = nullptr;     // flag + rows of its last MSM are in host memory (recorded before the clearing: what a caller waits for)
  hipEvent_t ev[ST_COUNT + 1] = {};
  plan_t plan; uint64_t n = 0; bool used = false;
  te_sched::slot_t slot;              // ticket of an MSM submitted on this set and not collected yet (0 = none) + the host-thread job of an asynchronous submit
  std::string job_err;                // why that job failed (written by the device's host thread before the job is marked done)
  int prof_level = 0;                 // profile level the events of the last enqueue were recorded at
  hipStream_t last_stream = nullptr;  // stream of the previous MSM on this set: a different one must wait for it (scratch reuse)
  // host-buffer MSMs (te_msm_run, te_msm_submit): device copies of the caller's buffers, sized in bytes for the curve of the
  // call, and the "piece i has arrived" events of an upload in pieces
  dev_buf<uint8_t> d_in_points, d_in_scalars;
  std::vector<hipEvent_t> piece_events;
  // option "host_staging": the set's own pinned ring for host-buffer uploads (allocated on first use; te_msm_trim / destroy free it)
  uint8_t* h_ring = nullptr; std::vector<hipEvent_t> ring_ev; size_t ring_next = 0;
  uint64_t idle_calls = 0;            // te_msm_trim: context-level calls since the set was last used
  dev_buf<uint32_t> d_fb_remap;       // fixed-base windows: [rows][cap] table index | sign << 31 of every entry (beside d_digits' codes)
  uint32_t* d_fb_fill = nullptr;      // ... [rows] entries reserved per row, in the zeroed block
  const void* fb_scalars = nullptr; uint64_t fb_n = 0;   // ... the scalars (device memory) of the MSM in flight: a row overflow falls back to the ordinary windows
  int slab = -1;                      // shared record slab the MSM in flight on this set uses (-1: its own d_recs, or a bound point set)
  bool slab_run = false;              // ... and that MSM is a whole-MSM call of the slab's occupancy run (rec_slab_t::run_users)
  const uint8_t* recs_last = nullptr; // where the records of the set's last MSM are (te_msm_debug_read "records"): d_recs or a shared slab
  te_bases* bound = nullptr;          // the bound point set the set's ticket in flight gathers from (te_msm_submit_scalars*): released only after the collect
  // a ticket whose points failed the check (option "check_points"): nothing was enqueued for it, its te_msm_collect reports TE_MSM_EPOINT
  int pt_rc = 0; int64_t pt_index = -1; int pt_reason = 0;
  dev_buf<uint8_t> d_batch_rows;      // te_msm_run_scalars_batch: the rows of a ragged sequence (all its MSMs)
  dev_buf<uint32_t> d_in_idx;         // te_msm_run_scalars_indexed*: device copy of a call's index list (host form, peer copies of tickets)
  // EVERY dev_buf of the set, once: what te_msm_trim / destroy free is what "device_bytes" counts
  template <typename WS, typename F> static void each_buffer(WS& ws, F&& f) {
    f(ws.d_recs); f(ws.d_digits); f(ws.d_part_keys); f(ws.d_part_start); f(ws.d_part_count); f(ws.d_part_idx); f(ws.d_seg_part_base);
    f(ws.d_bucket_start); f(ws.d_bucket_cursor); f(ws.d_sorted); f(ws.d_seg_base); f(ws.d_seg_bucket); f(ws.d_seg_lenv); f(ws.d_order);
    f(ws.d_split_list); f(ws.d_chunk_list); f(ws.d_seg_out); f(ws.d_buckets); for (auto& b : ws.d_red) f(b);
    f(ws.d_zero); f(ws.d_in_points); f(ws.d_in_scalars); f(ws.d_fb_remap); f(ws.d_batch_rows); f(ws.d_in_idx);
  }
};
constexpr int TE_MAX_WINDOWS = 64;    // window_bits >= 4
// words [Z_CLOCK, Z_ROWS): k_accumulate's profiling words, 4 x TE_CLK_SLOTS 64-bit values (first wave in / last wave out on the
// wall clock, core and wall ticks summed over the waves), see the kernel
constexpr size_t Z_KEEP = 4;            // words [0, Z_KEEP) are kept from piece to piece of one host-buffer MSM (flag, pad, 64-bit entry count)
constexpr size_t Z_ENTRIES = 2;         // the 64-bit entry count (8-byte aligned)
constexpr size_t Z_CLOCK = 8;
static_assert(Z_KEEP + 4 <= Z_CLOCK && Z_ENTRIES % 2 == 0 && Z_ENTRIES + 2 <= Z_KEEP, "flag words");
constexpr size_t Z_ROWS = Z_CLOCK + 4 * 2 * TE_CLK_SLOTS, Z_HIST = Z_ROWS + (size_t)TE_MAX_WINDOWS * TE_MAX_ROW_BYTES / 4, Z_CURSOR = Z_HIST + 1024 * TE_HIST_COPIES, Z_END = Z_CURSOR + 1024;

struct gpu_t {
  int device = 0;
  int w_first = 0, w_step = 1;
  workset_t ws[TE_MSM_WORKSETS];
  int last_ws = 0;
  int wall_clock_khz = 0;                // rate of wall_clock64() on this device
  int in_flight = 0;                     // submitted and not collected
  bool queues_probed = false;            // the hardware-queue measurement has run (spread_streams_over_queues)
  // SHARED RECORD SLABS (round 6): whole-MSM calls from device-resident inputs that name the SAME point buffer while they are in
  // flight convert into, and gather from, ONE record slab instead of one per work set (acquire_shared_recs).
  // users: work sets whose latest MSM names the slab.  pending / ev[]: users that let go of it while their MSM could still be running (the
  // building blocks te_msm_partial_device[_batch], whose completion the engine does not see): an event recorded behind that MSM; whoever
  // takes the slab for ANOTHER point buffer waits for those events first (joining the same buffer needs no wait: the same bytes).
  // run_users: the whole-MSM calls among the users (uncollected tickets, running synchronous calls) -- the slab's OCCUPANCY RUN lasts
  // while there is one.  converted / conv_ev: a call of the current run has enqueued the conversion, and an event stands right behind
  // that launch; a later call of the run whose query finds the event complete converts nothing (see acquire_shared_recs).
  struct rec_slab_t { const void* src = nullptr; uint64_t n = 0; int curve = 0; uint8_t* d = nullptr; size_t cap = 0; int users = 0;
                      uint32_t pending = 0; hipEvent_t ev[TE_MSM_WORKSETS] = {};
                      int run_users = 0; bool converted = false; hipEvent_t conv_ev = nullptr; };
  std::vector<rec_slab_t> slabs;
  // asynchronous scalars-only tickets (bound bases) cross the link ONE AT A TIME per device: lanes that upload side by side share the
  // link, every ticket reaches the device late and the tickets move in a convoy (two in flight: 1.05-1.23 ms per MSM with 2-4 lanes,
  // 0.90-0.92 with one; tools/exp_bound_lanes_depth.py).  Host-buffer tickets (points + scalars) do not take it: their pageable copies
  // fill each other's pin / unpin gaps (1.79 vs 1.89 ms with one lane).
  std::unique_ptr<std::mutex> scalar_link{new std::mutex};
  // input-point validation (option "check_points", te_msm_check_points*): a stream, a piece buffer for host points and the report word
  // of its own, shared by every thread that checks on this device (upload lanes of asynchronous tickets included) under chk_mu
  std::unique_ptr<std::mutex> chk_mu{new std::mutex};
  hipStream_t chk_stream = nullptr; dev_buf<uint8_t> chk_pts;
  unsigned long long *chk_word = nullptr, *chk_host = nullptr;
  bool streams_exported = false;         // te_msm_workset_stream handed a handle out: te_msm_destroy parks the streams instead of destroying them
  bool streams_final = false;            // ... and the work sets' streams will not be re-dealt any more
  uint8_t* h_batch_rows = nullptr; size_t h_batch_cap = 0;   // te_msm_run_scalars_batch: pinned landing area of every sequence's rows (grown on use)
};

}  // namespace

struct te_ctx {
  std::vector<gpu_t> devs;
  std::string err;
  std::mutex err_mu;           // the per-device host threads of a multi-device te_msm_run report into the one string
  std::vector<std::unique_ptr<te_sched::worker_t>> workers;   // devs[i]'s host thread (host_sched.hpp); created by the first call that needs them
  std::vector<std::unique_ptr<te_sched::worker_t>> lanes;     // the upload lanes of asynchronous tickets: opt_upload_threads per device (host_sched.hpp)
  uint64_t next_lane = 0;
  int opt_upload_threads = 4;       // option "upload_threads" (env TE_MSM_UPLOAD_THREADS)
  uint64_t next_ticket = 1;         // tickets are handed out in order, over all devices; a ticket lives on the work set whose slot holds it
  int last_dev = -1;                // the device the previous ticket went to (te_sched::pick_device deals idle devices round-robin)
  int opt_host_staging = 0;         // host-buffer uploads through the work sets' own pinned rings (staged_copy) instead of straight from the caller's memory
  std::vector<std::unique_ptr<te_sched::worker_t>> stagers;   // the threads that fill those rings (created on first use)
  int opt_stage_device_inputs = 0;  // tickets for device-resident inputs: copy them to the chosen device even when it is the one that holds them (tests on a one-GPU box)
  int64_t stat_peer_bytes = 0;      // bytes those copies moved (get_option "peer_bytes")
  int64_t stat_fb_fallbacks = 0;    // fixed-base MSMs whose rows overflowed (skewed scalars) and were run again with the ordinary windows
  int64_t stat_entries = 0;         // non-zero window digits (= accumulated entries) of the MSM whose result was fetched last (get_option "entries_accumulated")
  int opt_host_shard_min = 4096;    // multi-device te_msm_run: points per device below which fewer devices are used
  int opt_queue_probe = 1;          // 1 = the first te_msm_submit* measures the hardware queues (lazily); 0 = never; te_msm_probe_queues does it now
  int opt_window_bits = 0;
  int opt_sort = 1;
  int opt_curve = TE_MSM_CURVE_TE_BLS12;   // which group the point buffers are in (option "curve")
  int opt_signed = 1;          // signed window digits (the reference's shipped behaviour); 0 = plain unsigned windows, 2^c buckets
  int opt_profile = 0;
  int opt_seg_len = 0;         // work segment: at most this many entries of one bucket per thread; 0 = from n (make_plan)
  int opt_host_chunks = 0;     // te_msm_run: pieces a large host buffer is uploaded and processed in (0 = choose from n)
  int opt_workset = 0;         // work set used by te_msm_run* / te_msm_partial_device
  int opt_fold_pairs = 1;      // first fold level of small MSMs with two lanes per output (k_sum_groups<N, true>)
  int opt_packed = 1;          // level-1 sort entries as one 32-bit word where n <= 2^23 (make_plan)
  int opt_prezero = 1;         // clear a work set's zeroed block behind an MSM's read-back instead of in front of the next MSM's first kernel
  int opt_check_points = 0;    // validate input points before an MSM / a bind: 0 off, 1 form, 2 form + subgroup (include/te_msm.h)
  int64_t bad_point_index = -1; int bad_point_reason = 0;   // the last TE_MSM_EPOINT (get_option "bad_point_index" / "bad_point_reason")
  int64_t bad_index_position = -1;  // te_msm_run_scalars_indexed*: lowest position of an index outside the bound set, of the last call that failed on one
  float stage_ms[ST_COUNT + 2] = {};
  bool have_stage_ms = false;
  int64_t stat_peer_copies = 0;  // hipMemcpyPeerAsync calls issued so far (multi-device contexts fed from device 0's memory; get_option "peer_copies")
  std::vector<te_bases*> bases;  // the bound point sets of the context (te_msm_bind_points), freed by te_msm_release_points / te_msm_destroy
  int opt_bind_affine = 1;       // te_msm_bind_points, BLS12-377: affine records (one inversion per point, once) instead of the projective ones of the per-call conversion
  int opt_scalar_chunks = 0;     // te_msm_run_scalars / te_msm_submit_scalars: pieces the scalars of a bound set are uploaded and processed in (0 = from n)
  int opt_bind_fixed_base = 0;   // te_msm_bind_points (Twisted-Edwards curve): window bits c of a per-window table 2^(c w) P_i (16..21; 0 = none): MSMs over
                                 // the set then run fixed-base windows -- one bucket set for all windows (W x the record memory)
  int opt_share_records = 1;     // shared record slabs for calls in flight that name the same device-resident point buffer, converted once per occupancy run;
                                 // 2 = shared slabs, every call converts (the round-6 form; A/B: option "share_records", env TE_MSM_SHARE_RECORDS)
  int64_t stat_record_conversions = 0;   // point -> record conversions the MSM launch sequences enqueued (get_option "record_conversions")
  int64_t opt_batch_small_max = 1ll << 15;   // te_msm_run_scalars_batch: MSMs up to this length share launch sequences (option "batch_small_max")
  int64_t stat_batch_sequences = 0;          // launch sequences the last batch call ran (get_option "batch_sequences")
  int opt_scalars_montgomery = 0;   // scalar records are Montgomery residues k 2^256 mod m, decoded in the digit kernels (csrc/scalar_form.hpp); read when a call
                                    // starts, on the calling thread -- a ticket keeps the form it was submitted with (plan_t::scalar_mont)
  int opt_points_montgomery = 0;    // te_msm_bind_points[_device]: coordinates are Montgomery residues x 2^256 mod p / x 2^384 mod q; read at bind time
};

// A bound point set (include/te_msm.h, "resident bases"): the records of n points on EVERY device of its context, converted
// once.  The reference hands the same point buffer to compute_msm for every run of a size (full_benchmarks.ts:63-68,100-105).
struct te_bases {
  te_ctx* ctx = nullptr;
  uint64_t n = 0;
  int curve = TE_MSM_CURVE_TE_BLS12, rec_kind = 0;
  size_t rec_bytes = 0;
  std::vector<uint8_t*> recs;    // recs[i]: n records in the memory of ctx->devs[i]
  int fb_c = 0, fb_W = 0;        // fixed-base windows: recs[i] holds fb_W tables of n records, table w = records of 2^(fb_c w) P_i (table 0 = the ordinary records)
  int in_flight = 0;             // tickets not collected that gather from it (the set cannot be released under them)
};

namespace {

#define HIP_TRY(ctx, expr)                                                                       \
  do {                                                                                           \
    hipError_t e_ = (expr);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      char buf_[512];                                                                            \
      snprintf(buf_, sizeof buf_, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      { std::lock_guard<std::mutex> lk_((ctx)->err_mu); (ctx)->err = buf_; }                     \
      return TE_MSM_EDEVICE;                                                                     \
    }                                                                                            \
  } while (0)

int set_err(te_ctx* ctx, int code, const char* msg) { std::lock_guard<std::mutex> lk(ctx->err_mu); ctx->err = msg; return code; }

// The engine selects devices with hipSetDevice, which is state of the CALLING thread: every entry point that may do so puts the
// caller's device back when it returns.  (A host that shares the thread with another HIP user -- PyTorch in bench.py's rank 0,
// which opens all N devices in its own process -- would otherwise find its "current device" moved to wherever the last ticket
// went: tensors on the wrong GPU, collectives on the wrong communicator.)
struct device_guard {
  int prev = -1;
  device_guard() { if (hipGetDevice(&prev) != hipSuccess) { (void)hipGetLastError(); prev = -1; } }
  ~device_guard() { if (prev >= 0) (void)hipSetDevice(prev); }
  device_guard(const device_guard&) = delete;
  device_guard& operator=(const device_guard&) = delete;
};

uint32_t ilog2(uint32_t v) { uint32_t l = 0; while ((1u << l) < v) l++; return l; }

int auto_window_bits(uint64_t n) {
  // measured on MI355X (profiles/r01_window_sweep.txt, r04_n_sweep.txt, r04_n_sweep_small.txt): 16 bits from 3 * 2^17 points up,
  // 15 bits from 2^16 (fewer buckets to reduce, and at that size the fixed stages weigh more than the additions; at n = 2^18
  // 15 bits: 0.295 ms per MSM pipelined / 0.479 ms latency, 16 bits: 0.328 / 0.503; at 2^19 16 bits win the latency by 2 %, 15 bits
  // the throughput by 3 %).  Below the harness sizes the bucket reduction is the whole cost: 13 bits for 2^14 .. 2^16 (2^15: 0.099
  // ms per MSM / 0.235 ms latency against 0.112 / 0.247 with 15 bits), 11 bits for 2^11 .. 2^14 (2^13: 0.080 / 0.200 against
  // 0.095 / 0.235 with 14), below that about log2(n) + 1 bits so that the W * 2^(c-1) buckets do not dwarf the n points.
  if (n >= (3ull << 17)) return 16;
  if (n >= (1ull << 16)) return 15;
  if (n >= (1ull << 14)) return 13;
  if (n >= (1ull << 11)) return 11;
  int lg = 0; while ((1ull << (lg + 1)) <= n) lg++;
  int c = lg + 1;
  if (c < 8) c = 8;
  if (c > 11) c = 11;
  return c;
}

// Windows of the decomposition.  Unsigned digits cover all 256 bits of a scalar record.  Signed digits: the scalars of this
// boundary are below p < 2^253 (harness generator reference/webgpu/utils.ts:118-124), so the windows only have to reach bit 254
// -- 255 bits: 17 windows of 15 bits where 256 bits take 18 (and 51 of 5 instead of 52; every other size of the allowed range
// c in [4, 16] gives the same count).  Which scalars above p are still ACCEPTED therefore depends on c -- and through the
// automatic window size on n: everything below 2^(cW) - sum_w 2^(cw + c - 1), i.e. about 2^255.9 for 16 x 16 bits (the reference's
// plan, miscellaneous/utils.ts:52-95) and 2^254 - 2^240 for 17 x 15 bits (n = 2^16 .. 2^18); canonical scalars (< p < 2^253) always
// fit.  INTEGRATION.md section 5 states the range; option "window_bits" = 16 gives a caller the reference's own acceptance at any n.
// The 18th window of a 15-bit plan held bits 255..269 and never received a digit or a carry: 16 384 empty buckets folded and a
// tail block run for nothing at n = 2^16 .. 2^18, where the reduction is ~40 % of the device span.  The error rule stays exact:
// k_digits flags any bit of s + sum_w 2^(cw + c - 1) at or above c * W, the reference's "final carry is 1"
// (miscellaneous/utils.ts:80-83) -- with c * W = 255 that is every scalar from 2^254 - 2^240 up (all of them >= 2 p).
int num_windows_for(int c, int signed_digits) { return ((signed_digits ? 255 : 256) + c - 1) / c; }

// What a plan is asked for.  Only n is always needed; plan_whole() / plan_shard() below start the two common requests.
struct plan_req {
  uint64_t n = 0;                // entries of the launch sequence: every size of the plan derives from it
  bool whole = false;            // every window (a whole MSM: host buffers, tickets of a multi-device context) instead of the device's window shard
  int force_c = 0;               // window bits; 0 = option "window_bits", else from n
  int batch = 1;                 // MSMs that share the launch sequence
  uint32_t force_seg = 0;        // segment length; 0 = option "segment_len", else from n (the pieces of one host-buffer MSM share the largest piece's)
  // the form of the scalar records (plan_t::scalar_mont) where the caller fixed it earlier -- the jobs of asynchronous tickets, which run on an
  // upload lane and do not read the option, and the second run of a fixed-base ticket; -1 = option "scalars_montgomery" as it is now
  int scalar_form = -1;
  int rec_kind = 0;              // records k_accumulate gathers (plan_t::rec_kind): a bound point set's form
  uint64_t idx_count = 0;        // an indexed call: records of the bound set -- the entry form follows the SET (indexed_plan.hpp); 0 = not indexed
};
inline plan_req plan_shard(uint64_t n) { plan_req q; q.n = n; return q; }
inline plan_req plan_whole(uint64_t n) { plan_req q; q.n = n; q.whole = true; return q; }

#ifndef TE_SCATTER_BLOCKS
#define TE_SCATTER_BLOCKS 1024u       // measured at n = 2^20: 512 blocks 81.8 us, 1024 80.3, 2048 98.4, 4096 264 (every block sums P x CH counts)
#endif
#ifndef TE_SCATTER_MINCHUNK
#define TE_SCATTER_MINCHUNK 4096u      // one tile (8192: k_part_scatter_prep 12.1 -> 10.7 us at n = 2^16, equal from 2^18 on)
#endif
plan_t make_plan(const te_ctx* ctx, const gpu_t& d, const plan_req& q) {
  plan_t p;
  const uint64_t n = q.n;
  p.curve = ctx->opt_curve;
  p.scalar_mont = q.scalar_form >= 0 ? q.scalar_form : ctx->opt_scalars_montgomery;
  p.rec_kind = q.rec_kind;
  p.c = q.force_c ? q.force_c : ctx->opt_window_bits ? ctx->opt_window_bits : auto_window_bits(n);
  p.signed_digits = ctx->opt_signed;
  p.W = num_windows_for(p.c, p.signed_digits);
  p.w_first = q.whole ? 0 : d.w_first; p.w_step = q.whole ? 1 : d.w_step;
  p.nw = 0;
  for (int w = p.w_first; w < p.W; w += p.w_step) p.nw++;
  p.nw1 = p.nw; p.batch = q.batch; p.nw *= q.batch;
  p.logB = (uint32_t)(p.signed_digits ? p.c - 1 : p.c); p.B = 1u << p.logB;
  for (int k = 0; k < 4; k++) p.dw[k] = (p.logB + 3u - (uint32_t)k) / 4u;       // 15 -> 4,4,4,3
  // level-1 chunks per window: ~4 blocks of 512 threads per CU in k_part_scatter, at least one tile of digits per chunk (plan_arith.hpp)
  const te_plan::chunking k = te_plan::chunks_for((uint32_t)p.nw, n, TE_SCATTER_BLOCKS, TE_SCATTER_MINCHUNK);
  p.nst = k.nst; p.chunk_len = k.chunk_len; p.CH = k.CH;
  // level-1 partition = S consecutive buckets of one window
  p.S = p.B < 256u ? p.B : 256u;
  if (q.force_seg) {
    p.seg_len = q.force_seg;
  } else if (ctx->opt_seg_len) {
    p.seg_len = (uint32_t)ctx->opt_seg_len;
  } else {
    // Twice the mean bucket size, as a power of two in [16, 64].  A thread works one segment off serially (~8-11 us per
    // addition with four waves per SIMD): at n = 2^20 (32 entries per bucket) 64 balances the longest chains against the
    // VALU-bound whole, at smaller n the whole shrinks and long segments set the kernel's duration -- measured latency of
    // one MSM (profiles/r03_segment_len_sweep.txt): 2^16 0.366 -> 0.346 ms, 2^17 0.466 -> 0.410, 2^18 0.582 -> 0.53-0.54
    // with 16 / 16 / 16-32 instead of 64; 2^19 equal at 32; 2^20 1.23 (64) against 1.32 (32).
    p.seg_len = te_plan::default_seg_len(n, p.B);
  }
  p.P = p.B / p.S; p.logS = ilog2(p.S);
  // 4 bytes per level-1 entry instead of 6 (-32 MB written and -32 MB read per 2^20-point MSM) where the index fits 23 bits -- the
  // index of an indexed call is a record of the SET; option "packed_sort" = 0 (env TE_MSM_PACKED=0): the general form (A/B
  // measurements, tests; what larger n uses)
  p.packed = te_indexed::plan_for(n, q.idx_count ? q.idx_count : n, ctx->opt_packed).packed;
  return p;
}

// room for need_elems elements: never shrinks, the contents do NOT survive a growth, a need of 0 still allocates (16 bytes)
template <typename T> int make_room(te_ctx* ctx, dev_buf<T>& b, size_t need_elems) {
  const size_t need = need_elems * sizeof(T);
  if (b.p && need <= b.cap) return 0;
  if (b.p) HIP_TRY(ctx, hipFree(b.p));
  b.p = nullptr; b.cap = 0;
  HIP_TRY(ctx, hipMalloc((void**)&b.p, need ? need : 16));
  b.cap = need;
  return 0;
}

// The element counts that both an allocation (ensure_buffers) and a kernel argument (msm_launch) depend on, stated once.
struct seq_sizes {
  size_t wb, smax;                     // buckets of the sequence; segment ids: segments <= buckets + entries / seg_len
  // entries of d_chunk_list (pairs): a giant bucket contributes one chunk per TE_GIANT_RUN parts: at most one per bucket plus one per
  // TE_GIANT_RUN segments (slack: what the allocation adds to smax)
  size_t chunk_cap(size_t slack = 0) const { return wb + (smax + slack) / TE_GIANT_RUN + 2; }
};
inline seq_sizes sizes_for(const plan_t& p, uint64_t n) {
  const size_t wb = (size_t)p.nw * p.B;
  return {wb, wb + (size_t)p.nw * (size_t)(n / (uint64_t)p.seg_len)};
}

// need_recs = false: the launch sequence gathers from a bound point set, the work set needs no record slab of its own
int ensure_buffers(te_ctx* ctx, gpu_t& d, workset_t& ws, uint64_t n, const plan_t& p, bool need_recs = true) {
  HIP_TRY(ctx, hipSetDevice(d.device));
  // + 64: k_accumulate fetches its sorted indices TE_IDX_STRIP at a time and may read that far past the end of a list
  const seq_sizes sz = sizes_for(p, n);
  const size_t nd = (size_t)p.nw * p.nst + 64, wb = sz.wb, ab = sizes_of(p.curve).acc;
  int rc = 0;
  if (need_recs && (rc = make_room(ctx, ws.d_recs, (size_t)n * sizes_of(p.curve).rec * (size_t)p.batch))) return rc;
  if ((rc = make_room(ctx, ws.d_digits, nd))) return rc;
  if ((rc = make_room(ctx, ws.d_sorted, nd))) return rc;
  {
    const size_t c1 = (size_t)p.nw * p.CH * p.P;
    ws.zero_words = Z_END + c1 + wb + (size_t)p.nw * p.P + 64;            // (+ 64: the row fill counters of fixed-base windows)
    { const uint32_t* before = ws.d_zero; if ((rc = make_room(ctx, ws.d_zero, ws.zero_words))) return rc; if (ws.d_zero != before) ws.zero_clean_words = 0; }
    ws.d_err = ws.d_zero; ws.d_num_seg = ws.d_zero + Z_KEEP; ws.d_size_hist = ws.d_zero + Z_HIST; ws.d_size_cursor = ws.d_zero + Z_CURSOR;
    ws.d_partials = reinterpret_cast<uint8_t*>(ws.d_zero + Z_ROWS);
    ws.d_counts1 = ws.d_zero + Z_END; ws.d_bucket_count = ws.d_counts1 + c1; ws.d_part_ticket = ws.d_bucket_count + wb;
    ws.d_fb_fill = ws.d_part_ticket + (size_t)p.nw * p.P;
  }
  if (p.fb_rb && (rc = make_room(ctx, ws.d_fb_remap, nd))) return rc;
  if ((rc = make_room(ctx, ws.d_bucket_start, wb))) return rc;
  if ((rc = make_room(ctx, ws.d_bucket_cursor, wb))) return rc;
  if ((rc = make_room(ctx, ws.d_seg_part_base, (size_t)p.nw * p.P))) return rc;
  const size_t smax = sz.smax + 16;
  if ((rc = make_room(ctx, ws.d_order, smax))) return rc;
  if ((rc = make_room(ctx, ws.d_seg_bucket, smax))) return rc;
  if ((rc = make_room(ctx, ws.d_seg_lenv, smax))) return rc;
  if ((rc = make_room(ctx, ws.d_seg_out, smax * ab))) return rc;
  if ((rc = make_room(ctx, ws.d_seg_base, wb + 1))) return rc;
  if ((rc = make_room(ctx, ws.d_split_list, wb + 1))) return rc;
  if ((rc = make_room(ctx, ws.d_chunk_list, 2 * sz.chunk_cap(16)))) return rc;
  if ((rc = make_room(ctx, ws.d_part_start, (size_t)p.nw * p.P))) return rc;
  if ((rc = make_room(ctx, ws.d_buckets, wb * ab))) return rc;
  if ((rc = make_room(ctx, ws.d_part_count, (size_t)p.nw * p.P + (size_t)p.nw))) return rc;      // + the overflow pieces of each window
  if ((rc = make_room(ctx, ws.d_part_keys, p.packed ? 8 : nd))) return rc;       // packed level-1 entries carry their key
  if ((rc = make_room(ctx, ws.d_part_idx, nd))) return rc;
  // fold levels (by 8, 4 or 2): the first output is at most B/2 per window, the second at most B/4
  for (int k = 0; k < 4; k++) if ((rc = make_room(ctx, ws.d_red[k], (wb / (k % 2 ? 4 : 2) + 1) * ab))) return rc;
  return 0;
}

// f(integral_constant<int, C>) for the window bits C = c of the range [LO, HI]; any other c is served by HI
template <int LO, int HI, typename F> void with_window_bits(int c, F&& f) {
  if constexpr (LO < HI) { if (c != LO) return with_window_bits<LO + 1, HI>(c, f); }
  f(std::integral_constant<int, LO>{});
}

// FORM: te::SCALAR_FORM_* (scalar_form_of below)
template <int C, int FORM> void launch_digits(const te::batch_ptrs& sc, int batch, uint16_t* dg, const te::digits_params& prm, uint32_t* err, uint32_t* counts1, hipStream_t s) {
  hipLaunchKernelGGL((te::k_digits<C, FORM>), dim3((prm.nst + TE_DIG_BLOCK - 1u) / TE_DIG_BLOCK, batch), dim3(TE_DIG_THREADS), 0, s, sc, dg, prm, err, counts1);
}
static_assert(TE_BATCH_MAX == TE_MSM_MAX_BATCH, "batch tables");
template <int C, int FORM> void launch_digits_ragged(const void* sc, const te::ragged_tab& tab, int batch, uint16_t* dg, const te::digits_params& prm, uint32_t* err, uint32_t* counts1, hipStream_t s) {
  hipLaunchKernelGGL((te::k_digits_ragged<C, FORM>), dim3((prm.nst + TE_DIG_BLOCK - 1u) / TE_DIG_BLOCK, batch), dim3(TE_DIG_THREADS), 0, s, static_cast<const uint4*>(sc), tab, dg, prm, err, counts1);
}
static_assert(TE_RAGGED_MAX == TE_BATCH_SEQ_MAX && TE_BATCH_SEQ_MAX == TE_MSM_BATCH_SEQ_MAX, "ragged tables");
// the instantiation of the digit kernels a plan runs: canonical records, or Montgomery residues modulo the scalar field of the plan's curve
inline int scalar_form_of(const plan_t& p) {
  return !p.scalar_mont ? te::SCALAR_FORM_CANONICAL : p.curve == TE_MSM_CURVE_BLS12_377_G1 ? te::SCALAR_FORM_377 : te::SCALAR_FORM_TE;
}
// f(integral_constant<int, FORM>) for a form of scalar_form_of
template <typename F> void with_scalar_form(int form, F&& f) {
  if (form == te::SCALAR_FORM_TE) f(std::integral_constant<int, te::SCALAR_FORM_TE>{});
  else if (form == te::SCALAR_FORM_377) f(std::integral_constant<int, te::SCALAR_FORM_377>{});
  else f(std::integral_constant<int, te::SCALAR_FORM_CANONICAL>{});
}

// One MSM's device work in three parts: the stages before the dominant kernel, k_accumulate (bracketed by timing events),
// and the stages after it.
struct msm_launch {
  te_ctx* ctx; workset_t& ws; plan_t p;
  const void* d_points = nullptr; const void* d_scalars = nullptr; uint64_t n = 0;   // batch > 1: d_points / d_scalars are arrays of p.batch device pointers (on the host)
  void* d_partials_out = nullptr;
  int prof = 0;                   // event marks inside front()/back() only at profile level 2
  hipStream_t stream = nullptr;
  // the work set, the plan and what the launch runs over; everything else is set by name
  msm_launch(te_ctx* ctx_, workset_t& ws_, const plan_t& p_, uint64_t n_, hipStream_t stream_) : ctx(ctx_), ws(ws_), p(p_), n(n_), stream(stream_) {}
  bool own_rows = false;          // rows go to ws.d_partials: the caller fetches flag + rows with one copy
  bool onto = false;              // a later piece of a host-buffer MSM: keep the final-carry flag, add onto the buckets
  bool host_rows = false;         // own rows go straight to the work set's pinned host block, written by k_reduce_tail (no copy at all)
  uint8_t* recs_rw = nullptr;     // a shared record slab: the conversion writes it and k_accumulate gathers from it (instead of ws.d_recs)
  uint8_t* recs_out() const { return recs_rw ? recs_rw : ws.d_recs; }
  bool have_recs = false;         // recs_rw holds this call's records already (converted earlier in the slab's occupancy run): no conversion
  void count_conversion() const { __atomic_fetch_add(&ctx->stat_record_conversions, (int64_t)1, __ATOMIC_RELAXED); }
  const uint32_t* fb_remap = nullptr;   // fixed-base windows: the digit rows were filled by k_fb_digits (no k_digits launch); the level-1 scatter maps positions through it
  const uint8_t* bound = nullptr; // records of a bound point set (te_msm_bind_points), already offset to this launch's first point: no conversion,
                                  // k_accumulate gathers from here instead of ws.d_recs (p.rec_kind tells which record form)
  const te::ragged_tab* ragged = nullptr;   // a ragged sequence (te_msm_run_scalars_batch): d_scalars is ONE packed buffer, MSM m's scalars at
                                  // ragged->off[m] with ragged->len[m] of them (k_digits_ragged); every window gathers from `bound` itself
  // an indexed subset (te_msm_run_scalars_indexed*): entry j gathers record idx[j] of `bound` (which then stays at the set's FIRST record:
  // no per-piece offset); idx: device memory, this launch's n entries.  idx_count: records of the set; idx_pos: position of entry 0 in the
  // caller's whole list (what a bad index is reported at).  p.packed follows the SET's count (indexed_plan.hpp)
  const uint32_t* idx = nullptr; uint32_t idx_count = 0, idx_pos = 0;
  // Own rows of a context that computes ALL windows can be written to host memory by the tail kernel (every row slot is
  // rewritten by every MSM).  Not with window shards (rows of foreign windows must read as zero: they come from the cleared
  // device block), not with "prezero" = 0 (stage verifiers read the device rows).
  bool rows_to_host() const { return own_rows && p.nw > 0 && p.batch == 1 && p.w_first == 0 && p.w_step == 1 && ctx->opt_prezero; }
  uint32_t n32() const { return (uint32_t)n; }
  uint32_t smax() const { return (uint32_t)sizes_for(p, n).smax; }
  uint32_t chunk_cap() const { return (uint32_t)sizes_for(p, n).chunk_cap(); }
  const void* points_of(int m) const { return p.batch > 1 ? static_cast<const void* const*>(d_points)[m] : d_points; }
  const void* scalars_of(int m) const { return p.batch > 1 ? static_cast<const void* const*>(d_scalars)[m] : d_scalars; }
  void mark(int i) const { if (prof >= 2 || (prof == 1 && (i == ST_ACCUM || i == ST_ACCUM + 1))) (void)hipEventRecord(ws.ev[i], stream); }

  // device-resident inputs, no per-stage timing: the record conversion rides in the launch of the sort's first level
  bool can_fuse_conversion() const { return prof < 2 && p.nw > 0; }
  int front() {
    if (have_recs) return front_scalars();
    if (can_fuse_conversion()) return front_scalars(true);
    if (int rc = front_scalars()) return rc;
    return front_points();
  }

  // the distinct point buffers of the sequence (grid rows of the conversion) and the record slab of each
  int prep_rows(te::batch_ptrs& tab, te::batch_slabs& row_slab) const {
    const te::batch_slabs sl = slabs();
    memset(&tab, 0, sizeof tab); memset(&row_slab, 0, sizeof row_slab);
    int rows = 0;
    for (int m = 0; m < p.batch; m++) if ((int)sl.s[m] == m) { tab.p[rows] = (const uint4*)points_of(m); row_slab.s[rows] = (uint32_t)m; rows++; }
    return rows;
  }

  // record slab of MSM m: MSMs of one call that name the same point buffer share one conversion (same pointer in one call =
  // same data; nothing is remembered across calls).  slab = index of the first MSM with that pointer.
  te::batch_slabs slabs() const {
    te::batch_slabs r; memset(&r, 0, sizeof r);
    for (int m = 0; m < p.batch; m++) {
      int first = m;
      for (int j = 0; j < m; j++) if (points_of(j) == points_of(m)) { first = j; break; }
      r.s[m] = (uint32_t)first;
    }
    return r;
  }

  // points -> records (needs only the points; runs last of the front part): one launch, one grid row per DISTINCT point buffer
  int front_points() {
    const uint32_t n32 = this->n32();
    mark(ST_PREP);
    if (have_recs) return 0;
    te::batch_ptrs tab; te::batch_slabs row_slab;
    const int rows = prep_rows(tab, row_slab);
    count_conversion();
    if (p.curve == TE_MSM_CURVE_BLS12_377_G1)
      hipLaunchKernelGGL(te::k_prep_points377, dim3((n32 + 255) / 256, rows), dim3(256), 0, stream, tab, row_slab, reinterpret_cast<te::rec_slot<14>*>(recs_out()), n32);
    else
      hipLaunchKernelGGL(te::k_prep_points, dim3((n32 + 255) / 256, rows), dim3(256), 0, stream, tab, row_slab, reinterpret_cast<te::pnt_slot*>(recs_out()), n32);
    return 0;
  }

  // scalars -> digits, two-level counting sort, segment schedule (needs only the scalars); with_prep: the points -> records
  // conversion shares the launch of the sort's first level (k_part_scatter_prep)
  int front_scalars(bool with_prep = false) {
    const uint32_t n32 = this->n32();
    // flags, counters, histograms, bucket counts (a later piece of the same MSM keeps the final-carry flag and the entry count)
    // -- unless the block is still clean from the clearing that followed the set's previous MSM (finish_sequence)
    if (onto || ws.zero_clean_words < ws.zero_words)
      HIP_TRY(ctx, hipMemsetAsync(ws.d_zero + (onto ? Z_KEEP : 0), 0, (ws.zero_words - (onto ? Z_KEEP : 0)) * sizeof(uint32_t), stream));
    ws.zero_clean_words = 0;
    if (!p.fb_rb) mark(ST_DIGITS);                         // (fixed-base windows: enqueue_fixed_base marked it in front of k_fb_digits)
    te::sort_geom sg;
    sg.n = n32; sg.nst = p.nst; sg.B = p.B; sg.logS = p.logS; sg.S = p.S; sg.P = p.P; sg.CH = p.CH; sg.chunk_len = p.chunk_len; sg.half = p.signed_digits ? p.B : 0u; sg.packed = p.packed;
    if (p.nw > 0 && !p.fb_rb) {
      te::digits_params prm; memset(&prm, 0, sizeof prm);
      if (p.signed_digits) for (int w = 0; w < p.W; w++) { const int bit = w * p.c + p.c - 1; if (bit < 320) prm.half[bit >> 5] |= 1u << (bit & 31); }
      prm.zero_digit = p.signed_digits ? 1u << (p.c - 1) : 0u;
      prm.sc_stride = (uint32_t)(sizes_of(p.curve).scalar_in / 16);
      prm.n = n32; prm.nst = p.nst; prm.num_windows = p.W; prm.w_first = p.w_first; prm.w_step = p.w_step; prm.nw_local = p.nw1;
      prm.half_code = sg.half; prm.logS = p.logS; prm.P = p.P; prm.CH = p.CH; prm.chunk_len = p.chunk_len;
      // one launch over the MSMs of the sequence: MSM m (blockIdx.y) fills digit rows and level-1 counts [m * nw1, (m + 1) * nw1)
      te::batch_ptrs sc; memset(&sc, 0, sizeof sc);
      if (!ragged) for (int m = 0; m < p.batch; m++) sc.p[m] = (const uint4*)scalars_of(m);
      uint16_t* dg = ws.d_digits;
      uint32_t* c1 = ws.d_counts1;
      with_scalar_form(scalar_form_of(p), [&](auto FORM) {
        if (ragged) with_window_bits<4, 16>(p.c, [&](auto C) { launch_digits_ragged<decltype(C)::value, decltype(FORM)::value>(d_scalars, *ragged, p.batch, dg, prm, ws.d_err, c1, stream); });
        else with_window_bits<4, 16>(p.c, [&](auto C) { launch_digits<decltype(C)::value, decltype(FORM)::value>(sc, p.batch, dg, prm, ws.d_err, c1, stream); });
      });
    }
    const uint32_t cap_w = p.B + (uint32_t)(n / p.seg_len);        // segment ids of one window (see k_part_scatter)
    mark(ST_SCATTER);
    if (p.nw > 0) {
      te::scatter_args sa;
      sa.digits = ws.d_digits; sa.counts1 = ws.d_counts1; sa.part_keys = ws.d_part_keys; sa.part_idx = ws.d_part_idx; sa.part_start = ws.d_part_start;
      sa.part_count = ws.d_part_count; sa.seg_part_base = ws.d_seg_part_base; sa.entries = reinterpret_cast<unsigned long long*>(ws.d_zero + Z_ENTRIES); sa.seg_len = p.seg_len; sa.cap_w = cap_w; sa.nw = (uint32_t)p.nw; sa.g = sg; sa.remap = fb_remap; sa.row_fill = ws.d_fb_fill;
      if (with_prep) {
        te::batch_ptrs tab; te::batch_slabs row_slab;
        const uint32_t rows = (uint32_t)prep_rows(tab, row_slab), sblocks = p.CH * (uint32_t)p.nw;
        count_conversion();
        if (bls()) {                                      // 512 points per conversion block, one per thread
          const uint32_t per_row = (n32 + 511u) / 512u;
          hipLaunchKernelGGL(te::k_part_scatter_prep377, dim3(sblocks + rows * per_row), dim3(512), 0, stream, sa, sblocks, tab, row_slab,
                             reinterpret_cast<te::rec_slot<14>*>(recs_out()), n32, per_row, rows * per_row);
        } else {
          const uint32_t per_row = (n32 + 255u) / 256u;
          hipLaunchKernelGGL(te::k_part_scatter_prep, dim3(sblocks + rows * per_row), dim3(512), 0, stream, sa, sblocks, tab, row_slab,
                             reinterpret_cast<te::pnt_slot*>(recs_out()), n32, per_row, rows * per_row);
        }
      } else if (idx) {
        hipLaunchKernelGGL(te::k_part_scatter_indexed, dim3(p.CH, p.nw), dim3(512), 0, stream, sa, te::index_args{idx, idx_count, idx_pos, ws.d_err});
      } else {
        hipLaunchKernelGGL(te::k_part_scatter, dim3(p.CH, p.nw), dim3(512), 0, stream, sa);
      }
    }
    mark(ST_BSORT);
    if (p.nw > 0) {
      // level 2: one block per partition (+ extra blocks for the pieces of over-long partitions) counts, plans and places
      // it; d_num_seg[1..3] = split / giant bucket counters, zeroed with the rest
      const uint32_t l2_blocks = p.P + n32 / TE_L2_CAP + 1u;
      te::l2_args la;
      la.part_keys = ws.d_part_keys; la.part_idx = ws.d_part_idx; la.part_start = ws.d_part_start; la.part_count = ws.d_part_count;
      la.bucket_count = ws.d_bucket_count; la.sorted = ws.d_sorted; la.part_ticket = ws.d_part_ticket; la.g = sg;
      la.pa.part_start = ws.d_part_start; la.pa.part_count = ws.d_part_count; la.pa.seg_part_base = ws.d_seg_part_base;
      la.pa.bucket_start = ws.d_bucket_start; la.pa.bucket_cursor = ws.d_bucket_cursor; la.pa.seg_base = ws.d_seg_base; la.pa.seg_bucket = ws.d_seg_bucket;
      la.pa.seg_lenv = ws.d_seg_lenv; la.pa.size_hist = ws.d_size_hist; la.pa.split_list = ws.d_split_list; la.pa.split_count = ws.d_num_seg + 1;
      la.pa.chunk_list = ws.d_chunk_list; la.pa.seg_len = p.seg_len; la.pa.cap_w = cap_w; la.pa.chunk_cap = chunk_cap();
      if (p.packed) hipLaunchKernelGGL(te::k_l2_local<true>, dim3(l2_blocks, p.nw), dim3(256), 0, stream, la);
      else hipLaunchKernelGGL(te::k_l2_local<false>, dim3(l2_blocks, p.nw), dim3(256), 0, stream, la);
      // the segment schedule (counts the valid segments, d_num_seg[0]; with "sort_buckets" = 0 the schedule is simply not used)
      // + the placement of the pieces of over-long partitions in one launch
      te::order_args oa;
      oa.lenv = ws.d_seg_lenv; oa.ids = smax(); oa.size_hist = ws.d_size_hist; oa.rel_cursor = ws.d_size_cursor; oa.order = ws.d_order; oa.num_segments = ws.d_num_seg;
      // ~128 schedule blocks, more where a block's slice of the id space would not fit its registers (TE_ORDER_REGS * 256 ids)
      {
        const uint32_t by_regs = (smax() + TE_ORDER_REGS * 256u * (uint32_t)p.nw - 1u) / (TE_ORDER_REGS * 256u * (uint32_t)p.nw);
        oa.order_cols = std::min(64u, std::max(by_regs, (uint32_t)std::max(1, 128 / p.nw)));
      }
      oa.max_len = std::min(p.seg_len, 1023u);                     // no segment is longer: only the histogram chunks up to there are scanned
      if (p.packed)
        hipLaunchKernelGGL(te::k_l2_place_order<true>, dim3(oa.order_cols + l2_blocks, p.nw), dim3(256), 0, stream, ws.d_part_keys, ws.d_part_idx, ws.d_part_start,
                           ws.d_part_count, ws.d_bucket_cursor, ws.d_sorted, sg, oa);
      else
        hipLaunchKernelGGL(te::k_l2_place_order<false>, dim3(oa.order_cols + l2_blocks, p.nw), dim3(256), 0, stream, ws.d_part_keys, ws.d_part_idx, ws.d_part_start,
                           ws.d_part_count, ws.d_bucket_cursor, ws.d_sorted, sg, oa);
    }
    mark(ST_ORDER);
    return 0;
  }

  bool bls() const { return p.curve == TE_MSM_CURVE_BLS12_377_G1; }

  // K3: one thread per segment (at most seg_len entries of one bucket): 7-product mixed additions (8 for BLS12-377)
  template <int N, int RK> int accumulate_t() {
    mark(ST_ACCUM);
    if (p.nw > 0) {
      const uint32_t n32 = this->n32(), smax = this->smax();
      const uint32_t* order = ctx->opt_sort ? ws.d_order : nullptr;
      using slot_t = typename te::rec_kind<N, RK>::slot;
      hipLaunchKernelGGL((te::k_accumulate<N, RK>), dim3((smax + 255) / 256), dim3(256), 0, stream, reinterpret_cast<const slot_t*>(bound ? bound : recs_out()), ws.d_sorted,
                         ws.d_bucket_start, ws.d_bucket_count, ws.d_seg_base, ws.d_seg_bucket, ws.d_seg_lenv, order, ws.d_num_seg,
                         reinterpret_cast<te::ete_t<N>*>(ws.d_buckets.p), reinterpret_cast<te::ete_t<N>*>(ws.d_seg_out.p), n32, p.logB, p.seg_len, smax, onto ? 1u : 0u,
                         // (a ragged sequence: every window's k / nw is 0 -- record slab 0, the bound set itself, for any number of MSMs)
                         ragged ? (uint32_t)p.nw : (uint32_t)p.nw1, ragged ? te::batch_slabs{} : slabs(),
                         prof ? reinterpret_cast<unsigned long long*>(ws.d_zero + Z_CLOCK) : nullptr);
    }
    return 0;
  }
  int accumulate() { return bls() ? (p.rec_kind == 1 ? accumulate_t<14, 1>() : accumulate_t<14, 0>()) : accumulate_t<9, 0>(); }

  // sums of the buckets that were accumulated in several parts: buckets cut into 2..16 parts (quads) and the TE_GIANT_RUN-part runs
  // of giant buckets (blocks; the block that finishes a bucket's last run adds the runs up) in one launch
  template <int N> int combine_t() {
    if (p.nw <= 0) return 0;
    using E = te::ete_t<N>;
    hipLaunchKernelGGL(te::k_seg_combine_all<N>, dim3(256 + 1024), dim3(256), 0, stream, ws.d_split_list, ws.d_num_seg + 1, ws.d_chunk_list,
                       ws.d_bucket_count, ws.d_seg_base, reinterpret_cast<E*>(ws.d_seg_out.p), reinterpret_cast<E*>(ws.d_buckets.p), p.seg_len, chunk_cap(), 256u,
                       ws.d_bucket_start, ws.d_bucket_cursor);
    return 0;
  }
  int combine() { return bls() ? combine_t<14>() : combine_t<9>(); }

  // K4/K5: buckets -> one row per window (see kernels.hip.hpp, K4a and k_reduce_tail).  Bucket index j = hi * L + lo:
  //   rows chain  xin[hi * r + g]  -- the low L = 2^(w0+w1) part folded from the top, 8 (4, 2) sub-blocks at a time
  //   cols chain  yin[h * L + lo]  -- the high H = 2^(w2+w3) part folded from the top
  // Wide levels (both chains per launch, one thread or one quad per output) run until at most 4 partial sums per output
  // are left; k_reduce_tail (one block per window and digit) does the rest and writes the row.  n = 2^20, c = 16: two fold
  // launches (32768 -> 4096 -> 512 points per window and chain) + the tail, against nine launches of the first version.
  template <int N> int reduce_t() {
    if (p.nw > 0) {
      using E = te::ete_t<N>;
      const uint32_t w0 = p.dw[0], w1 = p.dw[1], w2 = p.dw[2], w3 = p.dw[3];
      const uint32_t L = 1u << (w0 + w1), H = 1u << (w2 + w3);
      struct chain_t { const E* cur; uint32_t n, r; E* buf[2]; int pp; };
      E* const bk = reinterpret_cast<E*>(ws.d_buckets.p);
      chain_t ch[2] = {{bk, p.B, L, {reinterpret_cast<E*>(ws.d_red[0].p), reinterpret_cast<E*>(ws.d_red[1].p)}, 0},
                       {bk, p.B, H, {reinterpret_cast<E*>(ws.d_red[2].p), reinterpret_cast<E*>(ws.d_red[3].p)}, 0}};
      for (;;) {
        te::sum_jobs_t<N> js; memset(&js, 0, sizeof js);
        uint32_t most = 0; int nj = 0;
        for (int i = 0; i < 2; i++) {
          chain_t& c = ch[i];
          if (c.r <= 4u) continue;
          const uint32_t K = (c.r % 8u == 0) ? 8u : (c.r % 4u == 0) ? 4u : 2u;
          // (folding by 4 where that keeps a level above the 65536 outputs a thread-per-output launch needs -- n = 2^16, 2^17 --
          // was measured: 42 + 26 + 16 us against 62 + 16 us: one more dependent level costs more than the cheaper first one saves)
          te::sum_job_t<N>& j = js.j[nj++];
          j.in = c.cur; j.out = c.buf[c.pp]; j.K = K; j.n_out = c.n / K;
          j.inner = i == 0 ? c.r / K : (c.r / K) * L;          // rows: sub-blocks inside one hi; cols: whole slabs of L
          j.in_per_window = c.n; j.out_per_window = c.n / K;
          c.cur = j.out; c.pp ^= 1; c.r /= K; c.n /= K;
          most = std::max(most, j.n_out * (uint32_t)p.nw);
        }
        if (!nj) break;
        // From 32768 outputs on a level runs one thread per output (9 products per addition, k_sum_groups); below that four
        // lanes per output (16 lane-products per addition, but three dependent products instead of nine: k_sum_groups_team).
        // The line was at 65536 ("one wave per SIMD") until round 3: at n = 2^16..2^18 (18 windows x 16384 buckets, first level
        // 36864 outputs) the thread form is as fast for one MSM (0.344 against 0.346 ms) and leaves more of the VALU to the
        // other MSMs in flight: 0.1645 against 0.1785 ms per MSM at 2^16, 0.224 against 0.239 at 2^17.  16384 would also move
        // the second level of unsigned 16-bit windows (64 blocks of serial additions: slower for one MSM).
        if (most >= 65536u || (most >= 32768u && !ctx->opt_fold_pairs)) {
          uint32_t blocks = (most + 255) / 256; if (blocks > 4096) blocks = 4096;
          hipLaunchKernelGGL((te::k_sum_groups<N, false>), dim3(blocks, nj), dim3(256), 0, stream, js, (uint32_t)p.nw);
        } else if (most >= 32768u) {
          // too few outputs for one thread each to fill the machine (n <= 2^18: 36 864 per chain): two lanes per output, half
          // the dependent additions (option "fold_pairs"; every level folds by 8, 4 or 2 -- K is even)
          uint32_t blocks = (2 * most + 255) / 256; if (blocks > 4096) blocks = 4096;
          hipLaunchKernelGGL((te::k_sum_groups<N, true>), dim3(blocks, nj), dim3(256), 0, stream, js, (uint32_t)p.nw);
        } else {                            // latency-bound level: four lanes per output.  (Sixteen lanes per output as a tree --
                                            // 3 dependent team additions instead of 7 -- was measured: 22.5 us against 18.5 at
                                            // n = 2^20: four times the lanes put four waves on every SIMD and each addition slows down.)
          uint32_t blocks = (most * 4 + 255) / 256; if (blocks > 4096) blocks = 4096; if (blocks < 1) blocks = 1;
          hipLaunchKernelGGL(te::k_sum_groups_team<N>, dim3(blocks, nj), dim3(256), 0, stream, js, (uint32_t)p.nw);
        }
      }
      mark(ST_WEIGHTED);
      te::tail_params_t<N> tp;
      tp.xin = ch[0].cur; tp.yin = ch[1].cur; tp.rx = ch[0].r; tp.ry = ch[1].r;
      tp.x_per_window = ch[0].n; tp.y_per_window = ch[1].n;
      tp.w[0] = w0; tp.w[1] = w1; tp.w[2] = w2; tp.w[3] = w3;
      // host_rows: the rows (and the flag words in front of them) are written to the pinned host block by the kernel itself
      uint8_t* const rows_base = host_rows ? reinterpret_cast<uint8_t*>(ws.h_err_dev + Z_ROWS) : static_cast<uint8_t*>(d_partials_out);
      tp.flag_src = host_rows ? ws.d_zero : nullptr; tp.flag_dst = host_rows ? ws.h_err_dev : nullptr; tp.flag_words = (uint32_t)Z_ROWS;
      tp.rows = reinterpret_cast<E*>(rows_base) + (size_t)p.w_first * 5; tp.row_stride = (uint32_t)p.w_step * 5u;
      tp.win_per_msm = (uint32_t)p.nw1; tp.msm_stride = (uint32_t)p.W * 5u;          // batch: MSM m's W rows follow MSM m-1's
      const size_t lds_bytes = (size_t)(std::max(H, L) + 16u) * sizeof(E);
      hipLaunchKernelGGL(te::k_reduce_tail<N>, dim3(4, p.nw), dim3(1024), lds_bytes, stream, tp);
    } else {
      mark(ST_WEIGHTED);
    }
    mark(ST_COUNT);
    if (!own_rows) HIP_TRY(ctx, hipMemcpyAsync(ws.h_err, ws.d_zero, Z_ROWS * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));   // flag + clock words
    return 0;
  }
  int reduce() { return bls() ? reduce_t<14>() : reduce_t<9>(); }

  // recombination of split buckets, digit marginals, weighted sums, error flag read-back
  int back() {
    if (int rc = combine()) return rc;
    return reduce();
  }
};

// d_partials_out == nullptr: the rows go to the work set's own buffer (ws.d_partials, inside the block that is zeroed per
// MSM) and the caller fetches flag + rows with fetch_rows().
// upload_points (optional): enqueues the host-to-device copy of the points on the given (side) stream -- te_msm_run; the
// upload then overlaps digits, sort and schedule.
// With an upload, the points -> records conversion follows it on the work set's side stream, beside the scalar-only
// stages, and joins before the accumulation.  Running it there for device-resident inputs as well was
// measured and is not used: for one MSM the conversion and the sort stages are both bandwidth-bound and merely slow each
// other down (latency 1.36 -> 1.38 ms), and with several MSMs in flight every extra stream competes for the runtime's few
// hardware queues (four by default; GPU_MAX_HW_QUEUES=8 did not help) and serialises the others: 941 -> 862 MSM/s.
// the copy stream of a work set exists from its first host-buffer MSM on (te_msm_run): a context that only ever sees
// device-resident inputs owns one stream per work set
int need_copy_stream(te_ctx* ctx, workset_t& ws) {
  if (ws.copy_stream) return 0;
  HIP_TRY(ctx, hipStreamCreateWithFlags(&ws.copy_stream, hipStreamNonBlocking));
  return 0;
}

// The runtime multiplexes all streams of a process onto a few hardware queues (four unless GPU_MAX_HW_QUEUES says otherwise)
// and kernels of one queue run in order: MSMs in flight on two streams of the same queue do not overlap.  Which stream
// gets which queue follows from how many streams the process created before (tools/queue_probe.hip: 0 1 2 3 3 2 1 0 3 2
// 1 0 ...), so a context created after other streams -- PyTorch's, RCCL's, another context's -- found its first four work
// sets on two queues: n = 2^16 / 2^17 / 2^18 ran at 0.23 / 0.32 / 0.42 instead of 0.19 / 0.24 / 0.35 ms per MSM.
// Only callers that keep several MSMs in flight care, so the measurement is LAZY: te_msm_init hands the streams out in
// creation order, and the first te_msm_submit_device (every work set idle, device synchronised) measures which of them
// share a queue (pairs of k_spin kernels: one duration when they overlap, two when they are serialised; ~16 ms once)
// and re-deals them so that sets 0..3 and sets 4..7 each sit on as many different queues as there are.  One-shot callers
// (te_msm_run, compute_msm with force_recompile) never pay it.  The host-timed pairs can be disturbed by other work on
// the GPU, so a classification is accepted only when a second, independent measurement gives the same classes;
// otherwise the creation order stays.  Option "queue_probe" = 0 (env TE_MSM_QUEUE_PROBE=0) turns the lazy measurement off;
// te_msm_probe_queues runs it at a moment the caller chooses.
// classes[i] = index of the hardware queue class of streams[i] (classes numbered by first appearance); returns the number of
// classes, or -1 when the measurement could not run (then classes[] is all -1)
int classify_streams_by_queue(gpu_t& d, const hipStream_t* streams, int n, int* cls) {
  for (int i = 0; i < n; i++) cls[i] = -1;
  if (d.wall_clock_khz <= 0 || n < 2) return -1;
  uint32_t* const flag = nullptr;       // k_spin takes an optional output word; none here (hipMalloc / hipFree would synchronise the whole device)
  const unsigned long long ticks = (unsigned long long)d.wall_clock_khz * 3 / 10;      // 0.3 ms
  auto pair_ms = [&](int a, int b) {
    (void)hipStreamSynchronize(streams[a]); (void)hipStreamSynchronize(streams[b]);
    const auto t0 = std::chrono::steady_clock::now();
    hipLaunchKernelGGL(te::k_spin, dim3(1), dim3(64), 0, streams[a], ticks, flag);
    hipLaunchKernelGGL(te::k_spin, dim3(1), dim3(64), 0, streams[b], ticks, flag);
    (void)hipStreamSynchronize(streams[a]); (void)hipStreamSynchronize(streams[b]);
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  (void)pair_ms(0, 1);                                                                    // first launch: code upload
  // one kernel alone (the same stream twice runs them back to back: half of that), best of two
  const double alone = std::min(pair_ms(0, 0), pair_ms(0, 0)) * 0.5;
  auto shared = [&](int a, int b) { return std::min(pair_ms(a, b), pair_ms(a, b)) > 1.6 * alone; };
  int ncls = 0;
  for (int i = 0; i < n; i++) {
    if (cls[i] >= 0) continue;
    cls[i] = ncls;
    for (int j = i + 1; j < n; j++) if (cls[j] < 0 && shared(i, j)) cls[j] = ncls;
    ncls++;
  }
  if (hipGetLastError() != hipSuccess) { for (int i = 0; i < n; i++) cls[i] = -1; return -1; }
  return ncls;
}

// order[k] = which stream comes k-th when the streams are dealt round-robin over their classes: first one stream of every
// class, then the next of every class, ... (identity when nothing was measured)
void deal_over_classes(const int* cls, int n, int ncls, int* order) {
  int k = 0;
  if (ncls > 1 && ncls < n) {
    std::vector<char> used(n, 0);
    while (k < n)
      for (int c = 0; c < ncls && k < n; c++)
        for (int i = 0; i < n; i++) if (!used[i] && cls[i] == c) { used[i] = 1; order[k++] = i; break; }
  } else {
    for (int i = 0; i < n; i++) order[i] = i;
  }
}

// EXPORTED STREAMS ARE NEVER DESTROYED.  te_msm_workset_stream hands a work set's stream out as a raw hipStream_t so that a
// caller can order its own work behind an MSM (PyTorch: torch.cuda.ExternalStream).  Such callers REMEMBER the handle in places
// the engine cannot see: PyTorch's pinned-memory allocator keeps, for every pinned block, the streams it was used on and records
// an event on each of them when the block is released -- for a tensor that outlives the context that is after te_msm_destroy,
// possibly at interpreter exit; hipEventRecord on a destroyed stream fails, the error is raised inside a deleter, and the
// process aborts (round 5: tools/exp_batch_small.py "dumped core" after its last result line; profiles/r06_batch_small_abort.txt).
// So the streams of a device whose handles were exported are PARKED by te_msm_destroy -- synchronised, kept alive, and taken
// over by the next context on that device -- and stay valid hipStream_t values until the process exits.  A context that never
// exported a handle destroys its streams as before.
struct parked_streams_t { std::mutex mu; std::vector<std::pair<int, hipStream_t>> v; };
parked_streams_t& parked_streams() { static parked_streams_t* p = new parked_streams_t(); return *p; }     // (leaked on purpose: no destructor at exit)
hipStream_t take_parked_stream(int device) {
  parked_streams_t& ps = parked_streams();
  std::lock_guard<std::mutex> lk(ps.mu);
  for (size_t i = 0; i < ps.v.size(); i++)
    if (ps.v[i].first == device) { hipStream_t s = ps.v[i].second; ps.v.erase(ps.v.begin() + (long)i); return s; }
  return nullptr;
}
void park_stream(int device, hipStream_t s) {
  parked_streams_t& ps = parked_streams();
  std::lock_guard<std::mutex> lk(ps.mu);
  ps.v.emplace_back(device, s);
}

// te_msm_init: one compute stream per work set, in creation order (no measurement); parked streams of the device first
int create_workset_streams(gpu_t& d) {
  for (int i = 0; i < TE_MSM_WORKSETS; i++) {
    d.ws[i].stream = take_parked_stream(d.device);
    if (d.ws[i].stream) d.streams_exported = true;      // somebody may still hold this handle: it goes back to the pool, never to hipStreamDestroy
    if (!d.ws[i].stream && hipStreamCreateWithFlags(&d.ws[i].stream, hipStreamNonBlocking) != hipSuccess) {
      for (int j = 0; j < i; j++) { if (d.streams_exported) park_stream(d.device, d.ws[j].stream); else (void)hipStreamDestroy(d.ws[j].stream); d.ws[j].stream = nullptr; }
      d.ws[i].stream = nullptr;
      return -1;
    }
    d.ws[i].hw_queue_class = -1;
  }
  return 0;
}

// The measurement itself (first te_msm_submit* of a context unless option "queue_probe" = 0, or te_msm_probe_queues at a moment
// the caller chooses).  Never fatal: any failure leaves the creation order in place.  It waits for THIS context's streams only
// -- no device-wide synchronisation: other streams of the process (PyTorch's, RCCL's) keep running; should their kernels
// disturb the host-timed pairs, the two passes disagree and the creation order stays.
void spread_streams_over_queues(gpu_t& d) {
  d.queues_probed = true;
  for (const workset_t& ws : d.ws) if (te_sched::slot_ticket(ws.slot)) return;            // cannot happen on the first submit; be safe
  for (workset_t& ws : d.ws) {
    if (ws.used && ws.ev_done && hipEventSynchronize(ws.ev_done) != hipSuccess) { (void)hipGetLastError(); return; }
    if (hipStreamSynchronize(ws.stream) != hipSuccess) { (void)hipGetLastError(); return; }
  }
  hipStream_t cand[TE_MSM_WORKSETS];
  for (int i = 0; i < TE_MSM_WORKSETS; i++) cand[i] = d.ws[i].stream;
  int cls[TE_MSM_WORKSETS], again[TE_MSM_WORKSETS], order[TE_MSM_WORKSETS];
  const int ncls = classify_streams_by_queue(d, cand, TE_MSM_WORKSETS, cls);
  const int ncls2 = ncls > 0 ? classify_streams_by_queue(d, cand, TE_MSM_WORKSETS, again) : -1;
  const bool agree = ncls > 0 && ncls2 == ncls && memcmp(cls, again, sizeof cls) == 0;
  if (getenv("TE_MSM_QUEUE_DUMP")) {
    fprintf(stderr, "[te_msm] hardware-queue classes of %d streams (%s):", TE_MSM_WORKSETS, agree ? "two measurements agree" : "measurements disagree: creation order kept");
    for (int i = 0; i < TE_MSM_WORKSETS; i++) fprintf(stderr, " %d/%d", cls[i], ncls2 > 0 ? again[i] : -1);
    fprintf(stderr, "\n");
  }
  if (!agree) return;
  deal_over_classes(cls, TE_MSM_WORKSETS, ncls, order);
  for (int i = 0; i < TE_MSM_WORKSETS; i++) {
    workset_t& ws = d.ws[i];
    // the set's buffers were last used on its old stream: the context's work is over (synchronised above), so the new stream
    // needs no wait; last_stream follows so that enqueue_partial does not add one
    if (ws.last_stream == ws.stream) ws.last_stream = cand[order[i]];
    ws.stream = cand[order[i]]; ws.hw_queue_class = cls[order[i]];
  }
}

int finish_sequence(te_ctx* ctx, workset_t& ws, hipStream_t stream);

// SHARED RECORD SLABS.  Every work set used to own the record slab its MSM converts into: four MSMs in flight gather from
// 4 x 128 MB of records (n = 2^20) -- twice the 256 MB Infinity Cache -- although a caller with MSMs in flight nearly always names ONE
// point buffer (the harness: full_benchmarks.ts:63-68,100-105; a prover: its SRS).  A gather footprint beyond the cache costs clock under
// the power ceiling (profiles/r06_fixed_base_windows.txt, step 1: 512 MB instead of 128 MB: -7 % MSMs in flight).  So whole-MSM calls
// from device-resident inputs that name the same point buffer (pointer, n, curve) while they are in flight share one slab, and gather
// from there (inputs of a call in flight must not change: include/te_msm.h).  A slab serves another point buffer only when no call in
// flight uses it any more.
// CONVERT ONCE PER OCCUPANCY RUN.  Until round 6 every call still converted its points into the slab (the same bytes again: 64 MB read,
// 128 MB written and four products per point, k_part_scatter_prep 76 us against 46 for the plain k_part_scatter).  But a whole-MSM
// call that joins a slab while another whole-MSM call of the same buffer is in flight (rec_slab_t::run_users > 0) finds that buffer
// unchanged since the run's first conversion: every call since then named it while in flight, so none of them let it change.  Such a
// call converts nothing when the event behind the run's conversion has completed (hipEventQuery: no packet, no wait); while that
// conversion may still be running -- the calls submitted right behind the first one of a run -- it converts itself, as before (no
// cross-stream wait: its own accumulation stays ordered behind its own conversion).  When the run ends (run_users 0), the slab is
// re-purposed or freed, the state is gone: the next call converts again, the buffer may hold other points by then.  Only whole-MSM calls
// whose completion the engine sees take part (share_mode SHARE_RUN): the building blocks te_msm_partial_device[_batch], x-only points,
// checked points ("check_points") and "share_records" = 2 convert on every call (SHARE_CONVERT), host buffers into their own slab.
// The reference converts per call (convert_point_coords...wgsl:37-77).
// (the slab's earlier users may still be running -- see rec_slab_t::pending: `stream`, on which the new user's conversion is about to be
// enqueued, waits for them; nullptr: the host waits -- trim, destroy)
int settle_slab(te_ctx* ctx, gpu_t::rec_slab_t& sl, hipStream_t stream, bool host) {
  for (int wi = 0; wi < TE_MSM_WORKSETS; wi++) if ((sl.pending >> wi) & 1u) {
    if (host) HIP_TRY(ctx, hipEventSynchronize(sl.ev[wi])); else HIP_TRY(ctx, hipStreamWaitEvent(stream, sl.ev[wi], 0));
  }
  sl.pending = 0;
  return 0;
}
// run: the caller is a whole-MSM call of the slab's occupancy run (SHARE_RUN); *have: its records are in the slab already (no conversion)
int acquire_shared_recs(te_ctx* ctx, gpu_t& d, const void* src, uint64_t n, int curve, hipStream_t stream, bool run, uint8_t** out, bool* have) {
  const size_t need = (size_t)n * sizes_of(curve).rec;
  int pick = -1;
  *have = false;
  // the same buffer, in use or just let go of (its records are the same bytes: no wait, and `pending` stays for whoever re-purposes the slab)
  for (size_t i = 0; i < d.slabs.size(); i++) if ((d.slabs[i].users > 0 || d.slabs[i].pending) && d.slabs[i].d && d.slabs[i].src == src && d.slabs[i].n == n && d.slabs[i].curve == curve) {
    gpu_t::rec_slab_t& sl = d.slabs[i];
    if (run) {
      if (sl.run_users > 0 && sl.converted) {
        const hipError_t q = hipEventQuery(sl.conv_ev);
        if (q == hipSuccess) *have = true;
        else (void)hipGetLastError();                 // hipErrorNotReady is an answer, not an error: this call converts as well
      }
      sl.run_users++;
    }
    sl.users++; *out = sl.d; return (int)i;
  }
  // a free slab: one nobody is waiting on first, the smallest that is large enough
  if (pick < 0) for (size_t i = 0; i < d.slabs.size(); i++) if (d.slabs[i].users == 0 && !d.slabs[i].pending && d.slabs[i].d && d.slabs[i].cap >= need && (pick < 0 || d.slabs[i].cap < d.slabs[(size_t)pick].cap)) pick = (int)i;
  if (pick < 0) for (size_t i = 0; i < d.slabs.size(); i++) if (d.slabs[i].users == 0 && d.slabs[i].d && d.slabs[i].cap >= need && (pick < 0 || d.slabs[i].cap < d.slabs[(size_t)pick].cap)) pick = (int)i;
  if (pick < 0) for (size_t i = 0; i < d.slabs.size(); i++) if (d.slabs[i].users == 0) { pick = (int)i; break; }
  if (pick < 0) { d.slabs.emplace_back(); pick = (int)d.slabs.size() - 1; }
  gpu_t::rec_slab_t& sl = d.slabs[(size_t)pick];
  sl.converted = false;                                                  // (users = 0: no occupancy run holds it)
  if (!sl.d || sl.cap < need) {
    if (int rc = settle_slab(ctx, sl, nullptr, true)) return rc;
    if (sl.d) HIP_TRY(ctx, hipFree(sl.d));
    sl.d = nullptr; sl.cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&sl.d, need ? need : 16));
    sl.cap = need;
  }
  if (int rc = settle_slab(ctx, sl, stream, false)) return rc;          // another buffer's records are about to be overwritten
  sl.src = src; sl.n = n; sl.curve = curve; sl.users++; sl.run_users = run ? 1 : 0;
  *out = sl.d;
  return pick;
}
// behind the conversion launch of a run's call: later calls of the run may skip theirs once this event has completed
int note_conversion(te_ctx* ctx, gpu_t::rec_slab_t& sl, hipStream_t stream) {
  if (!sl.conv_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&sl.conv_ev, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventRecord(sl.conv_ev, stream));
  sl.converted = true;
  return 0;
}
// completed: the set's MSM is known to be over (a collected ticket, a synchronous call).  Otherwise (the building blocks: the set is simply
// used again) an event behind that MSM -- on the stream it ran on, BEFORE anything new is enqueued there -- guards the slab.
void release_shared_recs(gpu_t& d, workset_t& ws, bool completed = true) {
  if (ws.slab >= 0 && (size_t)ws.slab < d.slabs.size() && d.slabs[(size_t)ws.slab].users > 0) {
    gpu_t::rec_slab_t& sl = d.slabs[(size_t)ws.slab];
    sl.users--;
    if (ws.slab_run && sl.run_users > 0 && --sl.run_users == 0) sl.converted = false;   // the occupancy run is over: the next call converts
    if (!completed && ws.last_stream) {
      const int wi = (int)(&ws - d.ws);
      if (!sl.ev[wi]) (void)hipEventCreateWithFlags(&sl.ev[wi], hipEventDisableTiming);
      if (sl.ev[wi] && hipEventRecord(sl.ev[wi], ws.last_stream) == hipSuccess) sl.pending |= 1u << wi;
      else (void)hipStreamSynchronize(ws.last_stream);                  // (no event: the host waits instead)
    }
  }
  ws.slab = -1; ws.slab_run = false;
}

// Where a call's records live (enqueue_partial): the work set's own d_recs; a shared slab the call converts into (the building blocks,
// whose completion the engine does not see, and whole-MSM calls whose input form keeps the per-call conversion); or a shared slab as a
// whole-MSM call of its occupancy run, which converts only when no earlier call of the run has (see SHARED RECORD SLABS above).
enum share_mode { SHARE_NONE = 0, SHARE_CONVERT = 1, SHARE_RUN = 2 };

// HOW EVERY LAUNCH SEQUENCE BEGINS ON A WORK SET (the four enqueue functions and enqueue_ragged).  The set lets go of the shared slab its previous MSM still
// named (guarded by an event unless that MSM was seen to end); L.stream waits for the set's previous MSM when that ran on another stream
// (the set's buffers are still the previous MSM's); the launch learns where its own rows go.  recs_last: where te_msm_debug_read finds the
// records of the sequence.  share (enqueue_partial alone): the sequence takes a shared record slab for that point buffer, which then is
// its recs_last -- taken between the two steps, so that the slab's own wait on L.stream stands in front of the set's.
struct slab_request { const void* src; bool run; };       // run: a whole-MSM call of the slab's occupancy run (SHARE_RUN)
int begin_sequence(gpu_t& d, msm_launch& L, const uint8_t* recs_last, const slab_request* share = nullptr) {
  te_ctx* const ctx = L.ctx; workset_t& ws = L.ws;
  release_shared_recs(d, ws, false);
  ws.recs_last = recs_last;
  if (share) {
    const int si = acquire_shared_recs(ctx, d, share->src, L.n, L.p.curve, L.stream, share->run, &L.recs_rw, &L.have_recs);
    if (si < 0) return si;
    ws.slab = si; ws.slab_run = share->run; ws.recs_last = L.recs_rw;
  }
  if (ws.used && ws.last_stream != L.stream) HIP_TRY(ctx, hipStreamWaitEvent(L.stream, ws.ev_done, 0));
  L.host_rows = L.rows_to_host();
  ws.rows_on_host = L.host_rows;
  return 0;
}
// ... and what it leaves on the set for the next sequence and for the read-back of its result.  The whole forms note it before their first
// launch; the piece forms after their last piece: copy_stream_behind_previous, behind begin_sequence, asks whether the set was used BEFORE
// this sequence, and plan and n are the last piece's.  (the device's host thread may be the writer of last_ws: asynchronous submits)
void note_sequence(gpu_t& d, workset_t& ws, const plan_t& p, uint64_t n, hipStream_t stream, int prof_level) {
  ws.plan = p; ws.n = n; ws.used = true; ws.last_stream = stream; ws.prof_level = prof_level;
  __atomic_store_n(&d.last_ws, (int)(&ws - d.ws), __ATOMIC_RELAXED);
}

// One launch sequence from device-resident inputs (enqueue_partial).  Only the scalars, n and the stream are always needed.
struct partial_req {
  const void* d_points = nullptr; const void* d_scalars = nullptr; uint64_t n = 0;   // batch > 1: arrays of `batch` device pointers (on the host)
  void* d_partials_out = nullptr;     // nullptr: the rows go to the work set's own buffer, the caller fetches flag + rows with fetch_rows()
  hipStream_t stream = nullptr;
  const std::function<int(hipStream_t)>* upload_points = nullptr;   // enqueues the host-to-device copy of the points on the given (side) stream
  int batch = 1;
  bool whole = false;                 // every window instead of the device's window shard (plan_req)
  const te_bases* bases = nullptr;    // the launch sequence gathers from a bound point set (d_points is not read: no conversion); batch must be 1
  share_mode share = SHARE_NONE;      // the record slab of the call; a shared slab only for device-resident points, without bound bases
  const uint32_t* d_idx = nullptr;    // (with bases) an indexed subset: the n entries gather records d_idx[0 .. n) of the set (device memory of d)
  int scalar_form = -1;               // plan_req's: -1 = option "scalars_montgomery" as it is now
};
int enqueue_partial(te_ctx* ctx, gpu_t& d, workset_t& ws, const partial_req& r) {
  const void* const d_points = r.d_points; const uint64_t n = r.n; hipStream_t const stream = r.stream;
  const int batch = r.batch; const te_bases* const bases = r.bases; const auto* const upload_points = r.upload_points;
  // (the plan is made for the n entries; only the entry form follows the set's count: indexed_plan.hpp)
  plan_req q; q.n = n; q.batch = batch; q.whole = r.whole; q.scalar_form = r.scalar_form;
  if (bases) q.rec_kind = bases->rec_kind;
  if (r.d_idx) q.idx_count = bases->n;
  const plan_t p = make_plan(ctx, d, q);
  // (a batch shares when all its MSMs name ONE point buffer: the batch then holds one conversion anyway -- slab 0 of msm_launch::slabs())
  const void* share_src = d_points;
  if (batch > 1 && d_points) { share_src = static_cast<const void* const*>(d_points)[0]; for (int m = 1; m < batch; m++) if (static_cast<const void* const*>(d_points)[m] != share_src) share_src = nullptr; }
  const bool share_recs = r.share != SHARE_NONE && ctx->opt_share_records && !bases && !upload_points && share_src != nullptr;
  const bool run = share_recs && r.share == SHARE_RUN && ctx->opt_share_records == 1 && !ctx->opt_check_points && batch == 1;
  if (batch > 1 && (uint64_t)p.nw * p.nst >= (1ull << 31)) return set_err(ctx, TE_MSM_EINVAL, "batch too large for this n: windows x points must stay below 2^31");
  HIP_TRY(ctx, hipSetDevice(d.device));
  if ((uint64_t)p.nw * p.B + (uint64_t)p.nw * (n / p.seg_len) + 1024u >= (1ull << 32))
    return set_err(ctx, TE_MSM_EINVAL, "segment_len is too small for this n: more than 2^32 segments");
  if (int rc = ensure_buffers(ctx, d, ws, n, p, bases == nullptr && !share_recs)) return rc;
  // profile 1: two events around the dominant kernel only (what bench.py times live); 2: every stage boundary
  // (an event between two kernels costs ~4 us of idle stream time, 11 of them ~2 % of a 2^20 MSM)
  msm_launch L(ctx, ws, p, n, stream);
  L.d_points = d_points; L.d_scalars = r.d_scalars; L.prof = ctx->opt_profile;
  L.own_rows = r.d_partials_out == nullptr;
  L.d_partials_out = L.own_rows ? ws.d_partials : r.d_partials_out;
  // a launch sequence that fails half-way lets go of its slab (and of the slab's occupancy run) at once
  struct slab_guard { gpu_t& d; workset_t& ws; bool armed; ~slab_guard() { if (armed) release_shared_recs(d, ws, false); } } guard{d, ws, share_recs};
  const slab_request slab{share_src, run};
  if (int rc = begin_sequence(d, L, bases ? nullptr : ws.d_recs.p, share_recs ? &slab : nullptr)) return rc;
  note_sequence(d, ws, p, n, stream, ctx->opt_profile);
  if (bases) {
    // resident bases: the scalar-only stages, then the accumulation straight from the bound records
    L.bound = bases->recs[(size_t)(&d - ctx->devs.data())];
    if (r.d_idx) { L.idx = r.d_idx; L.idx_count = (uint32_t)bases->n; }
    if (int rc = L.front_scalars()) return rc;
    L.mark(ST_PREP);
    if (int rc = L.accumulate()) return rc;
    L.mark(ST_TREE);
    if (int rc = L.back()) return rc;
  } else if (ctx->opt_profile >= 2 || !upload_points) {
    if (!upload_points && L.can_fuse_conversion()) {
      if (int rc = L.front()) return rc;
    } else {
      if (int rc = L.front_scalars()) return rc;
      if (upload_points) { if (int rc = (*upload_points)(stream)) return rc; }
      if (int rc = L.front_points()) return rc;
    }
    if (run && !L.have_recs) {                                 // the conversion is enqueued: later calls of the slab's run may skip theirs
      HIP_TRY(ctx, hipGetLastError());
      if (int rc = note_conversion(ctx, d.slabs[(size_t)ws.slab], stream)) return rc;
    }
    if (int rc = L.accumulate()) return rc;
    L.mark(ST_TREE);
    if (int rc = L.back()) return rc;
  } else {
    // side stream: upload of the points -> records; it starts behind everything already enqueued on `stream`
    HIP_TRY(ctx, hipEventRecord(ws.ev_start, stream));
    if (int rc = need_copy_stream(ctx, ws)) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(ws.copy_stream, ws.ev_start, 0));
    if (int rc = (*upload_points)(ws.copy_stream)) return rc;
    msm_launch S = L; S.stream = ws.copy_stream;
    if (int rc = S.front_points()) return rc;
    HIP_TRY(ctx, hipEventRecord(ws.ev_copy, ws.copy_stream));
    if (int rc = L.front_scalars()) return rc;
    HIP_TRY(ctx, hipStreamWaitEvent(stream, ws.ev_copy, 0));
    if (int rc = L.accumulate()) return rc;
    L.mark(ST_TREE);
    if (int rc = L.back()) return rc;
  }
  // rows in the caller's buffer: the sequence ends here (the flag's read-back is part of reduce()); rows in the set's own
  // block: the caller's fetch_rows() ends it
  if (!L.own_rows) { if (int rc = finish_sequence(ctx, ws, stream)) return rc; }
  HIP_TRY(ctx, hipGetLastError());
  guard.armed = false;
  return 0;
}

// one device-to-host copy: final-carry flag + the W rows of the work set's own row buffer (enqueue_partial with nullptr);
// ends the launch sequence
int fetch_rows(te_ctx* ctx, workset_t& ws, hipStream_t stream) {
  // (nothing to copy when k_reduce_tail wrote flag words and rows to the pinned block itself)
  if (!ws.rows_on_host)
    HIP_TRY(ctx, hipMemcpyAsync(ws.h_err, ws.d_zero, Z_ROWS * 4 + (size_t)ws.plan.W * sizes_of(ws.plan.curve).row, hipMemcpyDeviceToHost, stream));
  return finish_sequence(ctx, ws, stream);
}

// End of an MSM's launch sequence on `stream`: flag and rows are on their way to the host (ev_result); behind them the
// zeroed block is cleared for the set's NEXT MSM -- 4 us of fill and a launch gap that would otherwise sit in front of that
// MSM's first kernel, on its critical path -- and ev_done marks the set free.  Not with "prezero" = 0 (stage verifiers read
// counters and rows from the block afterwards).
int finish_sequence(te_ctx* ctx, workset_t& ws, hipStream_t stream) {
  HIP_TRY(ctx, hipEventRecord(ws.ev_result, stream));
  if (ctx->opt_prezero) {
    HIP_TRY(ctx, hipMemsetAsync(ws.d_zero, 0, ws.zero_words * sizeof(uint32_t), stream));
    ws.zero_clean_words = ws.zero_words;
  }
  HIP_TRY(ctx, hipEventRecord(ws.ev_done, stream));
  return 0;
}

// Stage times of the MSM that last ran on `ws`, read from the events recorded at ITS profile level (the option may have
// changed since).  Never fatal: a failed read leaves "no stage times" instead of losing the MSM's result.
int collect_stage_ms(te_ctx* ctx, const gpu_t& d, workset_t& ws) {
  if (!ws.prof_level) return 0;
  bool ok = true;
  for (int i = 0; i < ST_COUNT; i++) {
    float ms = -1.0f;
    if (ws.prof_level >= 2 || i == ST_ACCUM) ok = ok && hipEventElapsedTime(&ms, ws.ev[i], ws.ev[i + 1]) == hipSuccess;
    ctx->stage_ms[i] = ms;
  }
  {
    // k_accumulate stamped ~clock of its first wave and the clock of its last one (atomic max on zeroed words); they came
    // back with the flag.  Unlike the event interval this excludes the time the launch waited behind other streams' kernels.
    uint64_t raw[4 * TE_CLK_SLOTS]; memcpy(raw, ws.h_err + Z_CLOCK, sizeof raw);
    uint64_t c[4] = {0, 0, 0, 0};                      // max ~start, max end, sum of core ticks, sum of wall ticks over the copies
    for (uint32_t i = 0; i < TE_CLK_SLOTS; i++) {
      c[0] = std::max(c[0], raw[i]); c[1] = std::max(c[1], raw[TE_CLK_SLOTS + i]);
      c[2] += raw[2 * TE_CLK_SLOTS + i]; c[3] += raw[3 * TE_CLK_SLOTS + i];
    }
    const int khz = d.wall_clock_khz;
    const bool have = c[0] && c[1] && khz > 0 && c[1] > ~c[0];
    const double ms = have ? (double)(c[1] - ~c[0]) / khz : -1.0;
    ctx->stage_ms[ST_COUNT] = (float)ms;
    // c[2] / c[3]: core ticks / wall ticks summed over the kernel's waves; wall ticks run at khz
    ctx->stage_ms[ST_COUNT + 1] = (have && c[2] && c[3]) ? (float)((double)c[2] / (double)c[3] * khz * 1e-6) : -1.0f;
  }
  if (!ok) (void)hipGetLastError();
  ctx->have_stage_ms = ok;
  return 0;
}

void free_workset_buffers(workset_t& ws) {      // the big device buffers of a work set (te_msm_trim, free_dev); streams, events and the pinned block stay
  workset_t::each_buffer(ws, [](auto& b) { b.release(); });
  if (ws.h_ring) { (void)hipHostFree(ws.h_ring); ws.h_ring = nullptr; }       // the pinned ring of option "host_staging" (its events stay)
  ws.zero_words = ws.zero_clean_words = 0;
  ws.d_err = ws.d_num_seg = ws.d_size_hist = ws.d_size_cursor = ws.d_counts1 = ws.d_bucket_count = ws.d_part_ticket = nullptr; ws.d_partials = nullptr;
  ws.used = false;
}

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

// device copies of a host-buffer call's inputs, in bytes of the call's curve (64 + 32 per point for the Twisted-Edwards
// wire format, 96 + 48 for BLS12-377)
int ensure_staging(te_ctx* ctx, workset_t& ws, size_t bytes_points, size_t bytes_scalars) {
  if (int rc = make_room(ctx, ws.d_in_points, bytes_points)) return rc;
  return make_room(ctx, ws.d_in_scalars, bytes_scalars);
}
// The staging area may still be read by the set's previous MSM: the set's stream goes on behind it.  (ev_done exists from
// te_msm_init to te_msm_destroy, so `used` alone says whether there is a previous MSM -- as in begin_sequence.)
int wait_behind_previous(te_ctx* ctx, workset_t& ws) {
  if (ws.used) HIP_TRY(ctx, hipStreamWaitEvent(ws.stream, ws.ev_done, 0));
  return 0;
}

// Device-resident inputs of a call, and the peer pull that brings them from the memory of device src_dev into the staging area of a
// work set on another device of the context (tickets that land beside their inputs, the shares of run_bound_window_shards).
struct device_inputs { const void* scalars = nullptr; const void* points = nullptr; const uint32_t* idx = nullptr; };     // points / idx: where the call has them
struct peer_traffic { int64_t copies = 0, bytes = 0; };
// must device d pull what lies on src_dev?  ("stage_device_inputs": also when d IS the holder -- the one-GPU rehearsal)
bool must_pull(const te_ctx* ctx, const gpu_t& d, int src_dev) { return ctx->devs.size() > 1 && (d.device != src_dev || ctx->opt_stage_device_inputs); }
// The n entries of `in` over the peer link, on the set's stream; `in` then names the staging area.  moved: what was copied -- the caller
// adds it to the context's counters (plain integers: run_bound_window_shards pulls from one host thread per device and adds after the join).
int pull_inputs(te_ctx* ctx, const gpu_t& d, workset_t& ws, int src_dev, uint64_t n, device_inputs& in, peer_traffic& moved) {
  const curve_sizes sz = sizes_of(ctx->opt_curve);
  if (in.idx) { if (int rc = make_room(ctx, ws.d_in_idx, (size_t)n)) return rc; }
  if (int rc = ensure_staging(ctx, ws, in.points ? n * sz.point_in : 0, n * sz.scalar_in)) return rc;
  if (int rc = wait_behind_previous(ctx, ws)) return rc;
  HIP_TRY(ctx, hipMemcpyPeerAsync(ws.d_in_scalars, d.device, in.scalars, src_dev, n * sz.scalar_in, ws.stream));
  if (in.points) HIP_TRY(ctx, hipMemcpyPeerAsync(ws.d_in_points, d.device, in.points, src_dev, n * sz.point_in, ws.stream));
  if (in.idx) HIP_TRY(ctx, hipMemcpyPeerAsync(ws.d_in_idx, d.device, in.idx, src_dev, n * sizeof(uint32_t), ws.stream));
  moved.copies += 1 + (in.points != nullptr) + (in.idx != nullptr);
  moved.bytes += (int64_t)(n * (sz.scalar_in + (in.points ? sz.point_in : 0) + (in.idx ? sizeof(uint32_t) : 0)));
  in.scalars = ws.d_in_scalars;
  if (in.points) in.points = ws.d_in_points;
  if (in.idx) in.idx = ws.d_in_idx;
  return 0;
}
void note_peer_traffic(te_ctx* ctx, const peer_traffic& moved) { ctx->stat_peer_copies += moved.copies; ctx->stat_peer_bytes += moved.bytes; }

// Is this host address pinned (hipHostMalloc) or registered (hipHostRegister) memory?  A copy from such memory does not
// stage: hipMemcpyAsync returns before the data has left it.  Ordinary (pageable) memory is unknown to the runtime: the query
// fails with hipErrorInvalidValue or reports hipMemoryTypeUnregistered, depending on the ROCm version.
bool host_memory_is_pinned(const void* p) {
  hipPointerAttribute_t at; memset(&at, 0, sizeof at);
  if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
  return at.type == hipMemoryTypeHost;
}

// ---- option "host_staging" ------------------------------------------------------------------------------------------------
// A copy from pageable memory is fast only while the runtime still holds the caller's pages registered from an earlier copy
// of the SAME range: te_msm_run of 2^20 points takes 2.35 ms from buffers it has seen, 4.7-5.0 ms at the first touch of a
// buffer, and 4.4-27 ms when every call brings freshly allocated buffers (registration and the release of the previous
// buffers' registration sit on the call's critical path; eight threads touching new ranges at once serialise in it: round
// 4's "9.5 ms median" of the eight-device call -- profiles/r05_host_buffers_first_touch.txt, r05_point_shard_stamps_D8.txt).
// A prover that allocates its buffers per call never sees the fast case.  With "host_staging" = 1 the engine does not depend
// on the history of the caller's memory: the buffers are copied, 2 MB at a time, by a small crew of host threads into a pinned
// ring of the work set and travel from there; the call returns when the last chunk has left the caller's buffer.
constexpr size_t TE_RING_SLOT = 2u << 20;      // bytes per slot: 48 DMA calls per 96 MB, ~0.2 ms of enqueue cost
constexpr int TE_RING_SLOTS = 16;              // 32 MB pinned per work set that stages
// crew size: each thread copies ~5 GB/s into the ring while the DMA engine reads behind it (measurements:
// profiles/r05_host_staging_copy_ab.txt)
constexpr int TE_STAGERS = 8;
// chunk copy of the crew: the destination (a ring slot) is read next by the DMA engine, never by a core -- streaming stores keep it
// out of the caches and skip the read-for-ownership of every destination line
#if defined(__x86_64__)
__attribute__((target("avx2"))) void copy_streaming_avx2(uint8_t* to, const uint8_t* from, size_t len) {
  size_t i = 0;
  if ((reinterpret_cast<uintptr_t>(to) & 31u) == 0) {
    for (; i + 128 <= len; i += 128) {
      const __m256i a = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(from + i)), b = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(from + i + 32));
      const __m256i c = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(from + i + 64)), d = _mm256_loadu_si256(reinterpret_cast<const __m256i*>(from + i + 96));
      _mm256_stream_si256(reinterpret_cast<__m256i*>(to + i), a); _mm256_stream_si256(reinterpret_cast<__m256i*>(to + i + 32), b);
      _mm256_stream_si256(reinterpret_cast<__m256i*>(to + i + 64), c); _mm256_stream_si256(reinterpret_cast<__m256i*>(to + i + 96), d);
    }
    _mm_sfence();
  }
  if (i < len) memcpy(to + i, from + i, len - i);
}
#endif
void staging_chunk_copy(uint8_t* to, const uint8_t* from, size_t len) {
#if defined(__x86_64__)
  static const bool streaming = __builtin_cpu_supports("avx2");
  if (streaming) { copy_streaming_avx2(to, from, len); return; }
#endif
  memcpy(to, from, len);
}
int ensure_ring(te_ctx* ctx, workset_t& ws) {
  if (ws.h_ring) return 0;
  HIP_TRY(ctx, hipHostMalloc((void**)&ws.h_ring, TE_RING_SLOT * TE_RING_SLOTS, hipHostMallocDefault));
  if (ws.ring_ev.empty()) {
    ws.ring_ev.resize(TE_RING_SLOTS, nullptr);
    for (auto& e : ws.ring_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ws.ring_next = 0;
  return 0;
}
// the crew is shared by everything of the context that stages (its threads only ever run memcpy jobs); created under the
// context's error lock: the devices' host threads may get here together
int ensure_stagers(te_ctx* ctx) {
  std::lock_guard<std::mutex> lk(ctx->err_mu);
  while ((int)ctx->stagers.size() < TE_STAGERS) ctx->stagers.emplace_back(new te_sched::worker_t());
  return 0;
}
// dst (device) <- src (host), `bytes`, on `stream`, through the set's ring; returns when src has been read completely
int staged_copy(te_ctx* ctx, workset_t& ws, void* dst, const uint8_t* src, size_t bytes, hipStream_t stream) {
  if (int rc = ensure_ring(ctx, ws)) return rc;
  if (int rc = ensure_stagers(ctx)) return rc;
  struct pending_t { te_sched::job_ref job; te_sched::worker_t* who; int slot; size_t off, len; };
  std::deque<pending_t> fifo;
  auto flush_one = [&]() -> int {
    pending_t p = fifo.front(); fifo.pop_front();
    (void)p.who->wait(p.job);
    HIP_TRY(ctx, hipMemcpyAsync(static_cast<uint8_t*>(dst) + p.off, ws.h_ring + (size_t)p.slot * TE_RING_SLOT, p.len, hipMemcpyHostToDevice, stream));
    HIP_TRY(ctx, hipEventRecord(ws.ring_ev[(size_t)p.slot], stream));
    return 0;
  };
  // whatever happens, no crew thread may still be reading the caller's buffer when this function returns
  struct drain_t { std::deque<pending_t>& f; ~drain_t() { for (auto& p : f) (void)p.who->wait(p.job); } } drain_on_exit{fifo};
  for (size_t off = 0; off < bytes; off += TE_RING_SLOT) {
    const size_t len = std::min(TE_RING_SLOT, bytes - off);
    const size_t turn = ws.ring_next++;
    const int slot = (int)(turn % TE_RING_SLOTS);
    if ((int)fifo.size() >= std::min(TE_STAGERS, TE_RING_SLOTS - 4)) { if (int rc = flush_one()) return rc; }   // one chunk per crew thread filling, the rest of the ring draining
    if (turn >= (size_t)TE_RING_SLOTS) HIP_TRY(ctx, hipEventSynchronize(ws.ring_ev[(size_t)slot]));   // the slot's previous chunk has left it
    uint8_t* to = ws.h_ring + (size_t)slot * TE_RING_SLOT; const uint8_t* from = src + off;
    te_sched::worker_t* who = ctx->stagers[turn % (size_t)TE_STAGERS].get();
    fifo.push_back({who->post([to, from, len] { staging_chunk_copy(to, from, len); return 0; }), who, slot, off, len});
  }
  while (!fifo.empty()) { if (int rc = flush_one()) return rc; }
  return 0;
}
// every host-to-device copy of a caller's buffer goes through here
int upload(te_ctx* ctx, workset_t& ws, void* dst, const uint8_t* src, size_t bytes, hipStream_t stream) {
  if (ctx->opt_host_staging && bytes >= (256u << 10)) return staged_copy(ctx, ws, dst, src, bytes, stream);
  HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream));
  return 0;
}

// The uploads of a host-buffer MSM on work set `ws` (side stream) must not overtake the set's previous MSM, which may still read the
// staging area.  A marker on the set's stream and a stream wait say so -- but the marker is a packet in the hardware queue the set's
// stream shares with other work sets, and stands there behind THEIR kernels (a k_accumulate of 1.2-1.4 ms with eight tickets in flight):
// a third of the 32 MB scalar uploads of bound-bases tickets took 1.6-1.9 ms instead of 0.61 (TE_MSM_TRACE_HOST stamps,
// profiles/r06_bound_host_tickets_gap.txt).  A set whose previous MSM has delivered its result -- every ticket that was collected --
// needs no marker: everything that read the staging area precedes ev_result.
int copy_stream_behind_previous(te_ctx* ctx, workset_t& ws) {
  if (int rc = need_copy_stream(ctx, ws)) return rc;
  if (!ws.used) return 0;
  const hipError_t q = hipEventQuery(ws.ev_result);
  if (q == hipSuccess) return 0;
  (void)hipGetLastError();                                                        // hipErrorNotReady is an answer, not an error
  HIP_TRY(ctx, hipEventRecord(ws.ev_start, ws.stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ws.copy_stream, ws.ev_start, 0));
  return 0;
}

const char* const kFinalCarry = "final carry is 1: a scalar does not fit the signed window decomposition";

// "The kernels behind this point read what the upload recorded in `ev` (on the copy stream) brought."  Two forms:
//   the calling thread owns the call (te_msm_run*, te_msm_submit) and its buffers are PINNED: a stream wait -- nothing of the host is in
//     the MSM's critical path (pageable buffers: the host form as well, see caller_may_wait_on_host below);
//   a LANE thread enqueues an asynchronous ticket (wait_for_pinned == false): the thread itself waits for the upload and enqueues the
//     kernels afterwards.  A stream wait sits in the hardware queue of the work set's stream until the upload is over (2-3 ms with four
//     lanes sharing the link), and the runtime multiplexes the eight work-set streams onto four hardware queues, whose packets run in
//     order: the kernels of ANOTHER ticket that shares the queue stood behind that wait -- tickets from host scalars over bound bases
//     ran at 1.02-1.09 ms per MSM where the same tickets from device scalars take 0.89-0.92, with neither the link nor the device busy
//     (the round-6 lane measurement).  The lane thread has nothing else to do.
//     It waits for the copy STREAM, not for an event recorded behind the upload: an event record is one more packet in a hardware
//     queue the side stream shares with other work sets' streams, and stood behind their kernels for 0.5-0.7 ms in every fourth
//     ticket (stamps: "upload awaited"); the stream's last command -- the copy -- is known to the runtime without a packet.
// lane: the host form is wanted (a lane thread, or a calling thread whose copies have blocked anyway)
int lane_wait(te_ctx* ctx, workset_t& ws, hipEvent_t ev, bool lane) {
  if (lane) { HIP_TRY(ctx, hipStreamSynchronize(ws.copy_stream)); return 0; }
  HIP_TRY(ctx, hipEventRecord(ev, ws.copy_stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ws.stream, ev, 0));
  return 0;
}

// te_msm_run* / te_msm_submit (the calling thread uploads): from PAGEABLE memory hipMemcpyAsync returns when the copy is over, so
// waiting for the copy stream on the host costs nothing and keeps the event record and the stream wait out of the hardware queues
// as well: te_msm_run 2.30 vs 2.35 ms, te_msm_run_scalars 1.355 vs 1.38, te_msm_submit x8 in flight 1.90 vs 1.93-2.01 at 2^20;
// 0.78 vs 0.81, 0.573 vs 0.595, 0.555 vs 0.56-0.63 at 2^18 (profiles/r06_caller_host_waits.txt).
// Pinned sources keep the stream waits (their copies are asynchronous).
bool caller_may_wait_on_host(const void* a, const void* b) {
  return !(a && host_memory_is_pinned(a)) && !(b && host_memory_is_pinned(b));
}

// pieces a host buffer of n points is uploaded and processed in on ONE device (option "host_chunks", else from n).
// measured (tools/sweep_host_chunks.py, ms for 1 / 2 / 3 pieces): 2^17 0.672 / 0.659 / 0.773, 2^18 1.005 / 0.927 / 1.001,
// 2^19 1.642 / 1.407 / 1.424, 2^20 2.991 / 2.464 / 2.380
int host_pieces(const te_ctx* ctx, uint64_t n) {
  int K = ctx->opt_host_chunks ? ctx->opt_host_chunks : (n >= (3ull << 18) ? 3 : n >= (1ull << 17) ? 2 : 1);
  if ((uint64_t)K > n) K = (int)n;
  return K < 1 ? 1 : K;
}

// pieces the scalars of a bound point set are uploaded and processed in on ONE device (option "scalar_chunks", else from n)
int scalar_pieces(const te_ctx* ctx, uint64_t n) { return te_indexed::pieces(n, ctx->opt_scalar_chunks); }

// One MSM from HOST buffers (or one device's slice of it) on work set `ws` of device `d`, in one of two forms:
//   host points and scalars (`points`): both are uploaded, the points converted into the set's own record slab;
//   host scalars over a BOUND point set (`recs`, rec_kind: the form of the records): only the scalars travel.  `recs` are the records
//     of the slice's first point on this device -- or, with `idx` (te_msm_run_scalars_indexed*), the set's FIRST record: the slice is n
//     (index, scalar) pairs over a set of idx_count records, every piece carries its slice of both arrays and gathers records idx[j]
//     (msm_launch::idx); idx_pos: position of the slice's first pair in the caller's list.  The entry form follows the set's count,
//     everything else n (indexed_plan.hpp).
// The buffers are uploaded and processed in K pieces -- while piece i is on the GPU, piece i+1 crosses PCIe -- whose additions land on
// the SAME buckets, one reduction at the end, flag + rows on their way to the set's pinned block when the call returns.  Window bits
// are forced to c (the slices of a sharded MSM must agree on the geometry of their rows).  Does not wait: the caller synchronises
// ws.ev_result.  All windows, whatever the device's window shard says (host buffers always are whole MSMs or slices of one).
struct host_slice_req {
  const uint8_t* points = nullptr;      // host points -- or bound records:
  const uint8_t* recs = nullptr; int rec_kind = 0;
  const uint8_t* scalars = nullptr;     // host scalars
  uint64_t n = 0; int c = 0, K = 1;
  // the caller promises its buffers only until this call returns (te_msm_run*, te_msm_submit).  Copies from PAGEABLE memory have left
  // the caller's buffer when hipMemcpyAsync returns (the runtime stages them); from pinned or registered memory they are truly
  // asynchronous -- then the call waits for the last piece's upload before it returns.  false: a lane thread enqueues a ticket
  bool wait_for_pinned = true;
  const uint32_t* idx = nullptr; uint64_t idx_count = 0, idx_pos = 0;
  int scalar_form = -1;                 // plan_req's (a lane thread passes what its ticket was submitted with)
};
int enqueue_host_pieces(te_ctx* ctx, gpu_t& d, workset_t& ws, const host_slice_req& r) {
  HIP_TRY(ctx, hipSetDevice(d.device));
  const uint64_t n = r.n;
  const bool bound = r.points == nullptr;
  // what the plans of the whole slice and of every piece share; the pieces keep the slice's window bits and scalar form
  plan_req q = plan_whole(n); q.force_c = r.c; q.scalar_form = r.scalar_form;
  if (bound) { q.rec_kind = r.rec_kind; if (r.idx) q.idx_count = r.idx_count; }
  const plan_t pf = make_plan(ctx, d, q);
  q.force_c = pf.c; q.scalar_form = pf.scalar_mont;
  const curve_sizes sz = sizes_of(pf.curve);
  const size_t rec_bytes = rec_bytes_of(pf.curve, pf.rec_kind);
  if (int rc = ensure_staging(ctx, ws, bound ? 0 : n * sz.point_in, n * sz.scalar_in)) return rc;
  if (r.idx) { if (int rc = make_room(ctx, ws.d_in_idx, (size_t)n)) return rc; }
  const bool pinned_source = r.wait_for_pinned && !caller_may_wait_on_host(r.scalars, bound ? static_cast<const void*>(r.idx) : r.points);
  const bool host_waits = !pinned_source;
  uint8_t* dpts = static_cast<uint8_t*>(ws.d_in_points);
  uint8_t* dscs = static_cast<uint8_t*>(ws.d_in_scalars);
  // Pieces of n / K entries: piece i crosses PCIe on the side stream while piece i-1 is (converted and) ACCUMULATED ONTO THE SAME
  // BUCKETS on the main stream; one bucket reduction at the end.  (The first version ran every piece as a complete MSM with
  // its own reduction of all W x 2^(c-1) buckets: K reductions, which made more than four pieces a loss.)  Pageable copies
  // return once the data has left the caller's buffer, so the host alternates between staging a piece and enqueueing the
  // previous piece's kernels.
  // Measured (n = 2^20, tools/host_path.py, TE_MSM_TRACE_HOST=1, profiles/r03_host_buffer_path.txt): three equal pieces 2.48 ms,
  // two 2.56, four 2.59 (the device falls behind the uploads: every piece pays a sort and ~10 launches on a fraction of the
  // points), falling piece sizes 2.51-2.56 (profiles/r06_host_split_experiment.txt: equal thirds confirmed); the link alone needs 1.85 ms.
  int K = r.K < 1 ? 1 : r.K;
  if ((uint64_t)K > n) K = (int)n;                                         // no piece is empty: the last one ends the sequence
  auto piece_lo = [&](int i) -> uint64_t { return te_indexed::piece_lo(n, K, i); };     // first entry of piece i
  uint64_t m_max = 0;
  for (int i = 0; i < K; i++) m_max = std::max(m_max, piece_lo(i + 1) - piece_lo(i));
  {
    q.n = m_max;
    const plan_t pm = make_plan(ctx, d, q);
    q.force_seg = pm.seg_len;                                              // the pieces share the geometry (and the buffers) of the largest
    if (int rc = ensure_buffers(ctx, d, ws, m_max, pm, !bound)) return rc;    // every buffer at its final size before the first piece
  }
  // what every piece's launch shares; the piece sets its plan, its inputs and `onto`
  msm_launch L0(ctx, ws, pf, n, ws.stream);
  L0.d_partials_out = ws.d_partials; L0.own_rows = true;
  if (int rc = begin_sequence(d, L0, bound ? nullptr : ws.d_recs.p)) return rc;     // host points are converted into the set's own slab
  if (int rc = copy_stream_behind_previous(ctx, ws)) return rc;            // the staging area may still be read by the set's previous MSM
  // host stamps of every piece (stderr), one line format per form: tools/stamp_summary.py and tools/trace_point_shards.py parse them.
  // (host points: index of the device in the context's list / its HIP id; the absolute time tells the threads of one call apart from the next call's)
  const bool tr = getenv("TE_MSM_TRACE_HOST") != nullptr;
  const auto t00 = std::chrono::steady_clock::now();
  auto stamp = [&](const char* what, int i) {
    if (!tr) return;
    const auto now = std::chrono::steady_clock::now();
    const double us = std::chrono::duration<double, std::micro>(now - t00).count();
    if (bound) fprintf(stderr, "[scalar slice ws %d] %8.1f us  %s %d\n", (int)(&ws - d.ws), us, what, i);
    else fprintf(stderr, "[te_msm_run dev %d/%d] %8.1f us  %s %d   (t = %.1f us)\n", (int)(&d - ctx->devs.data()), d.device, us, what, i,
                 std::chrono::duration<double, std::micro>(now.time_since_epoch()).count());
  };
  std::vector<hipEvent_t>& evs = ws.piece_events;
  while ((int)evs.size() < K + 1) { hipEvent_t e; HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming)); evs.push_back(e); }
  auto upload_scalars = [&](uint64_t lo, uint64_t m) -> int {
    return upload(ctx, ws, dscs + lo * sz.scalar_in, r.scalars + lo * sz.scalar_in, m * sz.scalar_in, ws.copy_stream);
  };
  // Host points on Twisted-Edwards: ALL scalars first, in one copy (a third of the bytes): every extra pageable copy call costs ~43 us
  // of pipeline drain (six calls for three pieces ended at 2.02 ms where one pair of calls takes 1.85), and with the scalars there the
  // sort of piece i + 1 is enqueued behind piece i's accumulation and runs while piece i + 1's points are still crossing PCIe.
  // (There the link is the bottleneck.  BLS12-377 -- 144 MB to upload, but 2.0 ms of accumulation -- is bound by the device, which
  // must not sit idle while 48 MB of scalar records arrive: piece by piece, 4.1 against 4.7 ms.)
  const bool scalars_first = !bound && pf.curve == TE_MSM_CURVE_TE_BLS12;
  if (scalars_first) {
    if (int rc = upload_scalars(0, n)) return rc;
    if (int rc = lane_wait(ctx, ws, evs[(size_t)K], host_waits)) return rc;
    stamp("scalars staged", -1);
  }
  plan_t p;
  for (int i = 0; i < K; i++) {
    const uint64_t lo = piece_lo(i), m = piece_lo(i + 1) - lo;
    if (bound) {
      std::unique_lock<std::mutex> link(*d.scalar_link, std::defer_lock);
      if (!r.wait_for_pinned) link.lock();                                   // (a lane thread: see gpu_t::scalar_link)
      stamp("upload begins", i);
      if (r.idx) { if (int rc = upload(ctx, ws, ws.d_in_idx + lo, reinterpret_cast<const uint8_t*>(r.idx + lo), m * sizeof(uint32_t), ws.copy_stream)) return rc; }
      if (int rc = upload_scalars(lo, m)) return rc;
      stamp("upload call returned", i);
      if (int rc = lane_wait(ctx, ws, evs[(size_t)i], host_waits)) return rc;
      stamp("upload awaited", i);
    }
    q.n = m;
    p = make_plan(ctx, d, q);
    if (int rc = ensure_buffers(ctx, d, ws, m, p, !bound)) return rc;        // no reallocation: only the pointers into the zeroed block move
    msm_launch L = L0;
    L.p = p; L.d_scalars = dscs + lo * sz.scalar_in; L.n = m; L.onto = i > 0;
    if (!bound) L.d_points = dpts + lo * sz.point_in;
    else if (!r.idx) L.bound = r.recs + lo * rec_bytes;
    else { L.bound = r.recs; L.idx = ws.d_in_idx + lo; L.idx_count = (uint32_t)r.idx_count; L.idx_pos = (uint32_t)(r.idx_pos + lo); }
    if (!bound && !scalars_first) {
      if (int rc = upload_scalars(lo, m)) return rc;
      if (int rc = lane_wait(ctx, ws, evs[(size_t)K], host_waits)) return rc;
      stamp("scalars staged", i);
    }
    if (int rc = L.front_scalars()) return rc;                               // host points: digits, sort and schedule run while the piece's points cross PCIe
    if (!bound) {
      stamp("scalar stages enqueued", i);
      if (int rc = upload(ctx, ws, dpts + lo * sz.point_in, r.points + lo * sz.point_in, m * sz.point_in, ws.copy_stream)) return rc;
      stamp("points staged", i);
      if (int rc = lane_wait(ctx, ws, evs[(size_t)i], host_waits)) return rc;
      if (int rc = L.front_points()) return rc;
    }
    if (int rc = L.accumulate()) return rc;
    if (int rc = L.combine()) return rc;
    if (i == K - 1) { if (int rc = L.reduce()) return rc; }
    stamp("piece enqueued", i);
  }
  note_sequence(d, ws, p, piece_lo(K) - piece_lo(K - 1), ws.stream, 0);
  if (int rc = fetch_rows(ctx, ws, ws.stream)) return rc;
  HIP_TRY(ctx, hipGetLastError());
  if (pinned_source && !ctx->opt_host_staging) {
    // everything on the copy stream is ordered: the last recorded upload event covers the scalars and every piece
    HIP_TRY(ctx, hipEventSynchronize(evs[(size_t)K - 1]));
    if (!bound) stamp("pinned source: uploads awaited", -1);
  }
  return 0;
}

// ---- fixed-base windows (kernels.hip.hpp, "FIXED-BASE WINDOWS"): the plan of an MSM over a bound set that carries a per-window table.
// The sort / accumulation / reduction see fb_rb + 1 pseudo-windows ("rows") of 2^15 buckets and `cap` entries each: an unsigned
// geometry (codes lo + 1, half = 0), general sort entries (the table index needs 24 bits).
constexpr uint32_t FB_LOBITS = TE_FB_LOBITS;
int fb_windows_for(int c) { return te_fb::windows_for(c); }
// (the arithmetic -- rows, capacity, chunks, default segment length -- is te_fb::make_geometry, fb_plan.hpp; returned for the caller's
// refusal, `half` and the digit kernel's LDS size)
te_fb::geometry make_plan_fb(const te_ctx* ctx, const gpu_t& d, uint64_t n, int fb_c, plan_t& p, int scalar_form = -1) {
  const te_fb::geometry g = te_fb::make_geometry(n, fb_c, TE_SCATTER_BLOCKS, TE_SCATTER_MINCHUNK);
  plan_req q = plan_whole(g.cap); q.force_c = 16; q.scalar_form = scalar_form;
  p = make_plan(ctx, d, q);                                         // curve, scalar form, options for rows of `cap` entries
  p.fb_rb = (int)g.rb; p.fb_c = fb_c; p.fb_W = g.W;
  p.signed_digits = 0; p.c = (int)FB_LOBITS; p.W = (int)g.rows; p.nw = p.nw1 = (int)g.rows; p.batch = 1; p.w_first = 0; p.w_step = 1;
  p.logB = FB_LOBITS; p.B = 1u << FB_LOBITS;
  for (int k = 0; k < 4; k++) p.dw[k] = (p.logB + 3u - (uint32_t)k) / 4u;
  p.S = g.S; p.P = g.P; p.logS = g.logS;
  p.packed = 0; p.rec_kind = 0;
  p.nst = (uint32_t)g.cap;
  p.chunk_len = g.chunk_len;
  p.CH = g.CH;
  if (!ctx->opt_seg_len) p.seg_len = g.seg_len;
  return g;
}

template <int C, int FORM> void launch_fb_digits(const void* d_scalars, const te::fb_digit_args& a, uint32_t n, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL((te::k_fb_digits<C, FORM>), dim3((n + TE_FB_THREADS - 1u) / TE_FB_THREADS), dim3(TE_FB_THREADS), lds, st, static_cast<const uint4*>(d_scalars), a);
}

// An MSM of n scalars (device memory) over the fixed-base table of `bases` on device `d`: the scalars' digits address the table
// entries (w, idx_base + i) -- idx_base: the first point of this launch inside the bound set (a device's slice of a lone
// multi-device call).  Rows in the set's own block; the caller ends the sequence with fetch_rows().  scalar_form: plan_req's.
int enqueue_fixed_base(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases, const void* d_scalars, uint64_t n, uint64_t idx_base, hipStream_t stream,
                       int scalar_form = -1) {
  HIP_TRY(ctx, hipSetDevice(d.device));
  plan_t p; const te_fb::geometry g = make_plan_fb(ctx, d, n, bases->fb_c, p, scalar_form);
  const uint64_t cap = p.nst;
  if (te_fb::msm_refused(g, bases->n))
    return set_err(ctx, TE_MSM_EINVAL, "fixed-base windows: windows x points must stay below 2^31");
  if (int rc = ensure_buffers(ctx, d, ws, cap, p, false)) return rc;
  msm_launch L(ctx, ws, p, cap, stream);
  L.d_scalars = d_scalars; L.d_partials_out = ws.d_partials; L.own_rows = true; L.prof = ctx->opt_profile;
  if (int rc = begin_sequence(d, L, nullptr)) return rc;
  note_sequence(d, ws, p, cap, stream, ctx->opt_profile);
  ws.fb_scalars = d_scalars; ws.fb_n = n;
  L.bound = bases->recs[(size_t)(&d - ctx->devs.data())];
  L.fb_remap = ws.d_fb_remap;
  // the zeroed block (flags, counters, level-1 histogram, row fill) -- then the digits.  The digit rows are NOT cleared: the sort's
  // first level reads every row only up to its fill (scatter_args.row_fill)
  if (ws.zero_clean_words < ws.zero_words) HIP_TRY(ctx, hipMemsetAsync(ws.d_zero, 0, ws.zero_words * sizeof(uint32_t), stream));
  ws.zero_clean_words = ws.zero_words;                                  // front_scalars below must not clear it again (it would wipe the histogram)
  L.mark(ST_DIGITS);
  {
    te::fb_digit_args a; memset(&a, 0, sizeof a);
    memcpy(a.half, g.half, sizeof a.half);
    a.n = (uint32_t)n; a.idx_base = (uint32_t)idx_base; a.n_table = (uint32_t)bases->n; a.W = (uint32_t)p.fb_W;
    a.rows = (uint32_t)p.nw; a.rb = (uint32_t)p.fb_rb; a.cap = (uint32_t)cap;
    a.chunk_len = p.chunk_len; a.CH = p.CH; a.P = p.P; a.logS = p.logS;
    a.digits = ws.d_digits; a.remap = ws.d_fb_remap; a.row_fill = ws.d_fb_fill; a.counts1 = ws.d_counts1; a.err = ws.d_err;
    const size_t lds = g.lds_bytes;
    // (fixed-base sets exist on the Twisted-Edwards curve only: the one Montgomery form here is modulo L)
    if (p.scalar_mont) with_window_bits<16, 21>(p.fb_c, [&](auto C) { launch_fb_digits<decltype(C)::value, te::SCALAR_FORM_TE>(d_scalars, a, a.n, lds, stream); });
    else with_window_bits<16, 21>(p.fb_c, [&](auto C) { launch_fb_digits<decltype(C)::value, te::SCALAR_FORM_CANONICAL>(d_scalars, a, a.n, lds, stream); });
  }
  // the engine's own stages from here on (front_scalars skips k_digits for a fixed-base plan)
  if (int rc = L.front_scalars()) return rc;
  L.mark(ST_PREP);
  if (int rc = L.accumulate()) return rc;
  L.mark(ST_TREE);
  if (int rc = L.back()) return rc;
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

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
const char* const kAllSetsOwned = "every work set holds a submitted MSM that has not been collected: te_msm_collect one first";
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
// The status of the MSM whose flag words are in the set's pinned block (ev_result has passed): its entries noted, an index outside
// the bound set reported (bit 1 of word 0: only the indexed first-level scatter sets it -- the fixed-base overflow is word 1 alone),
// else the final carry.  entries_of_failed = false (te_msm_finalize): a failed MSM leaves "entries_accumulated" as it was.
int settle_status(te_ctx* ctx, const workset_t& ws, bool entries_of_failed = true) {
  if (entries_of_failed || !*ws.h_err) note_entries(ctx, ws);
  if (const int64_t bad = bad_index_of(ws); bad >= 0) return note_bad_index(ctx, bad);
  if (*ws.h_err) return set_err(ctx, TE_MSM_ESCALAR, kFinalCarry);
  return 0;
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
int run_host_sharded(te_ctx* ctx, const uint8_t* src_points, const uint8_t* src_scalars, uint64_t n, uint8_t* out, const te_bases* bases = nullptr,
                     const uint32_t* src_idx = nullptr) {
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
    host_slice_req r; r.scalars = src_scalars + lo * sz.scalar_in; r.n = hi - lo; r.c = p0.c; r.K = K;
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
    if (int rc = ensure_staging(ctx, ws, n * sz.point_in, n * sz.scalar_in)) return rc;
    if (int rc = wait_behind_previous(ctx, ws)) return rc;
    const uint64_t lo = lo_of(i), m = lo_of(i + 1) - lo;
    if (m) {
      HIP_TRY(ctx, hipMemcpyPeerAsync(static_cast<uint8_t*>(ws.d_in_points) + lo * sz.point_in, d.device, sp + lo * sz.point_in, src_dev, m * sz.point_in, ws.stream));
      HIP_TRY(ctx, hipMemcpyPeerAsync(static_cast<uint8_t*>(ws.d_in_scalars) + lo * sz.scalar_in, d.device, ss + lo * sz.scalar_in, src_dev, m * sz.scalar_in, ws.stream));
      ctx->stat_peer_copies += 2; ctx->stat_peer_bytes += (int64_t)(m * (sz.point_in + sz.scalar_in));
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
        HIP_TRY(ctx, hipMemcpyPeerAsync(static_cast<uint8_t*>(ws.d_in_scalars) + lo * sz.scalar_in, d.device, fs + lo * sz.scalar_in, o.device, m * sz.scalar_in, ws.stream));
        copies[i] += 2; bytes[i] += (int64_t)(m * (sz.point_in + sz.scalar_in));
      }
      dp = ws.d_in_points; ds = ws.d_in_scalars;
    }
    partial_req r; r.d_points = dp; r.d_scalars = ds; r.n = n; r.stream = ws.stream;
    if (int rc = enqueue_partial(ctx, d, ws, r)) return rc;
    return fetch_rows(ctx, ws, ws.stream);
  };
  const int rc = te_sched::on_devices(*ctx, nd, share);
  // a device whose staging area other devices read must not reuse it before they are done: every set's next MSM waits for
  // its own ev_done only, so the call ends with all of them complete (settle_window_shards) -- the copies are over by then
  for (size_t i = 0; i < nd; i++) { ctx->stat_peer_copies += copies[i]; ctx->stat_peer_bytes += bytes[i]; }
  return settle_window_shards(ctx, wsel, p0, rc, true, out);
}

// ---- input-point validation (option "check_points", te_msm_check_points*; kernels in check.hip.hpp) ----------------------------
// Runs on device devs[di] in front of whatever the call does with the points, and waits for its verdict: a point that fails must
// stop the call before an MSM result exists.  Device-resident points are checked where they lie (one launch per check); host points
// cross PCIe in pieces of kCheckPiece through the device's own buffer -- the same bytes the MSM uploads again afterwards: checking is
// opt-in and priced in the header.  The report word takes the lowest failing index of a launch (check_code); pieces run in order,
// so the first piece that reports holds the lowest index of the whole buffer.
constexpr uint64_t kCheckPiece = 1ull << 18;

// The check lane of a device (its stream, report word and pinned host word: check_points_on, recover_on, mul_on), held while this
// lives: chk_mu locked, the device made current, the three created on first use.  rc: 0, or the HIP error (noted) that left it unusable.
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
 private:
  static int open(te_ctx* ctx, gpu_t& d) {
    HIP_TRY(ctx, hipSetDevice(d.device));
    if (!d.chk_stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&d.chk_stream, hipStreamNonBlocking));
    if (!d.chk_word) HIP_TRY(ctx, hipMalloc(&d.chk_word, sizeof(unsigned long long)));
    if (!d.chk_host) HIP_TRY(ctx, hipHostMalloc(&d.chk_host, sizeof(unsigned long long), hipHostMallocDefault));
    return 0;
  }
};

// mont: the coordinates are Montgomery residues (option "points_montgomery": te_msm_bind_points*, te_msm_check_points*); every per-call
// check of an MSM or a multiplication reads canonical coordinates
int check_points_on(te_ctx* ctx, size_t di, const void* src, bool src_is_host, uint64_t n, int curve, int level, int64_t* bad, int* reason, bool mont = false) {
  *bad = -1; *reason = 0;
  if (n == 0) return 0;
  gpu_t& d = ctx->devs[di];
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  const size_t pb = sizes_of(curve).point_in;
  const uint64_t piece = src_is_host ? std::min(n, kCheckPiece) : n;
  if (src_is_host) { if (int rc = make_room(ctx, d.chk_pts, piece * pb)) return rc; }
  hipStream_t st = lane.stream();
  for (uint64_t off = 0; off < n; off += piece) {
    const uint32_t m = (uint32_t)std::min(piece, n - off);
    const uint8_t* at = static_cast<const uint8_t*>(src) + off * pb;
    if (src_is_host) { HIP_TRY(ctx, hipMemcpyAsync(d.chk_pts, at, (size_t)m * pb, hipMemcpyHostToDevice, st)); at = d.chk_pts; }
    const uint4* p4 = reinterpret_cast<const uint4*>(at);
    HIP_TRY(ctx, hipMemsetAsync(d.chk_word, 0, sizeof(unsigned long long), st));
    const dim3 grid((m + 255u) / 256u), block(256);
    if (mont && curve == TE_MSM_CURVE_BLS12_377_G1) {
      hipLaunchKernelGGL((te::k_check_form<1, true>), grid, block, 0, st, p4, m, d.chk_word);
      if (level >= 2) hipLaunchKernelGGL((te::k_check_subgroup<1, true>), grid, block, 0, st, p4, m, d.chk_word, te::kNaf377Order);
    } else if (mont) {
      hipLaunchKernelGGL((te::k_check_form<0, true>), grid, block, 0, st, p4, m, d.chk_word);
      if (level >= 2) hipLaunchKernelGGL((te::k_check_subgroup<0, true>), grid, block, 0, st, p4, m, d.chk_word, te::kNafTeOrder);
    } else if (curve == TE_MSM_CURVE_BLS12_377_G1) {
      hipLaunchKernelGGL(te::k_check_form<1>, grid, block, 0, st, p4, m, d.chk_word);
      if (level >= 2) hipLaunchKernelGGL(te::k_check_subgroup<1>, grid, block, 0, st, p4, m, d.chk_word, te::kNaf377Order);
    } else {
      hipLaunchKernelGGL(te::k_check_form<0>, grid, block, 0, st, p4, m, d.chk_word);
      if (level >= 2) hipLaunchKernelGGL(te::k_check_subgroup<0>, grid, block, 0, st, p4, m, d.chk_word, te::kNafTeOrder);
    }
    HIP_TRY(ctx, hipGetLastError());
    int64_t i = -1;
    const int rc = lane.verdict(ctx, m, &i, reason);
    if (rc == TE_MSM_EPOINT) *bad = (int64_t)off + i;
    if (rc) return rc;
  }
  return 0;
}
// A failed check (kBadPoint) or recovery (kBadX, x-only points) as the outcome of a call: the failure is remembered for get_option
// ("bad_point_index" / "bad_point_reason"), described in the error text and written to the caller's outputs where given.
enum bad_kind { kBadPoint, kBadX };
int note_bad(te_ctx* ctx, bad_kind kind, int64_t index, int reason, int64_t* first_bad = nullptr, int* reason_out = nullptr) {
  ctx->bad_point_index = index; ctx->bad_point_reason = reason;
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
int check_call(te_ctx* ctx, size_t di, const void* src, bool src_is_host, uint64_t n, bool mont = false) {
  if (!ctx->opt_check_points) return 0;
  int64_t bad = -1; int reason = 0;
  const int rc = check_points_on(ctx, di, src, src_is_host, n, ctx->opt_curve, ctx->opt_check_points, &bad, &reason, mont);
  if (rc == TE_MSM_EPOINT) return note_bad(ctx, kBadPoint, bad, reason);
  return rc;
}

// te_msm_run_x and te_msm_mul* read canonical scalars only: with option "scalars_montgomery" set they are refused (a silent canonical
// reading would be a wrong answer)
const char* const kNoMontgomeryScalars = "option \"scalars_montgomery\" is set: te_msm_run_x and te_msm_mul* take canonical scalars only";
int check_n(te_ctx* ctx, uint64_t n) { return n >= (1ull << 31) ? set_err(ctx, TE_MSM_EINVAL, "n must be < 2^31") : 0; }

// share: how a single-device call from device-resident points keeps its records (share_mode; x-only points: SHARE_CONVERT)
int run_common(te_ctx* ctx, const void* src_points, const void* src_scalars, bool src_is_host, uint64_t n, uint8_t out[64], share_mode share = SHARE_RUN) {
  if (!ctx || !out) return TE_MSM_EINVAL;
  if (int rc = check_n(ctx, n)) return rc;
  if (n == 0) { write_identity(ctx->opt_curve, out); return 0; }
  if (!src_points || !src_scalars) return set_err(ctx, TE_MSM_EINVAL, "null input buffer");
  // (device-resident inputs live on the first device: a multi-device call checks them there, before the scatter)
  if (int rc = check_call(ctx, 0, src_points, src_is_host, n)) return rc;
  const size_t nd = ctx->devs.size();
  // several devices: host buffers -> slices of the points, one upload thread per device; device-resident inputs -> window shards
  if (nd > 1) {
    if (src_is_host) return run_host_sharded(ctx, static_cast<const uint8_t*>(src_points), static_cast<const uint8_t*>(src_scalars), n, out);
    return run_device_window_shards(ctx, src_points, src_scalars, n, out);
  }
  gpu_t& d = ctx->devs[0];
  if (src_is_host && !ctx->opt_profile && ctx->opt_workset == 0 && d.w_step == 1 && d.in_flight == 0) {
    // no tickets in flight, no stage timing requested: every work set is free for the pieces
    const int K = host_pieces(ctx, n);
    if (K > 1) return run_host_chunked(ctx, static_cast<const uint8_t*>(src_points), static_cast<const uint8_t*>(src_scalars), n, K, out);
  }
  const int wsel = lone_set(ctx, d, ctx->opt_workset);
  if (wsel < 0) return wsel;
  const plan_t p0 = make_plan(ctx, d, plan_shard(n));
  const curve_sizes sz = sizes_of(p0.curve);
  workset_t& ws = d.ws[wsel];
  HIP_TRY(ctx, hipSetDevice(d.device));
  const void *dp = src_points, *ds = src_scalars;
  if (src_is_host) {
    if (int rc = ensure_staging(ctx, ws, n * sz.point_in, n * sz.scalar_in)) return rc;
    // scalars first; the points follow from inside enqueue_partial (pageable copies return when the data has left
    // the caller's buffer, so the scalar-only stages enqueued in between run while the points are still in flight)
    if (int rc = upload(ctx, ws, ws.d_in_scalars, static_cast<const uint8_t*>(src_scalars), n * sz.scalar_in, ws.stream)) return rc;
    dp = ws.d_in_points; ds = ws.d_in_scalars;
  }
  const std::function<int(hipStream_t)> upload_points = [&](hipStream_t side) -> int {
    // on the side stream, beside the scalar-only kernels on ws.stream; the conversion to records follows it there
    return upload(ctx, ws, ws.d_in_points, static_cast<const uint8_t*>(src_points), n * sz.point_in, side);
  };
  partial_req r; r.d_points = dp; r.d_scalars = ds; r.n = n; r.stream = ws.stream;
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

}  // namespace

// ================================================================================================ C-ABI
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
    if (er == hipSuccess)                // k_reduce_tail keeps up to 256 + 16 points in LDS (39 KB / 61 KB)
      er = hipFuncSetAttribute(reinterpret_cast<const void*>(te::k_reduce_tail<9>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
    if (er == hipSuccess)
      er = hipFuncSetAttribute(reinterpret_cast<const void*>(te::k_reduce_tail<14>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
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
// The work set a new ticket is opened on, as every submit form uses it: index of its device in ctx->devs, the device, the set.
struct ticket_set { int di; gpu_t& d; workset_t& ws; };
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
// option "check_points" (level) on the points of a ticket, on device ci: 0 = go on; TE_MSM_EPOINT = the ticket's outcome, kept in the
// set for te_msm_collect (nothing is enqueued for the ticket); else a device error
int check_ticket(te_ctx* ctx, workset_t& ws, size_t ci, const void* src, bool src_is_host, uint64_t n, int curve, int level) {
  if (!level) return 0;
  ws.pt_rc = check_points_on(ctx, ci, src, src_is_host, n, curve, level, &ws.pt_index, &ws.pt_reason);
  const int rc = ws.pt_rc;
  if (rc != TE_MSM_EPOINT) ws.pt_rc = 0;
  return rc;
}
// the status of a ticket's job on an upload lane; the error text of a failure is kept in the set for te_msm_collect (TE_MSM_EPOINT
// is reported from the set's pt_index / pt_reason)
int lane_status(te_ctx* ctx, workset_t& ws, int rc) {
  if (rc && rc != TE_MSM_EPOINT) { std::lock_guard<std::mutex> lk(ctx->err_mu); ws.job_err = ctx->err; }
  return rc;
}
// bound: the point set the ticket gathers from (te_msm_submit_scalars*) -- it cannot be released before the collect (retire_ticket)
void hand_out_ticket(te_ctx* ctx, const ticket_set& t, uint64_t* ticket, te_bases* bound = nullptr, te_sched::job_ref job = nullptr) {
  if (bound) { t.ws.bound = bound; bound->in_flight++; }
  te_sched::hand_out(*ctx, t.di, t.ws, ticket, std::move(job));      // te_msm_ticket_wait looks the ticket up from other threads
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
int pull_for_ticket(te_ctx* ctx, const ticket_set& t, int owner, uint64_t n, device_inputs& in, bool* pulled = nullptr) {
  const int src_dev = ctx->devs[(size_t)owner].device;
  const bool pull = must_pull(ctx, t.d, src_dev);
  if (pulled) *pulled = pull;
  if (!pull) return 0;
  peer_traffic moved;
  if (int rc = pull_inputs(ctx, t.d, t.ws, src_dev, n, in, moved)) return rc;
  note_peer_traffic(ctx, moved);
  return 0;
}
const char* const kNoTicket = "no such ticket in flight (already collected, or never handed out)";
int fixed_base_settle(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases);     // (resident bases, further down)
}  // namespace

int te_msm_submit_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n, uint64_t* ticket) {
  device_guard restore_callers_device;
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (!d_points_xy_le || !d_scalars_le || n == 0 || n >= (1ull << 31)) return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
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
  if (int rc = pull_for_ticket(ctx, t, owner, n, in, &pull)) return rc;
  // a single-device context keeps its window shard (te_msm_set_window_shard); on several devices a ticket is a whole MSM
  partial_req r; r.d_points = in.points; r.d_scalars = in.scalars; r.n = n; r.stream = t.ws.stream; r.whole = multi; r.share = pull ? SHARE_NONE : SHARE_RUN;
  if (int rc = enqueue_partial(ctx, t.d, t.ws, r)) return rc;
  if (int rc = fetch_rows(ctx, t.ws, t.ws.stream)) return rc;
  hand_out_ticket(ctx, t, ticket);
  return 0;
}

namespace {
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

// An asynchronous ticket: `enqueue` (the upload and the launches of one whole MSM; 0 or an error already noted) runs on an upload lane
// of the ticket's device, and the call returns at once -- D of them keep D links busy.  The job's status, and the error text of a failure,
// stay with the set for te_msm_collect (lane_status).  The job reads the context's options as they are NOW only by accident of timing
// -- so te_msm_set_option waits for the host threads first (drain_workers); what the enqueue depends on is fixed by its captures.
// (a template inside the C-ABI block: C++ linkage said by name)
extern "C++" template <typename F> te_sched::job_ref post_to_lane(te_ctx* ctx, const ticket_set& t, F enqueue) {
  t.ws.job_err.clear();
  warm_upload_lanes(ctx);                            // (once per process and device: all of the context's devices together)
  workset_t* wsp = &t.ws;
  return te_sched::next_lane_of(*ctx, (size_t)t.di, ctx->opt_upload_threads).post([ctx, wsp, enqueue]() -> int { return lane_status(ctx, *wsp, enqueue()); });
}

int submit_host(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, uint64_t* ticket, bool async) {
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (!points_xy_le || !scalars_le || n == 0 || n >= (1ull << 31)) return set_err(ctx, TE_MSM_EINVAL, "bad arguments");
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
  r.wait_for_pinned = false; r.scalar_form = pf.scalar_mont;
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

// ---- resident bases (include/te_msm.h): points bound once, scalars per call ---------------------------------------------------
namespace {
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

// The records of the set on device i: raw points -> (temporary) -> records, on a stream of its own; returns when they are there.
// src on the host: the device's own upload (D devices: D links side by side, one host thread each); src on a device of the
// context: read in place on its holder, pulled over the peer link elsewhere.
// mont: the raw coordinates are Montgomery residues (option "points_montgomery"): the conversion's other instantiation, the same records.
int bind_on_device(te_ctx* ctx, te_bases* b, size_t i, const void* src, bool src_is_host, int src_dev, bool mont) {
  gpu_t& d = ctx->devs[i];
  HIP_TRY(ctx, hipSetDevice(d.device));
  const curve_sizes sz = sizes_of(b->curve);
  const uint64_t n = b->n;
  uint8_t* recs = nullptr; void* raw = nullptr; void* proj = nullptr; hipStream_t st = nullptr;
  struct cleanup_t { void*& raw; void*& proj; hipStream_t& st; ~cleanup_t() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } if (raw) (void)hipFree(raw); if (proj) (void)hipFree(proj); } } cleanup{raw, proj, st};
  HIP_TRY(ctx, hipMalloc((void**)&recs, (size_t)n * b->rec_bytes * (size_t)(b->fb_c ? b->fb_W : 1)));
  b->recs[i] = recs;                                                       // (freed by the caller on failure: free_bases)
  HIP_TRY(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  const void* pts = src;
  if (src_is_host) {
    HIP_TRY(ctx, hipMalloc(&raw, (size_t)n * sz.point_in));
    HIP_TRY(ctx, hipMemcpyAsync(raw, src, (size_t)n * sz.point_in, hipMemcpyHostToDevice, st));
    pts = raw;
  } else if (src_dev != d.device || ctx->opt_stage_device_inputs) {
    HIP_TRY(ctx, hipMalloc(&raw, (size_t)n * sz.point_in));
    HIP_TRY(ctx, hipMemcpyPeerAsync(raw, d.device, src, src_dev, (size_t)n * sz.point_in, st));
    { std::lock_guard<std::mutex> lk(ctx->err_mu); ctx->stat_peer_copies += 1; ctx->stat_peer_bytes += (int64_t)(n * sz.point_in); }
    pts = raw;
  }
  const uint32_t n32 = (uint32_t)n;
  te::batch_ptrs tab; te::batch_slabs row_slab; memset(&tab, 0, sizeof tab); memset(&row_slab, 0, sizeof row_slab);
  tab.p[0] = (const uint4*)pts;
  if (b->curve == TE_MSM_CURVE_BLS12_377_G1) {
    te::rec_slot<14>* pr = reinterpret_cast<te::rec_slot<14>*>(recs);
    if (b->rec_kind == 1) { HIP_TRY(ctx, hipMalloc(&proj, (size_t)n * sizeof(te::rec_slot<14>))); pr = static_cast<te::rec_slot<14>*>(proj); }
    if (mont) hipLaunchKernelGGL(te::k_prep_points377<true>, dim3((n32 + 255) / 256, 1), dim3(256), 0, st, tab, row_slab, pr, n32);
    else hipLaunchKernelGGL(te::k_prep_points377<false>, dim3((n32 + 255) / 256, 1), dim3(256), 0, st, tab, row_slab, pr, n32);
    if (b->rec_kind == 1) {
      const uint32_t groups = (n32 + TE_AFF_GROUP - 1u) / TE_AFF_GROUP;
      hipLaunchKernelGGL(te::k_affine377, dim3((groups + 255) / 256), dim3(256), 0, st, pr, reinterpret_cast<te::rec_aff377*>(recs), n32);
    }
  } else if (mont) {
    hipLaunchKernelGGL(te::k_prep_points<true>, dim3((n32 + 255) / 256, 1), dim3(256), 0, st, tab, row_slab, reinterpret_cast<te::pnt_slot*>(recs), n32);
  } else {
    hipLaunchKernelGGL(te::k_prep_points<false>, dim3((n32 + 255) / 256, 1), dim3(256), 0, st, tab, row_slab, reinterpret_cast<te::pnt_slot*>(recs), n32);
  }
  if (b->fb_c) {
    // fixed-base windows: table w = the records of 2^(c w) P_i; the extended points travel from window to window by c doublings
    HIP_TRY(ctx, hipMalloc(&proj, (size_t)n * sizeof(te::ete)));       // (the second temporary: unused on this curve otherwise)
    te::ete* ext = static_cast<te::ete*>(proj);
    const dim3 grid((n32 + 255) / 256), grid_g(((n32 + TE_AFF_GROUP - 1u) / TE_AFF_GROUP + 255) / 256);
    hipLaunchKernelGGL(te::k_fb_ext_from_recs, grid, dim3(256), 0, st, reinterpret_cast<const te::pnt_slot*>(recs), ext, n32);
    for (int w = 1; w < b->fb_W; w++) {
      hipLaunchKernelGGL(te::k_fb_double, grid, dim3(256), 0, st, ext, n32, (uint32_t)b->fb_c);
      hipLaunchKernelGGL(te::k_fb_records, grid_g, dim3(256), 0, st, ext, reinterpret_cast<te::pnt_slot*>(recs) + (size_t)w * n, n32);
    }
  }
  HIP_TRY(ctx, hipGetLastError());
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}

// mont: option "points_montgomery" as te_msm_bind_points[_device] found it (te_msm_bind_points_x binds points it recovered itself: canonical)
int bind_common(te_ctx* ctx, const void* src, bool src_is_host, uint64_t n, te_bases** out, bool mont = false) {
  if (!ctx || !out) return TE_MSM_EINVAL;
  *out = nullptr;
  if (int rc = check_n(ctx, n)) return rc;
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
    if (int rc = check_call(ctx, ci, src, src_is_host, n, mont)) return rc;
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
  const int rc = n > 0 ? te_sched::on_devices(*ctx, nd, [=](size_t i) { return bind_on_device(ctx, b, i, src, src_is_host, src_dev, mont); }) : 0;
  if (rc) { free_bases(ctx, b); delete b; return rc; }
  // a set bound from HOST memory announces tickets from host scalars: the lanes' first concurrent copies (15-30 ms once per process,
  // warm_upload_lanes) happen here, in the call that blocks anyway, not in the first te_msm_submit_scalars -- which the N-API addon
  // issues on the JavaScript thread (js/promise_protocol.hpp: enter)
  if (src_is_host && n > 0) warm_upload_lanes(ctx);
  ctx->bases.push_back(b);
  *out = b;
  return 0;
}

// A whole MSM over a fixed-base set from HOST scalars on work set `ws`: all scalars cross PCIe in one copy (the digits of every
// window address one bucket set: there are no pieces to accumulate onto), then the fixed-base launch sequence and its read-back.
int enqueue_fixed_base_host(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases, const uint8_t* src_scalars, uint64_t n, bool wait_for_pinned,
                            int scalar_form = -1) {
  HIP_TRY(ctx, hipSetDevice(d.device));
  const curve_sizes sz = sizes_of(bases->curve);
  if (int rc = ensure_staging(ctx, ws, 0, n * sz.scalar_in)) return rc;
  if (int rc = wait_behind_previous(ctx, ws)) return rc;
  if (!wait_for_pinned) {
    // an asynchronous ticket: the lane thread waits for the upload itself (lane_wait), no wait enters the work set's stream
    if (ws.used) HIP_TRY(ctx, hipEventSynchronize(ws.ev_done));
    if (int rc = need_copy_stream(ctx, ws)) return rc;
    if (int rc = upload(ctx, ws, ws.d_in_scalars, src_scalars, n * sz.scalar_in, ws.copy_stream)) return rc;
    if (int rc = lane_wait(ctx, ws, ws.ev_copy, true)) return rc;
  } else {
    if (int rc = upload(ctx, ws, ws.d_in_scalars, src_scalars, n * sz.scalar_in, ws.stream)) return rc;
    if (wait_for_pinned && !ctx->opt_host_staging && host_memory_is_pinned(src_scalars)) {
      HIP_TRY(ctx, hipEventRecord(ws.ev_copy, ws.stream));
      HIP_TRY(ctx, hipEventSynchronize(ws.ev_copy));
    }
  }
  if (int rc = enqueue_fixed_base(ctx, d, ws, bases, ws.d_in_scalars, n, 0, ws.stream, scalar_form)) return rc;
  return fetch_rows(ctx, ws, ws.stream);
}

// The rows of a fixed-base MSM are on the host (ev_result passed).  A row of the pseudo-window buffers overflowed -- badly skewed
// scalars: all equal, a few distinct values -- : the MSM runs again with the ordinary windows over table 0 of the same set (the
// ordinary records), on the same work set; the caller then folds ws.plan's rows as usual.  0 = the rows in the pinned block are final.
int fixed_base_settle(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases) {
  if (!ws.plan.fb_rb || *ws.h_err || !ws.h_err[1]) return 0;
  ctx->stat_fb_fallbacks++;
  HIP_TRY(ctx, hipSetDevice(d.device));
  partial_req r; r.d_scalars = ws.fb_scalars; r.n = ws.fb_n; r.stream = ws.stream; r.whole = true; r.bases = bases;
  r.scalar_form = ws.plan.scalar_mont;                 // (a ticket: the form it was submitted with, whatever the option says at its collect)
  if (int rc = enqueue_partial(ctx, d, ws, r)) return rc;
  if (int rc = fetch_rows(ctx, ws, ws.stream)) return rc;
  HIP_TRY(ctx, hipEventSynchronize(ws.ev_result));
  return 0;
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
    if (must_pull(ctx, d, src_dev)) { if (int rc = pull_inputs(ctx, d, ws, src_dev, n, in, moved[i])) return rc; }
    partial_req r; r.d_scalars = in.scalars; r.n = n; r.stream = ws.stream; r.bases = bases;
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
  const uint64_t n = bases->n;
  if (n == 0) { write_identity(ctx->opt_curve, out); return 0; }
  if (!src) return set_err(ctx, TE_MSM_EINVAL, "null scalar buffer");
  size_t di = 0;
  if (ctx->devs.size() > 1) {
    if (!bases->fb_c) {
      if (src_is_host) return run_host_sharded(ctx, nullptr, static_cast<const uint8_t*>(src), n, out, bases);
      return run_bound_window_shards(ctx, bases, src, n, out);
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
  const curve_sizes sz = sizes_of(p0.curve);
  const bool fb = bases->fb_c && (ctx->devs.size() > 1 || d.w_step == 1);      // (a window-sharded single-device context keeps the ordinary windows)
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
      if (int rc = ensure_staging(ctx, ws, 0, n * sz.scalar_in)) return rc;
      if (int rc = wait_behind_previous(ctx, ws)) return rc;
      if (int rc = upload(ctx, ws, ws.d_in_scalars, static_cast<const uint8_t*>(src), n * sz.scalar_in, ws.stream)) return rc;
      ds = ws.d_in_scalars;
    }
    partial_req r; r.d_scalars = ds; r.n = n; r.stream = ws.stream; r.bases = bases;
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
}  // namespace

int te_msm_bind_points(te_ctx* ctx, const uint8_t* points_xy_le, uint64_t n, te_bases** out) {
  device_guard restore_callers_device;
  return bind_common(ctx, points_xy_le, true, n, out, ctx && ctx->opt_points_montgomery);
}

int te_msm_bind_points_device(te_ctx* ctx, const void* d_points_xy_le, uint64_t n, te_bases** out) {
  device_guard restore_callers_device;
  return bind_common(ctx, d_points_xy_le, false, n, out, ctx && ctx->opt_points_montgomery);
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
  r.wait_for_pinned = false; r.scalar_form = pf.scalar_mont;
  te_sched::job_ref job = post_to_lane(ctx, t, [ctx, t, bases, r]() -> int {
    return bases->fb_c ? enqueue_fixed_base_host(ctx, t.d, t.ws, bases, r.scalars, r.n, false, r.scalar_form) : enqueue_host_pieces(ctx, t.d, t.ws, r);
  });
  hand_out_ticket(ctx, t, ticket, bases, std::move(job));
  return 0;
}

int te_msm_submit_scalars_device(te_ctx* ctx, te_bases* bases, const void* d_scalars_le, uint64_t* ticket) {
  device_guard restore_callers_device;
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (int rc = check_bases(ctx, bases)) return rc;
  const uint64_t n = bases->n;
  if (!d_scalars_le || n == 0) return set_err(ctx, TE_MSM_EINVAL, "bad arguments (an empty point set has no tickets: te_msm_run_scalars_device returns the identity)");
  const bool multi = ctx->devs.size() > 1;
  const int owner = multi ? owner_of(ctx, "te_msm_submit_scalars_device: the scalars must be resident on a device of the context", {d_scalars_le}) : 0;
  if (owner < 0) return owner;
  std::optional<ticket_set> taken;
  if (int rc = take_free_workset(ctx, owner, true, taken)) return rc;
  const ticket_set& t = *taken;
  device_inputs in; in.scalars = d_scalars_le;
  if (int rc = pull_for_ticket(ctx, t, owner, n, in)) return rc;
  if (bases->fb_c && (multi || t.d.w_step == 1)) { if (int rc = enqueue_fixed_base(ctx, t.d, t.ws, bases, in.scalars, n, 0, t.ws.stream)) return rc; }
  else {
    partial_req r; r.d_scalars = in.scalars; r.n = n; r.stream = t.ws.stream; r.whole = multi; r.bases = bases;
    if (int rc = enqueue_partial(ctx, t.d, t.ws, r)) return rc;
  }
  if (int rc = fetch_rows(ctx, t.ws, t.ws.stream)) return rc;
  hand_out_ticket(ctx, t, ticket, bases);
  return 0;
}

// ---- MSMs over an indexed subset of a bound point set (include/te_msm.h) ------------------------------------------------------
namespace {
// the arguments all four calls share; 0 = go on
int indexed_args(te_ctx* ctx, const te_bases* bases, const void* idx, const void* scalars, uint64_t m) {
  if (int rc = check_bases(ctx, bases)) return rc;
  if (int rc = check_n(ctx, m)) return rc;
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
  if (int rc = indexed_args(ctx, bases, idx, src, m)) return rc;
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
}  // namespace

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
  r.wait_for_pinned = false; r.scalar_form = pf.scalar_mont;
  te_sched::job_ref job = post_to_lane(ctx, t, [ctx, t, r]() -> int { return enqueue_host_pieces(ctx, t.d, t.ws, r); });
  hand_out_ticket(ctx, t, ticket, bases, std::move(job));
  return 0;
}

int te_msm_submit_scalars_indexed_device(te_ctx* ctx, te_bases* bases, const void* d_idx, const void* d_scalars_le, uint64_t m, uint64_t* ticket) {
  device_guard restore_callers_device;
  if (!ctx || !ticket) return TE_MSM_EINVAL;
  if (int rc = indexed_args(ctx, bases, d_idx, d_scalars_le, m)) return rc;
  if (m == 0) return set_err(ctx, TE_MSM_EINVAL, "bad arguments (an empty index list has no tickets: te_msm_run_scalars_indexed_device returns the identity)");
  const int owner = owner_of(ctx, kIndexedResident, {d_idx, d_scalars_le});
  if (owner < 0) return owner;
  std::optional<ticket_set> taken;
  if (int rc = take_free_workset(ctx, owner, true, taken)) return rc;
  const ticket_set& t = *taken;
  device_inputs in; in.scalars = d_scalars_le; in.idx = static_cast<const uint32_t*>(d_idx);
  if (int rc = pull_for_ticket(ctx, t, owner, m, in)) return rc;
  partial_req r; r.d_scalars = in.scalars; r.n = m; r.stream = t.ws.stream; r.whole = true; r.bases = bases; r.d_idx = in.idx;
  if (int rc = enqueue_partial(ctx, t.d, t.ws, r)) return rc;
  if (int rc = fetch_rows(ctx, t.ws, t.ws.stream)) return rc;
  hand_out_ticket(ctx, t, ticket, bases);
  return 0;
}

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
  if (!strcmp(key, "batch_sequences")) { *value = ctx->stat_batch_sequences; return 0; }
  if (!strcmp(key, "bind_fixed_base")) { *value = ctx->opt_bind_fixed_base; return 0; }
  if (!strcmp(key, "fixed_base_fallbacks")) { *value = ctx->stat_fb_fallbacks; return 0; }
  if (!strcmp(key, "bases_bound")) { *value = (int64_t)ctx->bases.size(); return 0; }
  if (!strcmp(key, "bases_bytes")) { int64_t t = 0; for (const te_bases* b : ctx->bases) for (const uint8_t* r : b->recs) if (r) t += (int64_t)(b->n * b->rec_bytes) * (b->fb_c ? b->fb_W : 1); *value = t; return 0; }
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

namespace {
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
  const int rc = check_points_on(ctx, (size_t)di, src, src_is_host, n, ctx->opt_curve, level, &bad, &why, ctx->opt_points_montgomery != 0);
  if (rc != TE_MSM_EPOINT) return rc;
  return note_bad(ctx, kBadPoint, bad, why, first_bad, reason);
}
}  // namespace

int te_msm_check_points(te_ctx* ctx, const uint8_t* points_xy_le, uint64_t n, int level, int64_t* first_bad, int* reason) {
  return check_standalone(ctx, points_xy_le, true, n, level, first_bad, reason);
}
int te_msm_check_points_device(te_ctx* ctx, const void* d_points_xy_le, uint64_t n, int level, int64_t* first_bad, int* reason) {
  return check_standalone(ctx, d_points_xy_le, false, n, level, first_bad, reason);
}

// ---- x-only points (te_msm_points_from_x[_device], te_msm_bind_points_x, te_msm_run_x; kernels in from_x.hip.hpp) ----------------
// Recovery runs on device devs[di] into a buffer of the call's own, and the call waits for the verdict: on a failure nothing reaches
// the caller's output and no MSM runs.  Host x-coordinates cross PCIe in pieces of kCheckPiece through a staging buffer, on the
// check stream of the device (one stream: a piece's copy waits for the previous piece's kernel); every piece reports into one word
// over the whole buffer, so the lowest failing index wins without a wait per piece.  The temporary buffers are freed before the call
// returns (dev_tmp): nothing is cached, nothing counts in "device_bytes".
namespace {
struct dev_tmp {
  int dev = -1; void* p = nullptr;
  dev_tmp() = default;
  dev_tmp(const dev_tmp&) = delete;
  dev_tmp& operator=(const dev_tmp&) = delete;
  ~dev_tmp() { if (p) { (void)hipSetDevice(dev); (void)hipFree(p); } }
};
int tmp_alloc(te_ctx* ctx, gpu_t& d, dev_tmp& t, size_t bytes) {
  HIP_TRY(ctx, hipSetDevice(d.device));
  HIP_TRY(ctx, hipMalloc(&t.p, bytes ? bytes : 16));
  t.dev = d.device;
  return 0;
}
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
    if (curve == TE_MSM_CURVE_BLS12_377_G1) hipLaunchKernelGGL(te::k_points_from_x<1>, grid, block, 0, st, x4, m, o4, d.chk_word, n, off, te::kRootExp377, te::kNaf377Order);
    else hipLaunchKernelGGL(te::k_points_from_x<0>, grid, block, 0, st, x4, m, o4, d.chk_word, n, off, te::kRootExpTe, te::kNafTeOrder);
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
}  // namespace

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
  if (int rc = from_x_args(ctx, x_le, n, scalars_le)) return rc;
  if (n == 0) return run_common(ctx, x_le, scalars_le, true, 0, out_xy_le);
  dev_tmp pts, sc;
  if (int rc = recover_host_to_first(ctx, x_le, n, pts)) return rc;
  gpu_t& d = ctx->devs[0];
  const size_t sbytes = n * sizes_of(ctx->opt_curve).scalar_in;
  if (int rc = tmp_alloc(ctx, d, sc, sbytes)) return rc;
  {
    check_lane lane(ctx, d);
    if (lane.rc) return lane.rc;
    HIP_TRY(ctx, hipMemcpyAsync(sc.p, scalars_le, sbytes, hipMemcpyHostToDevice, lane.stream()));
    HIP_TRY(ctx, hipStreamSynchronize(lane.stream()));
  }
  return run_common(ctx, pts.p, sc.p, false, n, out_xy_le, SHARE_CONVERT);   // as te_msm_run_device (window shards, check_points, TE_MSM_ESCALAR)
}

// ---- batch scalar multiplication (te_msm_mul[_device], te_msm_mul_x; kernels in scalar_mul.hip.hpp) ------------------------------
// Host buffers: contiguous slices over the context's devices, one host thread per device (on_devices), as te_msm_run's point slices.
// Every slice is staged whole on its device -- points (or x), scalars and results -- checked (recovery, option "check_points"),
// multiplied, and copied out only when no slice reported a bad point: on a failure `out` is untouched.  The chain writes projective
// results of a piece of kMulPiece points into a buffer of the call's own; the affine pass turns them into the wire format.  Every
// temporary is freed before the call returns (dev_tmp).
namespace {
constexpr uint64_t kMulPiece = 1ull << 18;
// te_msm_mul* as te_msm_run_x: canonical scalars only -- refused under the option instead of a silent canonical reading
int mul_refused(te_ctx* ctx) { return ctx->opt_scalars_montgomery ? set_err(ctx, TE_MSM_EINVAL, kNoMontgomeryScalars) : 0; }

inline te::naf_t shared_naf_of(const uint8_t* k32, int curve) {
  uint32_t k[8];
  memcpy(k, k32, 32);
  return te::sm_shared_naf(k, curve);
}
// n points and scalars (memory of devs[di]) -> n affine results at d_out (memory of devs[di]); returns when they are there
int mul_on(te_ctx* ctx, size_t di, const void* d_pts, const void* d_sc, uint64_t n, bool shared, const te::naf_t& kn, void* d_out) {
  if (n == 0) return 0;
  gpu_t& d = ctx->devs[di];
  const int curve = ctx->opt_curve;
  const bool bls = curve == TE_MSM_CURVE_BLS12_377_G1;
  const size_t pb = sizes_of(curve).point_in, sb = sizes_of(curve).scalar_in;
  const size_t jb = 4u * (bls ? te::sm_sizes<1>::JW : te::sm_sizes<0>::JW);
  check_lane lane(ctx, d);
  if (lane.rc) return lane.rc;
  const uint64_t piece = std::min(n, kMulPiece);
  dev_tmp proj;
  if (int rc = tmp_alloc(ctx, d, proj, piece * jb)) return rc;
  hipStream_t st = lane.stream();
  for (uint64_t off = 0; off < n; off += piece) {
    const uint32_t m = (uint32_t)std::min(piece, n - off);
    const uint4* p4 = reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(d_pts) + off * pb);
    const uint4* s4 = shared ? nullptr : reinterpret_cast<const uint4*>(static_cast<const uint8_t*>(d_sc) + off * sb);
    uint4* j4 = static_cast<uint4*>(proj.p);
    uint32_t* o32 = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(d_out) + off * pb);
    const dim3 grid((m + 255u) / 256u), block(256), agrid((m + 256u * SM_AFF_GROUP - 1u) / (256u * SM_AFF_GROUP));
    if (bls) {
      if (shared) hipLaunchKernelGGL((te::k_scalar_mul<1, true>), grid, block, 0, st, p4, s4, m, j4, kn);
      else hipLaunchKernelGGL((te::k_scalar_mul<1, false>), grid, block, 0, st, p4, s4, m, j4, kn);
      hipLaunchKernelGGL(te::k_scalar_mul_affine<1>, agrid, block, 0, st, static_cast<const uint32_t*>(proj.p), m, o32, te::kInvExp377);
    } else {
      if (shared) hipLaunchKernelGGL((te::k_scalar_mul<0, true>), grid, block, 0, st, p4, s4, m, j4, kn);
      else hipLaunchKernelGGL((te::k_scalar_mul<0, false>), grid, block, 0, st, p4, s4, m, j4, kn);
      hipLaunchKernelGGL(te::k_scalar_mul_affine<0>, agrid, block, 0, st, static_cast<const uint32_t*>(proj.p), m, o32, te::kInvExpTe);
    }
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipStreamSynchronize(st));
  return 0;
}
int mul_args(te_ctx* ctx, const void* pts, const void* sc, uint64_t n, const void* out) {
  if (int rc = check_n(ctx, n)) return rc;
  if (n > 0 && (!pts || !sc || !out)) return set_err(ctx, TE_MSM_EINVAL, "null buffer");
  return 0;
}
// te_msm_mul (x_only = false) and te_msm_mul_x (true): host buffers, sliced over the devices
int mul_host(te_ctx* ctx, const uint8_t* src, bool x_only, const uint8_t* scalars_le, uint64_t n, bool shared, uint8_t* out) {
  if (int rc = mul_args(ctx, src, scalars_le, n, out)) return rc;
  if (n == 0) return 0;
  const int curve = ctx->opt_curve, level = ctx->opt_check_points;
  const size_t pb = sizes_of(curve).point_in, sb = sizes_of(curve).scalar_in, ib = x_only ? x_bytes_of(curve) : pb;
  const te::naf_t kn = shared ? shared_naf_of(scalars_le, curve) : te::naf_t{};
  const size_t D = (size_t)std::min<uint64_t>(ctx->devs.size(), n);
  const uint64_t per = (n + D - 1) / D;
  struct slice_t { dev_tmp pts, sc, res; int64_t bad = -1; int why = 0; bool from_x = false; };
  std::vector<slice_t> sl(D);
  auto stage = [&](size_t i) -> int {                             // upload, recover, check, multiply: everything but the copy out
    const uint64_t lo = std::min<uint64_t>(n, per * i), m = std::min<uint64_t>(n, lo + per) - lo;
    if (m == 0) return 0;
    gpu_t& d = ctx->devs[i];
    slice_t& s = sl[i];
    if (int rc = tmp_alloc(ctx, d, s.pts, m * pb)) return rc;
    if (int rc = tmp_alloc(ctx, d, s.res, m * pb)) return rc;
    if (!shared) {
      if (int rc = tmp_alloc(ctx, d, s.sc, m * sb)) return rc;
      HIP_TRY(ctx, hipMemcpy(s.sc.p, scalars_le + lo * sb, m * sb, hipMemcpyHostToDevice));
    }
    if (x_only) {
      const int rc = recover_on(ctx, i, src + lo * ib, true, m, s.pts.p, nullptr, false, &s.bad, &s.why);
      if (rc == TE_MSM_EPOINT) { s.from_x = true; return 0; }
      if (rc) return rc;
    } else {
      HIP_TRY(ctx, hipMemcpy(s.pts.p, src + lo * ib, m * pb, hipMemcpyHostToDevice));
    }
    if (level) {
      const int rc = check_points_on(ctx, i, s.pts.p, false, m, curve, level, &s.bad, &s.why);
      if (rc == TE_MSM_EPOINT) return 0;
      if (rc) return rc;
    }
    return mul_on(ctx, i, s.pts.p, s.sc.p, m, shared, kn, s.res.p);
  };
  auto copy_out = [&](size_t i) -> int {
    const uint64_t lo = std::min<uint64_t>(n, per * i), m = std::min<uint64_t>(n, lo + per) - lo;
    if (m == 0) return 0;
    HIP_TRY(ctx, hipSetDevice(ctx->devs[i].device));
    HIP_TRY(ctx, hipMemcpy(out + lo * pb, sl[i].res.p, m * pb, hipMemcpyDeviceToHost));
    return 0;
  };
  if (int rc = te_sched::on_devices(*ctx, D, stage)) return rc;
  for (size_t i = 0; i < D; i++) {                                // slices in order: the first that reports holds the lowest index
    if (sl[i].bad < 0) continue;
    return note_bad(ctx, sl[i].from_x ? kBadX : kBadPoint, (int64_t)(per * i) + sl[i].bad, sl[i].why);
  }
  return te_sched::on_devices(*ctx, D, copy_out);
}
}  // namespace

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
  return mul_on(ctx, (size_t)owner, d_points_xy_le, d_scalars_le, n, shared_scalar != 0, kn, d_out_points_xy_le);
}

// ---- batched MSMs over prefixes of a bound point set (te_msm_run_scalars_batch[_device]) -------------------------------------------
namespace {
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

struct batch_seq_run {              // one sequence of the plan, as the engine runs it
  const te_batch::sequence* s = nullptr;
  plan_t p;                         // the plan of its launch sequence (n = its largest length, batch = its MSMs)
  size_t rows_at = 0;               // offset of its rows in its device's pinned landing area
};

// One ragged sequence on work set ws: the scalar stages over the packed buffer, the accumulation from the bound records, the reduction
// into the set's batch rows, their read-back to h_rows, and the clearing of the zeroed block (finish_sequence)
int enqueue_ragged(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases, const void* d_scalars, const te::ragged_tab& tab, const plan_t& p,
                   uint8_t* h_rows) {
  if ((uint64_t)p.nw * p.nst >= (1ull << 31)) return set_err(ctx, TE_MSM_EINVAL, "batch sequence too large: windows x points must stay below 2^31");
  HIP_TRY(ctx, hipSetDevice(d.device));
  const uint64_t n_max = [&] { uint64_t m = 0; for (int j = 0; j < p.batch; j++) m = std::max<uint64_t>(m, tab.len[j]); return m; }();
  if ((uint64_t)p.nw * p.B + (uint64_t)p.nw * (n_max / p.seg_len) + 1024u >= (1ull << 32))
    return set_err(ctx, TE_MSM_EINVAL, "segment_len is too small for this batch: more than 2^32 segments");
  if (int rc = ensure_buffers(ctx, d, ws, n_max, p, false)) return rc;
  const size_t row_bytes = (size_t)p.batch * p.W * sizes_of(p.curve).row;
  if (int rc = make_room(ctx, ws.d_batch_rows, row_bytes)) return rc;
  hipStream_t stream = ws.stream;
  msm_launch L(ctx, ws, p, n_max, stream);
  L.d_scalars = d_scalars; L.d_partials_out = ws.d_batch_rows;        // (not the set's own rows: none of them go to the pinned block)
  if (int rc = begin_sequence(d, L, nullptr)) return rc;
  note_sequence(d, ws, p, n_max, stream, 0);
  L.bound = bases->recs[(size_t)(&d - ctx->devs.data())];      // (a fixed-base set: table 0, the ordinary records)
  L.ragged = &tab;
  if (int rc = L.front_scalars()) return rc;
  if (int rc = L.accumulate()) return rc;
  if (int rc = L.back()) return rc;                             // ... ends with the flag words' read-back into ws.h_err
  HIP_TRY(ctx, hipMemcpyAsync(h_rows, ws.d_batch_rows, row_bytes, hipMemcpyDeviceToHost, stream));
  if (int rc = finish_sequence(ctx, ws, stream)) return rc;
  HIP_TRY(ctx, hipGetLastError());
  return 0;
}

// The sequences of one device, dealt over its free work sets in plan order (up to TE_MSM_WORKSETS in flight: a set is reused once its
// previous sequence is over).  d_sc: the packed scalars on this device, off[m]: where MSM m's start (records).
int run_batch_on_device(te_ctx* ctx, size_t di, const te_bases* bases, const void* d_sc, const std::vector<uint64_t>& off, const uint64_t* lens,
                        std::vector<batch_seq_run>& runs, bool* carry, int64_t* entries) {
  gpu_t& d = ctx->devs[di];
  HIP_TRY(ctx, hipSetDevice(d.device));
  std::vector<int> sets;
  for (int wi = 0; wi < TE_MSM_WORKSETS; wi++) if (!te_sched::slot_ticket(d.ws[wi].slot)) sets.push_back(wi);
  if (sets.empty()) return set_err(ctx, TE_MSM_ESTATE, kAllSetsOwned);
  size_t total = 0;
  for (batch_seq_run& r : runs) { r.rows_at = total; total += (size_t)r.p.batch * r.p.W * sizes_of(r.p.curve).row; }
  if (total > d.h_batch_cap) {
    if (d.h_batch_rows) HIP_TRY(ctx, hipHostFree(d.h_batch_rows));
    d.h_batch_rows = nullptr; d.h_batch_cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&d.h_batch_rows, total ? total : 16, hipHostMallocDefault));
    d.h_batch_cap = total;
  }
  std::vector<int> busy(sets.size(), 0);
  auto settle = [&](size_t slot) -> int {
    workset_t& ws = d.ws[sets[slot]];
    HIP_TRY(ctx, hipEventSynchronize(ws.ev_done));
    *carry = *carry || *ws.h_err != 0;
    *entries += entries_of(ws);
    busy[slot] = 0;
    return 0;
  };
  int rc = 0;
  for (size_t k = 0; k < runs.size() && !rc; k++) {
    const size_t slot = k % sets.size();
    if (busy[slot] && (rc = settle(slot))) break;
    te::ragged_tab tab; memset(&tab, 0, sizeof tab);
    const std::vector<uint32_t>& ms = runs[k].s->msms;
    for (size_t j = 0; j < ms.size(); j++) { tab.off[j] = off[ms[j]]; tab.len[j] = (uint32_t)lens[ms[j]]; }
    rc = enqueue_ragged(ctx, d, d.ws[sets[slot]], bases, d_sc, tab, runs[k].p, d.h_batch_rows + runs[k].rows_at);
    busy[slot] = 1;
  }
  for (size_t slot = 0; slot < sets.size(); slot++) {
    if (!busy[slot]) continue;
    if (rc) { (void)hipStreamSynchronize(d.ws[sets[slot]].stream); continue; }
    rc = settle(slot);
  }
  return rc;
}

int run_batch_common(te_ctx* ctx, te_bases* bases, int count, const uint64_t* lens, const void* src, bool src_is_host, uint8_t* out) {
  if (!ctx) return TE_MSM_EINVAL;
  drain_workers(ctx);
  if (int rc = check_bases(ctx, bases)) return rc;
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
      if (int rc = tmp_alloc(ctx, d, tmp[i], total * sz.scalar_in)) return rc;
      HIP_TRY(ctx, hipMemcpy(tmp[i].p, src, total * sz.scalar_in, hipMemcpyHostToDevice));
    } else {
      offs[i].assign((size_t)count, 0);
      std::vector<uint32_t> mine;
      for (const batch_seq_run& r : runs[i]) mine.insert(mine.end(), r.s->msms.begin(), r.s->msms.end());
      std::sort(mine.begin(), mine.end());
      uint64_t here = 0;
      for (uint32_t m : mine) { offs[i][m] = here; here += lens[m]; }
      std::vector<uint8_t> pack((size_t)(here * sz.scalar_in));
      for (uint32_t m : mine) memcpy(&pack[(size_t)(offs[i][m] * sz.scalar_in)], static_cast<const uint8_t*>(src) + off[m] * sz.scalar_in, (size_t)(lens[m] * sz.scalar_in));
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

int te_msm_run_scalars_batch(te_ctx* ctx, te_bases* bases, int count, const uint64_t* lens, const uint8_t* scalars_le, uint8_t* out) {
  device_guard restore_callers_device;
  return run_batch_common(ctx, bases, count, lens, scalars_le, true, out);
}

int te_msm_run_scalars_batch_device(te_ctx* ctx, te_bases* bases, int count, const uint64_t* lens, const void* d_scalars_le, uint8_t* out) {
  device_guard restore_callers_device;
  return run_batch_common(ctx, bases, count, lens, d_scalars_le, false, out);
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
