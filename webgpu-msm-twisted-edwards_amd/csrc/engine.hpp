// engine.hpp -- what the translation units of libtemsm.so share: the context and its work sets, the plan, the requests a launch
// sequence is asked with, and the functions that more than one unit calls.  No kernel header in here: te_msm.hip alone includes
// kernels.hip.hpp and probe.hip.hpp, points.hip the check / x-recovery / scalar-multiplication / fixed-base / group-addition / field-arithmetic / NTT / polynomial / sparse-matrix kernels
// (a non-template __global__ function may be defined once per library, and every inclusion repeats the device compile).
//
// The units:   te_msm.hip   the engine core: plan and buffers, the launch sequences, streams and queue probe, record slabs, uploads
//              run.hip      te_msm_init / destroy, the lone calls te_msm_run[_device], how a call's status is settled
//              tickets.hip  te_msm_submit* / ticket_wait / collect
//              bases.hip    bound point sets: bind, scalars-only, indexed and batched MSMs
//              points.hip   point checks, x-only points, batch scalar multiplication (per point, and over one bound point with its
//                           fixed-base table), batched group addition and point-set sums, batched field arithmetic, batched NTTs,
//                           polynomial openings, bound sparse matrices and their products
//              abi.hip      the rest of the C-ABI: options, trim, building blocks, host tails, debug reads
// Everything in here has hidden visibility; a function only one unit calls is file-local there.  The library exports the C-ABI of
// include/te_msm.h and nothing else of the engine.
#pragma once
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

#include "../../include/te_msm.h"
#include "batch_plan.hpp"
#include "indexed_plan.hpp"
#include "plan_arith.hpp"
#include "fb_plan.hpp"
#include "ntt_plan.hpp"
#include "poly_plan.hpp"
#include "scan_plan.hpp"
#include "spmv_plan.hpp"

#pragma GCC visibility push(hidden)
#include "host_sched.hpp"

namespace te_eng {

// What the engine must know of kernels.hip.hpp without including it: te_msm.hip, which does, asserts every one against the real thing.
constexpr uint32_t kClkSlots = 64u, kHistCopies = 32u;                       // TE_CLK_SLOTS, TE_HIST_COPIES
constexpr size_t kAccBytes = 144, kAccBytes377 = 224;                        // te::ete, te::ete_t<14>
constexpr size_t kRecBytes = 128, kRecBytes377 = 224, kRecBytesAff377 = 168; // te::rec_slot<9>, te::rec_slot<14>, te::rec_aff377

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
  return curve == TE_MSM_CURVE_BLS12_377_G1 ? curve_sizes{96, 48, kAccBytes377, kRecBytes377, TE_MSM_PARTIAL_BYTES_BLS12_377, 96}
                                            : curve_sizes{TE_MSM_POINT_BYTES, TE_MSM_SCALAR_BYTES, kAccBytes, kRecBytes, TE_MSM_PARTIAL_BYTES, 64};
}
// bytes of one record: the curve's own (converted per call), or -- rec_kind 1 -- the affine BLS12-377 record of a bound point set
inline size_t rec_bytes_of(int curve, int rec_kind) { return (curve == TE_MSM_CURVE_BLS12_377_G1 && rec_kind == 1) ? kRecBytesAff377 : sizes_of(curve).rec; }
static_assert(kAccBytes377 * 5 == TE_MSM_PARTIAL_BYTES_BLS12_377 && kAccBytes * 5 == TE_MSM_PARTIAL_BYTES, "row layout");
constexpr size_t TE_MAX_ROW_BYTES = TE_MSM_PARTIAL_BYTES_BLS12_377;

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
  int sc_bytes = 0;                  // bytes of one scalar record, 8, 16, 32 or 48: option "scalar_record_bytes" as it was when the call started (scalar_bytes_now)
  int sc_bits = 0;                   // every scalar is below 2^sc_bits, as the caller declared when the call started (scalar_bits_now); 0 = nothing declared.
                                     // c and W cover this width only (te_plan::windows_for)
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
// words [Z_CLOCK, Z_ROWS): k_accumulate's profiling words, 4 x kClkSlots 64-bit values (first wave in / last wave out on the
// wall clock, core and wall ticks summed over the waves), see the kernel
constexpr size_t Z_KEEP = 4;            // words [0, Z_KEEP) are kept from piece to piece of one host-buffer MSM (flag, pad, 64-bit entry count)
constexpr size_t Z_ENTRIES = 2;         // the 64-bit entry count (8-byte aligned)
constexpr size_t Z_CLOCK = 8;
static_assert(Z_KEEP + 4 <= Z_CLOCK && Z_ENTRIES % 2 == 0 && Z_ENTRIES + 2 <= Z_KEEP, "flag words");
constexpr size_t Z_ROWS = Z_CLOCK + 4 * 2 * kClkSlots, Z_HIST = Z_ROWS + (size_t)TE_MAX_WINDOWS * TE_MAX_ROW_BYTES / 4, Z_CURSOR = Z_HIST + 1024 * kHistCopies, Z_END = Z_CURSOR + 1024;

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
  dev_buf<uint32_t> ntt_tab;             // te_msm_ntt*: the twiddle tables hi | lo (ntt_plan.hpp), built at the first transform on the device under chk_mu;
                                         // te_msm_trim / destroy free them (get_option "ntt_table_bytes")
  dev_buf<uint8_t> ntt_tmp;              // ... and the buffer between the passes of a multi-pass transform (ntt_plan.hpp, tmp_records_for: at most 512 MB), grown on
                                         // use under chk_mu, freed with the tables (get_option "ntt_scratch_bytes")
  dev_buf<uint8_t> poly_tmp;             // te_msm_poly_divide*: the tile sums, carries and powers of a call (poly_plan.hpp, scratch_bytes: about count * n / T records),
                                         // grown on use under chk_mu, freed by te_msm_trim / destroy (get_option "poly_scratch_bytes")
  dev_buf<uint8_t> scan_tmp;             // te_msm_field_scan*: the tile totals, carries and seeds of a call (scan_plan.hpp, scratch_bytes: about count * n / T records),
                                         // grown on use under chk_mu, freed by te_msm_trim / destroy (get_option "scan_scratch_bytes")
  dev_buf<uint8_t> spmv_tmp;             // te_msm_spmv*: the fragments of rows that span tiles (spmv_plan.hpp, scratch_bytes: two records a tile and vector),
                                         // grown on use under chk_mu, freed by te_msm_trim / destroy (get_option "spmv_scratch_bytes")
};

}  // namespace te_eng

// (the two types include/te_msm.h names: global, with external linkage, made of te_eng's)
struct te_ctx {
  std::vector<te_eng::gpu_t> devs;
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
  int bad_point_operand = -1;       // ... and which operand of te_msm_add* held it: 0 = a (every call with one point buffer), 1 = b; -1 before any failure
  int64_t bad_field_index = -1; int bad_field_reason = 0;   // the last TE_MSM_EFIELD (get_option "bad_field_index" / "bad_field_reason")
  int64_t bad_index_position = -1;  // te_msm_run_scalars_indexed*: lowest position of an index outside the bound set, of the last call that failed on one
  float stage_ms[te_eng::ST_COUNT + 2] = {};
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
  std::vector<te_base*> mul_bases;  // the bound points of fixed-base scalar multiplication (te_msm_bind_base), freed by te_msm_release_base / te_msm_destroy
  std::vector<te_matrix*> matrices; // the bound sparse matrices (te_msm_bind_matrix), freed by te_msm_release_matrix / te_msm_destroy
  int opt_scalar_record_bytes = 0;  // bytes of one scalar record: 0 = the curve's own (32 / 48), 32 = BLS12-377 scalars as a native prover holds them, 8 / 16 = a
                                    // native &[u64] / &[u128]; read when a call starts, on the calling thread -- a ticket keeps the size it was submitted with (plan_t::sc_bytes)
  int opt_scalar_bits = 0;          // the caller declares every scalar below 2^b (0 = nothing declared; 8-byte records: their width; 16-byte records need it set); read when a call starts, as
                                    // the record size -- a ticket keeps the width it was submitted with (plan_t::sc_bits)
  int opt_point_stride = 0;         // te_msm_bind_points[_device], te_msm_check_points[_device]: bytes from one point record to the next, 0 = packed x || y; read at bind time
  int opt_point_infinity_flag = 0;  // ... BLS12-377: the byte at offset 96 of every record flags the point at infinity (needs a stride >= 104); read at bind time
  int opt_mul_base_window = 12;     // te_msm_bind_base: window bits W of the table, 4..12 (option "mul_base_window"; 12 measured fastest at every size: DESIGN.md section 17); read at bind time
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

// A bound point of fixed-base batch scalar multiplication (include/te_msm.h, te_msm_bind_base; csrc/mul_base.hip.hpp): the table
// [j 2^(W i)] P, i < M, j <= 2^(W-1), in 128-byte entries on EVERY device of its context, built once.
struct te_base {
  te_ctx* ctx = nullptr;
  int curve = TE_MSM_CURVE_TE_BLS12;
  int W = 0, M = 0;              // window bits, windows
  uint32_t per = 0;              // entries of a window: 2^(W-1) + 1
  std::vector<uint8_t*> tab;     // tab[i]: M * per entries in the memory of ctx->devs[i]
  size_t bytes() const { return (size_t)M * per * 128; }
};

// A bound sparse matrix (include/te_msm.h, te_msm_bind_matrix; csrc/spmv_plan.hpp): its CSR arrays on EVERY device of its context, the
// values converted once; with_t: the same for its transpose, a CSR matrix of cols rows.
struct te_matrix {
  te_ctx* ctx = nullptr;
  uint64_t rows = 0, cols = 0, nnz = 0;
  bool with_t = false;
  std::vector<uint8_t*> side, side_t;    // side[i] / side_t[i]: one allocation of te_spmv::layout_of in the memory of ctx->devs[i]
  size_t bytes() const { return (size_t)(te_spmv::layout_of(rows, nnz).bytes + (with_t ? te_spmv::layout_of(cols, nnz).bytes : 0)); }
};

namespace te_eng {

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

inline int set_err(te_ctx* ctx, int code, const char* msg) { std::lock_guard<std::mutex> lk(ctx->err_mu); ctx->err = msg; return code; }

// Bytes of one scalar record of a call that starts NOW (option "scalar_record_bytes"; 0 = the curve's own record).  Every buffer size and
// piece offset of the call's scalars, and the stride its kernels read them at, come from this value -- never from sizes_of().scalar_in.
inline size_t scalar_bytes_now(const te_ctx* ctx) { return ctx->opt_scalar_record_bytes ? (size_t)ctx->opt_scalar_record_bytes : sizes_of(ctx->opt_curve).scalar_in; }
inline bool narrow_records(int bytes) { return bytes == 8 || bytes == 16; }
// The width a call that starts NOW declares for its scalars (plan_t::sc_bits): option "scalar_bits", else the width of 8- / 16-byte records,
// else 0 -- nothing declared, the full-width windows.  A call with a declared width runs the ordinary windows (a fixed-base set serves it
// from its table 0).
inline int scalar_bits_now(const te_ctx* ctx) {
  if (ctx->opt_scalar_bits) return ctx->opt_scalar_bits;
  return narrow_records(ctx->opt_scalar_record_bytes) ? 8 * ctx->opt_scalar_record_bytes : 0;
}
// ... and what every entry point that reads scalars asks first (the options may have changed one after the other): the Twisted-Edwards
// curve has no 48-byte record; a residue is 32 bytes, so 8- / 16-byte records are never Montgomery forms; a declared width fits the record.
// d_scalars: the scalars of a _device form, which the kernels load in units of the record (8- / 16-byte records).  0 = go on
inline int check_scalar_record(te_ctx* ctx, const void* d_scalars = nullptr) {
  const int rb = ctx->opt_scalar_record_bytes;
  if (rb == 48 && ctx->opt_curve != TE_MSM_CURVE_BLS12_377_G1)
    return set_err(ctx, TE_MSM_EINVAL, "option \"scalar_record_bytes\" is 48: the Twisted-Edwards curve has 32-byte scalar records only");
  if (narrow_records(rb)) {
    if (ctx->opt_scalars_montgomery) return set_err(ctx, TE_MSM_EINVAL, "option \"scalars_montgomery\" needs 32-byte records: a residue does not fit 8 or 16 bytes");
    if (ctx->opt_scalar_bits > 8 * rb) return set_err(ctx, TE_MSM_EINVAL, "option \"scalar_bits\" is larger than the width of the scalar records");
    if (rb == 16 && !ctx->opt_scalar_bits) return set_err(ctx, TE_MSM_EINVAL, "16-byte scalar records need a declared width: option \"scalar_bits\" was reset to 0");
    if (d_scalars && (reinterpret_cast<uintptr_t>(d_scalars) & (uintptr_t)(rb - 1)))
      return set_err(ctx, TE_MSM_EINVAL, "device scalars must be aligned to the size of their records");
  }
  return 0;
}
// te_msm_mul* / te_msm_mul_base*: 32- / 48-byte records only (they do not read "scalar_bits")
inline int check_mul_scalar_record(te_ctx* ctx) {
  if (narrow_records(ctx->opt_scalar_record_bytes)) return set_err(ctx, TE_MSM_EINVAL, "scalar multiplication reads 32- or 48-byte scalar records: reset option \"scalar_record_bytes\"");
  return check_scalar_record(ctx);
}

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

// How the points of a bind or a standalone check lie in the caller's buffer (options "point_stride" / "point_infinity_flag" as the call
// found them; csrc/strided.hip.hpp).  The per-call point paths and te_msm_bind_points_x pass the default: packed, no flag.
struct point_layout {
  uint32_t stride = 0; bool flag = false;
  size_t bytes(int curve) const { return stride ? stride : sizes_of(curve).point_in; }      // from one point to the next
};
constexpr uint32_t kPointStrideMax = 128;      // TE_STRIDE_MAX: a block's tile of 256 records fits 32 KB of LDS

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
  int scalar_bytes = 0;          // ... and their size (plan_t::sc_bytes), fixed by the same callers; 0 = option "scalar_record_bytes" as it is now
  int scalar_bits = -1;          // ... and their declared width (plan_t::sc_bits), likewise; -1 = as the options have it now (scalar_bits_now)
  int rec_kind = 0;              // records k_accumulate gathers (plan_t::rec_kind): a bound point set's form
  uint64_t idx_count = 0;        // an indexed call: records of the bound set -- the entry form follows the SET (indexed_plan.hpp); 0 = not indexed
};
inline plan_req plan_shard(uint64_t n) { plan_req q; q.n = n; return q; }
inline plan_req plan_whole(uint64_t n) { plan_req q; q.n = n; q.whole = true; return q; }

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

// Where a call's records live (enqueue_partial): the work set's own d_recs; a shared slab the call converts into (the building blocks,
// whose completion the engine does not see, and whole-MSM calls whose input form keeps the per-call conversion); or a shared slab as a
// whole-MSM call of its occupancy run, which converts only when no earlier call of the run has (see SHARED RECORD SLABS, te_msm.hip).
enum share_mode { SHARE_NONE = 0, SHARE_CONVERT = 1, SHARE_RUN = 2 };

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
  int scalar_bytes = 0;               // plan_req's: 0 = option "scalar_record_bytes" as it is now
  int scalar_bits = -1;               // plan_req's: -1 = the declared width as the options have it now
};

// Device-resident inputs of a call, and the peer pull that brings them from the memory of device src_dev into the staging area of a
// work set on another device of the context (tickets that land beside their inputs, the shares of run_bound_window_shards).
struct device_inputs { const void* scalars = nullptr; const void* points = nullptr; const uint32_t* idx = nullptr; };     // points / idx: where the call has them
struct peer_traffic { int64_t copies = 0, bytes = 0; };

// One MSM from host buffers, or one device's slice of it (enqueue_host_pieces, te_msm.hip, says what the fields mean together)
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
  int scalar_bytes = 0;                 // plan_req's (likewise)
  int scalar_bits = -1;                 // plan_req's (likewise)
};

const char* const kFinalCarry = "final carry is 1: a scalar does not fit the signed window decomposition";
const char* const kAllSetsOwned = "every work set holds a submitted MSM that has not been collected: te_msm_collect one first";

enum bad_kind { kBadPoint, kBadX };       // what note_bad reports: a failed point check, an x-coordinate without a point

// The work set a new ticket is opened on, as every submit form uses it: index of its device in ctx->devs, the device, the set.
struct ticket_set { int di; gpu_t& d; workset_t& ws; };

// a device allocation of one call's own (tmp_alloc), freed when the call returns: nothing cached, nothing counted in "device_bytes"
struct dev_tmp {
  int dev = -1; void* p = nullptr;
  dev_tmp() = default;
  dev_tmp(const dev_tmp&) = delete;
  dev_tmp& operator=(const dev_tmp&) = delete;
  ~dev_tmp() { if (p) { (void)hipSetDevice(dev); (void)hipFree(p); } }
};

struct batch_seq_run {              // one sequence of the plan, as the engine runs it
  const te_batch::sequence* s = nullptr;
  plan_t p;                         // the plan of its launch sequence (n = its largest length, batch = its MSMs)
  size_t rows_at = 0;               // offset of its rows in its device's pinned landing area
};

// ---- the functions more than one unit calls, by the unit that defines them (each is described where it is defined) ----
// te_msm.hip
plan_t make_plan(const te_ctx* ctx, const gpu_t& d, const plan_req& q);
void free_workset_buffers(workset_t& ws);
int need_copy_stream(te_ctx* ctx, workset_t& ws);
void park_stream(int device, hipStream_t s);
int create_workset_streams(gpu_t& d);
void spread_streams_over_queues(gpu_t& d);
int settle_slab(te_ctx* ctx, gpu_t::rec_slab_t& sl, hipStream_t stream, bool host);
void release_shared_recs(gpu_t& d, workset_t& ws, bool completed = true);
hipError_t allow_tail_lds();
int enqueue_partial(te_ctx* ctx, gpu_t& d, workset_t& ws, const partial_req& r);
int fetch_rows(te_ctx* ctx, workset_t& ws, hipStream_t stream);
int collect_stage_ms(te_ctx* ctx, const gpu_t& d, workset_t& ws);
int enqueue_host_pieces(te_ctx* ctx, gpu_t& d, workset_t& ws, const host_slice_req& r);
int fb_windows_for(int c);
int enqueue_fixed_base(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases, const void* d_scalars, uint64_t n, uint64_t idx_base, hipStream_t stream,
                       int scalar_form = -1);
int run_batch_on_device(te_ctx* ctx, size_t di, const te_bases* bases, const void* d_sc, const std::vector<uint64_t>& off, const uint64_t* lens,
                        std::vector<batch_seq_run>& runs, bool* carry, int64_t* entries);
int bind_on_device(te_ctx* ctx, te_bases* b, size_t i, const void* src, bool src_is_host, int src_dev, bool mont, point_layout lay);
int ensure_staging(te_ctx* ctx, workset_t& ws, size_t bytes_points, size_t bytes_scalars);
int wait_behind_previous(te_ctx* ctx, workset_t& ws);
bool must_pull(const te_ctx* ctx, const gpu_t& d, int src_dev);
int pull_inputs(te_ctx* ctx, const gpu_t& d, workset_t& ws, int src_dev, uint64_t n, size_t scalar_bytes, device_inputs& in, peer_traffic& moved);
void note_peer_traffic(te_ctx* ctx, const peer_traffic& moved);
bool host_memory_is_pinned(const void* p);
int upload(te_ctx* ctx, workset_t& ws, void* dst, const uint8_t* src, size_t bytes, hipStream_t stream);
int lane_wait(te_ctx* ctx, workset_t& ws, hipEvent_t ev, bool lane);
int host_pieces(const te_ctx* ctx, uint64_t n);
int scalar_pieces(const te_ctx* ctx, uint64_t n);
// run.hip
void fold_rows(const plan_t& p, const uint8_t* rows, uint8_t* out);
void write_identity(int curve, uint8_t* out);
void drain_workers(te_ctx* ctx);
int free_workset_index(const gpu_t& d);
int free_sets(te_ctx* ctx, size_t D, std::vector<int>& wsel);
int lone_set(te_ctx* ctx, const gpu_t& d, int selected);
int64_t entries_of(const workset_t& ws);
int settle_status(te_ctx* ctx, const workset_t& ws, bool entries_of_failed = true);
int run_host_sharded(te_ctx* ctx, const uint8_t* src_points, const uint8_t* src_scalars, uint64_t n, uint8_t* out, const te_bases* bases = nullptr,
                     const uint32_t* src_idx = nullptr);
int settle_window_shards(te_ctx* ctx, const std::vector<int>& wsel, const plan_t& p0, int rc, bool stage_ms, uint8_t* out);
int check_n(te_ctx* ctx, uint64_t n);
int run_common(te_ctx* ctx, const void* src_points, const void* src_scalars, bool src_is_host, uint64_t n, uint8_t out[64], share_mode share = SHARE_RUN);
// tickets.hip
int take_free_workset(te_ctx* ctx, int prefer, bool probe, std::optional<ticket_set>& t);
int lane_status(te_ctx* ctx, workset_t& ws, int rc);
void hand_out_ticket(te_ctx* ctx, const ticket_set& t, uint64_t* ticket, te_bases* bound = nullptr, te_sched::job_ref job = nullptr);
int owner_of(te_ctx* ctx, const char* msg, std::initializer_list<const void*> ptrs);
int pull_for_ticket(te_ctx* ctx, const ticket_set& t, int owner, uint64_t n, size_t scalar_bytes, device_inputs& in, bool* pulled = nullptr);
void warm_upload_lanes(te_ctx* ctx);
// bases.hip
int bind_common(te_ctx* ctx, const void* src, bool src_is_host, uint64_t n, te_bases** out, bool mont = false, point_layout lay = {});
int fixed_base_settle(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases);
// points.hip
int check_points_on(te_ctx* ctx, size_t di, const void* src, bool src_is_host, uint64_t n, int curve, int level, int64_t* bad, int* reason, bool mont = false,
                    point_layout lay = {});
int check_layout(te_ctx* ctx, const point_layout& lay, const void* src, bool src_is_host);
point_layout layout_now(const te_ctx* ctx);
int note_bad(te_ctx* ctx, bad_kind kind, int64_t index, int reason, int64_t* first_bad = nullptr, int* reason_out = nullptr);
int check_call(te_ctx* ctx, size_t di, const void* src, bool src_is_host, uint64_t n, bool mont = false, point_layout lay = {});
int tmp_alloc(te_ctx* ctx, gpu_t& d, dev_tmp& t, size_t bytes);
void free_mul_base(te_ctx* ctx, te_base* b);
void free_matrix(te_ctx* ctx, te_matrix* m);

// An asynchronous ticket: `enqueue` (the upload and the launches of one whole MSM; 0 or an error already noted) runs on an upload lane
// of the ticket's device, and the call returns at once -- D of them keep D links busy.  The job's status, and the error text of a failure,
// stay with the set for te_msm_collect (lane_status).  The job reads the context's options as they are NOW only by accident of timing
// -- so te_msm_set_option waits for the host threads first (drain_workers); what the enqueue depends on is fixed by its captures.
template <typename F> te_sched::job_ref post_to_lane(te_ctx* ctx, const ticket_set& t, F enqueue) {
  t.ws.job_err.clear();
  warm_upload_lanes(ctx);                            // (once per process and device: all of the context's devices together)
  workset_t* wsp = &t.ws;
  return te_sched::next_lane_of(*ctx, (size_t)t.di, ctx->opt_upload_threads).post([ctx, wsp, enqueue]() -> int { return lane_status(ctx, *wsp, enqueue()); });
}

}  // namespace te_eng

#pragma GCC visibility pop
