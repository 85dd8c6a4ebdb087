/*
 * te_msm.h -- C-ABI of the MI355X-native Twisted-Edwards-BLS12 MSM engine (libtemsm.so).
 *
 * This is the drop-in boundary for the reference's hot path.  Nothing like it exists in the
 * reference (a browser program); each entry point names the reference interface it stands behind
 * (paths relative to /root/reference/src).  INTEGRATION.md shows the N-API binding that keeps
 * `compute_msm(bufferPoints, bufferScalars)` (submission/submission.ts:73-78) intact.
 *
 * Wire format (README.md:297-299; encoder reference/webgpu/utils.ts:90-99):
 *   points : n x (x[32 B little-endian] || y[32 B little-endian]), canonical affine, NOT Montgomery.  With option
 *            "check_points" = 0 a coordinate may be any 256-bit value: it stands for its residue mod p (x + k p gives the
 *            result of x)
 *   scalars: n x 32 B little-endian integers (< p < 2^253; signed digits accept anything below 2^254 - 2^240 at every
 *            window size -- TE_MSM_ESCALAR above --, unsigned digits any 256-bit value)
 *   result : x[32 B LE] || y[32 B LE], canonical affine  ( == result.toAffine(), submission.ts:412 )
 * A NATIVE PROVER'S FORM (arkworks, snarkVM: a field element is a = k * 2^256 mod m in four u64 limbs -- in memory a 32-byte little-endian
 * integer -- six limbs and 2^384 for the BLS12-377 base field): options "scalars_montgomery" and "points_montgomery" below make the engine
 * read exactly those bytes, the scalars on every MSM call and the points at te_msm_bind_points*.  Those two options do not change
 * record sizes; results are always canonical.
 * A NATIVE PROVER'S SCALAR RECORD: on BLS12-377 G1 the wire format below is a 48-byte record per scalar, a native prover's `Fr` or
 * `BigInt<4>` is 32 bytes.  Option "scalar_record_bytes" = 32 makes every scalar buffer of a BLS12-377 call n x 32 bytes, so that
 * `&[Fr]` (with "scalars_montgomery" = 1) or `&[BigInt<4>]` (without) goes in as it is: no repacking on the CPU, a third fewer bytes
 * over the link.  The 32-byte layout is pinned as written here (four little-endian u64 limbs, least significant first, no padding);
 * it was not checked against the arkworks sources.
 * A NATIVE PROVER'S POINT RECORD: te_msm_bind_points[_device] and te_msm_check_points[_device] take packed x || y by default.  Option
 * "point_stride" makes point i start at byte i * stride, and on BLS12-377 G1 option "point_infinity_flag" reads the byte at offset 96 of
 * every record as "this is the point at infinity".  Together "points_montgomery" = 1, "point_stride" = 104, "point_infinity_flag" = 1 and
 * "scalar_record_bytes" = 32 are meant to be `&[G1Affine]` and `&[Fr]` of arkworks 0.4 on a 64-bit little-endian host, G1Affine being
 * x[48] | y[48] | infinity: bool | 7 bytes of padding = 104 bytes.  That struct layout is pinned as written here; it was not checked
 * against the arkworks sources.
 *
 * All functions return 0 on success or a negative TE_MSM_E* code; te_msm_last_error() gives text.
 * A context is not thread-safe: serialise the calls on one context (the one exception is te_msm_ticket_wait).
 * Every entry point leaves the calling thread's current HIP device as it found it (hipSetDevice is per-thread state that a
 * multi-device context has to change while it works).
 * There is NO CPU fallback: without a usable HIP device te_msm_init fails.
 */
#ifndef TE_MSM_H
#define TE_MSM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct te_ctx te_ctx;

#define TE_MSM_OK            0
#define TE_MSM_EINVAL      (-1)   /* bad argument */
#define TE_MSM_EDEVICE     (-2)   /* HIP error (no device, out of memory, launch failure) */
#define TE_MSM_ESCALAR     (-3)   /* a scalar left a final carry: the reference's "final carry is 1"
                                     (submission/miscellaneous/utils.ts:80-83) */
#define TE_MSM_ESTATE      (-4)   /* call order / capacity */
#define TE_MSM_EPOINT      (-5)   /* an input point failed the check selected by option `check_points` */
#define TE_MSM_EFIELD      (-6)   /* a field element has no result (te_msm_field_op*): see "bad_field_index" / "bad_field_reason" */

/* Why a point failed (option "bad_point_reason", te_msm_check_points*):  */
#define TE_MSM_POINT_NONCANONICAL     1   /* a coordinate >= p (Twisted-Edwards) / q (BLS12-377) */
#define TE_MSM_POINT_OFF_CURVE        2   /* the curve equation fails; BLS12-377: or the map to the twisted-Edwards form is undefined */
#define TE_MSM_POINT_NOT_IN_SUBGROUP  3   /* on the curve, outside the subgroup of prime order */

/* Groups (option "curve").  0: the Twisted-Edwards BLS12 curve of the competition (default; everything above).
 * 1: BLS12-377 G1, y^2 = x^3 + 1 over the 377-bit base field (README.md:57-73, BASELINE config 5): points are
 * n x (x || y) with 48-byte little-endian coordinates (96 bytes), scalars n x 48-byte little-endian records holding
 * values below 2^256 (README.md:325-331) -- or, under option "scalar_record_bytes" = 32, n x 32-byte records --, the result is x || y in 96 bytes (the point at infinity as 96 zero bytes) --
 * `out_xy_le` of te_msm_run / run_device / collect must then hold TE_MSM_RESULT_BYTES_MAX bytes.  Inputs must lie in G1 (the
 * subgroup of prime order r, as the harness generates them): the engine works in the curve's twisted-Edwards form, whose
 * map from y^2 = x^3 + 1 is undefined at the points of order 2 and 4.  As on the other curve, with "check_points" = 0 a
 * coordinate may be any 48-byte value below 2^384 and stands for its residue mod q (x + k q, y + k q for every k that stays
 * below 2^384: 151 for a typical coordinate), bound sets included.  Every entry point serves both curves; partial
 * rows of this curve are TE_MSM_PARTIAL_BYTES_BLS12_377 bytes per window (te_msm_partial_device, te_msm_finalize*). */
#define TE_MSM_CURVE_TE_BLS12      0
#define TE_MSM_CURVE_BLS12_377_G1  1
#define TE_MSM_RESULT_BYTES_MAX    96

#define TE_MSM_POINT_BYTES   64
#define TE_MSM_SCALAR_BYTES  32
#define TE_MSM_X_BYTES              32   /* one x-only point (te_msm_points_from_x): x, little-endian */
#define TE_MSM_X_BYTES_BLS12_377    48   /* the same for BLS12-377 G1: x with two flag bits in byte 47 */
#define TE_MSM_WORKSETS      8    /* MSMs one context can have in flight (submit/collect, partial_device) */
#define TE_MSM_PARTIAL_BYTES 720  /* per window: 5 extended points x 144 B (see te_msm_partial_device) */
#define TE_MSM_PARTIAL_BYTES_BLS12_377 1120   /* the same row for BLS12-377 G1: 5 points x 224 B (14 limbs per coordinate) */

/* Replaces get_device() + per-call buffer/pipeline creation (implementation/cuzk/gpu.ts:14-25,
 * submission.ts:96-97).  The context is persistent: buffers and streams live across calls.
 * n_dev == 1: one GPU.  n_dev > 1: the listed devices (ids may repeat) work for this one context -- this is how a
 * single-process host (the reference's JavaScript, README.md:551 "multi-device" future work) uses a node's GPUs.
 * Two shapes:
 *   MSMs in flight (te_msm_submit / te_msm_submit_async / te_msm_submit_device + te_msm_collect): one WHOLE MSM per
 *     device, a ticket goes to the device with the fewest in flight -- D PCIe links, no replicated bucket reduction, no
 *     row merge.  The throughput form for a caller with several MSMs to do (concurrent compute_msm promises).
 *   the lone call (te_msm_run / te_msm_run_device): every device works on the one MSM:
 *   te_msm_run (host buffers): POINT shards.  Points and scalars are cut into n_dev contiguous slices; one
 *     host thread per device uploads its slice over that device's own PCIe link (the upload is most of a
 *     host-buffer call: 1.85 of 2.47 ms at n = 2^20 on one device) and runs all windows on it; the host tail
 *     folds the sum of the devices' rows.  Window bits follow the slice size.  Option "host_shard_min": fewer
 *     devices are used when a slice would hold fewer points than that (default 4096).
 *   te_msm_run_device (inputs resident on the first device): WINDOW shards; the inputs travel as a scatter + all-gather
 *     over the peer links (slice i to device i, then every device pulls the other slices from their holders:
 *     2 (D - 1) / D of the input leaves the first device instead of D - 1 copies of it), enqueued by one host thread per device.
 * For one-process-per-GPU deployments use n_dev == 1 plus te_msm_set_window_shard / te_msm_partial_device /
 * te_msm_finalize and exchange the partial sums yourself (bench.py does it with an RCCL all-gather). */
int te_msm_init(const int* device_ids, int n_dev, te_ctx** out);
void te_msm_destroy(te_ctx* ctx);
const char* te_msm_last_error(const te_ctx* ctx);   /* ctx may be NULL: last init error */

/* compute_msm(bufferPoints, bufferScalars) -- submission.ts:73-413.  Host buffers; the callee copies
 * them to the device and does not retain them.  out_xy_le receives 64 bytes. */
int te_msm_run(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n,
               uint8_t out_xy_le[64]);

/* Same with inputs already resident in device memory of the context's (first) device. */
int te_msm_run_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n,
                      uint8_t out_xy_le[64]);

/* Pipelined form of te_msm_run_device: te_msm_submit_device enqueues every device stage plus
 * the 11 KB read-back and returns at once with a ticket; te_msm_collect waits for that MSM, runs the host tail and
 * writes the result.  Up to TE_MSM_WORKSETS MSMs may be in flight, each on its own stream and device work set: the host
 * tail of MSM k overlaps the device work of MSM k+1, and on the GPU the launch gaps and the latency-bound reduction tail
 * of one MSM are filled by the wide kernels of the others (the reference's full_benchmarks.ts loop awaits each call; a
 * prover calling MSMs back to back does not have to).
 * Inputs must stay valid AND UNCHANGED until the ticket is collected.  Tickets may be collected in any order (until round 4: in
 * submission order only).
 * Calls in flight that name the SAME point buffer (pointer, n) share one record slab (round 6, option "share_records"): they convert into,
 * and gather from, the same 128 bytes per point instead of one slab per work set -- four MSMs in flight keep their gathers inside the
 * 256 MB Infinity Cache (+4-5 % MSM/s at n = 2^20: profiles/r06_share_records_ab.txt).  And they convert the points ONCE per occupancy
 * run of that slab: a call that joins while another whole-MSM call (a ticket not collected yet, a te_msm_run_device still
 * running) names the same buffer, and finds the conversion of that run complete, skips it (k_part_scatter instead of
 * k_part_scatter_prep: 64 MB read, 128 MB written and three field products per point less).  When the last of them is collected the run
 * ends and the slab forgets it: the buffer may hold other points for the next call.  This is why "unchanged" matters: overwriting a
 * point buffer that a ticket in flight still names, and submitting it again, would gather the old records -- or rewrite them under that
 * ticket.  Checked points (option "check_points"), x-only points and the building blocks te_msm_partial_device[_batch] convert on
 * every call.
 * Contexts of several devices: the inputs may be resident on ANY device of the context (both buffers on the same one); the
 * ticket goes to the device with the fewest MSMs in flight -- ties to the device that holds the inputs -- and a device that
 * does not hold them pulls them over its peer link first (hipMemcpyPeerAsync on the work set's stream; option
 * "stage_device_inputs" = 1 forces that copy even onto the holder: tests on a one-GPU box).  A ticket is a whole MSM there
 * (the window shards of a multi-device context belong to te_msm_run_device).
 * A work set owned by an uncollected ticket is never reused underneath it: te_msm_run / te_msm_run_device move to a
 * free work set (TE_MSM_ESTATE when all TE_MSM_WORKSETS are owned), te_msm_partial_device on such a set returns
 * TE_MSM_ESTATE.  A ticket is consumed by te_msm_collect whether it ends in a result or in TE_MSM_ESCALAR. */
int te_msm_submit_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n, uint64_t* ticket);
int te_msm_collect(te_ctx* ctx, uint64_t ticket, uint8_t out_xy_le[64]);
/* The same pipeline for HOST buffers -- what N concurrent compute_msm() promises of a JavaScript prover map onto
 * (ui/Benchmark.tsx:32 awaits an async call; nothing stops a caller from having several in flight): uploads the buffers
 * (in pieces, like te_msm_run) into the staging area of a free work set, enqueues every device stage and returns a ticket
 * for te_msm_collect.  The call returns when the data has LEFT the caller's buffers (pageable copies are staged by the
 * calling thread; for pinned / hipHostRegister'ed buffers, whose copies are truly asynchronous, the call waits for the last
 * upload), so points_xy_le / scalars_le may be released as soon as it returns; the upload of MSM k+1 overlaps the
 * device work of MSM k.  Contexts of several devices: the ticket goes to the device with the fewest in flight (idle
 * devices in turn); the uploads of consecutive calls still follow each other on the calling thread -- see te_msm_submit_async. */
int te_msm_submit(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, uint64_t* ticket);
/* The same with the upload itself in the background: the call picks device and work set, hands upload + enqueue to that
 * device's host thread and returns AT ONCE.  D calls in a row put D uploads on D PCIe links at the same time -- what a
 * single-threaded caller (the JavaScript event loop behind the N-API addon, a Python prover) needs to keep D devices busy
 * from host buffers: an EXTRAPOLATION from one device -- 8 x (1 / 2.2 ms) MSM/s, eight times the measured one-device rate, against
 * 1 / 0.69 ms for point slices of one call (one device's rehearsed share); two physical devices have never run either.
 * The price: points_xy_le / scalars_le must stay valid and unchanged until te_msm_ticket_wait or te_msm_collect has
 * returned for the ticket.  A failure of the upload or the enqueue (TE_MSM_EDEVICE) is reported by te_msm_collect, which
 * frees the ticket.  Every device has several upload threads (option "upload_threads", default 4): while one ticket's copy is
 * inside the runtime, the next ticket's is being prepared -- on ONE device that alone takes tickets in flight from 2.10 to
 * 1.8-1.9 ms per 2^20-point MSM; the uploads of one device's tickets may therefore complete out of submission order (each owns
 * its work set: nothing depends on the order).  Works on single-device contexts too. */
int te_msm_submit_async(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, uint64_t* ticket);
/* Blocks until the MSM of `ticket` has left the device (its rows are in host memory); te_msm_collect then returns without
 * waiting.  This is the ONE entry point that may be called from another thread while the context is in use elsewhere -- it
 * only waits on the ticket's event -- so a multi-threaded host (libuv's pool under the N-API addon) serialises submit and
 * collect with a lock of its own and waits outside it. */
int te_msm_ticket_wait(te_ctx* ctx, uint64_t ticket);
/* Where a ticket in flight runs: index into the context's device list and the HIP device id there (either may be NULL). */
int te_msm_ticket_device(te_ctx* ctx, uint64_t ticket, int* device_index, int* device_id);

/* ---- resident bases: points bound once, scalars per call ------------------------------------------------------------------
 * The reference's harness hands the SAME bufferPoints to compute_msm for every run of a size (ui/AllBenchmarks.tsx:213-222,
 * submission/miscellaneous/full_benchmarks.ts:63-68,100-105: one buffer, six calls), and a prover runs every MSM over one
 * SRS; te_msm_run re-uploads 64 of its 96 bytes per point and converts the points again on every call.  A bound point set
 * pays that once: te_msm_bind_points uploads the points, converts them to records ON EVERY DEVICE of the context and keeps
 * only the records (128 bytes per point; BLS12-377: 168 bytes, see below); the MSMs over it take scalars alone -- 32 of 96
 * bytes over PCIe, no conversion.  compute_msm's signature (submission.ts:73-78) is untouched: the N-API addon offers
 * setBases(buffer) as an opt-in, after which compute_msm(thatBuffer, scalars) takes this path.
 *   The curve is the one selected at bind time (option "curve"); the MSMs must run under the same curve (TE_MSM_EINVAL
 *   otherwise).  Window bits, digit form, segment length follow the options at the time of each MSM, as for te_msm_run.
 *   BLS12-377 G1: because the conversion is paid once, the bound records are AFFINE -- one inversion per point at bind time
 *   (Montgomery's trick, a fixed Fermat chain per eight points) -- 168-byte records and 7 field products per accumulated
 *   point instead of 224 bytes and 8 (option "bind_affine" = 0 keeps the projective records: A/B measurements).  Results are
 *   identical either way.
 *   A bound set holds device memory until te_msm_release_points or te_msm_destroy (option "bases_bytes" reports it); it may be
 *   released only when no ticket that uses it is in flight (TE_MSM_ESTATE).  The caller's point buffer is not retained.
 * te_msm_bind_points_device: the same from points already resident on a device of the context. */
typedef struct te_bases te_bases;
/* With option "check_points" != 0 the points are checked once, here, at the level in force now (TE_MSM_EPOINT: no handle, no
 * set bound, "bases_bound" unchanged); MSMs over the set never check them again. */
int te_msm_bind_points(te_ctx* ctx, const uint8_t* points_xy_le, uint64_t n, te_bases** out);
int te_msm_bind_points_device(te_ctx* ctx, const void* d_points_xy_le, uint64_t n, te_bases** out);
int te_msm_release_points(te_ctx* ctx, te_bases* bases);
/* number of points of a bound set (0 for NULL) */
uint64_t te_msm_bases_count(const te_bases* bases);
/* compute_msm over a bound set: scalars_le holds te_msm_bases_count(bases) scalars (host memory, the wire format of te_msm_run).
 * One device: the scalars are uploaded and processed in pieces (option "host_chunks"; piece i + 1 crosses PCIe while piece i
 * is sorted and accumulated onto the same buckets).  Several devices: every device takes a slice of the scalars over its own
 * link and the matching slice of its copy of the records (the point shards of te_msm_run without the points). */
int te_msm_run_scalars(te_ctx* ctx, te_bases* bases, const uint8_t* scalars_le, uint8_t out_xy_le[64]);
/* the same with the scalars resident on a device of the context (te_msm_run_device without the points) */
int te_msm_run_scalars_device(te_ctx* ctx, te_bases* bases, const void* d_scalars_le, uint8_t out_xy_le[64]);
/* Tickets over a bound set (te_msm_ticket_wait / te_msm_collect as for every ticket; the ticket goes to the device with the
 * fewest in flight, every device holds the records).  te_msm_submit_scalars is ASYNCHRONOUS like te_msm_submit_async: it
 * returns at once, the upload runs on one of the device's upload lanes, and scalars_le must stay valid and unchanged until
 * te_msm_ticket_wait or te_msm_collect has returned for the ticket.  With MSMs in flight the 32 bytes per point of one MSM cross
 * PCIe (0.6 ms at n = 2^20) under the device work of the others (1.0 ms): the boundary stops being the link. */
int te_msm_submit_scalars(te_ctx* ctx, te_bases* bases, const uint8_t* scalars_le, uint64_t* ticket);
int te_msm_submit_scalars_device(te_ctx* ctx, te_bases* bases, const void* d_scalars_le, uint64_t* ticket);

/* ---- batched MSMs over prefixes of a bound point set -------------------------------------------------------------------------
 * A prover commits to many polynomials of different degrees against ONE SRS: every commitment is an MSM over a PREFIX of the same point
 * set.  te_msm_run_scalars* needs a scalar for every point of the set (a shorter polynomial pays for zero padding), and every MSM is a
 * launch sequence of its own with a latency-bound reduction tail.  These two calls take the whole list:
 *   MSM m = sum_{i < lens[m]} k_{m,i} P_i over the bound set's points.  scalars_le is PACKED: MSM m's lens[m] scalar records start at
 *   record sum_{j<m} lens[j]; the record format is the MSM's own (32 bytes Twisted-Edwards; BLS12-377: 48-byte records, or 32 under option
 *   "scalar_record_bytes").  out receives
 *   `count` results in input order, each encoded as te_msm_run_scalars encodes its result (64 / 96 bytes; the Twisted-Edwards identity as
 *   (0, 1), the BLS12-377 point at infinity as zeros).  lens[m] == 0 gives the identity; count == 0 does nothing.
 *   TE_MSM_EINVAL, out untouched: lens[m] > te_msm_bases_count(bases); a null pointer (lens, out, or the scalars while some lens[m] > 0);
 *   a bases handle of another curve or one already released; a context with a window shard set (te_msm_set_window_shard, step > 1).
 *   TE_MSM_ESCALAR, out untouched: a scalar anywhere in the batch trips the final-carry check (the rule of te_msm_partial_device_batch).
 *   A set bound with "bind_fixed_base" is served from its table 0 (the ordinary records) with the ordinary windows: the same results as
 *   an ordinary set.
 *   How it runs (csrc/batch_plan.hpp): MSMs of at most option "batch_small_max" points (default 2^15) are grouped by
 *   length class (the largest length of a group below twice its smallest) and packed, up to TE_MSM_BATCH_SEQ_MAX of them and within a
 *   scratch budget of 1 GB, into SHARED launch sequences -- one digit launch over all of them (a ragged form of the digit kernel: MSM m
 *   reads its own slice of the packed scalars, entries past its length are digit 0), one sort, one accumulation, one reduction.  Window
 *   bits, digit form and segment length follow the options, with the sequence's largest length standing for n.  Longer MSMs run as
 *   whole-MSM sequences of their own.  The sequences of a device are dealt over its free work sets, up to TE_MSM_WORKSETS in flight (the
 *   call returns TE_MSM_ESTATE when tickets own every set).  The host tails (one fold per MSM) run on up to 8 host threads.
 *   Host form: with several devices, whole MSMs are spread over them, longest first to the least loaded (sum of lengths), and every
 *   device gathers from its own copy of the records.  Device form: the packed scalars lie on one device of the context and the whole
 *   batch runs there.
 *   Synchronous; the calling thread's current device is left as it was.  Read-only option "batch_sequences": the launch sequences the
 *   last batch call ran.  Option "profile" does not apply (no stage times). */
#define TE_MSM_BATCH_SEQ_MAX 64   /* MSMs one shared launch sequence of te_msm_run_scalars_batch holds at most */
int te_msm_run_scalars_batch(te_ctx* ctx, te_bases* bases, int count, const uint64_t* lens, const uint8_t* scalars_le, uint8_t* out);
int te_msm_run_scalars_batch_device(te_ctx* ctx, te_bases* bases, int count, const uint64_t* lens, const void* d_scalars_le, uint8_t* out);

/* ---- MSMs over an indexed subset of a bound point set -----------------------------------------------------------------------------
 * Real scalar vectors over an SRS are mostly zeros (a witness, a selector), touch a few thousand of a million points (a sparse basis) or a
 * strided range of them -- neither the set nor a prefix.  te_msm_run_scalars* makes such a caller zero-pad to te_msm_bases_count(bases)
 * scalars: 32 bytes per BOUND point over PCIe, a digit pass and a sort over n entries, a plan made for n.  These calls take the pairs:
 *   result = sum_{j < m} k_j P_{idx[j]}.  idx: m little-endian u32, each below te_msm_bases_count(bases), in any order, repeats allowed
 *   (the sum is defined either way); scalars_le: m scalar records in the MSM's own format (32 bytes Twisted-Edwards, 48-byte records for
 *   BLS12-377 unless option "scalar_record_bytes" says 32).  m may exceed the set's size and is bounded as n of te_msm_run (m < 2^31).  The result is encoded as te_msm_run_scalars_batch
 *   encodes it (64 / 96 bytes); m == 0 gives the identity.
 *   How it runs (csrc/indexed_plan.hpp): entry j's scalar is record j of the CALL, so the digit pass, the sort and the
 *   schedule run over m entries, and window bits, digit form and segment length follow the options with m standing for n.  The sort's first
 *   level writes idx[j] where it writes the position j for every other call (a kernel of its own: the other paths keep their code), and the
 *   accumulation gathers from the set's records as it always does.  The packed level-1 entries ("packed_sort") give the index 23 bits, and
 *   here the field holds a POINT index: they are used when the SET's count is at most 2^23, whatever m is; larger sets take the general
 *   form.  A set bound with "bind_fixed_base" is served from its table 0 (the ordinary records) with the ordinary windows.
 *   Host form: one device uploads and processes the pairs in pieces (option "scalar_chunks"; each piece carries its slice of both arrays);
 *   several devices take contiguous slices of the m pairs over their own links (as te_msm_run_scalars cuts its scalars; "host_shard_min"
 *   applies to m) -- every device holds all records.  Device form: both buffers lie on ONE device of the context (else TE_MSM_EINVAL) and
 *   the whole MSM runs on that device.
 *   Tickets: te_msm_submit_scalars_indexed[_device] behave as te_msm_submit_scalars[_device] -- the host form is ASYNCHRONOUS (idx as well as
 *   scalars_le must stay valid and unchanged until te_msm_ticket_wait or te_msm_collect has returned for the ticket), the ticket goes to
 *   the device with the fewest in flight (a device that does not hold device-resident pairs pulls them over its peer link), "in_flight"
 *   counts it, tickets are collected in any order, and a set with tickets in flight cannot be released.  m == 0 has no ticket
 *   (TE_MSM_EINVAL, as an empty set has none).
 *   Errors, all with the output untouched and the context usable.  TE_MSM_EINVAL: a null pointer while m > 0; a bases handle that was
 *   released or belongs to the other curve; a context with a window shard set (te_msm_set_window_shard, step > 1).  TE_MSM_ESCALAR: a
 *   scalar trips the final-carry check.  TE_MSM_EINVAL: an index >= te_msm_bases_count(bases); the LOWEST offending position j is reported
 *   in the read-only option "bad_index_position" (-1 before any).  The indices are checked ON THE DEVICE, where they are first read, every
 *   one of them whatever its scalar; a bad index is replaced by a valid one before any address is formed from it (no kernel ever gathers
 *   outside the record slab), the MSM runs to its end and the call -- for a ticket: its te_msm_collect, as with TE_MSM_ESCALAR; other
 *   tickets are not affected -- reports the error instead of a result.
 *   Synchronous calls leave the calling thread's current device as it was.
 * COST (MI355X, a set of 2^20 points, against te_msm_run_scalars* over the zero-padded vector; tools/indexed_sparse.py,
 *   profiles/indexed_subset_sparse.txt).  The identity index list (m = n) prices the translation and the 4 more
 *   bytes per entry: +2 % per MSM with four tickets in flight, host or device buffers (0.98 against 0.97 ms, 0.91 against 0.89 ms),
 *   +9 % for the lone host call (1.51 against 1.38 ms: one more upload call per piece on its critical path); BLS12-377: 0 to +1 % in
 *   flight, +8 % lone.  A dense vector belongs to te_msm_run_scalars*.  At density 1/2 the indexed call gains 1.0-1.2x (the zero digits of a
 *   padded vector are never sorted or accumulated either; what is saved is link bytes), at 1/8 2.1x lone, 3.4x with host tickets in
 *   flight, 1.3x device-resident, at 1/64 3.4x, 7.0x and 1.9x (BLS12-377: 2.4x, 4.9x, 1.4x). */
int te_msm_run_scalars_indexed(te_ctx* ctx, te_bases* bases, const uint32_t* idx, const uint8_t* scalars_le, uint64_t m, uint8_t* out_xy_le);
int te_msm_run_scalars_indexed_device(te_ctx* ctx, te_bases* bases, const void* d_idx, const void* d_scalars_le, uint64_t m, uint8_t* out_xy_le);
int te_msm_submit_scalars_indexed(te_ctx* ctx, te_bases* bases, const uint32_t* idx, const uint8_t* scalars_le, uint64_t m, uint64_t* ticket);
int te_msm_submit_scalars_indexed_device(te_ctx* ctx, te_bases* bases, const void* d_idx, const void* d_scalars_le, uint64_t m, uint64_t* ticket);

/* ---- input-point validation ------------------------------------------------------------------------------------------------
 * The engine trusts its points unless asked: the wire format above says what a caller must pass, and a point that breaks it gives a
 * wrong result, not an error.  Level 1, FORM: both coordinates canonical (below p / q), the curve equation holds
 * (-x^2 + y^2 = 1 + d x^2 y^2, resp. y^2 = x^3 + 1), and for BLS12-377 the map to the engine's twisted-Edwards form is defined
 * (y != 0 and s x + s + 1 != 0: the points of order 2 and 4).  Level 2, FORM + SUBGROUP: also [order] P = O -- the prime-order
 * subgroup of the Twisted-Edwards curve (cofactor 4), resp. G1.  On BLS12-377 only level 2 makes the engine's addition law safe:
 * it is complete on G1 alone.
 * The BLS12-377 point at infinity as an INPUT (96 zero bytes) is rejected as off the curve (0 != 0^3 + 1): the engine's map sends
 * (0, 0) to a record with Z = 0, which is not the neutral element, so it never stood for "nothing" in an MSM.
 * COST: level 1 is a few field products per point -- cheap beside any MSM.  Level 2 is a double-and-add chain over the 251 / 253-bit
 * order, about 3 000 field products per point: meant for te_msm_bind_points (once per point set) and the stand-alone check below;
 * per-call use is allowed and costly (DESIGN.md section "Input-point validation" has the measured times).
 *
 * te_msm_check_points / _device: checks n points (host memory / memory of a device of the context) at `level` (1 or 2) and runs no
 * MSM.  Returns 0 when every point passes (*first_bad = -1, *reason = 0), TE_MSM_EPOINT with *first_bad = the LOWEST failing index
 * and *reason = TE_MSM_POINT_* otherwise.  The curve is option "curve".  Host memory is uploaded in pieces through a buffer of the
 * first device; device memory is checked where it lies. */
int te_msm_check_points(te_ctx* ctx, const uint8_t* points_xy_le, uint64_t n, int level, int64_t* first_bad, int* reason);
int te_msm_check_points_device(te_ctx* ctx, const void* d_points_xy_le, uint64_t n, int level, int64_t* first_bad, int* reason);

/* ---- x-only points -----------------------------------------------------------------------------------------------------------
 * The reference passes its CPU MSM x-coordinates only (Address.msm takes "<x>group" strings): an Aleo group value IS its
 * x-coordinate, and the point is the one with that x in the prime-order subgroup.  These entry points recover y on the device.
 * Curve 0 (Twisted-Edwards BLS12): n x TE_MSM_X_BYTES little-endian x.  y^2 = (a x^2 - 1) / (d x^2 - 1), a = -1, d = 3021; of the two
 *   roots the one whose point lies in the subgroup of order L (one [L] chain decides).  x = 0 gives (0, 1).
 *   Reasons: x >= p TE_MSM_POINT_NONCANONICAL; no root TE_MSM_POINT_OFF_CURVE; neither root in the subgroup (x = +-sqrt(-1), and every
 *   x of the order-4 cosets) TE_MSM_POINT_NOT_IN_SUBGROUP.  The reference's getPointFromX returns (x, -y) in that last case; Address.msm
 *   cannot build such a group, and neither does the engine.
 * Curve 1 (BLS12-377 G1): n x TE_MSM_X_BYTES_BLS12_377 little-endian x with flags in byte 47: bit 7 = y is the larger root
 *   (y > q - y), bit 6 = the point at infinity (rejected, TE_MSM_POINT_OFF_CURVE, as in the uncompressed form); bits 377..381 must be 0
 *   (else TE_MSM_POINT_NONCANONICAL, as x >= q).  y = sqrt(x^3 + 1); no root, y = 0, or s x + s + 1 = 0 (the engine's map to the
 *   twisted-Edwards form undefined): TE_MSM_POINT_OFF_CURVE -- a recovered point always passes check_points level 1.  Recovery does not
 *   decide membership in G1 (both roots share it): option "check_points" = 2 still applies.  The flag layout is meant to be the one
 *   arkworks / snarkVM use for compressed short-Weierstrass points; that could not be verified against them -- pinned as written here.
 * Output: canonical x || y, the wire format above (64 / 96 bytes per point), ready for every other entry point.
 * All four: the curve is option "curve"; on a failure TE_MSM_EPOINT with the LOWEST failing index and its reason (*first_bad / *reason,
 *   and the read-only options "bad_point_index" / "bad_point_reason"), outputs untouched, no MSM run, the context still usable.  Host
 *   x-coordinates are uploaded in pieces through a buffer of the first device; the temporary device memory is freed before the call
 *   returns.  The calling thread's current device is left as it was.
 * te_msm_points_from_x / _device: n points into out (host memory / memory of the device that holds d_x_le: both buffers on one device
 *   of the context, else TE_MSM_EINVAL).  Returns 0 (*first_bad = -1, *reason = 0) when every x has its point.
 * te_msm_bind_points_x: recovers on the first device, then proceeds as te_msm_bind_points_device (conversion on every device, option
 *   "check_points" applied as there).
 * te_msm_run_x: Address.msm's counterpart: uploads x and the scalars to the first device, recovers there, then proceeds as
 *   te_msm_run_device on the recovered points (window shards over several devices, "check_points", TE_MSM_ESCALAR, a 64 / 96-byte
 *   result; its x half is Address.msm's output).
 * COST: recovery is a square root (an exponentiation of ~1 600 field products) plus, for curve 0, the [L] chain of check_points level 2
 *   (~3 000): correct per call, and slower than the MSM itself -- x-only input belongs at bind time. */
int te_msm_points_from_x(te_ctx* ctx, const uint8_t* x_le, uint64_t n, uint8_t* out_points_xy_le, int64_t* first_bad, int* reason);
int te_msm_points_from_x_device(te_ctx* ctx, const void* d_x_le, uint64_t n, void* d_out_points_xy_le, int64_t* first_bad, int* reason);
int te_msm_bind_points_x(te_ctx* ctx, const uint8_t* x_le, uint64_t n, te_bases** out);
int te_msm_run_x(te_ctx* ctx, const uint8_t* x_le, const uint8_t* scalars_le, uint64_t n, uint8_t* out_xy_le);

/* ---- batch scalar multiplication ----------------------------------------------------------------------------------------------
 * out[i] = [k_i] P_i for every i, no sum: the reference's bulkGroupScalarMul / groupScalarMul (utils/wasmFunctions.ts:127-138, Aleo's
 * Address.group_scalar_mul) and FieldMath.multiply (utils/FieldMath.ts:71-84).  The curve is option "curve".
 * Points: the wire format above (64 / 96 bytes); te_msm_mul_x takes x-only points in te_msm_points_from_x's format and recovers them
 *   first (on the device, no host round trip).  Scalars: the MSM's format -- 32-byte little-endian (Twisted-Edwards), 48-byte records
 *   holding values below 2^256 (BLS12-377; bytes 32..47 are not read), 32-byte records there under option "scalar_record_bytes" = 32.
 *   shared_scalar != 0: scalars_le holds ONE scalar, used for all
 *   n points (one account scalar applied to many group values).
 * The result is exactly [k] P for every k below 2^256, with no reduction of k that could be wrong for the input:
 *   Twisted-Edwards: any point of the curve, cofactor part included (the group law is complete on the whole curve; a shared scalar is
 *   reduced mod 4 L, the exponent of the group).  BLS12-377: inputs must lie in G1, as for the MSM (a shared scalar is reduced mod r).
 * Output: canonical affine x || y, 64 / 96 bytes a point.  The Twisted-Edwards identity is (0, 1); the BLS12-377 point at infinity
 *   is 96 zero bytes, as the MSM result encodes it.  n = 0 is a no-op.
 * Bad points: option "check_points" (1, 2) applies to te_msm_mul[_device] as to te_msm_run; te_msm_mul_x reports recovery failures as
 *   te_msm_points_from_x does (and applies "check_points" to the recovered points).  A failure is TE_MSM_EPOINT with the LOWEST failing
 *   index and its reason in the read-only options "bad_point_index" / "bad_point_reason"; the output is untouched.
 * Host buffers: contiguous slices over the context's devices, one host thread per device; each slice is staged on its device (inputs
 *   and results) and copied out only after every slice passed.  Temporary device memory is freed before the call returns.
 * te_msm_mul_device: the points, the scalars and the output on one device of the context (else TE_MSM_EINVAL); returns with the result
 *   complete in d_out.  The calling thread's current device is left as it was.
 * COST: a chain of 256 doublings and 129 additions a point (signed 2-bit windows), about 1.2 / 1.8 x option "check_points" = 2
 *   (Twisted-Edwards / BLS12-377); a shared scalar runs the NAF chain of the subgroup check, about 1.0 / 1.2 x. */
int te_msm_mul(te_ctx* ctx, const uint8_t* points_xy_le, const uint8_t* scalars_le, uint64_t n, int shared_scalar, uint8_t* out_points_xy_le);
int te_msm_mul_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n, int shared_scalar, void* d_out_points_xy_le);
int te_msm_mul_x(te_ctx* ctx, const uint8_t* x_le, const uint8_t* scalars_le, uint64_t n, int shared_scalar, uint8_t* out_points_xy_le);

/* ---- fixed-base batch scalar multiplication -----------------------------------------------------------------------------------
 * out[i] = [k_i] P for ONE point P bound in advance and n scalars: arkworks' FixedBase::msm / batch_mul ([tau^i] G of an SRS, [sk_i] G
 * of many addresses, Pedersen generators).  te_msm_bind_base tabulates [j 2^(W i)] P once (i < M = ceil(257 / W), j = 0 .. 2^(W-1);
 * W = option "mul_base_window", 4..12, default 12, read at bind time), on EVERY device of the context; [k] P is then one table
 * look-up and one mixed addition per window -- no doublings (csrc/mul_base.hip.hpp).
 * te_msm_bind_base: one point in host memory, wire format (64 / 96 bytes), canonical -- option "points_montgomery" is NOT read.  The
 *   curve is option "curve" at bind time; a later call under the other curve, or with a released handle, is TE_MSM_EINVAL with the
 *   output untouched.  Twisted-Edwards: any point of the curve, cofactor part included.  BLS12-377: P must lie in G1.  Option
 *   "check_points" (1, 2) applies to the point: a failure is TE_MSM_EPOINT with "bad_point_index" 0 and its reason, no handle is made
 *   and nothing stays bound.  The table, M (2^(W-1) + 1) entries of 128 bytes a device (0.54 MB at W = 8, 1.7 MB at W = 10, 5.8 MB at
 *   W = 12), is held until te_msm_release_base or te_msm_destroy; it is the only resident memory (read-only options "mul_bases_bound",
 *   "mul_base_bytes": handles bound, bytes held on all devices -- not counted in "bases_bound" / "bases_bytes").
 * te_msm_mul_base[_device]: exactly [k_i] P for every k_i below 2^256, with no reduction of k_i that could be wrong for the input.
 *   Scalars: the MSM's records (32 bytes; BLS12-377: 48-byte records whose bytes 32..47 are not read, or 32-byte records under option
 *   "scalar_record_bytes" = 32, read when the call starts; the bind does not read that option).  Option "scalars_montgomery" is
 *   read when a call starts: with it set a record holds a and the call uses k = a 2^-256 mod m (m = L or r as for the MSMs), decoded
 *   in registers -- a native prover's &[Fr] of powers of tau goes in as it is (te_msm_mul* keep refusing the option).
 *   Output: as te_msm_mul -- canonical affine x || y; the Twisted-Edwards identity is (0, 1), BLS12-377 infinity 96 zero bytes.
 *   n = 0 is a no-op.  Host form: contiguous slices of the scalars over the context's devices, one host thread per device; results are
 *   staged and copied out only when every slice succeeded.  Device form: the scalars and the output on one device of the context
 *   (else TE_MSM_EINVAL); returns with d_out complete.  Every call leaves the calling thread's current device as it found it and
 *   frees its temporaries before it returns.
 * te_msm_base_read (stage verification, as te_msm_bases_read): entries [first, first + count) of window `window` on one device,
 *   at most cap bytes; returns the bytes written, *entry_bytes (optional) receives 128.  An entry is [j 2^(W window)] P, j its index in
 *   the window: Twisted-Edwards hm | hp | dt of 9 words each (te_msm_bases_read's record; entry 0 is the record of (0, 1));
 *   BLS12-377 affine short-Weierstrass x | y of 14 words each in the engine's Montgomery form (entry 0 holds x = y = 0 mod q and is never added).
 * COST (MI355X, device buffers, three alternating rounds, lowest .. highest; tools/mul_base_cost.py, profiles/mul_base_cost.txt), per call
 *   of 2^20 scalars against te_msm_mul_device over the point replicated:
 *     Twisted-Edwards  20.9 .. 21.1 ms replicated;  bound: W = 6 3.01 .. 3.10, W = 8 2.56 .. 2.57, W = 10 2.24 .. 2.28, W = 12 2.08 .. 2.10 ms
 *     BLS12-377        72.0 .. 72.3 ms replicated;  bound: W = 6 11.5 .. 11.7, W = 8 9.59 .. 9.71, W = 10 8.33 .. 8.47, W = 12 7.66 .. 7.75 ms
 *   W = 12 is lowest in every round at every size measured (2^10 .. 2^20), hence the default.  Of a W = 12 call the affine pass
 *   (k_scalar_mul_affine, unchanged) is 0.82 of 1.9 ms / 3.5 of 7.5 ms kernel time.  The bind took 1.7 .. 2.8 ms (Twisted-Edwards) and
 *   5.2 .. 7.5 ms (BLS12-377) per table on one device, W = 6 .. 12. */
typedef struct te_base te_base;
int te_msm_bind_base(te_ctx* ctx, const uint8_t* point_xy_le, te_base** out);
int te_msm_release_base(te_ctx* ctx, te_base* base);
int te_msm_mul_base(te_ctx* ctx, te_base* base, const uint8_t* scalars_le, uint64_t n, uint8_t* out_points_xy_le);
int te_msm_mul_base_device(te_ctx* ctx, te_base* base, const void* d_scalars_le, uint64_t n, void* d_out_points_xy_le);
int64_t te_msm_base_read(te_ctx* ctx, const te_base* base, int device_index, uint32_t window, uint32_t first, uint32_t count, void* dst, uint64_t cap,
                         int* entry_bytes);

/* ---- batched group addition and point-set sums ---------------------------------------------------------------------------------
 * te_msm_add*: out[i] = A_i + B_i for every i -- the reference's bulkAddGroups / addGroups (utils/wasmFunctions.ts:112-119).
 * te_msm_sum*: ONE point, the sum of all P_i -- the reference's reduceGroups (utils/wasmFunctions.ts:121-125).  With them, results the
 * engine leaves in device memory are combined there: a Pedersen commitment [v_i] G + [r_i] H is two te_msm_mul_base_device calls and one
 * te_msm_add_device; an accumulator update acc[i] += new[i] is te_msm_add_device with d_out = d_a.  The curve is option "curve".
 * flags: TE_MSM_ADD_SUBTRACT out[i] = A_i - B_i; TE_MSM_ADD_SHARED_B b holds ONE point, used for every i.  Any other bit: TE_MSM_EINVAL.
 *   Negation and doubling are SUBTRACT from the identity and add(a, a).
 * Points: the wire format above (64 / 96 bytes).  te_msm_add_x / te_msm_sum_x take x-only points in te_msm_points_from_x's format, with
 *   its recovery and its rules (on the device, no host round trip).  Output: canonical affine x || y exactly as te_msm_mul writes it --
 *   the Twisted-Edwards identity is (0, 1), the BLS12-377 point at infinity 96 zero bytes.  n = 0: add is a no-op, sum returns the
 *   identity ((0, 1), or zeros).  n < 2^31, as for te_msm_mul.
 * Exact for: Twisted-Edwards -- any two points of the curve, cofactor part included (A = B, A = -B, the identity, the points of order 2
 *   and 4: one complete addition).  BLS12-377 -- inputs in G1, as for te_msm_mul; and because these calls PRODUCE the all-zero record,
 *   the full-point forms also ACCEPT it as the point at infinity, so add(add(a, b), c) or sum(add(a, b)) never needs a host fix-up.
 *   te_msm_add_x / te_msm_sum_x keep te_msm_points_from_x's rules and refuse infinity.
 * Buffers: te_msm_add_device -- a, b (one point under SHARED_B) and out on one device of the context, else TE_MSM_EINVAL; d_out may be
 *   exactly d_a or exactly d_b (partial overlap is the caller's error and is not detected); returns with d_out complete.  te_msm_add may
 *   likewise be called with out == a.  te_msm_sum_device: the points on one device of the context; the result goes to HOST memory, as
 *   an MSM's.  Host forms: contiguous slices over the context's devices, one host thread per device, each slice staged on its device;
 *   results are copied out only when every slice passed.  te_msm_sum on several devices reduces every slice on its device and adds the
 *   partial results on the first.  Temporaries are freed before return; the calling thread's current device is left as it was.
 * Bad points: option "check_points" 1 / 2 applies to both operands of add and to sum's input, before anything is written -- in THESE
 *   calls the all-zero BLS12-377 record passes both levels.  A failure is TE_MSM_EPOINT with the output untouched; "bad_point_index" /
 *   "bad_point_reason" hold the LOWEST failing pair index and its reason, and the read-only option "bad_point_operand" which operand
 *   failed: 0 = a / the sum's input, 1 = b (-1 before any failure; at equal index a is reported before b; a failing shared b is
 *   reported at index 0).  The _x forms report recovery failures the same way, then apply "check_points" to the recovered points.
 * Options "points_montgomery", "point_stride" and "point_infinity_flag" are NOT read: these are per-call point paths, like te_msm_mul*.
 * How it runs (csrc/group_add.hip.hpp): one lane per pair and one complete addition into a projective slot, then
 *   the affine pass; pieces of TE_MSM_GROUP_ADD_PIECE pairs share one temporary buffer.  The sum runs a grid of at most
 *   TE_MSM_GROUP_SUM_GRID blocks of 256 lanes, each lane adding points i, i + stride, ..; a block folds to one partial, a second launch
 *   of one block folds the partials, and one point is normalised.  Both constants are also the read-only options "group_add_piece" /
 *   "group_sum_grid".
 * COST (MI355X, device buffers, three alternating rounds, lowest .. highest; tools/group_add_cost.py, profiles/group_add_cost.txt):
 *   te_msm_add_device at 2^20 pairs: 0.71 .. 0.78 ms (Twisted-Edwards), 1.69 .. 1.74 ms (BLS12-377) a call, of which k_group_add is
 *   0.10 / 0.29 ms and the affine pass (k_scalar_mul_affine, unchanged) 0.43 / 1.27 ms; the host path it replaces spends 3.5 / 5.3 ms
 *   on the link alone (both operands down, the result up, pinned memory).  A block-wide batch inversion in the affine pass's place
 *   (one inversion per 2048 points) measured 0.82 .. 0.85 / 1.69 .. 1.72 ms against 0.78 .. 0.79 / 1.71 .. 1.75 ms in the same rounds:
 *   not lower in every round on either curve, so it is not in the library.  te_msm_sum_device against te_msm_run_device over
 *   all-ones scalars: 2^16 points 0.12 against 0.29 ms / 0.41 against 0.63 ms, 2^20 points 0.23 .. 0.24 against 0.56 ms / 0.83 .. 0.86
 *   against 1.22 .. 1.23 ms, and no scalar buffer to make. */
#define TE_MSM_ADD_SUBTRACT 1
#define TE_MSM_ADD_SHARED_B 2
#define TE_MSM_GROUP_ADD_PIECE (1u << 21)
#define TE_MSM_GROUP_SUM_GRID 1024u
int te_msm_add(te_ctx* ctx, const uint8_t* a_xy_le, const uint8_t* b_xy_le, uint64_t n, int flags, uint8_t* out_xy_le);
int te_msm_add_device(te_ctx* ctx, const void* d_a, const void* d_b, uint64_t n, int flags, void* d_out);
int te_msm_add_x(te_ctx* ctx, const uint8_t* ax_le, const uint8_t* bx_le, uint64_t n, int flags, uint8_t* out_xy_le);
int te_msm_sum(te_ctx* ctx, const uint8_t* points_xy_le, uint64_t n, uint8_t* out_xy_le);
int te_msm_sum_device(te_ctx* ctx, const void* d_points_xy_le, uint64_t n, uint8_t* out_xy_le);
int te_msm_sum_x(te_ctx* ctx, const uint8_t* x_le, uint64_t n, uint8_t* out_xy_le);

/* ---- batched field arithmetic ---------------------------------------------------------------------------------------------------
 * te_msm_field_op*: out[i] = a_i op b_i for every i -- the reference's bulkAddFields, bulkSubFields, bulkMulFields, bulkDoubleFields,
 * bulkInvertFields, bulkPowFields, bulkPowFields17 and bulkSqrtFields (utils/wasmFunctions.ts), so that a vector of field elements in
 * device memory stays there between the calls that use it.  Aleo's `field` is the integers mod p, the base field of the Twisted-Edwards
 * curve -- and the same p is BLS12-377's scalar field: a vector of Aleo fields on the device is also the &[Fr] a BLS12-377 prover hands
 * to te_msm_run_scalars_device / te_msm_submit_scalars_device (option "scalars_montgomery" for its native residues).
 * field: TE_MSM_FIELD_P    p = 8444461749428370424248824938781546531375899335154063827935233455917409239041, 32-byte elements
 *        TE_MSM_FIELD_Q377 q, BLS12-377's base field (the modulus of the 48-byte coordinates above), 48-byte elements
 *   The field is an argument, not option "curve": p serves both curves.
 * op:    TE_MSM_FIELD_ADD a + b, SUB a - b, MUL a b, POW a^b read b;  DOUBLE 2 a, NEG -a, SQUARE a^2, INV 1 / a, SQRT take a alone:
 *   b must be NULL and TE_MSM_FIELD_SHARED_B clear, else TE_MSM_EINVAL.
 * flags: TE_MSM_FIELD_SHARED_B    b holds ONE record, used for every i (the addend, the factor, the exponent: bulkPowFields17 is POW
 *                                 with the shared exponent 17)
 *        TE_MSM_FIELD_MONTGOMERY  a, b (not an exponent) and out hold v * 2^256 mod p / v * 2^384 mod q: a native prover's residues
 *        TE_MSM_FIELD_ZERO_OK     INV only: the inverse of 0 is 0 (arkworks' batch_inversion) instead of a failure
 *   Any other bit, an unknown op or field, or ZERO_OK on another op: TE_MSM_EINVAL, the output untouched.
 * Values: little-endian, 32 / 48 bytes.  ANY 256- / 384-bit value is accepted and stands for its residue (the reference does the
 *   same: its add_fields(p, 1) is 1); outputs are canonical (< p, < q).  Under MONTGOMERY a stored value likewise stands for its
 *   residue, and the output is the canonical residue of result * 2^256 / result * 2^384.  An exponent is ALWAYS a plain 256-bit
 *   integer in a 32-byte record, on both fields and under MONTGOMERY, used as that integer without reduction; 0^0 = 1, as the
 *   reference has it.  sqrt(0) = 0.  n = 0: a no-op.  n < 2^31, as for te_msm_mul.
 * WHICH SQUARE ROOT: the numerically smaller one, r <= (m - 1) / 2 (under MONTGOMERY: of the value r, not of its residue form).  The
 *   reference returns whichever root its Tonelli-Shanks lands on (sqrt(4) = p - 2, sqrt(3) the small root): no rule to reproduce.
 * Failures: INV of 0 without ZERO_OK and SQRT of a non-square are TE_MSM_EFIELD (the reference's WASM traps on both) with the output
 *   untouched and the context usable.  The read-only options "bad_field_index" (-1 before any failure) and "bad_field_reason"
 *   (0 before any; TE_MSM_FIELD_ZERO, TE_MSM_FIELD_NOT_SQUARE) hold the LOWEST failing index into the caller's whole buffer and its reason.
 * Buffers: te_msm_field_op_device -- a, b (one record under SHARED_B) and out on one device of the context, else TE_MSM_EINVAL; d_out
 *   may be exactly d_a or exactly d_b (partial overlap is the caller's error and is not detected; POW on TE_MSM_FIELD_Q377 refuses
 *   d_out == d_b, whose records differ in size, with TE_MSM_EINVAL); returns with d_out complete.  te_msm_field_op: contiguous slices
 *   over the context's devices, one host thread per device, each slice staged on its device; results are copied out only when every
 *   slice passed; out may be a.  Temporaries are freed before return; the calling thread's current device is left as it was.
 * How it runs (csrc/field_ops.hip.hpp): one lane per element, 256-lane blocks.  add / sub / double / neg are one
 *   or two field products on the raw limbs and a conditional subtraction, the same code in both forms; mul / square two products.
 *   INV without ZERO_OK first runs a scan for zero residues (one product and compares per element) and waits for its verdict; the
 *   inversion is Montgomery's trick, one Fermat chain per TE_MSM_FIELD_INV_GROUP elements of a lane (read-only option
 *   "field_inv_group"), the prefix products in a slab of the call's own (48 / 64 bytes an element, pieces of 2^20).  POW with
 *   per-element exponents is 384 products in fixed 2-bit windows; a shared exponent runs square-and-multiply from its top bit (17: five
 *   products).  SQRT is the x-recovery's root (te_msm_points_from_x) and writes into a temporary of n elements, copied on success.
 * COST (MI355X, device buffers, three alternating rounds, lowest .. highest; tools/field_ops_cost.py, profiles/field_ops_cost.txt):
 *   n = 2^20 elements, p / q: add 0.029 .. 0.032 / 0.038 .. 0.041 ms, sub 0.034 .. 0.037 / 0.048 .. 0.053, mul 0.035 .. 0.037 / 0.048 .. 0.053 (the
 *   same under MONTGOMERY), double, neg and square between add and mul; INV 0.49 .. 0.53 / 1.19 .. 1.33 ms (with ZERO_OK, no scan:
 *   0.46 .. 0.50 / 1.17 .. 1.24); POW per element 2.70 .. 2.82 / 6.33 .. 6.41 ms, with the shared exponent 17 0.071 .. 0.072 / 0.115 ..
 *   0.120; SQRT 8.52 .. 8.65 / 21.7 .. 21.9 ms.  At 2^16: the map ops 0.015 .. 0.020 ms (a launch), INV 0.47 .. 0.48 / 1.20 .. 1.21 ms --
 *   as long as at 2^20: an inversion is the latency of one lane's chain until the device is full -- POW 0.24 / 0.65, SQRT 0.77 .. 0.95 /
 *   2.69 .. 2.76 ms.  Chains of 1, 8, 16, 32, 64 elements at 2^20 (ZERO_OK, the candidates alternating): p 2.74 .. 2.84, 0.63 .. 0.67,
 *   0.49 .. 0.52, 0.52 .. 0.57, 0.61 .. 0.66 ms; q 7.90 .. 8.10, 1.26 .. 1.30, 1.15 .. 1.24, 1.28 .. 1.34, 1.59 .. 1.64 ms -- 16 is the
 *   lowest in every round on both fields, and the trick buys 5.6x / 6.8x over n independent chains.  The floor, a device copy of the
 *   same bytes: 0.022 / 0.025 ms at 2^20 -- add is within 1.5x of it, an inversion 23x / 47x above.  Host form at 2^20 (pageable
 *   memory, through the Python method): MUL 17.4 .. 20.5 / 25.1 .. 27.2 ms, INV 19.4 .. 22.9 / 25.0 .. 37.0 ms, against 1.8 / 2.7 and
 *   1.2 / 1.8 ms for the same bytes over the link from pinned memory: the host form is the staging copies, not the arithmetic. */
#define TE_MSM_FIELD_P 0
#define TE_MSM_FIELD_Q377 1
#define TE_MSM_FIELD_ADD 0
#define TE_MSM_FIELD_SUB 1
#define TE_MSM_FIELD_MUL 2
#define TE_MSM_FIELD_DOUBLE 3
#define TE_MSM_FIELD_NEG 4
#define TE_MSM_FIELD_SQUARE 5
#define TE_MSM_FIELD_INV 6
#define TE_MSM_FIELD_POW 7
#define TE_MSM_FIELD_SQRT 8
#define TE_MSM_FIELD_SHARED_B 1
#define TE_MSM_FIELD_MONTGOMERY 2
#define TE_MSM_FIELD_ZERO_OK 4
#define TE_MSM_FIELD_ZERO 1
#define TE_MSM_FIELD_NOT_SQUARE 2
#define TE_MSM_FIELD_INV_GROUP 16u
int te_msm_field_op(te_ctx* ctx, int field, int op, const uint8_t* a, const uint8_t* b, uint64_t n, int flags, uint8_t* out);
int te_msm_field_op_device(te_ctx* ctx, int field, int op, const void* d_a, const void* d_b, uint64_t n, int flags, void* d_out);

/* ---- batched NTTs ---------------------------------------------------------------------------------------------------------------
 * te_msm_ntt*: `count` number-theoretic transforms of n = 2^log_n elements each over p (TE_MSM_FIELD_P: Aleo's `field`, BLS12-377's
 * Fr), the radix-2 domains of arkworks / snarkVM (Radix2EvaluationDomain): the step of a Marlin / KZG prover between its pointwise
 * arithmetic (te_msm_field_op_device) and its commitments (te_msm_run_scalars_device), so that the vector stays on the device.
 * a holds the count transforms back to back, 32-byte little-endian records, natural order in and out.
 *   W = 22^((p - 1) / 2^47) mod p = 8065159656716812877374967518403273466521432693661810619979959746626482506078 (order 2^47: arkworks'
 *   TWO_ADIC_ROOT_OF_UNITY), w = W^(2^(47 - log_n)), s = the shift (1 when `shift` is NULL):
 *     forward                       out[j] = sum_i a_i s^i w^(i j)                     (coset_fft with generator s)
 *     TE_MSM_NTT_INVERSE            out[i] = s^-i n^-1 sum_j a_j w^(-i j)              (coset_ifft: undoes the forward with the same s)
 * shift: a HOST pointer to one 32-byte record in both forms, or NULL.
 * flags: TE_MSM_NTT_INVERSE; TE_MSM_NTT_MONTGOMERY -- a, s and out hold v * 2^256 mod p (a native prover's residues).  Any other bit:
 *   TE_MSM_EINVAL.
 * Values: as te_msm_field_op -- ANY 256-bit value stands for its residue, outputs are canonical.  log_n = 0 is the reduced copy.
 *   count = 0 succeeds and touches nothing.
 * Refusals, all TE_MSM_EINVAL with the output untouched and the context usable: log_n > TE_MSM_NTT_MAX_LOG_N; an unknown flag bit;
 *   s = 0 mod p (s = p included), in either direction; NULL a / out with count > 0; count * n * 32 beyond 64 bits; te_msm_ntt_device:
 *   d_a and d_out not on one device of the context.
 * Buffers: out may be exactly a (partial overlap is the caller's error).  te_msm_ntt_device returns with d_out complete.  te_msm_ntt
 *   slices WHOLE transforms over the context's devices, one host thread per device, each slice staged on its device (one transform
 *   runs on one device).  Every element and byte offset is 64 bits wide: count * n * 32 may pass 2^32.  A shift's tables (384 KB) and the
 *   host form's staged copies are freed before return; the buffer between the passes of a multi-pass size (the records of the call's
 *   transforms, at most 2^24 elements: 512 MB) is the device's, grown on use and kept until te_msm_trim / te_msm_destroy -- allocating
 *   32 MB per call cost more than the three passes over it.  The calling thread's device is left as it was.
 * How it runs (csrc/ntt_plan.hpp, csrc/ntt.hip.hpp): one kernel; a 256-lane block stages a tile of 2^10 elements
 *   in LDS as 9 x 29-bit limbs and runs up to 10 radix-2 stages on it, one field product a butterfly.  n <= 2^10: one launch, 2^(10 -
 *   log_n) transforms a block.  n <= 2^16: two passes, above: three (2^24 = 8 + 8 + 8), over a buffer of the call's own; the last pass
 *   writes natural order (no bit-reversal pass).  Twiddles: w^e = hi[e >> 12] lo[e & 4095] from two tables of 4096 powers of a root of
 *   order 2^24 (384 KB a device, built on the device at the first transform, kept until te_msm_trim / te_msm_destroy; the inverse
 *   reads them at the negated index).  Read-only options: "ntt_max_log_n"; "ntt_table_bytes" and "ntt_scratch_bytes" (what the context's devices hold now
 *   of tables, and of the buffer between passes).
 * COST (MI355X, device form, in place, three alternating rounds, lowest .. highest; tools/ntt_cost.py, profiles/ntt_cost.txt), forward /
 *   inverse: 1024 x 2^10 0.095 .. 0.103 / 0.101 .. 0.107 ms; 16 x 2^16 0.145 .. 0.159 / 0.154 .. 0.158; 2^20 0.193 .. 0.210 / 0.199 ..
 *   0.208 (with a shift 0.225 .. 0.242); 2^24 2.70 .. 3.08 / 2.53 .. 2.67 ms.  Beside them, in the same rounds: a device copy of the same
 *   bytes times the passes 0.021, 0.030, 0.040, 0.61 ms; te_msm_field_op_device(MUL) over n log_n / 2 elements a transform 0.102, 0.151 ..
 *   0.156, 0.186 .. 0.193, 3.76 .. 3.84 ms -- the products bind everywhere, and a transform costs 0.72x .. 1.04x of that yardstick.
 *   The link alone of the host round trip the device form replaces: 1.19 ms for 2^20 elements, 18.7 ms for 2^24. */
#define TE_MSM_NTT_INVERSE 1
#define TE_MSM_NTT_MONTGOMERY 2
#define TE_MSM_NTT_MAX_LOG_N 24u
int te_msm_ntt(te_ctx* ctx, const uint8_t* a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, uint8_t* out);
int te_msm_ntt_device(te_ctx* ctx, const void* d_a, uint32_t log_n, uint64_t count, int flags, const uint8_t* shift, void* d_out);

/* ---- polynomial openings --------------------------------------------------------------------------------------------------------
 * te_msm_poly_divide*: evaluate `count` polynomials over p (TE_MSM_FIELD_P, the records of te_msm_ntt) at a point each and divide them
 * by X - z: the opening of a KZG / Marlin / Varuna round, between the inverse transform (te_msm_ntt_device) and the opening's MSM
 * (te_msm_run_scalars_device), so that the coefficients stay on the device.  Polynomial k is a[k n .. k n + n - 1], 32-byte
 * little-endian records, lowest coefficient first; n is ANY length from 1 to TE_MSM_POLY_MAX_N.  Its point z_k is record k of z, or
 * record 0 under TE_MSM_POLY_SHARED_Z.  With h_(n-1) = a_(n-1) and h_i = a_i + z h_(i+1):
 *     evals[k]       = h_0 = a(z)
 *     q[k n + i]     = h_(i+1), i < n - 1      the witness polynomial (a(X) - a(z)) / (X - z)
 *     q[k n + n - 1] = 0
 * The quotient keeps the stride n: q may be exactly a, and te_msm_run_scalars_batch_device takes it with the lengths n - 1.
 * z and evals are HOST pointers in both forms (a challenge comes from the host's transcript, an evaluation goes back into it).  Either
 *   evals or q may be NULL: with q NULL the call only evaluates -- it reads a once and writes nothing on the device but its scratch.
 * flags: TE_MSM_POLY_MONTGOMERY -- a, z, evals and q hold v * 2^256 mod p; TE_MSM_POLY_SHARED_Z.  Any other bit: TE_MSM_EINVAL.
 * Values: as te_msm_field_op -- ANY 256-bit coefficient or point stands for its residue (z = 0 and z = p are one point), outputs are
 *   canonical.  count = 0 succeeds and touches nothing.
 * Refusals, all TE_MSM_EINVAL with every output untouched and the context usable: n = 0 or n > TE_MSM_POLY_MAX_N; an unknown flag bit;
 *   evals and q both NULL; NULL a or z with count > 0; count * n * 32 beyond 64 bits (or more than 2^31 - 1 tiles in one launch);
 *   te_msm_poly_divide_device: d_a and d_q not on one device of the context.  evals is written only when the call succeeds.
 * Buffers: te_msm_poly_divide_device returns with d_q complete.  te_msm_poly_divide slices WHOLE polynomials over the context's devices,
 *   one host thread per device, each slice staged on its device.  Every element and byte offset is 64 bits wide.  The tile sums, the
 *   carries and the powers of the points live in a buffer of the device's (about count * n / T records), grown on use and kept until
 *   te_msm_trim / te_msm_destroy.  The calling thread's device is left as it was.
 * How it runs (csrc/poly_plan.hpp, csrc/poly.hip.hpp): a 256-lane block owns a tile of T = 256 chunk coefficients
 *   of one polynomial.  k_poly_sums leaves S_b = sum_k a_(bT+k) z^k for every tile; the carries h_(bT) are the quotient of S(X) by
 *   X - z^T -- the same call on ceil(n / T) coefficients, recursed until one tile is left, whose sum is a(z); k_poly_apply takes a
 *   tile's carry, scans its lanes and writes h_(i+1) at i (skipped when q is NULL).  z is in Montgomery form, coefficients never are:
 *   a step is one product and one normalised sum, and both forms run the same code.  chunk: TE_MSM_POLY_CHUNK (measured), or what the
 *   environment variable TE_MSM_POLY_CHUNK names (1 .. 16), read by every call -- and never more than one tile needs to cover n, so that
 *   a batch of short polynomials (1024 x 2^10) fills its blocks.  Read-only options: "poly_chunk" (the chunk in force),
 *   "poly_scratch_bytes" (what the context's devices hold now of that buffer).
 * COST (MI355X, device form, in place, one shared point, three alternating rounds, lowest .. highest; tools/poly_cost.py,
 *   profiles/poly_cost.txt), with the quotient / evaluation only: 1024 x 2^10 0.124 .. 0.132 / 0.061 .. 0.066 ms; 16 x 2^16 0.139 .. 0.143 /
 *   0.070 .. 0.071; 2^20 0.136 / 0.065 .. 0.067; 2^24 0.96 .. 1.05 / 0.28 .. 0.40 ms.  Beside them, in the same rounds: a device copy of the
 *   bytes the call moves (two reads and a write / one read) 0.026 / 0.019 ms at 2^20 elements and 0.31 / 0.11 ms at 2^24;
 *   te_msm_field_op_device(MUL) over n elements 0.035 and 0.28 .. 0.29 ms; the pinned link time of 32 n bytes down and up -- what the call
 *   replaces -- 1.19 ms and 18.7 ms.  Chunk 8 was the lowest of 4, 8 and 16 in every round at 2^20 and 16 x 2^16 (32 does not fit LDS). */
#define TE_MSM_POLY_MONTGOMERY 1   /* a, z, evals, q hold v * 2^256 mod p */
#define TE_MSM_POLY_SHARED_Z 2     /* z is ONE record, used for every polynomial */
#define TE_MSM_POLY_MAX_N (1ull << 30)
#define TE_MSM_POLY_CHUNK 8u
int te_msm_poly_divide(te_ctx* ctx, const uint8_t* a, uint64_t n, uint64_t count, const uint8_t* z, int flags, uint8_t* evals, uint8_t* q);
int te_msm_poly_divide_device(te_ctx* ctx, const void* d_a, uint64_t n, uint64_t count, const uint8_t* z, int flags, uint8_t* evals, void* d_q);

/* ---- prefix sums and products ---------------------------------------------------------------------------------------------------
 * te_msm_field_scan*: the running sum or running product of `count` vectors over p (TE_MSM_FIELD_P, the records of te_msm_ntt), each
 * from a seed: the grand product z_(i+1) = z_i num_i / den_i of a permutation or lookup argument (num / den from te_msm_field_op_device),
 * the running sums of logUp, the powers s g^i of one record (into te_msm_mul_base_device: an SRS), and the total of a vector -- so that
 * these vectors stay on the device.  Vector k is a[k n .. k n + n - 1], 32-byte little-endian records; n is ANY length from 1 to
 * TE_MSM_SCAN_MAX_N.  op: TE_MSM_SCAN_SUM or TE_MSM_SCAN_PRODUCT; write o for + or * mod p and e_k for record k of init:
 *     out[k n + i] = e_k o a_0 o .. o a_i          inclusive
 *     out[k n + i] = e_k o a_0 o .. o a_(i-1)      TE_MSM_SCAN_EXCLUSIVE: out[k n] = e_k
 *     totals[k]    = e_k o a_0 o .. o a_(n-1)      in both modes
 * init and totals are HOST pointers in both forms, `count` records each (a seed comes from the caller's previous call -- a scan continues
 *   across calls with it -- or from the transcript, and a total goes back there).  init is not modified; NULL stands for the identity (0
 *   for the sum, 1 for the product).  Either totals or out may be NULL: with out NULL the call reads a once and writes nothing on the
 *   device but its scratch.  totals is written only when the call succeeds.
 * flags: TE_MSM_SCAN_MONTGOMERY -- a, init, totals and out hold v * 2^256 mod p; TE_MSM_SCAN_EXCLUSIVE; TE_MSM_SCAN_SHARED_A -- a holds
 *   `count` records, and vector k is record k repeated n times (init * g^i, init + i g).  Any other bit: TE_MSM_EINVAL.
 * Values: as te_msm_field_op -- ANY 256-bit record stands for its residue, outputs are canonical.  A zero among the factors of a product
 *   is an ordinary value: nothing inverts.  count = 0 succeeds and touches nothing.  The result is the same bytes every time.
 * Aliasing: out may be exactly a, except under TE_MSM_SCAN_SHARED_A (the two have different sizes).
 * Refusals, all TE_MSM_EINVAL with every output untouched and the context usable: an unknown op or flag bit; n = 0 or
 *   n > TE_MSM_SCAN_MAX_N; totals and out both NULL; NULL a with count > 0; count * n * 32 beyond 64 bits (or more than 2^31 - 1 tiles in
 *   one launch); out = a under TE_MSM_SCAN_SHARED_A; te_msm_field_scan_device: d_a and d_out not on one device of the context.
 * Buffers: te_msm_field_scan_device returns with d_out complete.  te_msm_field_scan slices WHOLE vectors over the context's devices, one
 *   host thread per device, each slice staged on its device.  Every element and byte offset is 64 bits wide.  The tile totals, the
 *   carries and the seeds live in a buffer of the device's (about count * n / T records), grown on use and kept until te_msm_trim /
 *   te_msm_destroy.  The calling thread's device is left as it was.
 * How it runs (csrc/scan_plan.hpp, csrc/scan.hip.hpp): a 256-lane block owns a tile of T = 256 chunk elements of
 *   one vector.  k_scan_totals leaves every tile's total; the carries are the exclusive scan of the totals -- the same call on
 *   ceil(n / T) records, recursed until one tile is left, whose carry is the seed; k_scan_apply takes a tile's carry, scans its lanes and
 *   writes the values (skipped when out is NULL).  chunk: TE_MSM_SCAN_CHUNK, or what the environment variable TE_MSM_SCAN_CHUNK names
 *   (1 .. 16), read by every call -- and never more than one tile needs to cover n.  Read-only options: "scan_chunk" (the chunk in
 *   force), "scan_scratch_bytes" (what the context's devices hold now of that buffer).
 * COST: DESIGN.md section 25, profiles/scan_cost.txt (tools/scan_cost.py). */
#define TE_MSM_SCAN_SUM 0
#define TE_MSM_SCAN_PRODUCT 1
#define TE_MSM_SCAN_MONTGOMERY 1   /* a, init, totals, out hold v * 2^256 mod p */
#define TE_MSM_SCAN_EXCLUSIVE 2    /* out[i] leaves a_i out: out[0] = init */
#define TE_MSM_SCAN_SHARED_A 4     /* vector k is ONE record a[k], used for every i: init * g^i, init + i g */
#define TE_MSM_SCAN_MAX_N (1ull << 30)
#define TE_MSM_SCAN_CHUNK 8u
int te_msm_field_scan(te_ctx* ctx, int op, const uint8_t* a, uint64_t n, uint64_t count, int flags, const uint8_t* init, uint8_t* totals, uint8_t* out);
int te_msm_field_scan_device(te_ctx* ctx, int op, const void* d_a, uint64_t n, uint64_t count, int flags, const uint8_t* init, uint8_t* totals, void* d_out);

/* ---- sparse matrices --------------------------------------------------------------------------------------------------------------
 * te_msm_bind_matrix / te_msm_spmv*: products of a sparse matrix over p (TE_MSM_FIELD_P, the records of te_msm_ntt) with `count`
 * vectors -- the Az, Bz, Cz every R1CS prover (Groth16, Marlin, Varuna) starts with, and Varuna's products with the transposed matrices.
 * The matrices are fixed per circuit and the assignment changes per proof: bind once, as te_msm_bind_points binds the bases, then move
 * only the vector -- or leave it on the device, where te_msm_ntt_device takes the result.
 * Matrix: CSR from HOST memory, bound on EVERY device of the context.  row_ptr has rows + 1 entries, row_ptr[0] = 0, nnz = row_ptr[rows];
 *   row r holds the entries row_ptr[r] .. row_ptr[r + 1] - 1: column col_idx[e] (any order inside a row; a repeated column is summed;
 *   empty rows are allowed) and the 32-byte little-endian value vals[32 e ..].  The arrays are not read after the bind returns.
 * Result:  out[k * rows + r] = sum_e vals[e] * x[k * cols + col_idx[e]] mod p  over the entries e of row r, for k < count.
 *   Under TE_MSM_SPMV_TRANSPOSE the same for the transposed matrix: x is count x rows, out is count x cols.  A call may ask for it only
 *   if the bind kept the transpose (TE_MSM_MATRIX_TRANSPOSE: twice the device memory).
 * Montgomery forms: TE_MSM_MATRIX_MONTGOMERY -- vals hold v * 2^256 mod p; TE_MSM_SPMV_MONTGOMERY -- x and out do.  Independent of
 *   each other: the product is linear in x, the bind stores every value once in the engine's own form, and one code path serves both.
 * Values: as te_msm_field_op -- ANY 256-bit record stands for its residue, outputs are canonical.  count = 0 succeeds and touches nothing.
 * Refusals, all TE_MSM_EINVAL with every output untouched and the context usable.  Bind: rows or cols 0 or above 2^31; row_ptr[0] != 0 or
 *   a row_ptr that is not monotone; a column index >= cols (its lowest position: read-only option "bad_index_position"); a NULL array
 *   with nnz > 0 (row_ptr: always); an unknown flag bit; more than 2^40 entries.  Call: an unknown flag bit; TRANSPOSE on a matrix bound
 *   without it; a matrix that is not bound to this context; NULL x or out; out == x (the kernel gathers from x: never in place); byte
 *   counts beyond 64 bits (or more than 2^31 - 1 blocks in one launch); te_msm_spmv_device: d_x and d_out not on one device of the context.
 * Buffers: te_msm_spmv_device returns with d_out complete -- EVERY record written, empty rows as 0, whatever d_out held.  te_msm_spmv
 *   slices WHOLE vectors over the context's devices, one host thread per device.  Every element and byte offset is 64 bits wide.  The
 *   fragments of rows that span tiles (two records a tile and vector) live in a buffer of the device's, grown on use and kept until
 *   te_msm_trim / te_msm_destroy.  te_msm_destroy frees matrices left bound.  The calling thread's device is left as it was.
 * How it runs (csrc/spmv_plan.hpp, csrc/spmv.hip.hpp): a 256-lane block owns a tile of T = 256 chunk consecutive
 *   ENTRIES, cut by position, never by row -- a row of 2^20 entries (the constant column's row of a transpose) is 1024 tiles like any
 *   others.  k_spmv_tile forms the products, sums runs of equal row inside a lane and across the lanes with a segmented scan, and writes
 *   the rows that lie inside the tile; k_spmv_rows writes the empty rows and sums the fragments of rows that span tiles.  No atomics:
 *   the result is the same bytes every time.  chunk: TE_MSM_SPMV_CHUNK, or what the environment variable TE_MSM_SPMV_CHUNK names
 *   (1 .. 16), read by every call.  Read-only options: "spmv_chunk" (the chunk in force), "matrix_bytes" (what the context's devices
 *   hold of bound matrices: 0 once all are released), "spmv_scratch_bytes" (what they hold now of the fragment buffer).
 * COST: DESIGN.md section 24, profiles/spmv_cost.txt (tools/spmv_cost.py). */
typedef struct te_matrix te_matrix;
#define TE_MSM_MATRIX_MONTGOMERY 1   /* vals hold v * 2^256 mod p */
#define TE_MSM_MATRIX_TRANSPOSE 2    /* keep the transpose too: calls may then pass TE_MSM_SPMV_TRANSPOSE */
#define TE_MSM_SPMV_MONTGOMERY 1     /* x and out hold v * 2^256 mod p */
#define TE_MSM_SPMV_TRANSPOSE 2      /* multiply by the transposed matrix */
#define TE_MSM_SPMV_CHUNK 4u
int te_msm_bind_matrix(te_ctx* ctx, uint64_t rows, uint64_t cols, const uint64_t* row_ptr, const uint32_t* col_idx, const uint8_t* vals, int flags, te_matrix** out);
int te_msm_release_matrix(te_ctx* ctx, te_matrix* matrix);
int te_msm_matrix_shape(const te_matrix* matrix, uint64_t* rows, uint64_t* cols, uint64_t* nnz);
int te_msm_spmv(te_ctx* ctx, te_matrix* matrix, const uint8_t* x, uint64_t count, int flags, uint8_t* out);
int te_msm_spmv_device(te_ctx* ctx, te_matrix* matrix, const void* d_x, uint64_t count, int flags, void* d_out);

/* Options (the reference hard-codes these: chunk_size submission.ts:80, dispatch table :109-142).
 *   "scalars_montgomery" 0 (default) = scalar records hold the integers themselves (the wire format above); 1 = every scalar record holds
 *                   a = k * 2^256 mod m and the MSM uses k = a * 2^-256 mod m, where m is the scalar field of the curve in force:
 *                     TE_MSM_CURVE_TE_BLS12      L = 2111115437357092606062206234695386632838870926408408195193685246394721360383
 *                     TE_MSM_CURVE_BLS12_377_G1  r = 8444461749428370424248824938781546531375899335154063827935233455917409239041
 *                   ANY 256-bit a is accepted and stands for its residue; the decoded k is canonical (< m), so under the option signed digits
 *                   never return TE_MSM_ESCALAR on the Twisted-Edwards curve, and on BLS12-377 only for a non-zero byte 32..47 of a 48-byte
 *                   record (the value is in bytes 0..31, as always; a 32-byte record -- "scalar_record_bytes" -- then holds just a).  The reduction runs where the scalars are first read, in the digit
 *                   kernels (csrc/scalar_form.hpp: 8 rounds over 32-bit words, ~70 multiply-accumulates a scalar, in registers): no pass
 *                   over the scalars of its own, nothing for the caller to convert.  Read when a call STARTS, by: te_msm_run[_device],
 *                   te_msm_submit / _async / _device, te_msm_run_scalars[_device], te_msm_submit_scalars[_device],
 *                   te_msm_run_scalars_batch[_device], te_msm_run_scalars_indexed[_device], te_msm_submit_scalars_indexed[_device],
 *                   te_msm_partial_device[_batch]; MSMs over a "bind_fixed_base" set included, with their fallback to the ordinary
 *                   windows.  A ticket keeps the form it was submitted with: changing the option affects later calls only.
 *                   te_msm_mul* and te_msm_run_x take canonical scalars only: with the option set they return TE_MSM_EINVAL and leave the
 *                   output untouched (a silent canonical reading would be a wrong answer).
 *                   COST: not measured yet.  tools/montgomery_inputs.py times the option on against off and the CPU pass it takes off
 *                   the caller; until its output is filed, take the option as a convenience of unknown cost.
 *   "scalar_record_bytes" 0 (default) = the curve's own scalar record: 32 bytes on the Twisted-Edwards curve, 48 on BLS12-377 G1.  32 on BLS12-377:
 *                   EVERY scalar buffer of a call is n x 32 bytes little-endian -- where the 48-byte record held a value in bytes 0..31 and
 *                   zeros above, there is now just the value.  48 on BLS12-377 and 32 on the Twisted-Edwards curve are the defaults spelled
 *                   out; 8 and 16 are the narrow records described at the end of this entry; any other value is TE_MSM_EINVAL here.  48 on the Twisted-Edwards curve is TE_MSM_EINVAL when a call starts, its
 *                   output untouched (option "curve" may change after this one was set).  Read when a call STARTS, by every entry point
 *                   that reads "scalars_montgomery" (above) and by te_msm_run_x, te_msm_mul[_device], te_msm_mul_x and
 *                   te_msm_mul_base[_device].  It sizes every buffer the call reads: host uploads and their pieces ("host_chunks",
 *                   "scalar_chunks"), the packed buffer of te_msm_run_scalars_batch* (MSM m starts at record sum lens[j], in records of
 *                   this size), the pairs of the indexed calls, peer copies and the "peer_bytes" they count.  A ticket keeps the size it was
 *                   submitted with, as it keeps its scalar form: changing the option affects later calls only.  Composes with
 *                   "scalars_montgomery".  Unchanged: TE_MSM_ESCALAR under signed digits from about 2^254 - 2^240 up (exactly: from
 *                   2^(cW) - sum_w 2^(cw + c - 1), which at 17 windows of 15 bits is 2^254 - 2^239 - 2^224 - ...);
 *                   te_msm_bind_base builds its table from records of its own and does not read the option; te_msm_synth_inputs_bls12_377
 *                   writes 48-byte records.  The digit kernels take the record size at run time; te_msm_mul* and te_msm_mul_base* run
 *                   another instantiation of their kernels; the existing ones keep their code (profiles/native_layout_isa.txt).
 *                   MEASURED (MI355X, n = 2^20 over a bound set, scalars from host memory; profiles/native_layout_cost.txt): the lone
 *                   te_msm_run_scalars call 2.49-2.57 ms with 32-byte records against 2.61-2.67 ms with 48-byte ones, an MSM with four
 *                   tickets in flight 2.10-2.11 against 2.21-2.22 ms.
 *                   8 and 16, on BOTH curves: the scalars are a native &[u64] / &[u128] -- little-endian integers of that size, no padding --
 *                   for every entry point above except te_msm_mul* and te_msm_mul_base*, which return TE_MSM_EINVAL with the output
 *                   untouched.  With 8 the width stands for "scalar_bits" (64; a smaller one may be set, a larger one is TE_MSM_EINVAL when
 *                   a call starts).  16 is accepted only while "scalar_bits" is set (1..128: set it FIRST, 128 for full u128 values); with
 *                   "scalar_bits" at 0 the value 16 is TE_MSM_EINVAL here, as it always was, and a call that finds 16 with the width reset to 0
 *                   is TE_MSM_EINVAL when it starts.  With "scalars_montgomery" = 1 such a call is TE_MSM_EINVAL, output untouched: a residue is 32 bytes.
 *                   Device pointers of the _device forms must be aligned to the record size, else TE_MSM_EINVAL.  The digit kernels run
 *                   instantiations of their own (loads of the record's size, a working value of 2 / 4 words, only the windows that width
 *                   can have); the existing ones keep their code (profiles/narrow_scalars_isa.txt).
 *   "scalar_bits"   0 (default) = nothing declared; b in 1..256: the caller declares every scalar below 2^b (with "scalars_montgomery": the
 *                   decoded k), and the plan covers only what b needs.  With c0 the window size the plan would choose anyway
 *                   ("window_bits", else from n) and g = 2 for signed digits, 0 for unsigned: W = ceil((b + g) / c0) windows of c = c0 bits (the
 *                   smallest size with that count, max(4, ceil((b + g) / W)), measured 19-56 % slower at n = 2^20: set "window_bits"
 *                   to run it).  b = 253 signed and b = 256 unsigned give the counts of 0.  te_msm_plan reports the
 *                   narrow c and W (what te_msm_partial_device* produce and te_msm_finalize* take).  CONTRACT: every scalar below 2^b is
 *                   accepted and the result is exact; a scalar at or above the exact limit of the plan -- 2^(cW) - sum_{w<W} 2^(cw + c - 1)
 *                   signed, 2^(cW) unsigned -- is TE_MSM_ESCALAR with the output untouched; anything between is accepted and exact;
 *                   no scalar ever gives a wrong result.  Read when a call STARTS by every entry point that reads "scalars_montgomery",
 *                   and by te_msm_run_x; a ticket keeps the width it was submitted with.  te_msm_mul* and te_msm_mul_base* do not read
 *                   it.  A set bound with "bind_fixed_base" serves such a call from its table 0 with the ordinary windows.  Window shards:
 *                   on a context whose te_msm_set_window_shard step exceeds W a call is TE_MSM_EINVAL (a shard would hold no window); a
 *                   lone te_msm_run[_scalars]_device on a context of more devices than W runs whole on the device that holds the inputs.
 *                   MEASURED: profiles/narrow_scalars_cost.txt.
 *   "point_stride"  0 (default) = packed points; else the bytes from one point record to the next: point i starts at byte i * stride, x and y
 *                   are its first 2 x 32 / 2 x 48 bytes, and the bytes behind the pair (and the flag byte, below) are never interpreted.
 *                   A multiple of 8 from the pair size (64 / 96) up to 128, else TE_MSM_EINVAL here -- 128 because a block stages its 256
 *                   records through 32 KB of LDS (csrc/strided.hip.hpp); arkworks' G1Affine is 104.  Read at BIND time, like
 *                   "points_montgomery", by te_msm_bind_points[_device] and te_msm_check_points[_device], on both curves; a stride below
 *                   the pair size of the curve in force then is TE_MSM_EINVAL with no handle.  Device pointers of the _device forms must
 *                   be 8-byte aligned while a stride is set (TE_MSM_EINVAL otherwise); nothing issues a 16-byte load from the caller's
 *                   buffer.  Host points travel whole at the bind (n * stride bytes) and in pieces cut at record boundaries in the
 *                   checks.  The records of a set bound at a stride are those of the same points bound packed, bit for bit, so every
 *                   MSM over the set (ordinary, batch, indexed, tickets, fixed-base windows) is unchanged; multi-device contexts convert
 *                   on every device.  te_msm_bind_points_x, te_msm_bind_base and the per-call point paths (te_msm_run*, te_msm_submit*,
 *                   te_msm_partial_device*, te_msm_mul*) do NOT read it.  The packed path keeps its kernels and their code.
 *   "point_infinity_flag" 0 (default) or 1; BLS12-377 G1 only; read at bind time with "point_stride".  With 1 the byte at offset 96 of every
 *                   record is a flag, so the stride must be at least 104 (else the bind is TE_MSM_EINVAL; on the Twisted-Edwards curve a
 *                   bind or check with the option set is TE_MSM_EINVAL: (0, 1) is an ordinary input there).  A flagged record is the point
 *                   at infinity: its x and y bytes are not looked at (arkworks stores zeros there; the engine does not care) and its
 *                   record is the neutral element of the twisted-Edwards form, which the additions take as an ordinary operand: in every
 *                   MSM over the set it contributes nothing, whatever its scalar or digit sign; an MSM whose contributing points are all
 *                   flagged returns 96 zero bytes.  With "check_points" 1 or 2 at the bind, and in te_msm_check_points* while the option is
 *                   set, a record whose flag byte is 1 passes both levels and a flag byte other than 0 or 1 is
 *                   TE_MSM_POINT_NONCANONICAL at its index (lowest index first, as for every other failure); with "check_points" = 0 any
 *                   non-zero flag byte means infinity.
 *                   MEASURED (MI355X, 2^20 points from host memory; profiles/native_layout_cost.txt): the bind of arkworks' image (stride 104, flag
 *                   option, Montgomery coordinates) 4.11-4.13 ms against 3.92-3.95 ms for packed canonical points.
 *   "points_montgomery" 0 (default); 1 = te_msm_bind_points[_device] read coordinates as Montgomery residues: x * 2^256 mod p in 32 bytes
 *                   (Twisted-Edwards), x * 2^384 mod q in 48 bytes (BLS12-377).  Read at BIND time, like "bind_affine": the conversion
 *                   kernels take another constant in their first products, no more arithmetic; the records, and every MSM over the set
 *                   (ordinary and fixed-base), are identical to those of the set bound from canonical coordinates.  With "check_points" = 0
 *                   any 256- / 384-bit value stands for its residue, as above.  "check_points" at the bind, and te_msm_check_points[_device]
 *                   while the option is set, decode the same way: "canonical" stays "the STORED value is below p / q", the curve equation
 *                   and the subgroup are checked on the decoded coordinates.  The per-call point paths (te_msm_run*, te_msm_submit*,
 *                   te_msm_partial_device*, te_msm_mul*) do NOT read this option -- their points, and their "check_points", stay canonical --
 *                   and te_msm_bind_points_x keeps its own x-only format.
 *   "window_bits"   c in [4,16]; 0 = choose from n (default)
 *   "signed_digits" 1 = signed window digits, 2^(c-1) buckets per window (default; the reference's shipped behaviour,
 *                   miscellaneous/utils.ts:52-95); 0 = plain unsigned windows, 2^c buckets (utils.ts:34-50): same
 *                   result, accepts any 256-bit scalar (no final-carry error)
 *   "curve"         TE_MSM_CURVE_TE_BLS12 (default) or TE_MSM_CURVE_BLS12_377_G1, see above
 *   "sort_buckets"  1 = schedule buckets by descending size (default), 0 = natural order
 *   "segment_len"   a bucket longer than this is accumulated by several threads and the parts summed afterwards; 0 = from n
 *                   (default: twice the mean bucket size as a power of two in [16, 64]; read-only "segment_len_used" reports
 *                   what the last MSM ran with)
 *   "profile"       1 = HIP events around the dominant kernel (accumulate) only, 2 = around every stage
 *                   (te_msm_stage_ms); 0 = none (default)
 *   "host_chunks"   te_msm_run / te_msm_submit: pieces the point buffer (of one device's slice) is uploaded and processed
 *                   in, so that PCIe transfer and device work overlap; 0 = from n (3 from 3 * 2^18 points, 2 from 2^17,
 *                   else 1), 1 = whole.  Twisted-Edwards: all scalars go first, in one copy (the link is the bottleneck);
 *                   BLS12-377: scalars piece by piece with their points (the device is).  The result does not depend on it.
 *   "host_shard_min" multi-device te_msm_run: smallest slice worth a device of its own (default 4096 points)
 *   "upload_threads" host threads per device that take te_msm_submit_async / te_msm_submit_scalars tickets (1..16, default 4; env
 *                   TE_MSM_UPLOAD_THREADS).  Scalars-only tickets (bound bases) cross the link one at a time per device whatever the
 *                   number of threads (side by side they only delay each other: profiles/r06_bound_host_tickets_gap.txt).
 *                   A lane thread waits for each of its uploads on the host before it enqueues the kernels that read it (a stream wait in
 *                   front of them would hold up other tickets' kernels in a shared hardware queue).  The calling thread of te_msm_run* /
 *                   te_msm_submit waits the same way when its buffers are pageable (the copy call blocks for the copy anyway); pinned
 *                   buffers keep the stream waits.  No packet of the upload path enters a hardware queue shared with other tickets'
 *                   kernels (profiles/r06_caller_host_waits.txt).
 *   "host_staging"  0 (default) = host buffers are copied straight from the caller's memory: the fastest form while the caller
 *                   REUSES its buffers (the runtime keeps pages it has copied from registered: 2.35 ms per 2^20-point call), but
 *                   the first call on a buffer costs 4.7-5.0 ms and a caller that allocates fresh buffers for every call pays
 *                   4.4-27 ms per call (profiles/r05_host_buffers_first_touch.txt).  1 = the engine copies the buffers, 2 MB at a
 *                   time, with a crew of eight host threads into a pinned ring of the work set (32 MB, allocated on first use)
 *                   and uploads from there: the same cost whatever the history of the caller's memory (env TE_MSM_HOST_STAGING).
 *                   A caller that can register its arena once (hipHostRegister) should do that instead and keep 0.
 *   "queue_probe"   1 (default) = the first te_msm_submit_device on a device measures the hardware queues of its work sets' streams
 *                   (see te_msm_workset_stream); 0 = never (env TE_MSM_QUEUE_PROBE=0).  te_msm_probe_queues does it on request.
 *                   te_msm_submit / te_msm_submit_async never trigger it: a host-buffer ticket is bound by its upload
 *                   (until round 4 they did: 16 ms at the first submit).
 *   "workset"       which of the TE_MSM_WORKSETS device work sets te_msm_run* / te_msm_partial_device use (default 0)
 *   "stage_device_inputs"  see te_msm_submit_device (default 0)
 *   "bind_affine"   1 (default) = te_msm_bind_points converts BLS12-377 points to AFFINE records (one inversion per point, once);
 *                   0 = keeps the projective records of the per-call conversion (A/B measurements).  Read at bind time.
 *   "bind_fixed_base" c in [16, 21] (0 = off, default): te_msm_bind_points (Twisted-Edwards curve) also tabulates 2^(c w) P_i for the
 *                   ceil(255 / c) windows w (W x 128 bytes per point: 1.7 GB for c = 20 at n = 2^20, built once).  MSMs over such a set run
 *                   FIXED-BASE WINDOWS: every window's digit addresses the SAME set of 2^(c-1) buckets, so c can grow: 13 n + 2^20 additions
 *                   at c = 20 where 16-bit windows need 16 n + 2^20, and no window doublings in the host tail (csrc/kernels.hip.hpp,
 *                   "FIXED-BASE WINDOWS"; measurements: profiles/r06_fixed_base_windows.txt).  Same results.  The rows
 *                   of such an MSM are sized for well-spread digits; badly skewed scalars (all equal, ...) overflow one, which the engine
 *                   detects and answers by running that MSM again with the ordinary windows (read-only option "fixed_base_fallbacks"
 *                   counts them).  A lone call on several devices runs on ONE of them (one bucket set: nothing to shard); tickets use all.
 *                   "window_bits", "signed_digits", "segment_len" = 0 do not apply to such MSMs; a window-sharded single-device context
 *                   keeps the ordinary windows.  Read at bind time.
 *   "share_records" 1 (default) = whole-MSM calls from device-resident inputs (te_msm_submit_device, te_msm_run_device) that name the same
 *                   point buffer while in flight share one record slab and convert it once per occupancy run, see te_msm_submit_device;
 *                   2 = shared slabs, every call converts (the round-6 form); 0 = one slab per work set, every call converts (A/B; env
 *                   TE_MSM_SHARE_RECORDS).  Read-only "record_slabs": slabs allocated; read-only "record_conversions": point -> record
 *                   conversions the context's MSM launch sequences have enqueued (one per launch that converts; bound point sets
 *                   not included).
 *   "scalar_chunks" te_msm_run_scalars / te_msm_submit_scalars: pieces the scalars of a bound point set are uploaded and processed
 *                   in; 0 = from n (default), 1 = whole.  The result does not depend on it.
 *   "batch_small_max" te_msm_run_scalars_batch*: MSMs of at most this many points share launch sequences, longer ones run alone
 *                   (default 32768; 0 = every MSM alone).  The result does not depend on it.  Read-only "batch_sequences": see there.
 *   "mul_base_window" W in [4, 12] (default 12, the fastest measured): window bits of the table te_msm_bind_base builds, see "fixed-base batch scalar
 *                   multiplication" above.  Read at bind time; a handle keeps the W it was bound with.  Read-only "mul_bases_bound",
 *                   "mul_base_bytes": see there.
 *   read-only:      "num_devices", "segment_len_used", "peer_copies" / "peer_bytes" (hipMemcpyPeerAsync calls a multi-device
 *                   context issued, and the bytes they moved), "entries_accumulated" (non-zero window digits of the MSM whose
 *                   result was fetched last, counted on the device: the points k_accumulate gathered -- all windows of this
 *                   context's shard, all MSMs of a batch; bench.py prices its roofline with it),
 *                   "bases_bytes" (device memory held by bound point sets, all devices), "bases_bound" (how many sets),
 *                   "fixed_base_fallbacks" (fixed-base MSMs answered by the ordinary windows after a row overflow),
 *                   "in_flight" (tickets not collected, all devices), "streams_final" (te_msm_workset_stream's handles will not change any
 *                   more), "device_bytes" (device memory held in work-set buffers, see te_msm_trim)
 *   "check_points"  0 (default) = points are not checked (the launch sequence of every call is exactly the unchecked one);
 *                   1 = form, 2 = form + subgroup (see "input-point validation" above), read when a call starts: te_msm_run, te_msm_run_device,
 *                   te_msm_submit, te_msm_submit_async, te_msm_submit_device, te_msm_bind_points[_device].  The points are checked
 *                   BEFORE the MSM is enqueued -- host buffers in pieces through a buffer of their own (one more pass over PCIe), device
 *                   buffers where they lie (multi-device te_msm_run_device: on the device that holds them, before the scatter).  On a
 *                   failure the call returns TE_MSM_EPOINT and leaves out_xy_le untouched; tickets: te_msm_submit* still hands out the
 *                   ticket and ITS te_msm_collect returns TE_MSM_EPOINT (other tickets are not affected; te_msm_submit_async checks on
 *                   its upload lane).  MSMs over a bound set are not checked again.  te_msm_partial_device[_batch] refuse to run with
 *                   the option set (TE_MSM_EINVAL): use te_msm_check_points_device in front of them.  The context stays usable.
 *   read-only:      "bad_point_index" (the lowest failing index -- into the caller's whole buffer -- of the last call that returned
 *                   TE_MSM_EPOINT, -1 before any), "bad_point_reason" (its TE_MSM_POINT_* code, 0 before any)
 *   read-only:      "bad_index_position" (te_msm_run_scalars_indexed*: the lowest position j -- into the caller's whole list -- whose index was
 *                   not below te_msm_bases_count(bases), of the last call or collect that failed on one; -1 before any)
 *   "prezero"       1 (default) = a work set's block of counters is cleared BEHIND an MSM's read-back, for its next MSM
 *                   (the next MSM starts with its first kernel instead of a fill); 0 = cleared in front of every MSM --
 *                   te_msm_debug_read of "bucket_count" / "num_segments" / "partials" needs 0 (it refuses otherwise)
 *   "packed_sort"   1 (default) = the sort's level-1 entries are one 32-bit word (index | key << 23 | sign << 31) where n <= 2^23:
 *                   4 bytes per entry instead of 6; 0 = the general form (u16 key + u32 index; what larger n always uses).
 *                   Same result (A/B measurements, tests; env TE_MSM_PACKED)
 *   "fold_pairs"    1 (default) = a fold level of the bucket reduction with 32 768 .. 65 535 outputs (n <= 2^18) runs two lanes per
 *                   output -- half the dependent additions; 0 = one thread per output (A/B measurements; env TE_MSM_FOLD_PAIRS) */
int te_msm_set_option(te_ctx* ctx, const char* key, int64_t value);
int te_msm_get_option(te_ctx* ctx, const char* key, int64_t* value);

/* ---- window-sharded building blocks (multi-GPU: one process per GPU) --------------------------
 * This context computes windows w = first + k*step (k >= 0) of every MSM.  Default: first 0, step 1.
 * Number of windows W of a plan: ceil(255 / c) for signed digits (scalars below 2^254 - 2^240; 17 windows of 15 bits, 16 of
 * 16), ceil(256 / c) for unsigned ones; te_msm_plan reports it. */
int te_msm_set_window_shard(te_ctx* ctx, int first, int step);
/* Geometry for n points under the current options: window bits c and total number of windows W. */
int te_msm_plan(te_ctx* ctx, uint64_t n, int* window_bits, int* num_windows);
/* Runs every device stage for this context's windows and leaves the partial sums in DEVICE memory:
 * d_partials is W x TE_MSM_PARTIAL_BYTES; only the rows of this context's windows are written
 * (others untouched -- zero the buffer first; an all-zero row means "window not present").
 * Row w = [ T | W0 | W1 | W2 | W3 ]: T = sum of the window's buckets, Wk = sum_v v * (sum of the buckets whose index has
 * digit k equal to v), digits of (c+2-k)/4 bits; as extended points (x|y|z|t, each 9 limbs of 29 bits in
 * u32 words, Montgomery form R = 2^261, lazily reduced).  Asynchronous on `stream`: any hipStream_t (NULL is HIP's
 * default stream, which is also what PyTorch calls its default stream), or TE_MSM_OWN_STREAM for the context's
 * private stream; returns after enqueueing. */
#define TE_MSM_OWN_STREAM ((void*)(intptr_t)-1)
int te_msm_partial_device(te_ctx* ctx, const void* d_points_xy_le, const void* d_scalars_le, uint64_t n,
                          void* d_partials, void* stream);
/* `count` (1..TE_MSM_MAX_BATCH) MSMs of the same n in ONE sequence of launches: MSM m reads d_points_xy_le[m] /
 * d_scalars_le[m] (arrays of device pointers, in host memory, read before the call returns) and its W rows go to
 * d_partials + m * W * row bytes.  The windows of the batch are sorted, accumulated and reduced together, as if they were
 * count x (windows of this shard) windows of one MSM: what a rank of a D-GPU window-sharded job needs, because its W/D windows per
 * MSM are too little work for a launch sequence of their own (rehearsed per-rank step at D = 8: 0.25 ms per MSM one by one,
 * 0.17 ms in batches of eight).  MSMs of one call that name the SAME point buffer share one conversion
 * of it (same pointer in one call = same data; nothing is remembered across calls) -- a prover's batch over one SRS converts
 * it once per call; the scalars of all MSMs are decomposed by one launch.  There is no reference
 * counterpart: the reference awaits one compute_msm at a time (full_benchmarks.ts:97-110).  A scalar out of range anywhere
 * in the batch fails the whole batch (te_msm_partial_wait).  Same work set and stream rules as te_msm_partial_device. */
#define TE_MSM_MAX_BATCH 8
int te_msm_partial_device_batch(te_ctx* ctx, const void* const* d_points_xy_le, const void* const* d_scalars_le, uint64_t n,
                                int count, void* d_partials, void* stream);
/* A context owns TE_MSM_WORKSETS device work sets (option "workset" selects the one te_msm_partial_device uses), so a
 * caller can keep that many MSMs in flight on as many streams: their kernels overlap on the GPU.  te_msm_partial_wait blocks until the
 * last te_msm_partial_device call on that work set has finished and returns its status (TE_MSM_ESCALAR if a scalar was
 * out of range). */
int te_msm_partial_wait(te_ctx* ctx, int workset);
/* The private stream of a work set (what TE_MSM_OWN_STREAM selects) as a hipStream_t, for callers that order their own work
 * -- a collective, a copy -- behind te_msm_partial_device without a host round trip (PyTorch: torch.cuda.ExternalStream).
 * LIFETIME: a handle returned here stays a VALID hipStream_t until the process exits.  te_msm_destroy synchronises the streams
 * of a context whose handles were handed out and parks them (the next context on the same device takes them over) instead of
 * destroying them, because callers remember such handles where the engine cannot see them: PyTorch's pinned-memory allocator
 * records an event on every stream a pinned block was used on when the block is released -- for a tensor that outlives the
 * context, after te_msm_destroy or at interpreter exit -- and hipEventRecord on a destroyed stream aborts the process (round 5:
 * tools/exp_batch_small.py; profiles/r06_batch_small_abort.txt, tests/test_gpu_stream_export.py).  What the caller still owes:
 * work it enqueues on the handle AFTER te_msm_destroy is ordered with whatever the next owner of the stream runs there -- finish
 * (synchronise) your own work on the handle before the context goes away.
 * The FIRST te_msm_submit* of a context (not te_msm_init: one-shot callers never pay the ~16 ms) measures which of
 * its streams the runtime put on the same hardware queue (kernels of one queue run in order; see csrc/te_msm.hip,
 * spread_streams_over_queues), twice, and -- when both measurements agree -- re-deals them so that work sets 0..3, and 4..7,
 * sit on different queues: MSMs in flight on the context's own streams overlap whatever other streams the process has
 * created.  The measurement waits for the context's own streams only (no device-wide synchronisation: other streams of the
 * process keep running).  The handles may change at that call: query them after it, or call te_msm_probe_queues first
 * (option "streams_final" tells).  *hw_queue_class (optional) receives the measured class of the work set's stream, -1
 * before the measurement, when it is off (option "queue_probe" = 0) or when its two passes disagreed (creation order kept). */
int te_msm_workset_stream(te_ctx* ctx, int workset, void** stream, int* hw_queue_class);
/* Runs that measurement NOW (about 16 ms; nothing of this context may be in flight), at a quiet moment the caller chooses,
 * and fixes the work sets' streams for the life of the context.  Returns the number of hardware-queue classes found
 * (0: the two passes disagreed, creation order kept) or a negative error. */
int te_msm_probe_queues(te_ctx* ctx);
/* Gives device memory back: frees the buffers (about 0.7 GB each at n = 2^20) of the idle work sets numbered >=
 * keep_worksets, staging areas included (they are allocated on first use and otherwise held until te_msm_destroy -- fine on
 * 288 GB, unfriendly next to a prover).  Work sets owned by an uncollected ticket are skipped.  Returns the number of
 * work sets freed.  A later call simply allocates again. */
int te_msm_trim(te_ctx* ctx, int keep_worksets);
/* Host tail (replaces submission.ts:362-412: de-Montgomery, sum, Horner, toAffine): folds the W rows
 * (host memory; rows of absent windows all-zero are skipped as identity) into the affine result.
 * Waits for, and reports a pending TE_MSM_ESCALAR of, the last te_msm_partial_device call of this context.  The digit
 * form (signed / unsigned) is the one that call ran with, whatever the option says now; window_bits and num_windows
 * must be that call's (te_msm_plan), otherwise TE_MSM_ESTATE -- rows from elsewhere go to te_msm_finalize_host_ex. */
int te_msm_finalize(te_ctx* ctx, const uint8_t* partials, int window_bits, int num_windows,
                    uint8_t out_xy_le[64]);

/* The same tail without a context (pure host code, no device needed): used when the rows were produced
 * elsewhere, e.g. gathered from other ranks.  Does not know about scalar-range errors. */
int te_msm_finalize_host(const uint8_t* partials, int window_bits, int num_windows, uint8_t out_xy_le[64]);
/* Which form of the host tail's arithmetic this process uses: bit 0 = the mulx / adcx / adox field product (BMI2 + ADX; Twisted-Edwards
 * curve), bit 1 = the AVX-512 IFMA accumulator of both curves (the four coordinates of the running point in vector lanes: two vector
 * products per doubling; about half the time of the scalar form).  Both forms are checked against the portable one at te_msm_init; env
 * TE_MSM_HOST_TAIL=scalar turns bit 1 off, TE_MSM_HOST_MUL=c both (A/B measurements, tests). */
int te_msm_host_tail_features(void);
/* Same for either digit form: bucket_bits = window_bits - 1 (signed digits, what te_msm_finalize_host assumes) or
 * window_bits (option "signed_digits" = 0). */
int te_msm_finalize_host_ex(const uint8_t* partials, int window_bits, int bucket_bits, int num_windows, uint8_t out_xy_le[64]);
/* The tail for an all-gathered buffer: `gathered` holds `world` consecutive W x 720 B buffers, the r-th written by the
 * rank that owns windows {w : w mod world == r} (te_msm_set_window_shard(r, world)); row w is taken from buffer
 * w mod world.  Saves the caller the merge. */
int te_msm_finalize_gathered(const uint8_t* gathered, int world, int window_bits, int bucket_bits, int num_windows,
                             uint8_t out_xy_le[64]);

/* The two context-free tails for either curve (curve = TE_MSM_CURVE_*; rows of TE_MSM_PARTIAL_BYTES or
 * TE_MSM_PARTIAL_BYTES_BLS12_377 bytes; out_xy_le 64 or 96 bytes). */
int te_msm_finalize_host_curve(int curve, const uint8_t* partials, int window_bits, int bucket_bits, int num_windows, uint8_t* out_xy_le);
int te_msm_finalize_gathered_curve(int curve, const uint8_t* gathered, int world, int window_bits, int bucket_bits, int num_windows,
                                   uint8_t* out_xy_le);

/* The tail over the SUM of several row buffers (each W rows): the rows are linear in the bucket contents, so an MSM whose
 * POINTS were cut into slices -- every slice run through all windows with the same window_bits, e.g. one slice per GPU
 * (te_msm_run on a multi-device context does exactly this internally) or per process -- is the fold of the slices' rows
 * added up.  All-zero rows are skipped.  Pure host code. */
int te_msm_finalize_sum_curve(int curve, const uint8_t* const* row_sets, int sets, int window_bits, int bucket_bits, int num_windows,
                              uint8_t* out_xy_le);

/* ---- harness inputs (host code, no device needed).  The reference's harness generates its own random inputs when the
 * ZPrize files are not used (ui/AllBenchmarks.tsx:99-131, reference/webgpu/utils.ts:81-88,118-124): seeded scalars =
 * 256 random bits reduced mod p; points, by `fixed_point`: 0 = n distinct subgroup points (a + i*b)*G (an arithmetic
 * progression: one addition per point), 1 = the harness's one fixed point replicated n times (ui/AllBenchmarks.tsx:105-112),
 * 2 = n independent points a_i * G with seeded-random a_i ("random points", SURVEY.md 8d set (R); fixed-base table, all host
 * threads: about a second per 2^20).  Either output pointer may be NULL. */
#define TE_MSM_SYNTH_CHAIN  0
#define TE_MSM_SYNTH_FIXED  1
#define TE_MSM_SYNTH_RANDOM 2
int te_msm_synth_inputs(uint64_t seed, uint64_t n, int fixed_point, uint8_t* points_xy_le, uint8_t* scalars_le);
/* The same scheme for BLS12-377 G1: 96-byte points (a + i*b)*G, 48-byte scalar records (values below r). */
int te_msm_synth_inputs_bls12_377(uint64_t seed, uint64_t n, uint8_t* points_xy_le, uint8_t* scalars_le);

/* ---- measurement / stage verification (the reference's `debug` flags, submission.ts:892-1363) --- */
/* Per-stage device time of the last run in ms (needs option "profile" >= 1; level 1 reports "accumulate" only), from HIP events
 * on the engine's stream, plus "accumulate_on_device": the dominant kernel's own device clock from its first wave in to its last
 * wave out -- what a kernel trace reports; with several MSMs in flight the event interval also contains the time the launch
 * waited behind other streams' kernels -- and "accumulate_core_clock_ghz" (a frequency, not a time): the mean shader clock the
 * kernel's waves ran at, from per-wave shader-clock and wall-clock ticks.  Returns the number of entries written; names[i]
 * points to static strings. */
int te_msm_stage_ms(te_ctx* ctx, float* ms, const char** names, int max_stages);
/* Copies an intermediate buffer of the last run to host memory.  stage is one of
 * "records" (n x 128 B), "digits" / "part_keys" (nw rows of u16, row stride n rounded up to 8), "part_idx" (same rows, u32),
 * "part_start" / "part_count" (nw x P u32), "bucket_count" / "bucket_start" (nw x B u32), "sorted" (nw x n u32), "num_segments" (u32),
 * "seg_bucket" / "seg_len" / "order" (num_segments u32),
 * "buckets" (nw x B x 144 B), "partials" (W x 720 B).  Returns bytes copied
 * (<= cap) or a negative error. */
int64_t te_msm_debug_read(te_ctx* ctx, const char* stage, void* dst, uint64_t cap);
/* Copies records [first, first + count) of a bound point set from the memory of device `device_index` of the context to dst
 * (stage verification of te_msm_bind_points).  Record layouts, little-endian u32 limb words of 29 bits, Montgomery form:
 * Twisted-Edwards BLS12: 128-byte slots, hm | hp | dt of 9 words each; BLS12-377: 168 bytes, hm | hp | dt of 14 words (affine,
 * option "bind_affine" = 1) or 224 bytes, hm | hp | dt | z (projective).  *record_bytes (optional) receives the slot size.
 * Returns bytes copied (<= cap) or a negative error. */
int64_t te_msm_bases_read(te_ctx* ctx, const te_bases* bases, int device_index, uint64_t first, uint64_t count, void* dst, uint64_t cap,
                          int* record_bytes);

#ifdef __cplusplus
}
#endif
#endif /* TE_MSM_H */
