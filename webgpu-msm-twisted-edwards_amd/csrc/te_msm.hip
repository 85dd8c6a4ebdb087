// te_msm.hip -- the engine core of libtemsm.so: plan, launch sequences (every MSM stage kernel is launched here), streams, record slabs, uploads.
//
// Host-side counterpart of compute_msm's orchestration (submission/submission.ts:73-413) and of the
// WebGPU wrapper it drives (implementation/cuzk/gpu.ts:14-229).  Differences that matter:
//   * the context is persistent -- device buffers, streams and kernels survive across calls (the
//     reference re-creates device, buffers and pipelines on every call, submission.ts:96-97,360);
//   * every stage of one MSM is enqueued on one HIP stream with no host synchronisation in between, like the
//     reference's single command-encoder submit (gpu.ts:118); several MSMs are kept in flight on separate
//     work sets / streams so that they overlap on the device;
//   * windows can be sharded over contexts / devices; the reference is single-device.
#include "engine.hpp"
#if defined(__x86_64__)
#include <immintrin.h>
#endif
#include "kernels.hip.hpp"
#include "probe.hip.hpp"

namespace te_eng {

// what engine.hpp states of the kernel header for the units that do not include it
static_assert(kClkSlots == TE_CLK_SLOTS && kHistCopies == TE_HIST_COPIES, "engine.hpp: kernel constants");
static_assert(kAccBytes == sizeof(te::ete) && kAccBytes377 == sizeof(te::ete_t<14>), "engine.hpp: accumulator sizes");
static_assert(kRecBytes == sizeof(te::rec_slot<9>) && kRecBytes377 == sizeof(te::rec_slot<14>) && kRecBytesAff377 == sizeof(te::rec_aff377), "engine.hpp: record sizes");

// k_reduce_tail keeps up to 256 + 16 points in LDS (39 KB / 61 KB): te_msm_init allows it on every device of a context
hipError_t allow_tail_lds() {
  hipError_t er = hipFuncSetAttribute(reinterpret_cast<const void*>(te::k_reduce_tail<9>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  if (er == hipSuccess)
    er = hipFuncSetAttribute(reinterpret_cast<const void*>(te::k_reduce_tail<14>), hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  return er;
}

namespace {
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
// A declared width (option "scalar_bits", or the width of 8- / 16-byte records) cuts the windows to what it needs and keeps their size:
// te_plan::windows_for (plan_arith.hpp) is the one statement of the rule.
}  // namespace

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
  p.sc_bytes = q.scalar_bytes ? q.scalar_bytes : (int)scalar_bytes_now(ctx);
  p.sc_bits = q.scalar_bits >= 0 ? q.scalar_bits : scalar_bits_now(ctx);
  p.rec_kind = q.rec_kind;
  p.signed_digits = ctx->opt_signed;
  const te_plan::windows win = te_plan::windows_for(q.force_c ? q.force_c : ctx->opt_window_bits ? ctx->opt_window_bits : auto_window_bits(n), p.signed_digits, p.sc_bits);
  p.c = win.c; p.W = win.W;
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

namespace {
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
// -- or 8- / 16-byte records, which are never residues (check_scalar_record refuses the pair when a call starts)
inline int scalar_form_of(const plan_t& p) {
  if (p.sc_bytes == 8) return te::SCALAR_FORM_U64;
  if (p.sc_bytes == 16) return te::SCALAR_FORM_U128;
  return !p.scalar_mont ? te::SCALAR_FORM_CANONICAL : p.curve == TE_MSM_CURVE_BLS12_377_G1 ? te::SCALAR_FORM_377 : te::SCALAR_FORM_TE;
}
// f(integral_constant<int, FORM>) for a form of scalar_form_of
template <typename F> void with_scalar_form(int form, F&& f) {
  if (form == te::SCALAR_FORM_TE) f(std::integral_constant<int, te::SCALAR_FORM_TE>{});
  else if (form == te::SCALAR_FORM_377) f(std::integral_constant<int, te::SCALAR_FORM_377>{});
  else if (form == te::SCALAR_FORM_U64) f(std::integral_constant<int, te::SCALAR_FORM_U64>{});
  else if (form == te::SCALAR_FORM_U128) f(std::integral_constant<int, te::SCALAR_FORM_U128>{});
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
      prm.sc_stride = (uint32_t)p.sc_bytes / 16u;            // (8- and 16-byte records: not read, the instantiation carries the size)
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
}  // namespace

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

namespace {
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
}  // namespace

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
static int acquire_shared_recs(te_ctx* ctx, gpu_t& d, const void* src, uint64_t n, int curve, hipStream_t stream, bool run, uint8_t** out, bool* have) {
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
static int note_conversion(te_ctx* ctx, gpu_t::rec_slab_t& sl, hipStream_t stream) {
  if (!sl.conv_ev) HIP_TRY(ctx, hipEventCreateWithFlags(&sl.conv_ev, hipEventDisableTiming));
  HIP_TRY(ctx, hipEventRecord(sl.conv_ev, stream));
  sl.converted = true;
  return 0;
}
// completed: the set's MSM is known to be over (a collected ticket, a synchronous call).  Otherwise (the building blocks: the set is simply
// used again) an event behind that MSM -- on the stream it ran on, BEFORE anything new is enqueued there -- guards the slab.
void release_shared_recs(gpu_t& d, workset_t& ws, bool completed) {
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

namespace {
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
}  // namespace

int enqueue_partial(te_ctx* ctx, gpu_t& d, workset_t& ws, const partial_req& r) {
  const void* const d_points = r.d_points; const uint64_t n = r.n; hipStream_t const stream = r.stream;
  const int batch = r.batch; const te_bases* const bases = r.bases; const auto* const upload_points = r.upload_points;
  // (the plan is made for the n entries; only the entry form follows the set's count: indexed_plan.hpp)
  plan_req q; q.n = n; q.batch = batch; q.whole = r.whole; q.scalar_form = r.scalar_form; q.scalar_bytes = r.scalar_bytes; q.scalar_bits = r.scalar_bits;
  if (bases) q.rec_kind = bases->rec_kind;
  if (r.d_idx) q.idx_count = bases->n;
  const plan_t p = make_plan(ctx, d, q);
  // (a declared width can leave fewer windows than te_msm_set_window_shard dealt shards: one of them would hold no window)
  if (p.sc_bits && !q.whole && ctx->devs.size() == 1 && d.w_step > p.W)
    return set_err(ctx, TE_MSM_EINVAL, "the window shard's step is larger than the windows of the narrow plan: a shard would hold no window");
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

// device copies of a host-buffer call's inputs, in bytes of the call's curve and scalar record (64 + 32 per point for the Twisted-Edwards
// wire format, 96 + 48 for BLS12-377 -- 96 + 32 under option "scalar_record_bytes" = 32)
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

// must device d pull what lies on src_dev?  ("stage_device_inputs": also when d IS the holder -- the one-GPU rehearsal)
bool must_pull(const te_ctx* ctx, const gpu_t& d, int src_dev) { return ctx->devs.size() > 1 && (d.device != src_dev || ctx->opt_stage_device_inputs); }
// The n entries of `in` over the peer link, on the set's stream; `in` then names the staging area.  moved: what was copied -- the caller
// adds it to the context's counters (plain integers: run_bound_window_shards pulls from one host thread per device and adds after the join).
int pull_inputs(te_ctx* ctx, const gpu_t& d, workset_t& ws, int src_dev, uint64_t n, size_t scalar_bytes, device_inputs& in, peer_traffic& moved) {
  const curve_sizes sz = sizes_of(ctx->opt_curve);
  if (in.idx) { if (int rc = make_room(ctx, ws.d_in_idx, (size_t)n)) return rc; }
  if (int rc = ensure_staging(ctx, ws, in.points ? n * sz.point_in : 0, n * scalar_bytes)) return rc;
  if (int rc = wait_behind_previous(ctx, ws)) return rc;
  HIP_TRY(ctx, hipMemcpyPeerAsync(ws.d_in_scalars, d.device, in.scalars, src_dev, n * scalar_bytes, ws.stream));
  if (in.points) HIP_TRY(ctx, hipMemcpyPeerAsync(ws.d_in_points, d.device, in.points, src_dev, n * sz.point_in, ws.stream));
  if (in.idx) HIP_TRY(ctx, hipMemcpyPeerAsync(ws.d_in_idx, d.device, in.idx, src_dev, n * sizeof(uint32_t), ws.stream));
  moved.copies += 1 + (in.points != nullptr) + (in.idx != nullptr);
  moved.bytes += (int64_t)(n * (scalar_bytes + (in.points ? sz.point_in : 0) + (in.idx ? sizeof(uint32_t) : 0)));
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

namespace {
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
}  // namespace

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
static int copy_stream_behind_previous(te_ctx* ctx, workset_t& ws) {
  if (int rc = need_copy_stream(ctx, ws)) return rc;
  if (!ws.used) return 0;
  const hipError_t q = hipEventQuery(ws.ev_result);
  if (q == hipSuccess) return 0;
  (void)hipGetLastError();                                                        // hipErrorNotReady is an answer, not an error
  HIP_TRY(ctx, hipEventRecord(ws.ev_start, ws.stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ws.copy_stream, ws.ev_start, 0));
  return 0;
}

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
static bool caller_may_wait_on_host(const void* a, const void* b) {
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
int enqueue_host_pieces(te_ctx* ctx, gpu_t& d, workset_t& ws, const host_slice_req& r) {
  HIP_TRY(ctx, hipSetDevice(d.device));
  const uint64_t n = r.n;
  const bool bound = r.points == nullptr;
  // what the plans of the whole slice and of every piece share; the pieces keep the slice's window bits and scalar form
  plan_req q = plan_whole(n); q.force_c = r.c; q.scalar_form = r.scalar_form; q.scalar_bytes = r.scalar_bytes; q.scalar_bits = r.scalar_bits;
  if (bound) { q.rec_kind = r.rec_kind; if (r.idx) q.idx_count = r.idx_count; }
  const plan_t pf = make_plan(ctx, d, q);
  q.force_c = pf.c; q.scalar_form = pf.scalar_mont; q.scalar_bytes = pf.sc_bytes; q.scalar_bits = pf.sc_bits;
  const curve_sizes sz = sizes_of(pf.curve);
  const size_t sb = (size_t)pf.sc_bytes;                                   // the call's scalar record: every size and piece offset below
  const size_t rec_bytes = rec_bytes_of(pf.curve, pf.rec_kind);
  if (int rc = ensure_staging(ctx, ws, bound ? 0 : n * sz.point_in, n * sb)) return rc;
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
    return upload(ctx, ws, dscs + lo * sb, r.scalars + lo * sb, m * sb, ws.copy_stream);
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
    L.p = p; L.d_scalars = dscs + lo * sb; L.n = m; L.onto = i > 0;
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

namespace {
// (the arithmetic -- rows, capacity, chunks, default segment length -- is te_fb::make_geometry, fb_plan.hpp; returned for the caller's
// refusal, `half` and the digit kernel's LDS size)
te_fb::geometry make_plan_fb(const te_ctx* ctx, const gpu_t& d, uint64_t n, int fb_c, plan_t& p, int scalar_form = -1) {
  const te_fb::geometry g = te_fb::make_geometry(n, fb_c, TE_SCATTER_BLOCKS, TE_SCATTER_MINCHUNK);
  plan_req q = plan_whole(g.cap); q.force_c = 16; q.scalar_form = scalar_form; q.scalar_bits = 0;      // (the pseudo-windows are not windows of the scalar: no declared width)
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
}  // namespace

// An MSM of n scalars (device memory) over the fixed-base table of `bases` on device `d`: the scalars' digits address the table
// entries (w, idx_base + i) -- idx_base: the first point of this launch inside the bound set (a device's slice of a lone
// multi-device call).  Rows in the set's own block; the caller ends the sequence with fetch_rows().  scalar_form: plan_req's.
int enqueue_fixed_base(te_ctx* ctx, gpu_t& d, workset_t& ws, const te_bases* bases, const void* d_scalars, uint64_t n, uint64_t idx_base, hipStream_t stream,
                       int scalar_form) {
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

namespace {
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
}  // namespace

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

// The records of the set on device i: raw points -> (temporary) -> records, on a stream of its own; returns when they are there.
// src on the host: the device's own upload (D devices: D links side by side, one host thread each); src on a device of the
// context: read in place on its holder, pulled over the peer link elsewhere.
// mont: the raw coordinates are Montgomery residues (option "points_montgomery"): the conversion's other instantiation, the same records.
// lay: the points' stride and flag byte (options "point_stride" / "point_infinity_flag"): the strided conversions, the same records.
int bind_on_device(te_ctx* ctx, te_bases* b, size_t i, const void* src, bool src_is_host, int src_dev, bool mont, point_layout lay) {
  gpu_t& d = ctx->devs[i];
  HIP_TRY(ctx, hipSetDevice(d.device));
  const size_t in_bytes = lay.bytes(b->curve);                             // from one point to the next in the caller's buffer
  const uint64_t n = b->n;
  uint8_t* recs = nullptr; void* raw = nullptr; void* proj = nullptr; hipStream_t st = nullptr;
  struct cleanup_t { void*& raw; void*& proj; hipStream_t& st; ~cleanup_t() { if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); } if (raw) (void)hipFree(raw); if (proj) (void)hipFree(proj); } } cleanup{raw, proj, st};
  HIP_TRY(ctx, hipMalloc((void**)&recs, (size_t)n * b->rec_bytes * (size_t)(b->fb_c ? b->fb_W : 1)));
  b->recs[i] = recs;                                                       // (freed by the caller on failure: free_bases)
  HIP_TRY(ctx, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  const void* pts = src;
  if (src_is_host) {
    HIP_TRY(ctx, hipMalloc(&raw, (size_t)n * in_bytes));
    HIP_TRY(ctx, hipMemcpyAsync(raw, src, (size_t)n * in_bytes, hipMemcpyHostToDevice, st));
    pts = raw;
  } else if (src_dev != d.device || ctx->opt_stage_device_inputs) {
    HIP_TRY(ctx, hipMalloc(&raw, (size_t)n * in_bytes));
    HIP_TRY(ctx, hipMemcpyPeerAsync(raw, d.device, src, src_dev, (size_t)n * in_bytes, st));
    { std::lock_guard<std::mutex> lk(ctx->err_mu); ctx->stat_peer_copies += 1; ctx->stat_peer_bytes += (int64_t)(n * in_bytes); }
    pts = raw;
  }
  const uint32_t n32 = (uint32_t)n;
  te::batch_ptrs tab; te::batch_slabs row_slab; memset(&tab, 0, sizeof tab); memset(&row_slab, 0, sizeof row_slab);
  tab.p[0] = (const uint4*)pts;
  if (b->curve == TE_MSM_CURVE_BLS12_377_G1) {
    te::rec_slot<14>* pr = reinterpret_cast<te::rec_slot<14>*>(recs);
    if (b->rec_kind == 1) { HIP_TRY(ctx, hipMalloc(&proj, (size_t)n * sizeof(te::rec_slot<14>))); pr = static_cast<te::rec_slot<14>*>(proj); }
    const uint64_t* p8 = static_cast<const uint64_t*>(pts);
    if (lay.stride && mont) hipLaunchKernelGGL(te::k_prep_points377_strided<true>, dim3((n32 + 255) / 256), dim3(256), 0, st, p8, lay.stride, lay.flag ? 1u : 0u, pr, n32);
    else if (lay.stride) hipLaunchKernelGGL(te::k_prep_points377_strided<false>, dim3((n32 + 255) / 256), dim3(256), 0, st, p8, lay.stride, lay.flag ? 1u : 0u, pr, n32);
    else if (mont) hipLaunchKernelGGL(te::k_prep_points377<true>, dim3((n32 + 255) / 256, 1), dim3(256), 0, st, tab, row_slab, pr, n32);
    else hipLaunchKernelGGL(te::k_prep_points377<false>, dim3((n32 + 255) / 256, 1), dim3(256), 0, st, tab, row_slab, pr, n32);
    if (b->rec_kind == 1) {
      const uint32_t groups = (n32 + TE_AFF_GROUP - 1u) / TE_AFF_GROUP;
      hipLaunchKernelGGL(te::k_affine377, dim3((groups + 255) / 256), dim3(256), 0, st, pr, reinterpret_cast<te::rec_aff377*>(recs), n32);
    }
  } else if (lay.stride) {
    const uint64_t* p8 = static_cast<const uint64_t*>(pts);
    te::rec_slot<9>* pr = reinterpret_cast<te::rec_slot<9>*>(recs);
    if (mont) hipLaunchKernelGGL(te::k_prep_points_strided<true>, dim3((n32 + 255) / 256), dim3(256), 0, st, p8, lay.stride, pr, n32);
    else hipLaunchKernelGGL(te::k_prep_points_strided<false>, dim3((n32 + 255) / 256), dim3(256), 0, st, p8, lay.stride, pr, n32);
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

}  // namespace te_eng
