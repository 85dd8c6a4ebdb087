// addon.cc -- N-API binding of libtemsm.so for the reference's host language (JavaScript / TypeScript).
//
// Exposes  msmNative(points: Buffer, scalars: Buffer): Promise<Buffer /*64 bytes: x || y little-endian*/>
// which compute_msm.js wraps into the reference's entry point
//   compute_msm(bufferPoints, bufferScalars, log_result, force_recompile): Promise<{x: bigint, y: bigint}>
// (submission/submission.ts:73-78).  The MSM runs on a libuv worker thread (napi_create_async_work), so the
// JS event loop is not blocked -- the reference's call is async for the same reason (ui/Benchmark.tsx:32).
// Errors reject the promise, as the reference's `throw`s do (implementation/cuzk/gpu.ts:19-22).
//
// Devices: TE_MSM_DEVICES="0,1,2,3" (or setDevices([0,1,2,3])) puts several GPUs of the node behind the one entry point
// (a context of n_dev > 1 devices, include/te_msm.h).  Default: device 0.
// Concurrency: promises in flight at the same time (a prover that does not await each call) become TICKETS of the engine --
// te_msm_submit_async under the lock (it returns at once: the upload runs on the chosen device's host thread),
// te_msm_ticket_wait outside it on a libuv pool thread, te_msm_collect under it again.  On one device the upload of one
// MSM overlaps the device work of the previous ones; on D devices every ticket is a whole MSM on the device with the fewest
// in flight -- D uploads on D PCIe links at once.  Calls made while others are pending are submitted right from the
// JavaScript thread, so the number in flight is not bounded by libuv's pool (4 threads unless UV_THREADPOOL_SIZE says
// otherwise) but by the engine's work sets (TE_MSM_WORKSETS per device); beyond that, calls queue inside their pool thread.
// The LONE call on several devices -- nothing else pending when it starts -- uses all of them for its one MSM
// (te_msm_run: point slices, one upload thread per device): the latency form.
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <string>
#include <vector>
#include <memory>

#include "../../include/te_msm.h"
#include "promise_protocol.hpp"

namespace {

std::atomic<int> g_check_points{0};    // setCheckPoints(level): option "check_points" of every context created from now on
std::atomic<int> g_scalars_montgomery{0};   // setScalarsMontgomery(flag): option "scalars_montgomery" of every context created from now on
std::atomic<int> g_scalar_record_bytes{0};  // setScalarRecordBytes(n): option "scalar_record_bytes" of every context created from now on
std::atomic<int> g_scalar_bits{0};          // setScalarBits(b): option "scalar_bits" of every context created from now on
// bytes of one scalar record of an MSM call (compute_msm, msmBatch, msmIndexed): 8 or 16 under setScalarRecordBytes, else the curve's 32
size_t msm_scalar_bytes() { const int n = g_scalar_record_bytes.load(); return n == 8 || n == 16 ? (size_t)n : (size_t)TE_MSM_SCALAR_BYTES; }
// what setBases bound: the Buffer, kept alive so that its address cannot become another object's, and the form of its coordinates
// ({montgomery: true}: option "points_montgomery" for every bind of that buffer; a pool thread binds it again on a new context;
// {stride, infinityFlag}: options "point_stride" / "point_infinity_flag", remembered and applied in the same way)
struct BoundBuffer {
  napi_ref ref = nullptr;
  std::atomic<int> montgomery{0};
  std::atomic<int> stride{0};
  std::atomic<int> infinity_flag{0};
} g_bases;

// the engine behind te_promise::protocol (js/promise_protocol.hpp holds the lock protocol itself)
struct EngineApi {
  using ctx_t = te_ctx;
  using bases_t = te_bases;
  static constexpr int ESTATE = TE_MSM_ESTATE;
  static std::vector<int> default_devices() {        // TE_MSM_DEVICES="0,1,..", else device 0
    std::vector<int> ids;
    const char* e = getenv("TE_MSM_DEVICES");
    if (e && *e) {
      const char* q = e;
      while (*q) { char* end = nullptr; const long v = strtol(q, &end, 10); if (end == q) break; ids.push_back((int)v); q = *end == ',' ? end + 1 : end; }
    }
    if (ids.empty()) ids.push_back(0);
    return ids;
  }
  static int init(const int* ids, int n, te_ctx** out) {
    const int rc = te_msm_init(ids, n, out);
    if (rc == 0 && g_check_points.load()) {
      const int orc = te_msm_set_option(*out, "check_points", g_check_points.load());
      if (orc) { te_msm_destroy(*out); *out = nullptr; return orc; }
    }
    if (rc == 0 && g_scalars_montgomery.load()) {
      const int orc = te_msm_set_option(*out, "scalars_montgomery", 1);
      if (orc) { te_msm_destroy(*out); *out = nullptr; return orc; }
    }
    if (rc == 0 && g_scalar_bits.load()) {               // (before the record size: 16-byte records need a declared width)
      const int orc = te_msm_set_option(*out, "scalar_bits", g_scalar_bits.load());
      if (orc) { te_msm_destroy(*out); *out = nullptr; return orc; }
    }
    if (rc == 0 && g_scalar_record_bytes.load()) {
      const int orc = te_msm_set_option(*out, "scalar_record_bytes", g_scalar_record_bytes.load());
      if (orc) { te_msm_destroy(*out); *out = nullptr; return orc; }
    }
    return rc;
  }
  static void destroy(te_ctx* c) { te_msm_destroy(c); }
  static const char* last_error(te_ctx* c) { return te_msm_last_error(c); }
  static int run(te_ctx* c, const uint8_t* p, const uint8_t* s, uint64_t n, uint8_t* out) { return te_msm_run(c, p, s, n, out); }
  static int submit_async(te_ctx* c, const uint8_t* p, const uint8_t* s, uint64_t n, uint64_t* t) { return te_msm_submit_async(c, p, s, n, t); }
  static int ticket_wait(te_ctx* c, uint64_t t) { return te_msm_ticket_wait(c, t); }
  static int collect(te_ctx* c, uint64_t t, uint8_t* out) { return te_msm_collect(c, t, out); }
  static int64_t in_flight(te_ctx* c) { int64_t v = 0; te_msm_get_option(c, "in_flight", &v); return v; }
  static int64_t num_devices(te_ctx* c) { int64_t v = 1; te_msm_get_option(c, "num_devices", &v); return v; }
  // resident bases (include/te_msm.h): the opt-in behind setBases(buffer)
  // (the option is read at bind time: set for the length of this bind and put back -- also when the set is bound again on a new context)
  static int bind(te_ctx* c, const uint8_t* p, uint64_t n, te_bases** out) {
    const struct { const char* key; int64_t want; } opts[3] = {{"points_montgomery", g_bases.montgomery.load()}, {"point_stride", g_bases.stride.load()},
                                                               {"point_infinity_flag", g_bases.infinity_flag.load()}};
    int64_t before[3] = {0, 0, 0};
    bool was_set[3] = {false, false, false};                 // only an option this bind changed is put back
    int orc = 0;
    for (int i = 0; i < 3 && !orc; i++) {
      if (!opts[i].want) continue;
      orc = te_msm_get_option(c, opts[i].key, &before[i]);
      if (!orc) orc = te_msm_set_option(c, opts[i].key, opts[i].want);
      was_set[i] = !orc;
    }
    const int rc = orc ? orc : te_msm_bind_points(c, p, n, out);
    for (int i = 0; i < 3; i++) if (was_set[i]) (void)te_msm_set_option(c, opts[i].key, before[i]);
    return rc;
  }
  static int release(te_ctx* c, te_bases* b) { return te_msm_release_points(c, b); }
  static int run_scalars(te_ctx* c, te_bases* b, const uint8_t* s, uint8_t* out) { return te_msm_run_scalars(c, b, s, out); }
  static int submit_scalars(te_ctx* c, te_bases* b, const uint8_t* s, uint64_t* t) { return te_msm_submit_scalars(c, b, s, t); }
};
te_promise::protocol<EngineApi> g_proto;

struct Job {
  napi_async_work work = nullptr;
  napi_deferred deferred = nullptr;
  napi_ref points_ref = nullptr, scalars_ref = nullptr;   // keep the JS Buffers alive until completion (asynchronous uploads read them)
  te_promise::job_t j;
};

void Execute(napi_env, void* data) { g_proto.execute(&static_cast<Job*>(data)->j); }

void Complete(napi_env env, napi_status, void* data) {
  Job* j = static_cast<Job*>(data);
  if (j->j.rc == 0) {
    napi_value buf; void* dst = nullptr;
    napi_create_buffer_copy(env, 64, j->j.out, &dst, &buf);
    napi_resolve_deferred(env, j->deferred, buf);
  } else {
    napi_value msg, errv;
    std::string m = "te_msm error " + std::to_string(j->j.rc) + ": " + j->j.err;
    napi_create_string_utf8(env, m.c_str(), m.size(), &msg);
    napi_create_error(env, nullptr, msg, &errv);
    napi_reject_deferred(env, j->deferred, errv);
  }
  napi_delete_reference(env, j->points_ref);
  napi_delete_reference(env, j->scalars_ref);
  napi_delete_async_work(env, j->work);
  delete j;
}

napi_value MsmNative(napi_env env, napi_callback_info info) {
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool is0 = false, is1 = false;
  if (argc >= 2) { napi_is_buffer(env, argv[0], &is0); napi_is_buffer(env, argv[1], &is1); }
  if (!is0 || !is1) { napi_throw_type_error(env, nullptr, "msmNative(points: Buffer, scalars: Buffer)"); return nullptr; }
  void *p = nullptr, *s = nullptr; size_t pl = 0, sl = 0;
  napi_get_buffer_info(env, argv[0], &p, &pl);
  napi_get_buffer_info(env, argv[1], &s, &sl);
  // (the buffer setBases bound at a stride is stride*n bytes: it is recognised by identity and its points are not read again)
  bool bound_at_stride = false;
  const size_t sb = msm_scalar_bytes();
  if (g_bases.ref && g_bases.stride.load() && pl == (size_t)g_bases.stride.load() * (sl / sb)) {
    napi_value bound = nullptr;
    if (napi_get_reference_value(env, g_bases.ref, &bound) == napi_ok && bound) napi_strict_equals(env, bound, argv[0], &bound_at_stride);
  }
  if (sl % sb != 0 || (pl != TE_MSM_POINT_BYTES * (sl / sb) && !bound_at_stride)) {
    napi_throw_range_error(env, nullptr, "points must be 64*n bytes and scalars 32*n bytes (8*n / 16*n under setScalarRecordBytes)");
    return nullptr;
  }
  Job* j = new Job();
  j->j.points = static_cast<const uint8_t*>(p); j->j.scalars = static_cast<const uint8_t*>(s); j->j.n = sl / sb;
  napi_create_reference(env, argv[0], 1, &j->points_ref);
  napi_create_reference(env, argv[1], 1, &j->scalars_ref);
  napi_value promise, name;
  napi_create_promise(env, &j->deferred, &promise);
  napi_create_string_utf8(env, "te_msm_run", NAPI_AUTO_LENGTH, &name);
  napi_create_async_work(env, nullptr, name, Execute, Complete, j, &j->work);
  // other calls pending, the context exists and no pool thread is inside the engine: the waiting calls become tickets right here,
  // oldest first (microseconds), and their pool threads will only wait and collect (te_promise::protocol::enter)
  g_proto.enter(&j->j);
  napi_queue_async_work(env, j->work);
  return promise;
}

// resetContext(): drops the cached engine context (compute_msm's force_recompile) once no promise is pending
napi_value ResetContext(napi_env env, napi_callback_info) {
  g_proto.reset();
  napi_value u; napi_get_undefined(env, &u); return u;
}

// setDevices([0, 1, ...]): the GPUs later calls are sharded over (overrides TE_MSM_DEVICES; [] = back to the environment)
napi_value SetDevices(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool is_arr = false;
  if (argc >= 1) napi_is_array(env, argv[0], &is_arr);
  if (!is_arr) { napi_throw_type_error(env, nullptr, "setDevices(ids: number[])"); return nullptr; }
  uint32_t len = 0; napi_get_array_length(env, argv[0], &len);
  if (len > 64) { napi_throw_range_error(env, nullptr, "setDevices: at most 64 devices"); return nullptr; }
  std::vector<int> ids;
  for (uint32_t i = 0; i < len; i++) {
    napi_value v; int32_t id = 0;
    napi_get_element(env, argv[0], i, &v);
    if (napi_get_value_int32(env, v, &id) != napi_ok || id < 0) { napi_throw_type_error(env, nullptr, "setDevices: device ids are non-negative integers"); return nullptr; }
    ids.push_back(id);
  }
  g_proto.set_devices(ids);
  napi_value u; napi_get_undefined(env, &u); return u;
}

// setBases(points: Buffer | null): binds this point buffer (te_msm_bind_points: uploaded and converted once, on every device);
// compute_msm(thatBuffer, scalars) -- the same Buffer object: address and length are compared, its contents must not change --
// then uploads and decomposes the scalars only.  Every other buffer takes the ordinary path; setBases(null) unbinds.
// compute_msm's signature (submission.ts:73-78) is untouched; the reference's harness passes one point buffer to six calls per
// size (submission/miscellaneous/full_benchmarks.ts:63-68,100-105).  Blocks until no promise is pending (like resetContext).
// setBases(points, {montgomery: true}): the coordinates are a native prover's Montgomery residues, x * 2^256 mod p (include/te_msm.h,
// option "points_montgomery"); the set, and every result over it, is the same as from canonical coordinates.
// {stride: s}: point i starts at byte i * s of the buffer (option "point_stride"); {infinityFlag: true}: option "point_infinity_flag",
// BLS12-377 only -- on the curve this addon runs the engine refuses the bind (te_msm error -1).  All three are remembered with the buffer.
napi_value SetBases(napi_env env, napi_callback_info info) {
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool montgomery = false, infinity_flag = false;
  int32_t stride = 0;
  if (argc >= 2) {
    napi_valuetype ot = napi_undefined;
    napi_typeof(env, argv[1], &ot);
    if (ot == napi_object) {
      napi_value mv; bool has = false;
      napi_has_named_property(env, argv[1], "montgomery", &has);
      if (has && (napi_get_named_property(env, argv[1], "montgomery", &mv) != napi_ok || napi_coerce_to_bool(env, mv, &mv) != napi_ok ||
                  napi_get_value_bool(env, mv, &montgomery) != napi_ok)) {
        napi_throw_type_error(env, nullptr, "setBases: options.montgomery is a boolean");
        return nullptr;
      }
      has = false;
      napi_has_named_property(env, argv[1], "infinityFlag", &has);
      if (has && (napi_get_named_property(env, argv[1], "infinityFlag", &mv) != napi_ok || napi_coerce_to_bool(env, mv, &mv) != napi_ok ||
                  napi_get_value_bool(env, mv, &infinity_flag) != napi_ok)) {
        napi_throw_type_error(env, nullptr, "setBases: options.infinityFlag is a boolean");
        return nullptr;
      }
      has = false;
      napi_has_named_property(env, argv[1], "stride", &has);
      if (has && (napi_get_named_property(env, argv[1], "stride", &mv) != napi_ok || napi_get_value_int32(env, mv, &stride) != napi_ok ||
                  (stride != 0 && (stride % 8 != 0 || stride < 64 || stride > 128)))) {
        napi_throw_type_error(env, nullptr, "setBases: options.stride is 0 or a multiple of 8 in [64, 128]");
        return nullptr;
      }
    } else if (ot != napi_undefined && ot != napi_null) { napi_throw_type_error(env, nullptr, "setBases(points: Buffer | null, options?: { montgomery?: boolean, stride?: number, infinityFlag?: boolean })"); return nullptr; }
  }
  napi_valuetype vt = napi_undefined;
  if (argc >= 1) napi_typeof(env, argv[0], &vt);
  bool is_buf = false;
  if (argc >= 1 && vt == napi_object) napi_is_buffer(env, argv[0], &is_buf);
  if (!(is_buf || argc == 0 || vt == napi_null || vt == napi_undefined)) { napi_throw_type_error(env, nullptr, "setBases(points: Buffer | null)"); return nullptr; }
  std::string err;
  if (!is_buf) {
    (void)g_proto.set_bases(nullptr, 0, err);
    if (g_bases.ref) { napi_delete_reference(env, g_bases.ref); g_bases.ref = nullptr; }
    g_bases.montgomery.store(0); g_bases.stride.store(0); g_bases.infinity_flag.store(0);
  } else {
    void* p = nullptr; size_t pl = 0;
    napi_get_buffer_info(env, argv[0], &p, &pl);
    const size_t rec = stride ? (size_t)stride : 64;                  // from one point to the next
    if (pl % rec != 0) { napi_throw_range_error(env, nullptr, "setBases: points must be 64*n bytes (stride*n with options.stride)"); return nullptr; }
    napi_ref ref = nullptr;
    napi_create_reference(env, argv[0], 1, &ref);
    g_bases.montgomery.store(montgomery ? 1 : 0);                     // (Api::bind reads them inside set_bases)
    g_bases.stride.store(stride); g_bases.infinity_flag.store(infinity_flag ? 1 : 0);
    const int rc = g_proto.set_bases(static_cast<const uint8_t*>(p), pl / rec, err);
    if (g_bases.ref) napi_delete_reference(env, g_bases.ref);         // the previous buffer is unbound either way
    g_bases.ref = nullptr;
    if (rc) {
      g_bases.montgomery.store(0); g_bases.stride.store(0); g_bases.infinity_flag.store(0);      // nothing is bound
      napi_delete_reference(env, ref);
      const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
      napi_throw_error(env, nullptr, m.c_str());
      return nullptr;
    }
    g_bases.ref = ref;
  }
  napi_value u; napi_get_undefined(env, &u); return u;
}

// pointsFromX(xs: Buffer): Buffer -- x-only points (include/te_msm.h, te_msm_points_from_x): n x 32-byte little-endian x-coordinates
// (Aleo group values, the form Address.msm takes) -> n x 64-byte x || y with y recovered on the device, ready for compute_msm or
// setBases.  Twisted-Edwards curve only, like the rest of the addon.  Runs on the addon's context under its lock once no promise is
// pending (like setBases).  A bad x throws an Error that names the lowest failing index and the reason (TE_MSM_POINT_*); the Error
// also carries them as .index / .reason.
napi_value PointsFromX(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool is_buf = false;
  if (argc >= 1) napi_is_buffer(env, argv[0], &is_buf);
  if (!is_buf) { napi_throw_type_error(env, nullptr, "pointsFromX(xs: Buffer)"); return nullptr; }
  void* p = nullptr; size_t pl = 0;
  napi_get_buffer_info(env, argv[0], &p, &pl);
  if (pl % TE_MSM_X_BYTES != 0) { napi_throw_range_error(env, nullptr, "pointsFromX: x-coordinates must be 32*n bytes"); return nullptr; }
  const uint64_t n = pl / TE_MSM_X_BYTES;
  std::vector<uint8_t> out((size_t)n * TE_MSM_POINT_BYTES);
  int64_t bad = -1; int reason = 0;
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    return te_msm_points_from_x(c, static_cast<const uint8_t*>(p), n, out.data(), &bad, &reason);
  }, err);
  if (rc) {
    const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
    napi_value msg, errv;
    napi_create_string_utf8(env, m.c_str(), m.size(), &msg);
    napi_create_error(env, nullptr, msg, &errv);
    if (rc == TE_MSM_EPOINT) {
      napi_value iv, rv;
      napi_create_int64(env, bad, &iv); napi_create_int32(env, reason, &rv);
      napi_set_named_property(env, errv, "index", iv); napi_set_named_property(env, errv, "reason", rv);
    }
    napi_throw(env, errv);
    return nullptr;
  }
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, out.size(), out.data(), &dst, &buf);
  return buf;
}

// scalarMul(points: Buffer, scalars: Buffer): Buffer -- batch scalar multiplication (include/te_msm.h, te_msm_mul): n x 64-byte points
// and n x 32-byte little-endian scalars, or ONE 32-byte scalar for all of them -> n x 64-byte points [k_i] P_i (the identity as
// (0, 1)).  scalarMulX(xs, scalars) takes x-only points (pointsFromX's format) instead: bulkGroupScalarMul's counterpart
// (te_msm_mul_x).  Twisted-Edwards curve only, like the rest of the addon; run like pointsFromX.  A bad point (setCheckPoints) or a
// bad x throws an Error naming the lowest failing index and the reason, also as .index / .reason.
napi_value MulCommon(napi_env env, napi_callback_info info, bool x_only) {
  const char* const sig = x_only ? "scalarMulX(xs: Buffer, scalars: Buffer)" : "scalarMul(points: Buffer, scalars: Buffer)";
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool b0 = false, b1 = false;
  if (argc >= 2) { napi_is_buffer(env, argv[0], &b0); napi_is_buffer(env, argv[1], &b1); }
  if (!b0 || !b1) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  void *p = nullptr, *s = nullptr; size_t pl = 0, sl = 0;
  napi_get_buffer_info(env, argv[0], &p, &pl);
  napi_get_buffer_info(env, argv[1], &s, &sl);
  const size_t in_bytes = x_only ? TE_MSM_X_BYTES : TE_MSM_POINT_BYTES;
  const uint64_t n = pl / in_bytes;
  if (pl % in_bytes != 0 || (sl != TE_MSM_SCALAR_BYTES && sl != n * TE_MSM_SCALAR_BYTES)) {
    napi_throw_range_error(env, nullptr, x_only ? "scalarMulX: xs must be 32*n bytes, scalars 32 (shared) or 32*n bytes"
                                                : "scalarMul: points must be 64*n bytes, scalars 32 (shared) or 32*n bytes");
    return nullptr;
  }
  const int shared = sl == TE_MSM_SCALAR_BYTES ? 1 : 0;
  std::vector<uint8_t> out((size_t)n * TE_MSM_POINT_BYTES);
  int64_t bad = -1, reason = 0;
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    const int r = x_only ? te_msm_mul_x(c, static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(s), n, shared, out.data())
                         : te_msm_mul(c, static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(s), n, shared, out.data());
    if (r == TE_MSM_EPOINT) { (void)te_msm_get_option(c, "bad_point_index", &bad); (void)te_msm_get_option(c, "bad_point_reason", &reason); }
    return r;
  }, err);
  if (rc) {
    const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
    napi_value msg, errv;
    napi_create_string_utf8(env, m.c_str(), m.size(), &msg);
    napi_create_error(env, nullptr, msg, &errv);
    if (rc == TE_MSM_EPOINT) {
      napi_value iv, rv;
      napi_create_int64(env, bad, &iv); napi_create_int32(env, (int32_t)reason, &rv);
      napi_set_named_property(env, errv, "index", iv); napi_set_named_property(env, errv, "reason", rv);
    }
    napi_throw(env, errv);
    return nullptr;
  }
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, out.size(), out.data(), &dst, &buf);
  return buf;
}
// msmBatch(scalarBuffers: Buffer[]): Buffer -- batched MSMs over prefixes of the set bound by setBases (include/te_msm.h,
// te_msm_run_scalars_batch): MSM m runs over the first scalarBuffers[m].length / 32 points of that set.  Returns count x 64 bytes, the
// results in input order (the identity as (0, 1)); compute_msm.js turns them into {x, y}.  Run like pointsFromX; without setBases, with a
// buffer longer than the set, or with a scalar out of range it throws.
napi_value MsmBatch(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool is_arr = false;
  if (argc >= 1) napi_is_array(env, argv[0], &is_arr);
  if (!is_arr) { napi_throw_type_error(env, nullptr, "msmBatch(scalarBuffers: Buffer[])"); return nullptr; }
  uint32_t count = 0;
  napi_get_array_length(env, argv[0], &count);
  std::vector<uint64_t> lens(count);
  std::vector<uint8_t> packed;
  for (uint32_t m = 0; m < count; m++) {
    napi_value e; bool is_buf = false;
    napi_get_element(env, argv[0], m, &e);
    napi_is_buffer(env, e, &is_buf);
    if (!is_buf) { napi_throw_type_error(env, nullptr, "msmBatch(scalarBuffers: Buffer[])"); return nullptr; }
    void* p = nullptr; size_t pl = 0;
    napi_get_buffer_info(env, e, &p, &pl);
    if (pl % msm_scalar_bytes() != 0) { napi_throw_range_error(env, nullptr, "msmBatch: every scalar buffer must be 32*n bytes (8*n / 16*n under setScalarRecordBytes)"); return nullptr; }
    lens[m] = pl / msm_scalar_bytes();
    packed.insert(packed.end(), static_cast<const uint8_t*>(p), static_cast<const uint8_t*>(p) + pl);
  }
  std::vector<uint8_t> out((size_t)count * TE_MSM_POINT_BYTES);
  std::string err;
  const int rc = g_proto.with_bases([&](te_ctx* c, te_bases* b) {
    return te_msm_run_scalars_batch(c, b, (int)count, lens.data(), packed.data(), out.data());
  }, TE_MSM_ESTATE, err);
  if (rc) {
    const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
    napi_throw_error(env, nullptr, m.c_str());
    return nullptr;
  }
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, out.size(), out.data(), &dst, &buf);
  return buf;
}

// msmIndexed(indices: Uint32Array, scalars: Buffer): Buffer -- one MSM over an indexed subset of the set bound by setBases
// (include/te_msm.h, te_msm_run_scalars_indexed): sum_j scalars[j] * P[indices[j]], indices in any order, repeats allowed, each below the
// set's size.  Returns 64 bytes x || y (the identity as (0, 1)); compute_msm.js wraps it into a promise of {x, y}.  Run like msmBatch
// (under the context's lock once no promise is pending); without setBases, with an index outside the set (the Error names the lowest
// offending position, also as .index) or with a scalar out of range it throws.
napi_value MsmIndexed(napi_env env, napi_callback_info info) {
  const char* const sig = "msmIndexed(indices: Uint32Array, scalars: Buffer)";
  size_t argc = 2; napi_value argv[2];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool is_ta = false, is_buf = false;
  if (argc >= 2) { napi_is_typedarray(env, argv[0], &is_ta); napi_is_buffer(env, argv[1], &is_buf); }
  if (!is_ta || !is_buf) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  napi_typedarray_type tt; size_t m = 0; void* ip = nullptr; napi_value ab; size_t off = 0;
  napi_get_typedarray_info(env, argv[0], &tt, &m, &ip, &ab, &off);
  if (tt != napi_uint32_array) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  void* s = nullptr; size_t sl = 0;
  napi_get_buffer_info(env, argv[1], &s, &sl);
  if (sl != m * msm_scalar_bytes()) { napi_throw_range_error(env, nullptr, "msmIndexed: scalars must be 32 bytes per index (8 / 16 under setScalarRecordBytes)"); return nullptr; }
  uint8_t out[TE_MSM_POINT_BYTES];
  int64_t bad = -1;
  std::string err;
  const int rc = g_proto.with_bases([&](te_ctx* c, te_bases* b) {
    const int r = te_msm_run_scalars_indexed(c, b, static_cast<const uint32_t*>(ip), static_cast<const uint8_t*>(s), m, out);
    if (r == TE_MSM_EINVAL && !strncmp(te_msm_last_error(c), "index at position ", 18)) (void)te_msm_get_option(c, "bad_index_position", &bad);
    return r;
  }, TE_MSM_ESTATE, err);
  if (rc) {
    const std::string msg_s = "te_msm error " + std::to_string(rc) + ": " + err;
    napi_value msg, errv;
    napi_create_string_utf8(env, msg_s.c_str(), msg_s.size(), &msg);
    napi_create_error(env, nullptr, msg, &errv);
    if (bad >= 0) { napi_value iv; napi_create_int64(env, bad, &iv); napi_set_named_property(env, errv, "index", iv); }
    napi_throw(env, errv);
    return nullptr;
  }
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, sizeof out, out, &dst, &buf);
  return buf;
}

napi_value ScalarMul(napi_env env, napi_callback_info info) { return MulCommon(env, info, false); }
napi_value ScalarMulX(napi_env env, napi_callback_info info) { return MulCommon(env, info, true); }

// groupAdd(a: Buffer, b: Buffer, opts?: {subtract?: boolean}): Buffer -- batched group addition (include/te_msm.h, te_msm_add): n x 64-byte
// points a and n points b, or ONE 64-byte point b for all of them -> n x 64-byte points A_i + B_i (A_i - B_i with subtract; the identity as
// (0, 1)).  groupAddX(ax, bx, opts) takes x-only points (pointsFromX's format): bulkAddGroups' counterpart (te_msm_add_x).
// groupSum(points: Buffer): Buffer and groupSumX(xs: Buffer): Buffer -- 64 bytes x || y, the sum of the points (no points: (0, 1)):
// reduceGroups' counterpart (te_msm_sum / te_msm_sum_x).  Twisted-Edwards curve only, like the rest of the addon; run like scalarMul.  A bad
// point (setCheckPoints) or a bad x throws an Error naming the lowest failing index and the reason, also as .index / .reason / .operand
// (0 = a or the sum's input, 1 = b).
napi_value GroupThrow(napi_env env, int rc, const std::string& err, int64_t bad, int64_t reason, int64_t operand) {
  const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
  napi_value msg, errv;
  napi_create_string_utf8(env, m.c_str(), m.size(), &msg);
  napi_create_error(env, nullptr, msg, &errv);
  if (rc == TE_MSM_EPOINT) {
    napi_value iv, rv, ov;
    napi_create_int64(env, bad, &iv); napi_create_int32(env, (int32_t)reason, &rv); napi_create_int32(env, (int32_t)operand, &ov);
    napi_set_named_property(env, errv, "index", iv); napi_set_named_property(env, errv, "reason", rv); napi_set_named_property(env, errv, "operand", ov);
  }
  napi_throw(env, errv);
  return nullptr;
}
napi_value AddCommon(napi_env env, napi_callback_info info, bool x_only) {
  const char* const sig = x_only ? "groupAddX(ax: Buffer, bx: Buffer, opts?: {subtract?: boolean})" : "groupAdd(a: Buffer, b: Buffer, opts?: {subtract?: boolean})";
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool b0 = false, b1 = false;
  if (argc >= 2) { napi_is_buffer(env, argv[0], &b0); napi_is_buffer(env, argv[1], &b1); }
  if (!b0 || !b1) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  bool subtract = false;
  if (argc >= 3) {
    napi_valuetype t = napi_undefined;
    napi_typeof(env, argv[2], &t);
    if (t == napi_object) {
      napi_value v; bool has = false;
      napi_has_named_property(env, argv[2], "subtract", &has);
      if (has) { napi_get_named_property(env, argv[2], "subtract", &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &subtract); }
    } else if (t != napi_undefined && t != napi_null) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  }
  void *pa = nullptr, *pb = nullptr; size_t al = 0, bl = 0;
  napi_get_buffer_info(env, argv[0], &pa, &al);
  napi_get_buffer_info(env, argv[1], &pb, &bl);
  const size_t in_bytes = x_only ? TE_MSM_X_BYTES : TE_MSM_POINT_BYTES;
  const uint64_t n = al / in_bytes;
  if (al % in_bytes != 0 || (bl != in_bytes && bl != n * in_bytes)) {
    napi_throw_range_error(env, nullptr, x_only ? "groupAddX: ax must be 32*n bytes, bx 32 (shared) or 32*n bytes" : "groupAdd: a must be 64*n bytes, b 64 (shared) or 64*n bytes");
    return nullptr;
  }
  const int flags = (subtract ? TE_MSM_ADD_SUBTRACT : 0) | (bl != n * in_bytes ? TE_MSM_ADD_SHARED_B : 0);
  std::vector<uint8_t> out((size_t)n * TE_MSM_POINT_BYTES);
  int64_t bad = -1, reason = 0, operand = -1;
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    const int r = x_only ? te_msm_add_x(c, static_cast<const uint8_t*>(pa), static_cast<const uint8_t*>(pb), n, flags, out.data())
                         : te_msm_add(c, static_cast<const uint8_t*>(pa), static_cast<const uint8_t*>(pb), n, flags, out.data());
    if (r == TE_MSM_EPOINT) {
      (void)te_msm_get_option(c, "bad_point_index", &bad); (void)te_msm_get_option(c, "bad_point_reason", &reason); (void)te_msm_get_option(c, "bad_point_operand", &operand);
    }
    return r;
  }, err);
  if (rc) return GroupThrow(env, rc, err, bad, reason, operand);
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, out.size(), out.data(), &dst, &buf);
  return buf;
}
napi_value SumCommon(napi_env env, napi_callback_info info, bool x_only) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool b0 = false;
  if (argc >= 1) napi_is_buffer(env, argv[0], &b0);
  if (!b0) { napi_throw_type_error(env, nullptr, x_only ? "groupSumX(xs: Buffer)" : "groupSum(points: Buffer)"); return nullptr; }
  void* p = nullptr; size_t pl = 0;
  napi_get_buffer_info(env, argv[0], &p, &pl);
  const size_t in_bytes = x_only ? TE_MSM_X_BYTES : TE_MSM_POINT_BYTES;
  if (pl % in_bytes != 0) { napi_throw_range_error(env, nullptr, x_only ? "groupSumX: xs must be 32*n bytes" : "groupSum: points must be 64*n bytes"); return nullptr; }
  const uint64_t n = pl / in_bytes;
  uint8_t out[TE_MSM_POINT_BYTES];
  int64_t bad = -1, reason = 0, operand = -1;
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    const int r = x_only ? te_msm_sum_x(c, static_cast<const uint8_t*>(p), n, out) : te_msm_sum(c, static_cast<const uint8_t*>(p), n, out);
    if (r == TE_MSM_EPOINT) {
      (void)te_msm_get_option(c, "bad_point_index", &bad); (void)te_msm_get_option(c, "bad_point_reason", &reason); (void)te_msm_get_option(c, "bad_point_operand", &operand);
    }
    return r;
  }, err);
  if (rc) return GroupThrow(env, rc, err, bad, reason, operand);
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, sizeof out, out, &dst, &buf);
  return buf;
}
napi_value GroupAdd(napi_env env, napi_callback_info info) { return AddCommon(env, info, false); }
napi_value GroupAddX(napi_env env, napi_callback_info info) { return AddCommon(env, info, true); }
napi_value GroupSum(napi_env env, napi_callback_info info) { return SumCommon(env, info, false); }
napi_value GroupSumX(napi_env env, napi_callback_info info) { return SumCommon(env, info, true); }

// fieldOp(op: number, a: Buffer, b: Buffer | null, opts?: {field?: 0 | 1, sharedB?: boolean, montgomery?: boolean, zeroOk?: boolean}): Buffer --
// batched field arithmetic (include/te_msm.h, te_msm_field_op): n elements a of 32 (field 0: p, Aleo's `field`) or 48 bytes (field 1: q of
// BLS12-377) and, for TE_MSM_FIELD_ADD / SUB / MUL / POW, n records b (an exponent is 32 bytes on both fields) or ONE with sharedB ->
// n elements a_i op b_i; b null for the ops of one operand.  The counterpart of the reference's bulk*Fields; run like groupAdd.  The inverse
// of 0 without zeroOk and the root of a non-square throw an Error naming the lowest failing index, also as .index / .reason (1 zero, 2 not
// a square); compute_msm.js wraps the call into a promise, which then rejects with that Error.
napi_value FieldOp(napi_env env, napi_callback_info info) {
  const char* const sig = "fieldOp(op: number, a: Buffer, b: Buffer | null, opts?: {field?: 0 | 1, sharedB?: boolean, montgomery?: boolean, zeroOk?: boolean})";
  size_t argc = 4; napi_value argv[4];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool a_buf = false, b_buf = false;
  napi_valuetype t_op = napi_undefined, t_b = napi_undefined, t_opts = napi_undefined;
  if (argc >= 1) napi_typeof(env, argv[0], &t_op);
  if (argc >= 2) napi_is_buffer(env, argv[1], &a_buf);
  if (argc >= 3) { napi_typeof(env, argv[2], &t_b); napi_is_buffer(env, argv[2], &b_buf); }
  if (argc >= 4) napi_typeof(env, argv[3], &t_opts);
  const bool b_none = t_b == napi_undefined || t_b == napi_null, opts_none = t_opts == napi_undefined || t_opts == napi_null;
  if (t_op != napi_number || !a_buf || (!b_buf && !b_none) || (t_opts != napi_object && !opts_none)) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  int32_t op = -1, field = TE_MSM_FIELD_P;
  napi_get_value_int32(env, argv[0], &op);
  int flags = 0;
  if (t_opts == napi_object) {
    const struct { const char* name; int bit; } bits[] = {{"sharedB", TE_MSM_FIELD_SHARED_B}, {"montgomery", TE_MSM_FIELD_MONTGOMERY}, {"zeroOk", TE_MSM_FIELD_ZERO_OK}};
    for (const auto& f : bits) {
      napi_value v; bool has = false, on = false;
      napi_has_named_property(env, argv[3], f.name, &has);
      if (has) { napi_get_named_property(env, argv[3], f.name, &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &on); }
      if (on) flags |= f.bit;
    }
    napi_value v; bool has = false;
    napi_has_named_property(env, argv[3], "field", &has);
    if (has) { napi_get_named_property(env, argv[3], "field", &v); if (napi_get_value_int32(env, v, &field) != napi_ok) { napi_throw_type_error(env, nullptr, sig); return nullptr; } }
  }
  void *pa = nullptr, *pb = nullptr; size_t al = 0, bl = 0;
  napi_get_buffer_info(env, argv[1], &pa, &al);
  if (b_buf) napi_get_buffer_info(env, argv[2], &pb, &bl);
  const size_t eb = field == TE_MSM_FIELD_Q377 ? 48 : 32, bb = op == TE_MSM_FIELD_POW ? 32 : eb;
  const uint64_t n = al / eb;
  if (al % eb != 0 || (b_buf && bl != ((flags & TE_MSM_FIELD_SHARED_B) ? bb : n * bb))) {
    napi_throw_range_error(env, nullptr, "fieldOp: a must be 32*n (48*n on field 1) bytes, b one record per element (32 bytes for an exponent) or one record with sharedB");
    return nullptr;
  }
  std::vector<uint8_t> out((size_t)n * eb);
  int64_t bad = -1, reason = 0;
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    const int r = te_msm_field_op(c, field, op, static_cast<const uint8_t*>(pa), b_buf ? static_cast<const uint8_t*>(pb) : nullptr, n, flags, out.data());
    if (r == TE_MSM_EFIELD) { (void)te_msm_get_option(c, "bad_field_index", &bad); (void)te_msm_get_option(c, "bad_field_reason", &reason); }
    return r;
  }, err);
  if (rc) {
    const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
    napi_value msg, errv;
    napi_create_string_utf8(env, m.c_str(), m.size(), &msg);
    napi_create_error(env, nullptr, msg, &errv);
    if (rc == TE_MSM_EFIELD) {
      napi_value iv, rv;
      napi_create_int64(env, bad, &iv); napi_create_int32(env, (int32_t)reason, &rv);
      napi_set_named_property(env, errv, "index", iv); napi_set_named_property(env, errv, "reason", rv);
    }
    napi_throw(env, errv);
    return nullptr;
  }
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, out.size(), out.data(), &dst, &buf);
  return buf;
}

// ntt(a: Buffer, logN: number, opts?: {count?: number, inverse?: boolean, montgomery?: boolean, shift?: Buffer}): Buffer -- batched NTTs over p
// (include/te_msm.h, te_msm_ntt): `count` (default 1) transforms of 2^logN 32-byte elements each, natural order in and out, the radix-2
// domains of arkworks / snarkVM; shift: one 32-byte record, the coset generator.  Run like fieldOp; a refusal (logN above 24, a shift
// that is 0 mod p) throws; compute_msm.js wraps the call into a promise, which then rejects with that Error.
napi_value Ntt(napi_env env, napi_callback_info info) {
  const char* const sig = "ntt(a: Buffer, logN: number, opts?: {count?: number, inverse?: boolean, montgomery?: boolean, shift?: Buffer})";
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool a_buf = false;
  napi_valuetype t_log = napi_undefined, t_opts = napi_undefined;
  if (argc >= 1) napi_is_buffer(env, argv[0], &a_buf);
  if (argc >= 2) napi_typeof(env, argv[1], &t_log);
  if (argc >= 3) napi_typeof(env, argv[2], &t_opts);
  const bool opts_none = t_opts == napi_undefined || t_opts == napi_null;
  if (!a_buf || t_log != napi_number || (t_opts != napi_object && !opts_none)) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  uint32_t log_n = 0;
  napi_get_value_uint32(env, argv[1], &log_n);
  int flags = 0;
  int64_t count = 1;
  void* ps = nullptr; size_t sl = 0; bool s_buf = false;
  if (t_opts == napi_object) {
    const struct { const char* name; int bit; } bits[] = {{"inverse", TE_MSM_NTT_INVERSE}, {"montgomery", TE_MSM_NTT_MONTGOMERY}};
    for (const auto& f : bits) {
      napi_value v; bool has = false, on = false;
      napi_has_named_property(env, argv[2], f.name, &has);
      if (has) { napi_get_named_property(env, argv[2], f.name, &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &on); }
      if (on) flags |= f.bit;
    }
    napi_value v; bool has = false;
    napi_has_named_property(env, argv[2], "count", &has);
    if (has) { napi_get_named_property(env, argv[2], "count", &v); if (napi_get_value_int64(env, v, &count) != napi_ok || count < 0) { napi_throw_type_error(env, nullptr, sig); return nullptr; } }
    napi_has_named_property(env, argv[2], "shift", &has);
    if (has) {
      napi_valuetype t_s = napi_undefined;
      napi_get_named_property(env, argv[2], "shift", &v);
      napi_typeof(env, v, &t_s);
      napi_is_buffer(env, v, &s_buf);
      if (!s_buf && t_s != napi_undefined && t_s != napi_null) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
      if (s_buf) napi_get_buffer_info(env, v, &ps, &sl);
    }
  }
  void* pa = nullptr; size_t al = 0;
  napi_get_buffer_info(env, argv[0], &pa, &al);
  if ((s_buf && sl != 32) || (log_n <= TE_MSM_NTT_MAX_LOG_N && al != (((size_t)count * 32) << log_n))) {
    napi_throw_range_error(env, nullptr, "ntt: a must be count * 2^logN * 32 bytes, shift one record of 32");
    return nullptr;
  }
  std::vector<uint8_t> out(al);
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    return te_msm_ntt(c, static_cast<const uint8_t*>(pa), log_n, (uint64_t)count, flags, s_buf ? static_cast<const uint8_t*>(ps) : nullptr, out.data());
  }, err);
  if (rc) {
    const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
    napi_throw_error(env, nullptr, m.c_str());
    return nullptr;
  }
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, out.size(), out.data(), &dst, &buf);
  return buf;
}

// polyDivide(a: Buffer, n: number, z: Buffer, opts?: {count?: number, montgomery?: boolean, sharedZ?: boolean, quotient?: boolean}):
// {evals: Buffer, quotient: Buffer | null} -- polynomial openings over p (include/te_msm.h, te_msm_poly_divide): `count` (default 1)
// polynomials of n 32-byte coefficients each, lowest first; z one 32-byte record a polynomial, or one in all with sharedZ.  evals: a(z) of
// each; quotient: the coefficients of (a(X) - a(z)) / (X - z) at the stride n, or null with quotient: false (the call then only
// evaluates).  Run like ntt; a refusal (n = 0, n above 2^30) throws.
napi_value PolyDivide(napi_env env, napi_callback_info info) {
  const char* const sig = "polyDivide(a: Buffer, n: number, z: Buffer, opts?: {count?: number, montgomery?: boolean, sharedZ?: boolean, quotient?: boolean})";
  size_t argc = 4; napi_value argv[4];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool a_buf = false, z_buf = false;
  napi_valuetype t_n = napi_undefined, t_opts = napi_undefined;
  if (argc >= 1) napi_is_buffer(env, argv[0], &a_buf);
  if (argc >= 2) napi_typeof(env, argv[1], &t_n);
  if (argc >= 3) napi_is_buffer(env, argv[2], &z_buf);
  if (argc >= 4) napi_typeof(env, argv[3], &t_opts);
  const bool opts_none = t_opts == napi_undefined || t_opts == napi_null;
  if (!a_buf || !z_buf || t_n != napi_number || (t_opts != napi_object && !opts_none)) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  int64_t n = 0, count = 1;
  if (napi_get_value_int64(env, argv[1], &n) != napi_ok || n < 0) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  int flags = 0;
  bool want_q = true;
  if (t_opts == napi_object) {
    const struct { const char* name; int bit; } bits[] = {{"montgomery", TE_MSM_POLY_MONTGOMERY}, {"sharedZ", TE_MSM_POLY_SHARED_Z}};
    for (const auto& f : bits) {
      napi_value v; bool has = false, on = false;
      napi_has_named_property(env, argv[3], f.name, &has);
      if (has) { napi_get_named_property(env, argv[3], f.name, &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &on); }
      if (on) flags |= f.bit;
    }
    napi_value v; bool has = false;
    napi_has_named_property(env, argv[3], "count", &has);
    if (has) { napi_get_named_property(env, argv[3], "count", &v); if (napi_get_value_int64(env, v, &count) != napi_ok || count < 0) { napi_throw_type_error(env, nullptr, sig); return nullptr; } }
    napi_has_named_property(env, argv[3], "quotient", &has);
    if (has) { napi_get_named_property(env, argv[3], "quotient", &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &want_q); }
  }
  void *pa = nullptr, *pz = nullptr; size_t al = 0, zl = 0;
  napi_get_buffer_info(env, argv[0], &pa, &al);
  napi_get_buffer_info(env, argv[2], &pz, &zl);
  const bool n_ok = n >= 1 && (uint64_t)n <= TE_MSM_POLY_MAX_N;      // (the library refuses the others itself: any a is then passed through)
  if (zl != 32u * (size_t)((flags & TE_MSM_POLY_SHARED_Z) ? 1 : count) || (n_ok && (count > (int64_t)(SIZE_MAX >> 36) || al != (size_t)count * (size_t)n * 32u))) {
    napi_throw_range_error(env, nullptr, "polyDivide: a must be count * n * 32 bytes, z one record of 32 a polynomial (one in all with sharedZ)");
    return nullptr;
  }
  std::vector<uint8_t> evals((size_t)count * 32 + 1), q(want_q ? al + 1 : 0);      // (never empty: an output the call is given is not NULL)
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    return te_msm_poly_divide(c, static_cast<const uint8_t*>(pa), (uint64_t)n, (uint64_t)count, static_cast<const uint8_t*>(pz), flags, evals.data(), want_q ? q.data() : nullptr);
  }, err);
  if (rc) {
    const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
    napi_throw_error(env, nullptr, m.c_str());
    return nullptr;
  }
  napi_value res, be, bq; void* dst = nullptr;
  napi_create_object(env, &res);
  napi_create_buffer_copy(env, (size_t)count * 32, evals.data(), &dst, &be);
  if (want_q) napi_create_buffer_copy(env, al, q.data(), &dst, &bq); else napi_get_null(env, &bq);
  napi_set_named_property(env, res, "evals", be);
  napi_set_named_property(env, res, "quotient", bq);
  return res;
}

// fieldScan(op: number, a: Buffer, n: number, opts?: {count?: number, init?: Buffer, montgomery?: boolean, exclusive?: boolean, sharedA?: boolean,
// out?: boolean, totals?: boolean}): {out: Buffer | null, totals: Buffer | null} -- prefix sums (op 0) and products (op 1) over p
// (include/te_msm.h, te_msm_field_scan): `count` (default 1) vectors of n 32-byte records each -- ONE record each with sharedA -- from
// their seeds init (one 32-byte record a vector; absent: the identity).  out: the running values at the stride n, inclusive or exclusive;
// totals: seed o a_0 o .. o a_(n-1) of each vector; either is null when its option is false.  Run like ntt; a refusal throws.
napi_value FieldScan(napi_env env, napi_callback_info info) {
  const char* const sig = "fieldScan(op: number, a: Buffer, n: number, opts?: {count?: number, init?: Buffer, montgomery?: boolean, exclusive?: boolean, sharedA?: boolean, "
                          "out?: boolean, totals?: boolean})";
  size_t argc = 4; napi_value argv[4];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool a_buf = false;
  napi_valuetype t_op = napi_undefined, t_n = napi_undefined, t_opts = napi_undefined;
  if (argc >= 1) napi_typeof(env, argv[0], &t_op);
  if (argc >= 2) napi_is_buffer(env, argv[1], &a_buf);
  if (argc >= 3) napi_typeof(env, argv[2], &t_n);
  if (argc >= 4) napi_typeof(env, argv[3], &t_opts);
  const bool opts_none = t_opts == napi_undefined || t_opts == napi_null;
  if (!a_buf || t_op != napi_number || t_n != napi_number || (t_opts != napi_object && !opts_none)) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  int32_t op = 0;
  int64_t n = 0, count = 1;
  if (napi_get_value_int32(env, argv[0], &op) != napi_ok || napi_get_value_int64(env, argv[2], &n) != napi_ok || n < 0) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  int flags = 0;
  bool want_out = true, want_totals = true;
  void* pi = nullptr; size_t il = 0;
  if (t_opts == napi_object) {
    const struct { const char* name; int bit; } bits[] = {{"montgomery", TE_MSM_SCAN_MONTGOMERY}, {"exclusive", TE_MSM_SCAN_EXCLUSIVE}, {"sharedA", TE_MSM_SCAN_SHARED_A}};
    for (const auto& f : bits) {
      napi_value v; bool has = false, on = false;
      napi_has_named_property(env, argv[3], f.name, &has);
      if (has) { napi_get_named_property(env, argv[3], f.name, &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &on); }
      if (on) flags |= f.bit;
    }
    napi_value v; bool has = false;
    napi_has_named_property(env, argv[3], "count", &has);
    if (has) { napi_get_named_property(env, argv[3], "count", &v); if (napi_get_value_int64(env, v, &count) != napi_ok || count < 0) { napi_throw_type_error(env, nullptr, sig); return nullptr; } }
    napi_has_named_property(env, argv[3], "out", &has);
    if (has) { napi_get_named_property(env, argv[3], "out", &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &want_out); }
    napi_has_named_property(env, argv[3], "totals", &has);
    if (has) { napi_get_named_property(env, argv[3], "totals", &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &want_totals); }
    napi_has_named_property(env, argv[3], "init", &has);
    if (has) {
      napi_valuetype t_init = napi_undefined; bool init_buf = false;
      napi_get_named_property(env, argv[3], "init", &v);
      napi_typeof(env, v, &t_init);
      if (t_init != napi_undefined && t_init != napi_null) {
        napi_is_buffer(env, v, &init_buf);
        if (!init_buf) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
        napi_get_buffer_info(env, v, &pi, &il);
        if (il != 32u * (size_t)count) { napi_throw_range_error(env, nullptr, "fieldScan: init must be one record of 32 bytes a vector"); return nullptr; }
        if (!pi) pi = &il;                                            // (count = 0: an empty Buffer; any non-NULL pointer)
      }
    }
  }
  void* pa = nullptr; size_t al = 0;
  napi_get_buffer_info(env, argv[1], &pa, &al);
  const bool n_ok = n >= 1 && (uint64_t)n <= TE_MSM_SCAN_MAX_N;      // (the library refuses the others itself: any a is then passed through)
  const bool shared = (flags & TE_MSM_SCAN_SHARED_A) != 0;
  if (n_ok && (count > (int64_t)(SIZE_MAX >> 36) || (uint64_t)count * (uint64_t)n > (SIZE_MAX >> 6) || al != (size_t)count * (shared ? 1u : (size_t)n) * 32u)) {
    napi_throw_range_error(env, nullptr, "fieldScan: a must be count * n * 32 bytes (count * 32 with sharedA)");
    return nullptr;
  }
  const size_t ol = n_ok ? (size_t)count * (size_t)n * 32u : 0;
  std::vector<uint8_t> totals(want_totals ? (size_t)count * 32 + 1 : 0), out(want_out ? ol + 1 : 0);      // (never empty: an output the call is given is not NULL)
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    return te_msm_field_scan(c, op, static_cast<const uint8_t*>(pa), (uint64_t)n, (uint64_t)count, flags, static_cast<const uint8_t*>(pi), want_totals ? totals.data() : nullptr,
                             want_out ? out.data() : nullptr);
  }, err);
  if (rc) {
    const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
    napi_throw_error(env, nullptr, m.c_str());
    return nullptr;
  }
  napi_value res, bo, bt; void* dst = nullptr;
  napi_create_object(env, &res);
  if (want_out) napi_create_buffer_copy(env, ol, out.data(), &dst, &bo); else napi_get_null(env, &bo);
  if (want_totals) napi_create_buffer_copy(env, (size_t)count * 32, totals.data(), &dst, &bt); else napi_get_null(env, &bt);
  napi_set_named_property(env, res, "out", bo);
  napi_set_named_property(env, res, "totals", bt);
  return res;
}

// setBase(point: Buffer) and scalarMulBase(scalars: Buffer): Buffer -- fixed-base batch scalar multiplication (include/te_msm.h,
// te_msm_bind_base / te_msm_mul_base): one 64-byte point bound once, then n x 32-byte little-endian scalars -> n x 64-byte points
// [k_i] P (the identity as (0, 1)).  Twisted-Edwards curve only, like the rest of the addon; run like scalarMul.  The addon keeps the
// point: a context that replaces the cached one (setDevices, setCheckPoints, ...) binds it again at the next scalarMulBase.  The addon
// is the only one to bind points on its context, so "no point bound there" is the read-only option "mul_bases_bound" = 0.  A bad
// point (setCheckPoints) throws as scalarMul does, with .index 0; setScalarsMontgomery applies to the scalars.
uint8_t g_base_point[TE_MSM_POINT_BYTES];
bool g_have_base = false;
te_base* g_base = nullptr;      // the handle on the cached context (stale once that context is gone: see bound_base)

int bound_base(te_ctx* c, bool rebind) {
  int64_t bound = 0;
  (void)te_msm_get_option(c, "mul_bases_bound", &bound);
  if (bound && rebind) { (void)te_msm_release_base(c, g_base); bound = 0; }
  if (!bound) { g_base = nullptr; return te_msm_bind_base(c, g_base_point, &g_base); }
  return 0;
}
napi_value throw_te_error(napi_env env, int rc, const std::string& err, int64_t bad, int64_t reason) {
  const std::string m = "te_msm error " + std::to_string(rc) + ": " + err;
  napi_value msg, errv;
  napi_create_string_utf8(env, m.c_str(), m.size(), &msg);
  napi_create_error(env, nullptr, msg, &errv);
  if (rc == TE_MSM_EPOINT) {
    napi_value iv, rv;
    napi_create_int64(env, bad, &iv); napi_create_int32(env, (int32_t)reason, &rv);
    napi_set_named_property(env, errv, "index", iv); napi_set_named_property(env, errv, "reason", rv);
  }
  napi_throw(env, errv);
  return nullptr;
}
napi_value SetBase(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool b0 = false;
  if (argc >= 1) napi_is_buffer(env, argv[0], &b0);
  if (!b0) { napi_throw_type_error(env, nullptr, "setBase(point: Buffer)"); return nullptr; }
  void* p = nullptr; size_t pl = 0;
  napi_get_buffer_info(env, argv[0], &p, &pl);
  if (pl != TE_MSM_POINT_BYTES) { napi_throw_range_error(env, nullptr, "setBase: the point must be 64 bytes"); return nullptr; }
  memcpy(g_base_point, p, TE_MSM_POINT_BYTES);
  g_have_base = true;
  int64_t bad = -1, reason = 0;
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    const int r = bound_base(c, true);
    if (r == TE_MSM_EPOINT) { (void)te_msm_get_option(c, "bad_point_index", &bad); (void)te_msm_get_option(c, "bad_point_reason", &reason); }
    return r;
  }, err);
  if (rc) { g_have_base = false; return throw_te_error(env, rc, err, bad, reason); }
  napi_value u; napi_get_undefined(env, &u); return u;
}
napi_value ScalarMulBase(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool b0 = false;
  if (argc >= 1) napi_is_buffer(env, argv[0], &b0);
  if (!b0) { napi_throw_type_error(env, nullptr, "scalarMulBase(scalars: Buffer)"); return nullptr; }
  if (!g_have_base) { napi_throw_error(env, nullptr, "scalarMulBase: no point bound (setBase)"); return nullptr; }
  void* s = nullptr; size_t sl = 0;
  napi_get_buffer_info(env, argv[0], &s, &sl);
  if (sl % TE_MSM_SCALAR_BYTES != 0) { napi_throw_range_error(env, nullptr, "scalarMulBase: scalars must be 32*n bytes"); return nullptr; }
  const uint64_t n = sl / TE_MSM_SCALAR_BYTES;
  std::vector<uint8_t> out((size_t)n * TE_MSM_POINT_BYTES);
  int64_t bad = -1, reason = 0;
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    int r = bound_base(c, false);
    if (!r) r = te_msm_mul_base(c, g_base, static_cast<const uint8_t*>(s), n, out.data());
    if (r == TE_MSM_EPOINT) { (void)te_msm_get_option(c, "bad_point_index", &bad); (void)te_msm_get_option(c, "bad_point_reason", &reason); }
    return r;
  }, err);
  if (rc) return throw_te_error(env, rc, err, bad, reason);
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, out.size(), out.data(), &dst, &buf);
  return buf;
}

// bindMatrix(rows, cols, rowPtr: Buffer, colIdx: Buffer, vals: Buffer, opts?: {montgomery?: boolean, transpose?: boolean}): number,
// spmv(id, x: Buffer, opts?: {count?: number, montgomery?: boolean, transpose?: boolean}): Buffer and releaseMatrix(id) -- sparse matrices
// over p (include/te_msm.h "sparse matrices", te_msm_bind_matrix / te_msm_spmv): a CSR matrix -- rows + 1 offsets of 8 bytes, nnz column
// indices of 4 bytes and nnz values of 32 bytes, all little-endian -- bound once, then `count` (default 1) vectors of cols records each
// (rows with transpose, which the bind must have kept) -> count x rows records (count x cols).  Run like ntt; a refusal throws.  The addon
// keeps the arrays, as setBase keeps its point: a context that replaces the cached one binds the matrix again at the next spmv (a fresh
// context holds no matrix: read-only option "matrix_bytes" = 0).
struct BoundMatrix {
  uint64_t rows = 0, cols = 0; int flags = 0;
  std::vector<uint64_t> ptr; std::vector<uint32_t> col; std::vector<uint8_t> vals;
  te_ctx* owner = nullptr; te_matrix* handle = nullptr;      // stale once `owner` is gone: see bound_matrix
};
std::vector<std::unique_ptr<BoundMatrix>> g_matrices;          // id = index + 1; a released slot is empty
int bound_matrix(te_ctx* c, BoundMatrix& m) {
  int64_t held = 0;
  (void)te_msm_get_option(c, "matrix_bytes", &held);
  if (m.owner == c && held > 0 && m.handle) return 0;
  if (held == 0) for (auto& o : g_matrices) if (o) { o->owner = nullptr; o->handle = nullptr; }     // a fresh context: every handle is stale
  m.handle = nullptr;
  const int rc = te_msm_bind_matrix(c, m.rows, m.cols, m.ptr.data(), m.col.data(), m.vals.data(), m.flags, &m.handle);
  m.owner = rc ? nullptr : c;
  return rc;
}
bool flag_of(napi_env env, napi_value opts, const char* name) {
  napi_value v; bool has = false, on = false;
  napi_has_named_property(env, opts, name, &has);
  if (has) { napi_get_named_property(env, opts, name, &v); napi_coerce_to_bool(env, v, &v); napi_get_value_bool(env, v, &on); }
  return on;
}
napi_value BindMatrix(napi_env env, napi_callback_info info) {
  const char* const sig = "bindMatrix(rows: number, cols: number, rowPtr: Buffer, colIdx: Buffer, vals: Buffer, opts?: {montgomery?: boolean, transpose?: boolean})";
  size_t argc = 6; napi_value argv[6];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool b2 = false, b3 = false, b4 = false;
  napi_valuetype t_opts = napi_undefined;
  int64_t rows = -1, cols = -1;
  if (argc >= 5) { napi_is_buffer(env, argv[2], &b2); napi_is_buffer(env, argv[3], &b3); napi_is_buffer(env, argv[4], &b4); }
  if (argc >= 6) napi_typeof(env, argv[5], &t_opts);
  const bool opts_none = t_opts == napi_undefined || t_opts == napi_null;
  if (!b2 || !b3 || !b4 || napi_get_value_int64(env, argv[0], &rows) != napi_ok || napi_get_value_int64(env, argv[1], &cols) != napi_ok || rows < 0 || cols < 0 ||
      (t_opts != napi_object && !opts_none)) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  auto m = std::make_unique<BoundMatrix>();
  m->rows = (uint64_t)rows; m->cols = (uint64_t)cols;
  if (t_opts == napi_object) m->flags = (flag_of(env, argv[5], "montgomery") ? TE_MSM_MATRIX_MONTGOMERY : 0) | (flag_of(env, argv[5], "transpose") ? TE_MSM_MATRIX_TRANSPOSE : 0);
  void *pp = nullptr, *pc = nullptr, *pv = nullptr; size_t lp = 0, lc = 0, lv = 0;
  napi_get_buffer_info(env, argv[2], &pp, &lp);
  napi_get_buffer_info(env, argv[3], &pc, &lc);
  napi_get_buffer_info(env, argv[4], &pv, &lv);
  if ((uint64_t)rows >= (1ull << 32) || lp != 8u * ((size_t)rows + 1u)) { napi_throw_range_error(env, nullptr, "bindMatrix: rowPtr must be (rows + 1) * 8 bytes"); return nullptr; }
  m->ptr.resize((size_t)rows + 1u);
  memcpy(m->ptr.data(), pp, lp);
  const uint64_t nnz = m->ptr.back();
  if (lc / 4u < nnz || lv / 32u < nnz) { napi_throw_range_error(env, nullptr, "bindMatrix: colIdx and vals must hold rowPtr[rows] entries of 4 and 32 bytes"); return nullptr; }
  m->col.resize((size_t)nnz + 1u); m->vals.resize((size_t)nnz * 32u + 1u);      // (never empty: an array the bind is given is not NULL)
  if (nnz) { memcpy(m->col.data(), pc, (size_t)nnz * 4u); memcpy(m->vals.data(), pv, (size_t)nnz * 32u); }
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) { return bound_matrix(c, *m); }, err);
  if (rc) return throw_te_error(env, rc, err, -1, 0);
  g_matrices.push_back(std::move(m));
  napi_value id; napi_create_int64(env, (int64_t)g_matrices.size(), &id);
  return id;
}
BoundMatrix* matrix_by_id(napi_env env, napi_value v) {
  int64_t id = 0;
  if (napi_get_value_int64(env, v, &id) != napi_ok || id < 1 || (size_t)id > g_matrices.size() || !g_matrices[(size_t)id - 1]) return nullptr;
  return g_matrices[(size_t)id - 1].get();
}
napi_value Spmv(napi_env env, napi_callback_info info) {
  const char* const sig = "spmv(id: number, x: Buffer, opts?: {count?: number, montgomery?: boolean, transpose?: boolean})";
  size_t argc = 3; napi_value argv[3];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool x_buf = false;
  napi_valuetype t_opts = napi_undefined;
  if (argc >= 2) napi_is_buffer(env, argv[1], &x_buf);
  if (argc >= 3) napi_typeof(env, argv[2], &t_opts);
  const bool opts_none = t_opts == napi_undefined || t_opts == napi_null;
  if (!x_buf || (t_opts != napi_object && !opts_none)) { napi_throw_type_error(env, nullptr, sig); return nullptr; }
  BoundMatrix* m = matrix_by_id(env, argv[0]);
  if (!m) { napi_throw_error(env, nullptr, "spmv: no such matrix (bindMatrix; released?)"); return nullptr; }
  int64_t count = 1; int flags = 0;
  if (t_opts == napi_object) {
    flags = (flag_of(env, argv[2], "montgomery") ? TE_MSM_SPMV_MONTGOMERY : 0) | (flag_of(env, argv[2], "transpose") ? TE_MSM_SPMV_TRANSPOSE : 0);
    napi_value v; bool has = false;
    napi_has_named_property(env, argv[2], "count", &has);
    if (has) { napi_get_named_property(env, argv[2], "count", &v); if (napi_get_value_int64(env, v, &count) != napi_ok || count < 0) { napi_throw_type_error(env, nullptr, sig); return nullptr; } }
  }
  const bool tr = (flags & TE_MSM_SPMV_TRANSPOSE) != 0;
  const uint64_t n_in = tr ? m->rows : m->cols, n_out = tr ? m->cols : m->rows;
  void* px = nullptr; size_t xl = 0;
  napi_get_buffer_info(env, argv[1], &px, &xl);
  if (count > (int64_t)(SIZE_MAX >> 38) || xl != (size_t)count * (size_t)n_in * 32u) {
    napi_throw_range_error(env, nullptr, "spmv: x must be count * cols * 32 bytes (count * rows with transpose)");
    return nullptr;
  }
  std::vector<uint8_t> out((size_t)count * (size_t)n_out * 32u + 1u);
  std::string err;
  const int rc = g_proto.with_context([&](te_ctx* c) {
    int r = bound_matrix(c, *m);
    if (!r) r = te_msm_spmv(c, m->handle, static_cast<const uint8_t*>(px), (uint64_t)count, flags, out.data());
    return r;
  }, err);
  if (rc) return throw_te_error(env, rc, err, -1, 0);
  napi_value buf; void* dst = nullptr;
  napi_create_buffer_copy(env, out.size() - 1u, out.data(), &dst, &buf);
  return buf;
}
napi_value ReleaseMatrix(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  BoundMatrix* m = argc >= 1 ? matrix_by_id(env, argv[0]) : nullptr;
  if (!m) { napi_throw_error(env, nullptr, "releaseMatrix: no such matrix"); return nullptr; }
  std::string err;
  (void)g_proto.with_context([&](te_ctx* c) {
    int64_t held = 0;
    (void)te_msm_get_option(c, "matrix_bytes", &held);
    return m->owner == c && held > 0 && m->handle ? te_msm_release_matrix(c, m->handle) : 0;
  }, err);
  int64_t id = 0; napi_get_value_int64(env, argv[0], &id);
  g_matrices[(size_t)id - 1].reset();
  napi_value u; napi_get_undefined(env, &u); return u;
}

// setCheckPoints(level): opt-in validation of the input points (include/te_msm.h, option "check_points"): 0 = none (default),
// 1 = canonical and on the curve, 2 = also in the prime-order subgroup (costly: about 3 000 field products per point).  A call whose
// points fail rejects its promise with an Error that names the lowest failing index and the reason; setBases then throws for a bad
// set.  Takes effect for the next call: the cached context is dropped once no promise is pending (like resetContext), so call it
// before setBases.
napi_value SetCheckPoints(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  int32_t level = -1;
  if (argc < 1 || napi_get_value_int32(env, argv[0], &level) != napi_ok || level < 0 || level > 2) {
    napi_throw_range_error(env, nullptr, "setCheckPoints(level: 0 | 1 | 2)");
    return nullptr;
  }
  g_proto.reset();
  g_check_points.store(level);
  napi_value u; napi_get_undefined(env, &u); return u;
}

// setScalarsMontgomery(flag): the scalar buffers of later calls hold a native prover's Montgomery residues, k * 2^256 mod L (include/te_msm.h,
// option "scalars_montgomery": decoded on the device, in the digit kernels).  Applies to compute_msm, msmBatch and msmIndexed; scalarMul /
// scalarMulX take canonical scalars only and throw while it is set.  Takes effect for the next call, like setCheckPoints: the cached
// context is dropped once no promise is pending (a bound point set is bound again on the new one).
napi_value SetScalarsMontgomery(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  bool flag = false;
  if (argc < 1 || napi_coerce_to_bool(env, argv[0], &argv[0]) != napi_ok || napi_get_value_bool(env, argv[0], &flag) != napi_ok) {
    napi_throw_type_error(env, nullptr, "setScalarsMontgomery(flag: boolean)");
    return nullptr;
  }
  g_proto.reset();
  g_scalars_montgomery.store(flag ? 1 : 0);
  napi_value u; napi_get_undefined(env, &u); return u;
}

// setScalarRecordBytes(n): option "scalar_record_bytes" (include/te_msm.h) for the next call, like setScalarsMontgomery: 0 = the curve's own
// record, 32 or 48 spelled out, 8 / 16 = the scalar buffers of compute_msm, msmBatch and msmIndexed are a native u64 / u128 array (little-endian,
// n * 8 / n * 16 bytes; scalarMul* reject under them).  The addon runs the Twisted-Edwards curve, whose own record is 32 bytes: 0 and 32 change
// nothing, and under 48 every call that reads scalars rejects with the engine's TE_MSM_EINVAL.
napi_value SetScalarRecordBytes(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  int32_t n = -1;
  if (argc < 1 || napi_get_value_int32(env, argv[0], &n) != napi_ok || (n != 0 && n != 8 && n != 16 && n != 32 && n != 48)) {
    napi_throw_type_error(env, nullptr, "setScalarRecordBytes(n: 0 | 8 | 16 | 32 | 48)");
    return nullptr;
  }
  g_proto.reset();
  g_scalar_record_bytes.store(n);
  napi_value u; napi_get_undefined(env, &u); return u;
}

// setScalarBits(b): option "scalar_bits" (include/te_msm.h) for the next call, like setScalarRecordBytes: the caller declares every scalar of
// later MSM calls below 2^b (0 = nothing declared), and the engine runs only the windows that width needs; a scalar that does not fit
// the plan rejects with TE_MSM_ESCALAR, never a wrong result.
napi_value SetScalarBits(napi_env env, napi_callback_info info) {
  size_t argc = 1; napi_value argv[1];
  napi_get_cb_info(env, info, &argc, argv, nullptr, nullptr);
  int32_t b = -1;
  if (argc < 1 || napi_get_value_int32(env, argv[0], &b) != napi_ok || b < 0 || b > 256) {
    napi_throw_type_error(env, nullptr, "setScalarBits(b: 0..256)");
    return nullptr;
  }
  g_proto.reset();
  g_scalar_bits.store(b);
  napi_value u; napi_get_undefined(env, &u); return u;
}

// getStats(): how the promises so far were mapped onto the engine -- tickets submitted from the JavaScript thread / from pool
// threads, lone calls, jobs over bound bases, and the largest number of tickets seen in flight at a submit
napi_value GetStats(napi_env env, napi_callback_info) {
  const te_promise::stats_t st = g_proto.stats();
  napi_value o; napi_create_object(env, &o);
  const struct { const char* k; double v; } f[] = {{"submittedInEnter", (double)st.submitted_in_enter}, {"submittedInExecute", (double)st.submitted_in_execute},
                                                    {"loneRuns", (double)st.lone_runs}, {"boundJobs", (double)st.bound_jobs}, {"maxInFlight", (double)st.max_in_flight}};
  for (const auto& e : f) { napi_value v; napi_create_double(env, e.v, &v); napi_set_named_property(env, o, e.k, v); }
  return o;
}

// getDevices(): the device list the next context is (or the current one was) created with
napi_value GetDevices(napi_env env, napi_callback_info) {
  const std::vector<int> ids = g_proto.devices();
  napi_value arr; napi_create_array_with_length(env, ids.size(), &arr);
  for (size_t i = 0; i < ids.size(); i++) { napi_value v; napi_create_int32(env, ids[i], &v); napi_set_element(env, arr, (uint32_t)i, v); }
  return arr;
}

napi_value Init(napi_env env, napi_value exports) {
  const struct { const char* name; napi_callback fn; } fns[] = {
      {"msmNative", MsmNative}, {"resetContext", ResetContext}, {"setDevices", SetDevices}, {"getDevices", GetDevices},
      {"setBases", SetBases}, {"getStats", GetStats}, {"setCheckPoints", SetCheckPoints}, {"setScalarsMontgomery", SetScalarsMontgomery},
      {"setScalarRecordBytes", SetScalarRecordBytes}, {"setScalarBits", SetScalarBits},
      {"pointsFromX", PointsFromX}, {"scalarMul", ScalarMul}, {"scalarMulX", ScalarMulX}, {"msmBatch", MsmBatch}, {"msmIndexed", MsmIndexed},
      {"setBase", SetBase}, {"scalarMulBase", ScalarMulBase},
      {"groupAdd", GroupAdd}, {"groupAddX", GroupAddX}, {"groupSum", GroupSum}, {"groupSumX", GroupSumX},
      {"fieldOp", FieldOp},
      {"ntt", Ntt},
      {"polyDivide", PolyDivide},
      {"fieldScan", FieldScan},
      {"bindMatrix", BindMatrix}, {"spmv", Spmv}, {"releaseMatrix", ReleaseMatrix}};
  for (const auto& f : fns) {
    napi_value v;
    napi_create_function(env, f.name, NAPI_AUTO_LENGTH, f.fn, nullptr, &v);
    napi_set_named_property(env, exports, f.name, v);
  }
  return exports;
}

}  // namespace

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
