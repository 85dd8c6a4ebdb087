"""ctypes binding of include/te_msm.h.

Mirrors the reference's operator for this path -- `compute_msm(bufferPoints, bufferScalars, log_result,
force_recompile) -> {x, y}` (submission/submission.ts:73-78) -- with the same argument meaning and
error behaviour (errors raise; the reference rejects its promise).
"""
from __future__ import annotations

import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
PARTIAL_BYTES = 720                     # TE_MSM_PARTIAL_BYTES: one window's row, Twisted-Edwards BLS12
PARTIAL_BYTES_BLS12_377 = 1120          # TE_MSM_PARTIAL_BYTES_BLS12_377
CURVE_TE_BLS12, CURVE_BLS12_377_G1 = 0, 1        # option "curve" (TE_MSM_CURVE_*)
WORKSETS = 8            # TE_MSM_WORKSETS: MSMs one context can have in flight
MAX_BATCH = 8           # TE_MSM_MAX_BATCH: MSMs one te_msm_partial_device_batch call takes
BATCH_SEQ_MAX = 64      # TE_MSM_BATCH_SEQ_MAX: MSMs one shared launch sequence of te_msm_run_scalars_batch holds
EPOINT = -5             # TE_MSM_EPOINT: an input point failed the check of option "check_points"
# why a point failed (TE_MSM_POINT_*): MsmError.reason, the second item of MsmContext.check_points' answer
POINT_NONCANONICAL, POINT_OFF_CURVE, POINT_NOT_IN_SUBGROUP = 1, 2, 3
X_BYTES, X_BYTES_BLS12_377 = 32, 48      # TE_MSM_X_BYTES*: one x-only point (points_from_x, bind_points_x, run_x)
ADD_SUBTRACT, ADD_SHARED_B = 1, 2        # TE_MSM_ADD_*: flags of te_msm_add*
EFIELD = -6             # TE_MSM_EFIELD: a field element has no result (field_op*): MsmError.index / .reason
FIELD_P, FIELD_Q377 = 0, 1               # TE_MSM_FIELD_P / _Q377: 32-byte elements mod p (Aleo `field`, BLS12-377 Fr), 48-byte elements mod q
FIELD_ADD, FIELD_SUB, FIELD_MUL, FIELD_DOUBLE, FIELD_NEG, FIELD_SQUARE, FIELD_INV, FIELD_POW, FIELD_SQRT = range(9)     # TE_MSM_FIELD_<op>
FIELD_SHARED_B, FIELD_MONTGOMERY, FIELD_ZERO_OK = 1, 2, 4      # flags of te_msm_field_op*
NTT_INVERSE, NTT_MONTGOMERY = 1, 2                              # flags of te_msm_ntt*
NTT_MAX_LOG_N = 24
POLY_MONTGOMERY, POLY_SHARED_Z = 1, 2                            # flags of te_msm_poly_divide*
POLY_MAX_N = 1 << 30
SCAN_SUM, SCAN_PRODUCT = 0, 1                                    # ops of te_msm_field_scan*
SCAN_MONTGOMERY, SCAN_EXCLUSIVE, SCAN_SHARED_A = 1, 2, 4         # ... and its flags
SCAN_MAX_N = 1 << 30
MATRIX_MONTGOMERY, MATRIX_TRANSPOSE = 1, 2                        # flags of te_msm_bind_matrix
SPMV_MONTGOMERY, SPMV_TRANSPOSE = 1, 2                            # flags of te_msm_spmv*
FIELD_ZERO, FIELD_NOT_SQUARE = 1, 2      # why an element has no result (MsmError.reason)


class MsmError(RuntimeError):
    """code: the TE_MSM_E* value.  index / reason: the lowest failing point and TE_MSM_POINT_* when code is EPOINT, operand: which operand
    held it (0 = a, or the call's one point buffer; 1 = b of add*); index alone: the lowest position of an index outside the bound set
    (run_scalars_indexed*, code -1); index / reason: the lowest failing element and FIELD_ZERO / FIELD_NOT_SQUARE when code is EFIELD
    (field_op*); else None."""

    def __init__(self, code: int, msg: str, index: int | None = None, reason: int | None = None, operand: int | None = None):
        super().__init__(f"te_msm error {code}: {msg}")
        self.code = code
        self.index = index
        self.reason = reason
        self.operand = operand


def library_path() -> str:
    """libtemsm.so next to this file; TE_MSM_LIB names another build of the SAME library (A/B measurements of build variants)."""
    return os.environ.get("TE_MSM_LIB") or os.path.join(_HERE, "libtemsm.so")


def build_library(force: bool = False) -> str:
    """Compiles csrc/ for gfx950 with hipcc (cross-compiles without a GPU).  With TE_MSM_LIB set the named file is used as
    it is -- `make` only ever rebuilds the in-tree library -- and must exist."""
    so = library_path()
    if os.environ.get("TE_MSM_LIB"):
        if not os.path.exists(so):
            raise MsmError(-2, f"TE_MSM_LIB={so} does not exist (the override is never built: it names a finished build)")
        return so
    csrc = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(_HERE, "..", "include", "te_msm.h")]
    stale = (not os.path.exists(so)) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs if os.path.isfile(s))
    if force or stale:
        subprocess.check_call(["make", "-C", csrc, "-s"])
    return so


def _share_hip_runtime_with_torch() -> None:
    """A process must hold ONE HIP runtime: two copies of libamdhip64 (PyTorch wheels bundle their own)
    cannot both open the GPU -- whichever initialises second reports "no ROCm-capable device".  Both copies
    carry the SONAME libamdhip64.so.7, so loading torch's copy first (by path, without importing torch) makes
    libtemsm.so's DT_NEEDED resolve to it, and a later `import torch` finds the same file already mapped.
    Without torch in the environment libtemsm.so simply uses the system ROCm runtime (its RUNPATH)."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def _lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        so = library_path()
        if not os.path.exists(so):
            raise MsmError(-2, f"{so} is missing: build it with __graft_entry__.build() (there is no CPU fallback)")
        _share_hip_runtime_with_torch()
        L = ctypes.CDLL(so)
        vp, u64, ci, cp = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p
        L.te_msm_init.argtypes = [ctypes.POINTER(ci), ci, ctypes.POINTER(vp)]
        L.te_msm_init.restype = ci
        L.te_msm_destroy.argtypes = [vp]
        L.te_msm_destroy.restype = None
        L.te_msm_last_error.argtypes = [vp]
        L.te_msm_last_error.restype = cp
        L.te_msm_run.argtypes = [vp, cp, cp, u64, cp]
        L.te_msm_run.restype = ci
        L.te_msm_run_device.argtypes = [vp, vp, vp, u64, cp]
        L.te_msm_run_device.restype = ci
        L.te_msm_submit_device.argtypes = [vp, vp, vp, u64, ctypes.POINTER(u64)]
        L.te_msm_submit_device.restype = ci
        L.te_msm_collect.argtypes = [vp, u64, cp]
        L.te_msm_collect.restype = ci
        L.te_msm_submit.argtypes = [vp, cp, cp, u64, ctypes.POINTER(u64)]
        L.te_msm_submit.restype = ci
        L.te_msm_ticket_wait.argtypes = [vp, u64]
        L.te_msm_ticket_wait.restype = ci
        L.te_msm_submit_async.argtypes = [vp, cp, cp, u64, ctypes.POINTER(u64)]
        L.te_msm_submit_async.restype = ci
        L.te_msm_ticket_device.argtypes = [vp, u64, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.te_msm_ticket_device.restype = ci
        L.te_msm_bind_points.argtypes = [vp, cp, u64, ctypes.POINTER(vp)]
        L.te_msm_bind_points.restype = ci
        L.te_msm_bind_points_device.argtypes = [vp, vp, u64, ctypes.POINTER(vp)]
        L.te_msm_bind_points_device.restype = ci
        L.te_msm_release_points.argtypes = [vp, vp]
        L.te_msm_release_points.restype = ci
        L.te_msm_bases_count.argtypes = [vp]
        L.te_msm_bases_count.restype = u64
        L.te_msm_run_scalars.argtypes = [vp, vp, cp, cp]
        L.te_msm_run_scalars.restype = ci
        L.te_msm_run_scalars_device.argtypes = [vp, vp, vp, cp]
        L.te_msm_run_scalars_device.restype = ci
        L.te_msm_run_scalars_batch.argtypes = [vp, vp, ci, ctypes.POINTER(u64), cp, cp]
        L.te_msm_run_scalars_batch.restype = ci
        L.te_msm_run_scalars_batch_device.argtypes = [vp, vp, ci, ctypes.POINTER(u64), vp, cp]
        L.te_msm_run_scalars_batch_device.restype = ci
        L.te_msm_submit_scalars.argtypes = [vp, vp, cp, ctypes.POINTER(u64)]
        L.te_msm_submit_scalars.restype = ci
        L.te_msm_submit_scalars_device.argtypes = [vp, vp, vp, ctypes.POINTER(u64)]
        L.te_msm_submit_scalars_device.restype = ci
        L.te_msm_run_scalars_indexed.argtypes = [vp, vp, vp, cp, u64, cp]
        L.te_msm_run_scalars_indexed.restype = ci
        L.te_msm_run_scalars_indexed_device.argtypes = [vp, vp, vp, vp, u64, cp]
        L.te_msm_run_scalars_indexed_device.restype = ci
        L.te_msm_submit_scalars_indexed.argtypes = [vp, vp, vp, cp, u64, ctypes.POINTER(u64)]
        L.te_msm_submit_scalars_indexed.restype = ci
        L.te_msm_submit_scalars_indexed_device.argtypes = [vp, vp, vp, vp, u64, ctypes.POINTER(u64)]
        L.te_msm_submit_scalars_indexed_device.restype = ci
        L.te_msm_bases_read.argtypes = [vp, vp, ci, u64, u64, vp, u64, ctypes.POINTER(ci)]
        L.te_msm_bases_read.restype = ctypes.c_int64
        L.te_msm_probe_queues.argtypes = [vp]
        L.te_msm_probe_queues.restype = ci
        L.te_msm_trim.argtypes = [vp, ci]
        L.te_msm_trim.restype = ci
        L.te_msm_set_option.argtypes = [vp, cp, ctypes.c_int64]
        L.te_msm_set_option.restype = ci
        L.te_msm_get_option.argtypes = [vp, cp, ctypes.POINTER(ctypes.c_int64)]
        L.te_msm_get_option.restype = ci
        L.te_msm_set_window_shard.argtypes = [vp, ci, ci]
        L.te_msm_set_window_shard.restype = ci
        L.te_msm_plan.argtypes = [vp, u64, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.te_msm_plan.restype = ci
        L.te_msm_partial_device.argtypes = [vp, vp, vp, u64, vp, vp]
        L.te_msm_partial_device.restype = ci
        L.te_msm_partial_device_batch.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), u64, ci, vp, vp]
        L.te_msm_partial_device_batch.restype = ci
        L.te_msm_workset_stream.argtypes = [vp, ci, ctypes.POINTER(vp), ctypes.POINTER(ci)]
        L.te_msm_workset_stream.restype = ci
        L.te_msm_partial_wait.argtypes = [vp, ci]
        L.te_msm_partial_wait.restype = ci
        L.te_msm_finalize.argtypes = [vp, cp, ci, ci, cp]
        L.te_msm_finalize.restype = ci
        L.te_msm_finalize_host.argtypes = [cp, ci, ci, cp]
        L.te_msm_finalize_host.restype = ci
        L.te_msm_host_tail_features.argtypes = []
        L.te_msm_host_tail_features.restype = ci
        L.te_msm_finalize_host_ex.argtypes = [cp, ci, ci, ci, cp]
        L.te_msm_finalize_host_ex.restype = ci
        L.te_msm_finalize_gathered.argtypes = [vp, ci, ci, ci, ci, cp]
        L.te_msm_finalize_gathered.restype = ci
        L.te_msm_finalize_host_curve.argtypes = [ci, cp, ci, ci, ci, cp]
        L.te_msm_finalize_host_curve.restype = ci
        L.te_msm_finalize_gathered_curve.argtypes = [ci, vp, ci, ci, ci, ci, cp]
        L.te_msm_finalize_gathered_curve.restype = ci
        L.te_msm_finalize_sum_curve.argtypes = [ci, ctypes.POINTER(cp), ci, ci, ci, ci, cp]
        L.te_msm_finalize_sum_curve.restype = ci
        L.te_msm_synth_inputs.argtypes = [u64, u64, ci, vp, vp]
        L.te_msm_synth_inputs.restype = ci
        L.te_msm_synth_inputs_bls12_377.argtypes = [u64, u64, vp, vp]
        L.te_msm_synth_inputs_bls12_377.restype = ci
        L.te_msm_stage_ms.argtypes = [vp, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(cp), ci]
        L.te_msm_stage_ms.restype = ci
        L.te_msm_debug_read.argtypes = [vp, cp, vp, u64]
        L.te_msm_debug_read.restype = ctypes.c_int64
        L.te_msm_check_points.argtypes = [vp, cp, u64, ci, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ci)]
        L.te_msm_check_points.restype = ci
        L.te_msm_check_points_device.argtypes = [vp, vp, u64, ci, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ci)]
        L.te_msm_check_points_device.restype = ci
        L.te_msm_points_from_x.argtypes = [vp, cp, u64, cp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ci)]
        L.te_msm_points_from_x.restype = ci
        L.te_msm_points_from_x_device.argtypes = [vp, vp, u64, vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ci)]
        L.te_msm_points_from_x_device.restype = ci
        L.te_msm_bind_points_x.argtypes = [vp, cp, u64, ctypes.POINTER(vp)]
        L.te_msm_bind_points_x.restype = ci
        L.te_msm_run_x.argtypes = [vp, cp, cp, u64, cp]
        L.te_msm_run_x.restype = ci
        L.te_msm_mul.argtypes = [vp, cp, cp, u64, ci, cp]
        L.te_msm_mul.restype = ci
        L.te_msm_mul_device.argtypes = [vp, vp, vp, u64, ci, vp]
        L.te_msm_mul_device.restype = ci
        L.te_msm_mul_x.argtypes = [vp, cp, cp, u64, ci, cp]
        L.te_msm_mul_x.restype = ci
        # (a library TE_MSM_LIB names for an A/B against an OLDER build -- tools/mul_base_cost.py --parent-lib -- has no fixed-base entry
        # points: there they stay undeclared and MsmContext.bind_base raises AttributeError; the in-tree library must have them)
        if not os.environ.get("TE_MSM_LIB") or hasattr(L, "te_msm_bind_base"):
            L.te_msm_bind_base.argtypes = [vp, cp, ctypes.POINTER(vp)]
            L.te_msm_bind_base.restype = ci
            L.te_msm_release_base.argtypes = [vp, vp]
            L.te_msm_release_base.restype = ci
            L.te_msm_mul_base.argtypes = [vp, vp, cp, u64, cp]
            L.te_msm_mul_base.restype = ci
            L.te_msm_mul_base_device.argtypes = [vp, vp, vp, u64, vp]
            L.te_msm_mul_base_device.restype = ci
            L.te_msm_base_read.argtypes = [vp, vp, ci, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, vp, u64, ctypes.POINTER(ci)]
            L.te_msm_base_read.restype = ctypes.c_int64
        # (likewise for an older build named by TE_MSM_LIB: tools/group_add_cost.py times the parent's MSM beside te_msm_sum_device)
        if not os.environ.get("TE_MSM_LIB") or hasattr(L, "te_msm_add"):
            L.te_msm_add.argtypes = [vp, vp, vp, u64, ci, vp]
            L.te_msm_add.restype = ci
            L.te_msm_add_device.argtypes = [vp, vp, vp, u64, ci, vp]
            L.te_msm_add_device.restype = ci
            L.te_msm_add_x.argtypes = [vp, cp, cp, u64, ci, cp]
            L.te_msm_add_x.restype = ci
            L.te_msm_sum.argtypes = [vp, cp, u64, cp]
            L.te_msm_sum.restype = ci
            L.te_msm_sum_device.argtypes = [vp, vp, u64, cp]
            L.te_msm_sum_device.restype = ci
            L.te_msm_sum_x.argtypes = [vp, cp, u64, cp]
            L.te_msm_sum_x.restype = ci
        if not os.environ.get("TE_MSM_LIB") or hasattr(L, "te_msm_field_op"):
            L.te_msm_field_op.argtypes = [vp, ci, ci, vp, vp, u64, ci, vp]
            L.te_msm_field_op.restype = ci
            L.te_msm_field_op_device.argtypes = [vp, ci, ci, vp, vp, u64, ci, vp]
            L.te_msm_field_op_device.restype = ci
        if not os.environ.get("TE_MSM_LIB") or hasattr(L, "te_msm_ntt"):
            L.te_msm_ntt.argtypes = [vp, vp, ctypes.c_uint32, u64, ci, vp, vp]
            L.te_msm_ntt.restype = ci
            L.te_msm_ntt_device.argtypes = [vp, vp, ctypes.c_uint32, u64, ci, vp, vp]
            L.te_msm_ntt_device.restype = ci
        if not os.environ.get("TE_MSM_LIB") or hasattr(L, "te_msm_poly_divide"):
            L.te_msm_poly_divide.argtypes = [vp, vp, u64, u64, vp, ci, vp, vp]
            L.te_msm_poly_divide.restype = ci
            L.te_msm_poly_divide_device.argtypes = [vp, vp, u64, u64, vp, ci, vp, vp]
            L.te_msm_poly_divide_device.restype = ci
        if not os.environ.get("TE_MSM_LIB") or hasattr(L, "te_msm_bind_matrix"):
            L.te_msm_bind_matrix.argtypes = [vp, u64, u64, vp, vp, vp, ci, ctypes.POINTER(vp)]
            L.te_msm_bind_matrix.restype = ci
            L.te_msm_release_matrix.argtypes = [vp, vp]
            L.te_msm_release_matrix.restype = ci
            L.te_msm_matrix_shape.argtypes = [vp, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u64)]
            L.te_msm_matrix_shape.restype = ci
            L.te_msm_spmv.argtypes = [vp, vp, vp, u64, ci, vp]
            L.te_msm_spmv.restype = ci
            L.te_msm_spmv_device.argtypes = [vp, vp, vp, u64, ci, vp]
            L.te_msm_spmv_device.restype = ci
        if not os.environ.get("TE_MSM_LIB") or hasattr(L, "te_msm_field_scan"):
            L.te_msm_field_scan.argtypes = [vp, ci, vp, u64, u64, ci, vp, vp, vp]
            L.te_msm_field_scan.restype = ci
            L.te_msm_field_scan_device.argtypes = [vp, ci, vp, u64, u64, ci, vp, vp, vp]
            L.te_msm_field_scan_device.restype = ci
        _LIB = L
    return _LIB


class MsmContext:
    """Persistent engine context (device buffers, stream) -- te_msm_init / te_msm_destroy."""

    def __init__(self, device_ids=(0,)):
        L = _lib()
        ids = (ctypes.c_int * len(device_ids))(*device_ids)
        h = ctypes.c_void_p()
        rc = L.te_msm_init(ids, len(device_ids), ctypes.byref(h))
        if rc:
            raise MsmError(rc, L.te_msm_last_error(None).decode())
        self._h = h
        self._L = L
        self._sizes = (64, 32, 64)          # point, scalar, result bytes of the selected curve and scalar record (_resize)
        self.curve = CURVE_TE_BLS12
        self._scalar_record_bytes = 0       # option "scalar_record_bytes" as set_option left it (0 = the curve's own record; 8 / 16: narrow scalars)
        self._point_stride = 0              # option "point_stride" as set_option left it (0 = packed x || y)
        self._held = {}                     # ticket -> the buffers of an asynchronous submit (alive until collected)

    def close(self):
        if getattr(self, "_h", None):
            self._L.te_msm_destroy(self._h)        # (finishes the uploads of asynchronous tickets that were never collected)
            self._h = None
            self._held.clear()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int):
        if rc < 0:
            msg = self._L.te_msm_last_error(self._h).decode()
            if rc == EPOINT:
                raise MsmError(rc, msg, self.get_option("bad_point_index"), self.get_option("bad_point_reason"), self._bad_operand())
            if rc == EFIELD:
                raise MsmError(rc, msg, self.get_option("bad_field_index"), self.get_option("bad_field_reason"))
            if rc == -1 and msg.startswith("index at position "):       # an indexed MSM (a call, or the collect of its ticket)
                raise MsmError(rc, msg, self.get_option("bad_index_position"))
            raise MsmError(rc, msg)
        return rc

    def _bad_operand(self):
        """option "bad_point_operand" (None from a build without it: TE_MSM_LIB naming an older library)"""
        v = ctypes.c_int64()
        return v.value if self._L.te_msm_get_option(self._h, b"bad_point_operand", ctypes.byref(v)) == 0 else None

    # ---- input-point validation (include/te_msm.h: option "check_points" makes the calls below check; these run no MSM)
    def _verdict(self, rc: int, bad, why):
        if rc == EPOINT:
            return bad.value, why.value
        self._check(rc)
        return None

    def check_points(self, points: bytes, level: int = 1):
        """te_msm_check_points: None when every point passes, else (lowest failing index, POINT_* reason).  level 1: canonical
        and on the curve; 2: also in the prime-order subgroup (costly: meant for a point set that is used many times)."""
        pb = self._point_stride or self._sizes[0]         # option "point_stride" while it is set: n follows the stride
        if len(points) % pb:
            raise MsmError(-1, f"points must be {pb}*n bytes")
        bad, why = ctypes.c_int64(), ctypes.c_int()
        rc = self._L.te_msm_check_points(self._h, bytes(points), len(points) // pb, int(level), ctypes.byref(bad), ctypes.byref(why))
        return self._verdict(rc, bad, why)

    def check_points_device(self, d_points: int, n: int, level: int = 1):
        """te_msm_check_points_device: the same for n points in the memory of a device of the context"""
        bad, why = ctypes.c_int64(), ctypes.c_int()
        rc = self._L.te_msm_check_points_device(self._h, d_points, n, int(level), ctypes.byref(bad), ctypes.byref(why))
        return self._verdict(rc, bad, why)

    # ---- options
    def set_option(self, key: str, value: int):
        self._check(self._L.te_msm_set_option(self._h, key.encode(), int(value)))
        if key == "curve":
            self.curve = int(value)
        elif key == "scalar_record_bytes":
            self._scalar_record_bytes = int(value)
        elif key == "point_stride":
            self._point_stride = int(value)
        self._resize()

    def _resize(self):
        """_sizes is the one place that knows the byte sizes: the scalar record is option "scalar_record_bytes" where it is set (32 on
        BLS12-377: a native prover's records; 8 / 16 on either curve: a native u64 / u128 array, whose width stands for option "scalar_bits"),
        else the curve's own.  (48 on the Twisted-Edwards curve: the engine refuses the call.)"""
        pb, sb, rb = (96, 48, 96) if self.curve == CURVE_BLS12_377_G1 else (64, 32, 64)
        self._sizes = (pb, self._scalar_record_bytes or sb, rb)

    @property
    def row_bytes(self) -> int:
        """bytes of one window's partial row under the selected curve"""
        return partial_bytes(self.curve)

    def get_option(self, key: str) -> int:
        v = ctypes.c_int64()
        self._check(self._L.te_msm_get_option(self._h, key.encode(), ctypes.byref(v)))
        return v.value

    def set_window_shard(self, first: int, step: int):
        self._check(self._L.te_msm_set_window_shard(self._h, first, step))

    def plan(self, n: int):
        c, w = ctypes.c_int(), ctypes.c_int()
        self._check(self._L.te_msm_plan(self._h, n, ctypes.byref(c), ctypes.byref(w)))
        return c.value, w.value

    # ---- whole MSM
    def run(self, points: bytes, scalars: bytes) -> bytes:
        """Host buffers in the reference's wire format -> affine result x || y, little-endian (64 bytes; 96 for
        BLS12-377 G1, whose points are 96 and scalar records 48 bytes -- 32 under option "scalar_record_bytes" = 32)."""
        pb, sb, rb = self._sizes
        n = len(scalars) // sb
        if len(scalars) != sb * n or len(points) != pb * n:
            raise MsmError(-1, f"points must be {pb}*n bytes and scalars {sb}*n bytes")
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_run(self._h, bytes(points), bytes(scalars), n, out))
        return out.raw[:rb]

    def run_device(self, d_points: int, d_scalars: int, n: int) -> bytes:
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_run_device(self._h, d_points, d_scalars, n, out))
        return out.raw[:self._sizes[2]]

    # ---- pipelined form: up to WORKSETS MSMs in flight (host tail and device work of consecutive MSMs overlap)
    def submit_device(self, d_points: int, d_scalars: int, n: int) -> int:
        t = ctypes.c_uint64()
        self._check(self._L.te_msm_submit_device(self._h, d_points, d_scalars, n, ctypes.byref(t)))
        return t.value

    def collect(self, ticket: int) -> bytes:
        out = ctypes.create_string_buffer(96)
        try:
            self._check(self._L.te_msm_collect(self._h, ticket, out))
        finally:
            self._held.pop(ticket, None)
        return out.raw[:self._sizes[2]]

    def submit(self, points: bytes, scalars: bytes) -> int:
        """Pipelined form for HOST buffers (te_msm_submit): returns a ticket for collect() once the data has left the
        caller's buffers; the upload of the next MSM overlaps the device work of this one."""
        pb, sb, _ = self._sizes
        n = len(scalars) // sb
        if len(scalars) != sb * n or len(points) != pb * n:
            raise MsmError(-1, f"points must be {pb}*n bytes and scalars {sb}*n bytes")
        t = ctypes.c_uint64()
        self._check(self._L.te_msm_submit(self._h, bytes(points), bytes(scalars), n, ctypes.byref(t)))
        return t.value

    def submit_async(self, points: bytes, scalars: bytes) -> int:
        """te_msm_submit_async: returns at once, the upload runs on the chosen device's host thread (D calls in a row keep D
        PCIe links busy on a context of D devices).  The buffers must stay alive and unchanged until the ticket is collected:
        this object holds references to the two `bytes` objects until then."""
        pb, sb, _ = self._sizes
        n = len(scalars) // sb
        if len(scalars) != sb * n or len(points) != pb * n:
            raise MsmError(-1, f"points must be {pb}*n bytes and scalars {sb}*n bytes")
        points, scalars = bytes(points), bytes(scalars)
        t = ctypes.c_uint64()
        self._check(self._L.te_msm_submit_async(self._h, points, scalars, n, ctypes.byref(t)))
        self._held[t.value] = (points, scalars)
        return t.value

    def ticket_wait(self, ticket: int):
        self._check(self._L.te_msm_ticket_wait(self._h, ticket))

    # ---- resident bases: points bound once, scalars per call (te_msm_bind_points ...)
    def _bind(self, montgomery: bool, call, stride: int = 0, infinity_flag: bool = False) -> ctypes.c_void_p:
        """One bind call.  montgomery=True: option "points_montgomery" (read at bind time) is 1 for that call and put back afterwards.
        False asks for nothing: the option stays as set_option left it, so the keyword can switch the form on for one set but not off
        on a context whose option is 1 -- set_option("points_montgomery", 0) does that.  stride / infinity_flag: options "point_stride"
        and "point_infinity_flag" in the same way."""
        h = ctypes.c_void_p()
        want = [(k, v) for k, v in (("points_montgomery", 1 if montgomery else 0), ("point_stride", int(stride)),
                                    ("point_infinity_flag", 1 if infinity_flag else 0)) if v]
        before = [(k, self.get_option(k)) for k, _ in want]
        try:
            for k, v in want:
                self.set_option(k, v)
            self._check(call(ctypes.byref(h)))
        finally:
            for k, v in before:
                self.set_option(k, v)
        return h

    def bind_points(self, points: bytes, montgomery: bool = False, stride: int = 0, infinity_flag: bool = False) -> "Bases":
        """Uploads the points once, converts them to records on every device of the context and keeps only the records
        (te_msm_bind_points).  The harness hands the same point buffer to compute_msm for every run of a size
        (submission/miscellaneous/full_benchmarks.ts:63-68,100-105).
        montgomery=True: the coordinates are a native prover's Montgomery residues (x * 2^256 mod p in 32 bytes; BLS12-377: x * 2^384
        mod q in 48) -- option "points_montgomery" = 1 for this call; False leaves the option as set_option left it.  The records, and every
        MSM over the set, are the same either way.  (The scalars' counterpart is the option "scalars_montgomery" alone: set_option.)
        stride: point i starts at byte i * stride (a multiple of 8 from the size of x || y up to 128; 0 = as set_option left "point_stride",
        packed by default) -- option "point_stride" for this call.  infinity_flag=True (BLS12-377, stride >= 104): the byte at offset 96 of
        a record flags the point at infinity -- option "point_infinity_flag" for this call.  Together with montgomery=True and stride=104
        the buffer is meant to be arkworks' &[G1Affine]."""
        pb = int(stride) or self._point_stride or self._sizes[0]
        n = len(points) // pb
        if len(points) != pb * n:
            raise MsmError(-1, f"points must be {pb}*n bytes")
        points = bytes(points)
        h = self._bind(montgomery, lambda out: self._L.te_msm_bind_points(self._h, points, n, out), stride, infinity_flag)
        return Bases(self, h, n, self.curve)

    def bind_points_device(self, d_points: int, n: int, montgomery: bool = False, stride: int = 0, infinity_flag: bool = False) -> "Bases":
        """te_msm_bind_points_device; montgomery, stride, infinity_flag: as bind_points (the buffer 8-byte aligned under a stride)"""
        h = self._bind(montgomery, lambda out: self._L.te_msm_bind_points_device(self._h, d_points, n, out), stride, infinity_flag)
        return Bases(self, h, n, self.curve)

    # ---- x-only points (include/te_msm.h "x-only points"): y recovered on the device; a bad x raises MsmError(EPOINT) with .index / .reason
    def _x_count(self, xs) -> int:
        xb = X_BYTES_BLS12_377 if self.curve == CURVE_BLS12_377_G1 else X_BYTES
        n = len(xs) // xb
        if len(xs) != xb * n:
            raise MsmError(-1, f"x-coordinates must be {xb}*n bytes")
        return n

    def points_from_x(self, xs: bytes) -> bytes:
        """te_msm_points_from_x: n x-coordinates (32 bytes; BLS12-377: 48 with the flag bits) -> n points x || y (64 / 96 bytes)"""
        n = self._x_count(xs)
        out = ctypes.create_string_buffer(max(1, self._sizes[0] * n))
        bad, why = ctypes.c_int64(), ctypes.c_int()
        self._check(self._L.te_msm_points_from_x(self._h, bytes(xs), n, out, ctypes.byref(bad), ctypes.byref(why)))
        return out.raw[:self._sizes[0] * n]

    def points_from_x_device(self, d_x: int, n: int, d_out: int):
        """te_msm_points_from_x_device: the same between two buffers on one device of the context"""
        bad, why = ctypes.c_int64(), ctypes.c_int()
        self._check(self._L.te_msm_points_from_x_device(self._h, d_x, n, d_out, ctypes.byref(bad), ctypes.byref(why)))

    def bind_points_x(self, xs: bytes) -> "Bases":
        """te_msm_bind_points_x: recovers the points on the first device and binds them (as bind_points_device)"""
        n = self._x_count(xs)
        h = ctypes.c_void_p()
        self._check(self._L.te_msm_bind_points_x(self._h, bytes(xs), n, ctypes.byref(h)))
        return Bases(self, h, n, self.curve)

    def run_x(self, xs: bytes, scalars: bytes) -> bytes:
        """te_msm_run_x, Address.msm's counterpart: x-only points and scalars -> the affine result x || y (64 / 96 bytes).
        Correct per call, and slower than the MSM itself: bind_points_x is where x-only input belongs."""
        n = self._x_count(xs)
        sb = self._sizes[1]
        if len(scalars) != sb * n:
            raise MsmError(-1, f"scalars must be {sb}*n bytes")
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_run_x(self._h, bytes(xs), bytes(scalars), n, out))
        return out.raw[:self._sizes[2]]

    # ---- batch scalar multiplication (include/te_msm.h): out[i] = [k_i] P_i, no sum
    def _mul_scalars(self, scalars: bytes, n: int) -> bool:
        """True for a shared scalar (one scalar's bytes), False for one scalar per point"""
        sb = self._sizes[1]
        if len(scalars) == sb:
            return True
        if len(scalars) != sb * n:
            raise MsmError(-1, f"scalars must be {sb} bytes (one shared scalar) or {sb}*n bytes")
        return False

    def mul(self, points: bytes, scalars: bytes) -> bytes:
        """te_msm_mul: n points (64 / 96 bytes) and n scalars (32 / 48 bytes), or ONE scalar for all of them -> n points [k_i] P_i,
        canonical affine x || y (the Twisted-Edwards identity as (0, 1), the BLS12-377 point at infinity as 96 zero bytes)"""
        pb = self._sizes[0]
        if len(points) % pb:
            raise MsmError(-1, f"points must be {pb}*n bytes")
        n = len(points) // pb
        shared = self._mul_scalars(scalars, n)
        out = ctypes.create_string_buffer(max(1, pb * n))
        self._check(self._L.te_msm_mul(self._h, bytes(points), bytes(scalars), n, int(shared), out))
        return out.raw[:pb * n]

    def mul_device(self, d_points: int, d_scalars: int, n: int, d_out: int, shared: bool = False):
        """te_msm_mul_device: the same between buffers on one device of the context; shared: d_scalars holds one scalar"""
        self._check(self._L.te_msm_mul_device(self._h, d_points, d_scalars, n, int(bool(shared)), d_out))

    def mul_x(self, xs: bytes, scalars: bytes) -> bytes:
        """te_msm_mul_x, bulkGroupScalarMul's counterpart: n x-only points (32 / 48 bytes, points_from_x's format) and n scalars, or
        one -> n points x || y"""
        n = self._x_count(xs)
        shared = self._mul_scalars(scalars, n)
        out = ctypes.create_string_buffer(max(1, self._sizes[0] * n))
        self._check(self._L.te_msm_mul_x(self._h, bytes(xs), bytes(scalars), n, int(shared), out))
        return out.raw[:self._sizes[0] * n]

    # ---- batched group addition and point-set sums (include/te_msm.h): out[i] = A_i +- B_i; one point, the sum of all P_i
    def _add_flags(self, nb_bytes: int, unit: int, n: int, subtract: bool) -> int:
        """TE_MSM_ADD_*: b of one point (unit bytes) beside n > 1 of a means shared"""
        if nb_bytes == unit * n:
            return ADD_SUBTRACT if subtract else 0
        if nb_bytes != unit:
            raise MsmError(-1, f"b must be {unit} bytes (one shared point) or {unit}*n bytes")
        return ADD_SHARED_B | (ADD_SUBTRACT if subtract else 0)

    def add(self, a: bytes, b: bytes, subtract: bool = False) -> bytes:
        """te_msm_add, bulkAddGroups' counterpart on full points: n points a and n points b (64 / 96 bytes), or ONE point b for all of
        them -> n points A_i + B_i (A_i - B_i with subtract), canonical affine x || y as mul() writes them.  BLS12-377: the all-zero
        record is the point at infinity, in and out."""
        pb = self._sizes[0]
        if len(a) % pb:
            raise MsmError(-1, f"points must be {pb}*n bytes")
        n = len(a) // pb
        flags = self._add_flags(len(b), pb, n, subtract)
        out = ctypes.create_string_buffer(max(1, pb * n))
        self._check(self._L.te_msm_add(self._h, bytes(a), bytes(b), n, flags, out))
        return out.raw[:pb * n]

    def add_device(self, d_a: int, d_b: int, n: int, d_out: int, subtract: bool = False, shared_b: bool = False):
        """te_msm_add_device: the same between buffers on one device of the context; d_out may be d_a or d_b; shared_b: d_b holds one point"""
        flags = (ADD_SUBTRACT if subtract else 0) | (ADD_SHARED_B if shared_b else 0)
        self._check(self._L.te_msm_add_device(self._h, d_a, d_b, n, flags, d_out))

    # ---- batched field arithmetic (include/te_msm.h "batched field arithmetic"): the reference's bulk*Fields
    @staticmethod
    def _field_flags(shared_b: bool, montgomery: bool, zero_ok: bool) -> int:
        return (FIELD_SHARED_B if shared_b else 0) | (FIELD_MONTGOMERY if montgomery else 0) | (FIELD_ZERO_OK if zero_ok else 0)

    def field_op(self, op: int, a: bytes, b: bytes | None = None, *, field: int = FIELD_P, shared_b: bool = False, montgomery: bool = False,
                 zero_ok: bool = False) -> bytes:
        """te_msm_field_op: out[i] = a_i op b_i over n elements of 32 (FIELD_P) or 48 (FIELD_Q377) bytes; b for FIELD_ADD / SUB / MUL / POW
        (an exponent is a 32-byte integer on both fields), one record of it with shared_b.  Inverting 0 without zero_ok and the root of a
        non-square raise MsmError(EFIELD) with .index / .reason."""
        eb = 48 if field == FIELD_Q377 else 32
        if len(a) % eb:
            raise MsmError(-1, f"a must be {eb}*n bytes")
        n = len(a) // eb
        if b is not None:
            bb = 32 if op == FIELD_POW else eb
            if len(b) != (bb if shared_b else bb * n):
                raise MsmError(-1, f"b must be {bb} bytes for every element, or one record of them with shared_b")
        out = ctypes.create_string_buffer(max(1, eb * n))
        self._check(self._L.te_msm_field_op(self._h, field, op, bytes(a), None if b is None else bytes(b), n,
                                            self._field_flags(shared_b, montgomery, zero_ok), out))
        return out.raw[:eb * n]

    def field_op_device(self, op: int, d_a: int, d_b: int | None, n: int, d_out: int, *, field: int = FIELD_P, shared_b: bool = False,
                        montgomery: bool = False, zero_ok: bool = False):
        """te_msm_field_op_device: the same between buffers on one device of the context; d_out may be d_a or d_b; d_b None for the ops of one operand"""
        self._check(self._L.te_msm_field_op_device(self._h, field, op, d_a, d_b, n, self._field_flags(shared_b, montgomery, zero_ok), d_out))

    # ---- batched NTTs over p (include/te_msm.h "batched NTTs"): arkworks' radix-2 domains of BLS12-377's scalar field
    @staticmethod
    def _ntt_args(inverse: bool, montgomery: bool, shift):
        flags = (NTT_INVERSE if inverse else 0) | (NTT_MONTGOMERY if montgomery else 0)
        if shift is None:
            return flags, None
        rec = int(shift).to_bytes(32, "little") if isinstance(shift, int) else bytes(shift)
        if len(rec) != 32:
            raise MsmError(-1, "shift must be one 32-byte record (or an integer below 2^256)")
        return flags, rec

    def ntt(self, a: bytes, log_n: int, *, count: int = 1, inverse: bool = False, montgomery: bool = False, shift=None) -> bytes:
        """te_msm_ntt: `count` transforms of 2^log_n 32-byte elements of p each, natural order in and out; shift: the coset generator s
        (an integer or a 32-byte record; in the Montgomery form with `montgomery`), None for s = 1.  inverse undoes the forward with the same s."""
        if log_n < 0 or count < 0 or len(a) != (32 * count) << min(log_n, 40):
            raise MsmError(-1, "a must be count * 2^log_n * 32 bytes")
        flags, rec = self._ntt_args(inverse, montgomery, shift)
        out = ctypes.create_string_buffer(max(1, len(a)))
        self._check(self._L.te_msm_ntt(self._h, bytes(a), log_n, count, flags, rec, out))
        return out.raw[:len(a)]

    def ntt_device(self, d_a: int, log_n: int, count: int, d_out: int, *, inverse: bool = False, montgomery: bool = False, shift=None):
        """te_msm_ntt_device: the same between buffers on one device of the context; d_out may be d_a.  shift stays a host value"""
        flags, rec = self._ntt_args(inverse, montgomery, shift)
        self._check(self._L.te_msm_ntt_device(self._h, d_a, log_n, count, flags, rec, d_out))

    # ---- polynomial openings (include/te_msm.h "polynomial openings"): a(z) and the quotient by X - z, the witness of a KZG opening
    @staticmethod
    def _poly_args(z, count: int, montgomery: bool, shared_z: bool):
        flags = (POLY_MONTGOMERY if montgomery else 0) | (POLY_SHARED_Z if shared_z else 0)
        if isinstance(z, int):
            z = [z]
        rec = bytes(z) if isinstance(z, (bytes, bytearray, memoryview)) else b"".join(int(v).to_bytes(32, "little") for v in z)
        if len(rec) != 32 * (1 if shared_z else count):
            raise MsmError(-1, "z must be one 32-byte record a polynomial (one in all with shared_z): bytes, or integers below 2^256")
        return flags, rec

    def poly_divide(self, a: bytes, n: int, z, *, count: int = 1, montgomery: bool = False, shared_z: bool = False, quotient: bool = True):
        """te_msm_poly_divide: `count` polynomials of n 32-byte coefficients of p each, lowest first, and their points z (bytes, or integers)
        -> (evals, q): a(z) of each, and the coefficients of (a(X) - a(z)) / (X - z) at the stride n (the last one 0); q is None without
        `quotient` (the call then only evaluates)."""
        if n < 0 or count < 0 or len(a) != 32 * count * n:
            raise MsmError(-1, "a must be count * n * 32 bytes")
        flags, rec = self._poly_args(z, count, montgomery, shared_z)
        evals = ctypes.create_string_buffer(max(1, 32 * count))
        q = ctypes.create_string_buffer(max(1, len(a))) if quotient else None
        self._check(self._L.te_msm_poly_divide(self._h, bytes(a), n, count, rec, flags, evals, q))
        return evals.raw[:32 * count], q.raw[:len(a)] if quotient else None

    def poly_divide_device(self, d_a: int, n: int, count: int, z, d_q, *, montgomery: bool = False, shared_z: bool = False, evals: bool = True):
        """te_msm_poly_divide_device: the same from a buffer on one device of the context into d_q, which may be d_a, or None to evaluate
        only.  z stays a host value; returns the evaluations (None without `evals`)."""
        flags, rec = self._poly_args(z, count, montgomery, shared_z)
        ev = ctypes.create_string_buffer(max(1, 32 * count)) if evals else None
        self._check(self._L.te_msm_poly_divide_device(self._h, d_a, n, count, rec, flags, ev, d_q))
        return ev.raw[:32 * count] if evals else None

    # ---- sparse matrices (include/te_msm.h "sparse matrices"): a CSR matrix over p bound once, products with many vectors
    def bind_matrix(self, rows: int, cols: int, row_ptr, col_idx, vals, *, montgomery: bool = False, transpose: bool = False) -> "Matrix":
        """te_msm_bind_matrix: row_ptr (rows + 1 offsets) and col_idx as sequences of integers or packed little-endian bytes (8 / 4 bytes
        each), vals as 32-byte records (bytes) or integers below 2^256 (Montgomery residues with `montgomery`).  transpose: keep the
        transpose too, so that spmv(..., transpose=True) may be asked.  Bound on every device of the context."""
        def packed(v, width):
            return bytes(v) if isinstance(v, (bytes, bytearray, memoryview)) else b"".join(int(x).to_bytes(width, "little") for x in v)
        ptr, col, val = packed(row_ptr, 8), packed(col_idx, 4), packed(vals, 32)
        if rows < 0 or cols < 0 or len(ptr) != 8 * (rows + 1):
            raise MsmError(-1, "row_ptr must hold rows + 1 offsets")
        nnz = int.from_bytes(ptr[-8:], "little")
        if len(col) < 4 * nnz or len(val) < 32 * nnz:
            raise MsmError(-1, "col_idx and vals must hold row_ptr[rows] entries")
        flags = (MATRIX_MONTGOMERY if montgomery else 0) | (MATRIX_TRANSPOSE if transpose else 0)
        h = ctypes.c_void_p()
        self._check(self._L.te_msm_bind_matrix(self._h, rows, cols, ptr, col or None, val or None, flags, ctypes.byref(h)))
        return Matrix(self, h, rows, cols, nnz, transpose)

    def release_matrix(self, matrix: "Matrix"):
        self._check(self._L.te_msm_release_matrix(self._h, matrix._h))
        matrix._h = None

    def spmv(self, matrix: "Matrix", x: bytes, *, count: int = 1, montgomery: bool = False, transpose: bool = False) -> bytes:
        """te_msm_spmv: `count` vectors of cols 32-byte records each (rows with `transpose`) -> count x rows records (count x cols):
        out[k rows + r] = sum over the entries of row r of vals[e] x[k cols + col_idx[e]] mod p, canonical"""
        n_in, n_out = (matrix.rows, matrix.cols) if transpose else (matrix.cols, matrix.rows)
        if count < 0 or len(x) != 32 * count * n_in:
            raise MsmError(-1, "x must be count * cols * 32 bytes (count * rows with transpose)")
        flags = (SPMV_MONTGOMERY if montgomery else 0) | (SPMV_TRANSPOSE if transpose else 0)
        out = ctypes.create_string_buffer(max(1, 32 * count * n_out))
        self._check(self._L.te_msm_spmv(self._h, matrix._h, bytes(x) or None, count, flags, out))
        return out.raw[:32 * count * n_out]

    def spmv_device(self, matrix: "Matrix", d_x: int, count: int, d_out: int, *, montgomery: bool = False, transpose: bool = False):
        """te_msm_spmv_device: the same between buffers on one device of the context; d_out must not be d_x"""
        flags = (SPMV_MONTGOMERY if montgomery else 0) | (SPMV_TRANSPOSE if transpose else 0)
        self._check(self._L.te_msm_spmv_device(self._h, matrix._h, d_x, count, flags, d_out))

    # ---- prefix sums and products (include/te_msm.h "prefix sums and products"): running sums, grand products, powers of a record
    @staticmethod
    def _scan_args(op: int, count: int, montgomery: bool, exclusive: bool, shared_a: bool, init):
        flags = (SCAN_MONTGOMERY if montgomery else 0) | (SCAN_EXCLUSIVE if exclusive else 0) | (SCAN_SHARED_A if shared_a else 0)
        if init is None:
            return flags, None
        if isinstance(init, int):
            init = [init]
        rec = bytes(init) if isinstance(init, (bytes, bytearray, memoryview)) else b"".join(int(v).to_bytes(32, "little") for v in init)
        if len(rec) != 32 * count:
            raise MsmError(-1, "init must be one 32-byte record a vector: bytes, or integers below 2^256 (None: the identity)")
        return flags, rec

    def field_scan(self, op: int, a: bytes, n: int, *, count: int = 1, init=None, montgomery: bool = False, exclusive: bool = False, shared_a: bool = False,
                   out: bool = True, totals: bool = True):
        """te_msm_field_scan: `count` vectors of n 32-byte records of p each (shared_a: ONE record each) and their seeds (bytes, integers, or
        None for the identity) -> (out, totals): the running sums (SCAN_SUM) or products (SCAN_PRODUCT) from the seed, inclusive or
        exclusive, and seed o a_0 o .. o a_(n-1) of each vector; either is None when it was not asked for."""
        if n < 0 or count < 0 or len(a) != 32 * count * (1 if shared_a else n):
            raise MsmError(-1, "a must be count * n * 32 bytes (count * 32 with shared_a)")
        flags, rec = self._scan_args(op, count, montgomery, exclusive, shared_a, init)
        tot = ctypes.create_string_buffer(max(1, 32 * count)) if totals else None
        o = ctypes.create_string_buffer(max(1, 32 * count * n)) if out else None
        self._check(self._L.te_msm_field_scan(self._h, op, bytes(a), n, count, flags, rec, tot, o))
        return o.raw[:32 * count * n] if out else None, tot.raw[:32 * count] if totals else None

    def field_scan_device(self, op: int, d_a: int, n: int, count: int, d_out, *, init=None, montgomery: bool = False, exclusive: bool = False, shared_a: bool = False,
                          totals: bool = True):
        """te_msm_field_scan_device: the same from a buffer on one device of the context into d_out, which may be d_a (not with shared_a), or
        None for the totals alone.  init stays a host value; returns (d_out, totals) -- totals None when not asked for."""
        flags, rec = self._scan_args(op, count, montgomery, exclusive, shared_a, init)
        tot = ctypes.create_string_buffer(max(1, 32 * count)) if totals else None
        self._check(self._L.te_msm_field_scan_device(self._h, op, d_a, n, count, flags, rec, tot, d_out))
        return d_out, tot.raw[:32 * count] if totals else None

    def add_x(self, ax: bytes, bx: bytes, subtract: bool = False) -> bytes:
        """te_msm_add_x, bulkAddGroups' counterpart: n x-only points a and n (or one) b (32 / 48 bytes, points_from_x's format) -> n points x || y"""
        n = self._x_count(ax)
        xb = X_BYTES_BLS12_377 if self.curve == CURVE_BLS12_377_G1 else X_BYTES
        flags = self._add_flags(len(bx), xb, n, subtract)
        out = ctypes.create_string_buffer(max(1, self._sizes[0] * n))
        self._check(self._L.te_msm_add_x(self._h, bytes(ax), bytes(bx), n, flags, out))
        return out.raw[:self._sizes[0] * n]

    def sum(self, points: bytes) -> bytes:
        """te_msm_sum, reduceGroups' counterpart on full points: n points -> their sum, x || y (64 / 96 bytes; no points: the identity)"""
        pb = self._sizes[0]
        if len(points) % pb:
            raise MsmError(-1, f"points must be {pb}*n bytes")
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_sum(self._h, bytes(points), len(points) // pb, out))
        return out.raw[:self._sizes[2]]

    def sum_device(self, d_points: int, n: int) -> bytes:
        """te_msm_sum_device: the same over n points on one device of the context; the result comes to host memory, as an MSM's"""
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_sum_device(self._h, d_points, n, out))
        return out.raw[:self._sizes[2]]

    def sum_x(self, xs: bytes) -> bytes:
        """te_msm_sum_x, reduceGroups' counterpart: n x-only points -> their sum, x || y"""
        n = self._x_count(xs)
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_sum_x(self._h, bytes(xs), n, out))
        return out.raw[:self._sizes[2]]

    # ---- fixed-base batch scalar multiplication (include/te_msm.h): one point bound, [k_i] P for many scalars
    def bind_base(self, point: bytes) -> "Base":
        """te_msm_bind_base: tabulates one point (64 / 96 bytes, canonical) on every device of the context -- option "mul_base_window"
        (4..12, default 8) as it is now; option "check_points" applies to the point"""
        pb = self._sizes[0]
        if len(point) != pb:
            raise MsmError(-1, f"the point must be {pb} bytes")
        h = ctypes.c_void_p()
        self._check(self._L.te_msm_bind_base(self._h, bytes(point), ctypes.byref(h)))
        return Base(self, h, self.curve, self.get_option("mul_base_window"))

    def release_base(self, base: "Base"):
        self._check(self._L.te_msm_release_base(self._h, base._h))
        base._h = None

    def mul_base(self, base: "Base", scalars: bytes) -> bytes:
        """te_msm_mul_base: n scalar records (32 / 48 bytes; Montgomery residues under option "scalars_montgomery") -> n points [k_i] P,
        canonical affine x || y as mul() writes them"""
        pb, sb = self._sizes[0], self._sizes[1]
        if len(scalars) % sb:
            raise MsmError(-1, f"scalars must be {sb}*n bytes")
        n = len(scalars) // sb
        out = ctypes.create_string_buffer(max(1, pb * n))
        self._check(self._L.te_msm_mul_base(self._h, base._h, bytes(scalars), n, out))
        return out.raw[:pb * n]

    def mul_base_device(self, base: "Base", d_scalars: int, n: int, d_out: int):
        """te_msm_mul_base_device: the same between buffers on one device of the context"""
        self._check(self._L.te_msm_mul_base_device(self._h, base._h, d_scalars, n, d_out))

    def base_read(self, base: "Base", window: int, first: int, count: int, device_index: int = 0):
        """(entry bytes, raw entries [first, first + count) of one window of the table on one device) -- te_msm_base_read"""
        eb = ctypes.c_int(0)
        buf = ctypes.create_string_buffer(max(1, count * 128))
        got = self._check(self._L.te_msm_base_read(self._h, base._h, device_index, window, first, count, buf, count * 128, ctypes.byref(eb)))
        return eb.value, buf.raw[:got]

    def bases_read(self, bases: "Bases", first: int, count: int, device_index: int = 0):
        """(record bytes, raw records [first, first + count) of the bound set on one device) -- te_msm_bases_read"""
        rb = ctypes.c_int(0)
        buf = ctypes.create_string_buffer(max(1, count * 224))
        got = self._check(self._L.te_msm_bases_read(self._h, bases._h, device_index, first, count, buf, count * 224, ctypes.byref(rb)))
        return rb.value, buf.raw[:got]

    def release_points(self, bases: "Bases"):
        self._check(self._L.te_msm_release_points(self._h, bases._h))
        bases._h = None

    def _scalars_of(self, bases: "Bases", scalars: bytes) -> bytes:
        if bases._h is None or bases._ctx is not self:
            raise MsmError(-1, "not a bound point set of this context")
        sb = self._sizes[1]
        if len(scalars) != sb * bases.n:
            raise MsmError(-1, f"scalars must be {sb}*{bases.n} bytes for this point set")
        return bytes(scalars)

    def run_scalars(self, bases: "Bases", scalars: bytes) -> bytes:
        """compute_msm over a bound point set: only the scalars cross PCIe (te_msm_run_scalars)."""
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_run_scalars(self._h, bases._h, self._scalars_of(bases, scalars), out))
        return out.raw[:self._sizes[2]]

    def run_scalars_device(self, bases: "Bases", d_scalars: int) -> bytes:
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_run_scalars_device(self._h, bases._h, d_scalars, out))
        return out.raw[:self._sizes[2]]

    def run_scalars_batch(self, bases: "Bases", scalar_list) -> list:
        """Batched MSMs over prefixes of a bound point set (te_msm_run_scalars_batch): scalar_list holds one scalar buffer per MSM
        (bytes or a numpy array of the curve's scalar records); MSM m runs over the first len(scalar_list[m]) // scalar_bytes points.
        Returns the results in input order."""
        if bases._h is None or bases._ctx is not self:
            raise MsmError(-1, "not a bound point set of this context")
        sb = self._sizes[1]
        bufs = [bytes(memoryview(s).cast("B")) if not isinstance(s, (bytes, bytearray)) else bytes(s) for s in scalar_list]
        for b in bufs:
            if len(b) % sb:
                raise MsmError(-1, f"every scalar buffer must hold whole {sb}-byte records")
        lens = [len(b) // sb for b in bufs]
        return self._run_batch(bases, lens, b"".join(bufs), False)

    def run_scalars_batch_device(self, bases: "Bases", d_scalars: int, lens) -> list:
        """te_msm_run_scalars_batch_device: the packed scalars of all MSMs (MSM m's lens[m] records behind MSM m-1's) in the memory of
        a device of the context."""
        if bases._h is None or bases._ctx is not self:
            raise MsmError(-1, "not a bound point set of this context")
        return self._run_batch(bases, [int(x) for x in lens], d_scalars, True)

    def _run_batch(self, bases: "Bases", lens, scalars, device: bool) -> list:
        count, rb = len(lens), self._sizes[2]
        lv = (ctypes.c_uint64 * max(1, count))(*lens)
        out = ctypes.create_string_buffer(max(1, count * rb))
        fn = self._L.te_msm_run_scalars_batch_device if device else self._L.te_msm_run_scalars_batch
        self._check(fn(self._h, bases._h, count, lv, scalars, out))
        return [out.raw[rb * m:rb * (m + 1)] for m in range(count)]

    # ---- MSMs over an indexed subset of a bound point set: sum_j k_j P_{idx[j]} (include/te_msm.h)
    def _pairs_of(self, bases: "Bases", indices, scalars):
        """(the index list as a contiguous <u4 numpy array, the scalars as bytes, m)"""
        import numpy as np
        if bases._h is None or bases._ctx is not self:
            raise MsmError(-1, "not a bound point set of this context")
        if isinstance(indices, (bytes, bytearray, memoryview)):
            raw = bytes(indices)
            if len(raw) % 4:
                raise MsmError(-1, "indices given as bytes must hold whole little-endian u32 values")
            idx = np.frombuffer(raw, dtype="<u4")
        else:
            a = np.asarray(indices)
            if a.dtype != np.dtype("<u4"):          # (a <u4 array is passed as it is: no copy, no pass over it -- the device checks the range)
                if a.size and (a.dtype.kind not in "ui" or int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
                    raise MsmError(-1, "indices must be integers that fit 32 unsigned bits")
                a = a.astype("<u4")
            idx = np.ascontiguousarray(a.reshape(-1))
        sb = self._sizes[1]
        scalars = bytes(scalars) if isinstance(scalars, (bytes, bytearray)) else bytes(memoryview(scalars).cast("B"))
        if len(scalars) != sb * idx.size:
            raise MsmError(-1, f"scalars must be {sb}*{idx.size} bytes for {idx.size} indices")
        return idx, scalars, int(idx.size)

    def run_scalars_indexed(self, bases: "Bases", indices, scalars) -> bytes:
        """te_msm_run_scalars_indexed: sum_j scalars[j] * P[indices[j]] over a bound point set.  indices: anything numpy turns into <u4
        (a list, an array), or bytes of little-endian u32; any order, repeats allowed, each below bases.n -- else MsmError(-1) with
        .index = the lowest offending position.  Only the pairs cross PCIe, and the sort runs over len(indices) entries."""
        idx, scalars, m = self._pairs_of(bases, indices, scalars)
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_run_scalars_indexed(self._h, bases._h, idx.ctypes.data if m else None, scalars if m else None, m, out))
        return out.raw[:self._sizes[2]]

    def run_scalars_indexed_device(self, bases: "Bases", d_indices: int, d_scalars: int, m: int) -> bytes:
        """te_msm_run_scalars_indexed_device: m u32 indices and m scalar records resident on ONE device of the context"""
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_run_scalars_indexed_device(self._h, bases._h, d_indices, d_scalars, m, out))
        return out.raw[:self._sizes[2]]

    def submit_scalars_indexed(self, bases: "Bases", indices, scalars) -> int:
        """te_msm_submit_scalars_indexed: asynchronous ticket (this object holds both buffers until the ticket is collected)"""
        idx, scalars, m = self._pairs_of(bases, indices, scalars)
        t = ctypes.c_uint64()
        self._check(self._L.te_msm_submit_scalars_indexed(self._h, bases._h, idx.ctypes.data if m else None, scalars if m else None, m, ctypes.byref(t)))
        self._held[t.value] = (idx, scalars)
        return t.value

    def submit_scalars_indexed_device(self, bases: "Bases", d_indices: int, d_scalars: int, m: int) -> int:
        t = ctypes.c_uint64()
        self._check(self._L.te_msm_submit_scalars_indexed_device(self._h, bases._h, d_indices, d_scalars, m, ctypes.byref(t)))
        return t.value

    def submit_scalars(self, bases: "Bases", scalars: bytes) -> int:
        """te_msm_submit_scalars: asynchronous ticket over a bound point set (this object holds the scalars until the ticket
        is collected)."""
        scalars = self._scalars_of(bases, scalars)
        t = ctypes.c_uint64()
        self._check(self._L.te_msm_submit_scalars(self._h, bases._h, scalars, ctypes.byref(t)))
        self._held[t.value] = (scalars,)
        return t.value

    def submit_scalars_device(self, bases: "Bases", d_scalars: int) -> int:
        t = ctypes.c_uint64()
        self._check(self._L.te_msm_submit_scalars_device(self._h, bases._h, d_scalars, ctypes.byref(t)))
        return t.value

    def ticket_device(self, ticket: int):
        """(index into the context's device list, HIP device id) a ticket in flight runs on"""
        i, d = ctypes.c_int(-1), ctypes.c_int(-1)
        self._check(self._L.te_msm_ticket_device(self._h, ticket, ctypes.byref(i), ctypes.byref(d)))
        return i.value, d.value

    def probe_queues(self) -> int:
        """Measures the hardware queues of the work sets' streams now (te_msm_probe_queues); number of classes found."""
        return self._check(self._L.te_msm_probe_queues(self._h))

    def trim(self, keep_worksets: int = 0) -> int:
        """Frees the device buffers of idle work sets >= keep_worksets (te_msm_trim); number of sets freed."""
        return self._check(self._L.te_msm_trim(self._h, keep_worksets))

    # ---- window-sharded building blocks
    def partial_device(self, d_points: int, d_scalars: int, n: int, d_partials: int, stream: int = -1):
        """stream: a hipStream_t handle (0 = HIP's default stream, as torch.cuda.current_stream().cuda_stream
        reports for torch's default stream); -1 = the context's private stream (TE_MSM_OWN_STREAM)."""
        self._check(self._L.te_msm_partial_device(self._h, d_points, d_scalars, n, d_partials, ctypes.c_void_p(stream)))

    def partial_device_batch(self, d_points, d_scalars, n: int, d_partials: int, stream: int = -1):
        """len(d_points) MSMs of n points each (device pointers as ints) in one sequence of launches; MSM m's W rows land at
        d_partials + m * W * row_bytes (te_msm_partial_device_batch)."""
        count = len(d_points)
        if count != len(d_scalars) or not 1 <= count <= MAX_BATCH:
            raise MsmError(-1, "batch of %d point buffers and %d scalar buffers (1..%d of each)" % (count, len(d_scalars), MAX_BATCH))
        pv, sv = (ctypes.c_void_p * count)(*d_points), (ctypes.c_void_p * count)(*d_scalars)
        self._check(self._L.te_msm_partial_device_batch(self._h, pv, sv, n, count, d_partials, ctypes.c_void_p(stream)))

    def workset_stream(self, workset: int):
        """(hipStream_t handle as int, measured hardware-queue class or -1) of a work set's private stream
        (te_msm_workset_stream); wrap the handle with torch.cuda.ExternalStream to order torch work behind it.
        The handle stays a valid stream until the process exits (close() parks exported streams instead of destroying them:
        torch's pinned-memory allocator records an event on every stream a pinned block was used on when the block is
        released, which may be after close()); synchronise your own work on it before close()."""
        st, cls = ctypes.c_void_p(), ctypes.c_int(-1)
        self._check(self._L.te_msm_workset_stream(self._h, workset, ctypes.byref(st), ctypes.byref(cls)))
        return int(st.value or 0), int(cls.value)

    def partial_wait(self, workset: int = 0):
        """Blocks until the last partial_device call on that work set is done; raises on a scalar-range error."""
        self._check(self._L.te_msm_partial_wait(self._h, workset))

    def finalize(self, partials: bytes, window_bits: int, num_windows: int) -> bytes:
        out = ctypes.create_string_buffer(96)
        self._check(self._L.te_msm_finalize(self._h, bytes(partials), window_bits, num_windows, out))
        return out.raw[:self._sizes[2]]

    # ---- measurement / stage verification
    def stage_ms(self):
        ms = (ctypes.c_float * 16)()
        names = (ctypes.c_char_p * 16)()
        k = self._check(self._L.te_msm_stage_ms(self._h, ms, names, 16))
        return {names[i].decode(): float(ms[i]) for i in range(k)}

    def debug_read(self, stage: str, nbytes: int) -> bytes:
        buf = ctypes.create_string_buffer(max(nbytes, 1))
        got = self._check(self._L.te_msm_debug_read(self._h, stage.encode(), buf, nbytes))
        return buf.raw[:got]


class Bases:
    """A bound point set of one MsmContext (te_bases): n points as records on every device of the context."""

    def __init__(self, ctx: MsmContext, handle, n: int, curve: int):
        self._ctx, self._h, self.n, self.curve = ctx, handle, n, curve

    def release(self):
        if self._h is not None and getattr(self._ctx, "_h", None):
            self._ctx.release_points(self)
        self._h = None


class Base:
    """A bound point of one MsmContext (te_base): the table of fixed-base scalar multiplication on every device of the context."""

    def __init__(self, ctx: MsmContext, handle, curve: int, window: int):
        self._ctx, self._h, self.curve, self.window = ctx, handle, curve, window

    def release(self):
        if self._h is not None and getattr(self._ctx, "_h", None):
            self._ctx.release_base(self)
        self._h = None


class Matrix:
    """A bound sparse matrix of one MsmContext (te_matrix): its CSR arrays, and its transpose's when asked, on every device of the context."""

    def __init__(self, ctx: MsmContext, handle, rows: int, cols: int, nnz: int, transpose: bool):
        self._ctx, self._h, self.rows, self.cols, self.nnz, self.transpose = ctx, handle, rows, cols, nnz, transpose

    def release(self):
        if self._h is not None and getattr(self._ctx, "_h", None):
            self._ctx.release_matrix(self)
        self._h = None


def partial_bytes(curve: int = CURVE_TE_BLS12) -> int:
    return PARTIAL_BYTES_BLS12_377 if curve == CURVE_BLS12_377_G1 else PARTIAL_BYTES


def host_tail_features() -> int:
    """te_msm_host_tail_features: bit 0 = mulx/adcx field product, bit 1 = AVX-512 IFMA accumulator in the host tail"""
    return int(_lib().te_msm_host_tail_features())


def finalize_host(partials: bytes, window_bits: int, num_windows: int, bucket_bits: int | None = None, curve: int = CURVE_TE_BLS12) -> bytes:
    """Context-free host tail (te_msm_finalize_host_curve): Horner + affine over W rows of 720 bytes (1120 for
    curve = CURVE_BLS12_377_G1).  bucket_bits: window_bits - 1 for signed digits (default), window_bits for unsigned ones."""
    out = ctypes.create_string_buffer(96)
    bb = window_bits - 1 if bucket_bits is None else bucket_bits
    rc = _lib().te_msm_finalize_host_curve(curve, bytes(partials), window_bits, bb, num_windows, out)
    if rc:
        raise MsmError(rc, "te_msm_finalize_host_curve failed")
    return out.raw[:96 if curve == CURVE_BLS12_377_G1 else 64]


def finalize_gathered(gathered_ptr: int, world: int, window_bits: int, num_windows: int, bucket_bits: int | None = None,
                      curve: int = CURVE_TE_BLS12) -> bytes:
    """Host tail over an all-gathered buffer in HOST memory (te_msm_finalize_gathered_curve); gathered_ptr is its address."""
    out = ctypes.create_string_buffer(96)
    bb = window_bits - 1 if bucket_bits is None else bucket_bits
    rc = _lib().te_msm_finalize_gathered_curve(curve, gathered_ptr, world, window_bits, bb, num_windows, out)
    if rc:
        raise MsmError(rc, "te_msm_finalize_gathered_curve failed")
    return out.raw[:96 if curve == CURVE_BLS12_377_G1 else 64]


def finalize_sum(row_sets, window_bits: int, num_windows: int, bucket_bits: int | None = None, curve: int = CURVE_TE_BLS12) -> bytes:
    """Host tail over the SUM of several row buffers (te_msm_finalize_sum_curve): the slices of a point-sharded MSM."""
    out = ctypes.create_string_buffer(96)
    bb = window_bits - 1 if bucket_bits is None else bucket_bits
    arr = (ctypes.c_char_p * len(row_sets))(*[bytes(r) for r in row_sets])
    rc = _lib().te_msm_finalize_sum_curve(curve, arr, len(row_sets), window_bits, bb, num_windows, out)
    if rc:
        raise MsmError(rc, "te_msm_finalize_sum_curve failed")
    return out.raw[:96 if curve == CURVE_BLS12_377_G1 else 64]


def synth_inputs(seed: int, n: int, fixed_point=False, points: bool = True, scalars: bool = True, curve: int = CURVE_TE_BLS12):
    """Seeded harness inputs in compute_msm's wire format (te_msm_synth_inputs): (points 64n bytes, scalars 32n bytes)
    -- 96n / 48n bytes for curve = CURVE_BLS12_377_G1; a part not asked for is None.  Host code only.
    fixed_point: False / "chain" = (a + i*b)*G, True / "fixed" = the harness's one point replicated, "random" = independent
    seeded-random a_i*G (SURVEY 8d set (R))."""
    fixed_point = {"chain": 0, "fixed": 1, "random": 2}.get(fixed_point, fixed_point)
    bls = curve == CURVE_BLS12_377_G1
    pb = ctypes.create_string_buffer((96 if bls else 64) * n) if points else None
    sb = ctypes.create_string_buffer((48 if bls else 32) * n) if scalars else None
    pp = ctypes.cast(pb, ctypes.c_void_p) if pb is not None else None
    sp = ctypes.cast(sb, ctypes.c_void_p) if sb is not None else None
    rc = _lib().te_msm_synth_inputs_bls12_377(seed, n, pp, sp) if bls else _lib().te_msm_synth_inputs(seed, n, int(fixed_point), pp, sp)
    if rc:
        raise MsmError(rc, "te_msm_synth_inputs failed")
    return (pb.raw if pb is not None else None), (sb.raw if sb is not None else None)


_DEFAULT_CTX = None
_DEFAULT_BASES = None           # (the caller's buffer object, Bases) after set_bases()


def devices_from_env(default=(0,)):
    """TE_MSM_DEVICES="0,1,2,3" (or "all"): the GPUs one compute_msm call is sharded over (the N-API addon reads the same
    variable).  Unset: device 0."""
    env = os.environ.get("TE_MSM_DEVICES", "").strip()
    if not env:
        return tuple(default)
    if env == "all":
        import torch
        return tuple(range(max(1, torch.cuda.device_count())))
    return tuple(int(t) for t in env.split(",") if t.strip() != "")


def compute_msm(bufferPoints, bufferScalars, log_result: bool = True, force_recompile: bool = False):
    """Python mirror of `compute_msm` (submission/submission.ts:73-78).

    bufferPoints: n x (x || y), 32-byte little-endian each; bufferScalars: n x 32-byte little-endian.
    Returns {"x": int, "y": int} (the reference resolves to {x: bigint, y: bigint}).  `force_recompile`
    only exists to defeat WGSL pipeline caching (shader_manager.ts:85-92); here it drops the cached context.
    """
    global _DEFAULT_CTX, _DEFAULT_BASES
    if force_recompile and _DEFAULT_CTX is not None:
        _DEFAULT_CTX.close()
        _DEFAULT_CTX = None
        if _DEFAULT_BASES is not None:          # the records went with the context: bind again on the new one
            buf = _DEFAULT_BASES[0]
            _DEFAULT_BASES = None
            set_bases(buf)
    if _DEFAULT_CTX is None:
        _DEFAULT_CTX = MsmContext(devices_from_env())
    if _DEFAULT_BASES is not None and bufferPoints is _DEFAULT_BASES[0] and len(bufferScalars) == 32 * _DEFAULT_BASES[1].n:
        out = _DEFAULT_CTX.run_scalars(_DEFAULT_BASES[1], bytes(bufferScalars))      # the bound buffer itself: scalars only
    else:
        out = _DEFAULT_CTX.run(bytes(bufferPoints), bytes(bufferScalars))
    res = {"x": int.from_bytes(out[:32], "little"), "y": int.from_bytes(out[32:], "little")}
    if log_result:
        print(res)
    return res


def set_bases(bufferPoints):
    """Opt-in beside compute_msm (not part of the reference's interface): binds this point buffer (te_msm_bind_points); later
    compute_msm(bufferPoints, scalars) calls that pass THE SAME buffer object -- identity and length are checked, its contents
    must not change -- upload and decompose the scalars only.  set_bases(None) unbinds.  The reference's harness passes one
    point buffer to six calls per size (submission/miscellaneous/full_benchmarks.ts:63-68,100-105)."""
    global _DEFAULT_CTX, _DEFAULT_BASES
    if _DEFAULT_BASES is not None:
        _DEFAULT_BASES[1].release()
        _DEFAULT_BASES = None
    if bufferPoints is None:
        return
    if _DEFAULT_CTX is None:
        _DEFAULT_CTX = MsmContext(devices_from_env())
    _DEFAULT_BASES = (bufferPoints, _DEFAULT_CTX.bind_points(bytes(bufferPoints)))
