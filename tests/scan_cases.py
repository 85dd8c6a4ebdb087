"""Shared by tests/test_scan_host.py and tests/test_gpu_scan.py: the host shim of csrc/scan.hip.hpp (tests/csrc/scancheck.cpp), the model of
te_msm_field_scan in Python integers -- out[i] = e o a_0 o .. o a_i, or without a_i, and totals = e o a_0 o .. o a_(n-1) -- and the case
lists.  Expected values never come from a kernel of the library."""
import ctypes
import functools
import os
import random
import subprocess

import field_cases as fc
from oracle import model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = m.P
A = 1 << 256
SUM, PRODUCT = 0, 1                                                 # TE_MSM_SCAN_SUM / _PRODUCT
MONTGOMERY, EXCLUSIVE, SHARED_A = 1, 2, 4                            # TE_MSM_SCAN_*
MAX_N = 1 << 30
LANES = 256
CHUNK_MAX = 16
EINVAL = -1
BOUNDS = -100
SCAN_BAD_OP, SCAN_BAD_N, SCAN_BAD_FLAGS, SCAN_NO_OUTPUT, SCAN_TOO_LARGE, SCAN_NULL, SCAN_ALIAS = range(1, 8)
M_CARRY, M_UNSHIFTED, M_NO_SEED, M_SEED_EVERYWHERE, M_ZERO_PAD, M_NO_REDUCE, M_INTERNAL_OUT = range(1, 8)    # the shim's deliberate mistakes
pack, unpack = fc.pack, fc.unpack
OPS = (SUM, PRODUCT)
ALL_FLAGS = tuple(range(8))
FILL = 0xA5


def shim():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libscancheck.so"), os.path.join(d, "scancheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("scan.hip.hpp", "scan_plan.hpp", "plan_arith.hpp", "field_ops.hip.hpp", "scalar_mul.hip.hpp", "from_x.hip.hpp",
                                                         "check.hip.hpp", "fp.hpp", "fq377.hpp", "field.hpp", "curve.hpp", "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    ci, vp, u64, u32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.scan_emulate.argtypes = [ci, vp, u64, u64, ci, u32, ci, vp, vp, vp, ctypes.POINTER(ci)]
    L.scan_emulate.restype = ci
    L.scan_replay.argtypes = [u64, u64, u32, ci, ctypes.POINTER(u64)]
    L.scan_replay.restype = ci
    L.scan_plan_info.argtypes = [u64, u64, u32, ctypes.POINTER(u64)]
    L.scan_chunk_for.argtypes = [u64, u32]
    L.scan_chunk_for.restype = u32
    L.scan_points.argtypes = [ctypes.POINTER(u32)]
    L.scan_constants.argtypes = [ctypes.POINTER(u64)]
    return L


def plan_info(L, n, count=1, chunk=0):
    out = (ctypes.c_uint64 * 16)()
    L.scan_plan_info(n, count, chunk or default_chunk(L), out)
    lv = int(out[0])
    return dict(levels=lv, T=int(out[1]), records=int(out[2]), scratch_bytes=int(out[3]), lds_bytes=int(out[4]),
                n=[int(out[7 + 2 * l]) for l in range(lv)], tiles=[int(out[8 + 2 * l]) for l in range(lv)])


def default_chunk(L):
    out = (ctypes.c_uint64 * 16)()
    L.scan_plan_info(1, 1, 1, out)
    return int(out[5])


def reduction_points(L):
    """where the plan says the sum path reduces: dict(lane_total, prefix, steps[8])"""
    out = (ctypes.c_uint32 * 10)()
    L.scan_points(out)
    return dict(lane_total=bool(out[0]), prefix=bool(out[1]), steps=[bool(out[2 + s]) for s in range(8)])


def emulate(L, op, a, n, count=1, flags=0, chunk=0, init=None, mistake=0, want_out=True, want_totals=True, in_place=False, null_a=False, out_len=None):
    """(rc, out bytes, totals bytes, reason): scan_emulate.  Outputs start as FILL bytes -- or, in_place, out is a itself.  out_len: the bytes
    of the out buffer when 32 * count * n is not what a (refused) call should get"""
    out_len = 32 * count * n if out_len is None else out_len
    src = ctypes.create_string_buffer(bytes(a), max(1, len(a)))
    out = src if in_place else ctypes.create_string_buffer(bytes([FILL]) * max(1, out_len), max(1, out_len))
    tot = ctypes.create_string_buffer(bytes([FILL]) * max(1, 32 * count), max(1, 32 * count))
    seeds = ctypes.create_string_buffer(bytes(init), max(1, len(init))) if init is not None else None
    why = ctypes.c_int()
    rc = L.scan_emulate(op, None if null_a else ctypes.addressof(src), n, count, flags, chunk, mistake, ctypes.addressof(seeds) if seeds is not None else None,
                        ctypes.addressof(tot) if want_totals else None, ctypes.addressof(out) if want_out else None, ctypes.byref(why))
    if seeds is not None:
        assert seeds.raw[:len(init)] == bytes(init)                     # the call does not modify init
    return rc, out.raw[:out_len], tot.raw[:32 * count], why.value


# ---- the model: Python integers ---------------------------------------------------------------------------------------------------
def decode(vals, flags):
    ia = pow(A, -1, P)
    return [v * ia % P for v in vals] if flags & MONTGOMERY else [v % P for v in vals]


def encode(vals, flags):
    return [v * A % P for v in vals] if flags & MONTGOMERY else [v % P for v in vals]


def model(op, a, n, count=1, flags=0, init=None):
    """te_msm_field_scan on wire bytes -> (out bytes, totals bytes)"""
    vals = decode(unpack(a, 32), flags)
    seeds = decode(unpack(init, 32), flags) if init is not None else [op] * count       # the identity: 0 for the sum, 1 for the product
    outs, tots = [], []
    for k in range(count):
        h = seeds[k]
        for i in range(n):
            x = vals[k] if flags & SHARED_A else vals[k * n + i]
            if flags & EXCLUSIVE:
                outs.append(h)
            h = (h * x if op == PRODUCT else h + x) % P
            if not flags & EXCLUSIVE:
                outs.append(h)
        tots.append(h)
    return pack(encode(outs, flags), 32), pack(encode(tots, flags), 32)


# ---- case lists -------------------------------------------------------------------------------------------------------------------
def lengths(T, squares):
    """n = 1, 2, 255, 256, 257, T - 1, T, T + 1, 2 T + 300 and -- squares -- T^2 - 1, T^2, T^2 + 1"""
    v = [1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T + 300]
    if squares:
        v += [T * T - 1, T * T, T * T + 1]
    return sorted(set(x for x in v if x >= 1))


@functools.lru_cache(maxsize=None)
def values(n, seed=0, zero_free=False):
    """n raw 256-bit records: the limb-class extremes of field_cases first (0, 1, p - 1, p, p + 1, 2^256 - 1, limb boundaries, ..), shuffled,
    then random residues and random full-width integers.  zero_free: no record is 0 mod p (a product then tells every position apart)"""
    rnd = random.Random(0x5CA + 1000003 * seed + n)
    ex = list(fc.extremes(fc.FIELD_P))
    rnd.shuffle(ex)
    v = ex[:n]
    while len(v) < n:
        v.append(rnd.randrange(P) if len(v) & 1 else rnd.randrange(1 << 256))
    if zero_free:
        v = [x if x % P else 2 for x in v]
    return pack(v, 32)


def with_record(a, index, value):
    b = bytearray(a)
    b[32 * index:32 * index + 32] = pack([value], 32)
    return bytes(b)


def seeds(count, seed=0):
    rnd = random.Random(0x5EED + 7919 * seed + count)
    return pack([rnd.randrange(1 << 256) for _ in range(count)], 32)


@functools.lru_cache(maxsize=None)
def expected(op, n, count, flags, seed, with_init=True):
    """(a, init, out, totals) of a case, computed once and shared; a product's records are free of zeros (the zero cases place their own)"""
    a = values(count if flags & SHARED_A else n * count, seed, zero_free=op == PRODUCT)
    init = seeds(count, seed) if with_init else None
    out, tot = model(op, a, n, count, flags, init)
    return a, init, out, tot
