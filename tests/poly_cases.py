"""Shared by tests/test_poly_host.py and tests/test_gpu_poly.py: the host shim of csrc/poly.hip.hpp (tests/csrc/polycheck.cpp), the model
of te_msm_poly_divide in Python integers -- the recurrence h_(n-1) = a_(n-1), h_i = a_i + z h_(i+1) -- and the case lists.  Expected
values never come from a kernel of the library."""
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
MONTGOMERY, SHARED_Z = 1, 2                                         # TE_MSM_POLY_*
MAX_N = 1 << 30
LANES = 256
CHUNK_MAX = 16
EINVAL = -1
BOUNDS = -100
POLY_BAD_N, POLY_BAD_FLAGS, POLY_NO_OUTPUT, POLY_TOO_LARGE, POLY_NULL = range(1, 6)
M_CARRY, M_POINT, M_FULL_TILE, M_UNSHIFTED, M_LAST = range(1, 6)    # the shim's deliberate mistakes
pack, unpack = fc.pack, fc.unpack
FORMS = (0, MONTGOMERY)


def shim():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libpolycheck.so"), os.path.join(d, "polycheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("poly.hip.hpp", "poly_plan.hpp", "plan_arith.hpp", "field_ops.hip.hpp", "scalar_mul.hip.hpp", "from_x.hip.hpp",
                                                         "check.hip.hpp", "fp.hpp", "fq377.hpp", "field.hpp", "curve.hpp", "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    ci, vp, u64, u32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.poly_emulate.argtypes = [vp, u64, u64, vp, ci, u32, ci, vp, vp, ctypes.POINTER(ci)]
    L.poly_emulate.restype = ci
    L.poly_replay.argtypes = [u64, u64, u32, ci, ctypes.POINTER(u64)]
    L.poly_replay.restype = ci
    L.poly_plan_info.argtypes = [u64, u64, u32, ci, ctypes.POINTER(u64)]
    L.poly_chunk_for.argtypes = [u64, u32]
    L.poly_chunk_for.restype = u32
    return L


def plan_info(L, n, count=1, chunk=0, shared=False):
    out = (ctypes.c_uint64 * 16)()
    L.poly_plan_info(n, count, chunk or default_chunk(L), int(shared), out)
    lv = int(out[0])
    return dict(levels=lv, T=int(out[1]), records=int(out[2]), scratch_bytes=int(out[3]), lds_bytes=int(out[4]),
                n=[int(out[7 + 2 * l]) for l in range(lv)], tiles=[int(out[8 + 2 * l]) for l in range(lv)])


def default_chunk(L):
    out = (ctypes.c_uint64 * 16)()
    L.poly_plan_info(1, 1, 1, 0, out)
    return int(out[5])


def emulate(L, a, n, z, count=1, flags=0, chunk=0, mistake=0, quotient=True, evals=True, in_place=False, fill=0xA5, null=None):
    """(rc, evals bytes, q bytes, reason): poly_emulate.  Outputs start as `fill` bytes -- or, in_place, q is a itself.  null: "a" / "z" passes
    NULL; quotient / evals False pass NULL for that output"""
    size = max(1, len(a))
    src = ctypes.create_string_buffer(bytes(a), size)
    zb = ctypes.create_string_buffer(bytes(z), max(1, len(z)))
    q = src if in_place else ctypes.create_string_buffer(bytes([fill]) * size, size)
    ev = ctypes.create_string_buffer(bytes([fill]) * max(1, 32 * count), max(1, 32 * count))
    why = ctypes.c_int()
    rc = L.poly_emulate(None if null == "a" else ctypes.addressof(src), n, count, None if null == "z" else ctypes.addressof(zb), flags, chunk, mistake,
                        ctypes.addressof(ev) if evals else None, ctypes.addressof(q) if quotient else None, ctypes.byref(why))
    return rc, ev.raw[:32 * count], q.raw[:len(a)], why.value


# ---- the model: Python integers ---------------------------------------------------------------------------------------------------
def decode(vals, flags):
    ia = pow(A, -1, P)
    return [v * ia % P for v in vals] if flags & MONTGOMERY else [v % P for v in vals]


def encode(vals, flags):
    return [v * A % P for v in vals] if flags & MONTGOMERY else [v % P for v in vals]


def horner(coeffs, z):
    """(a(z), [q_0 .. q_(n-1)]) by the recurrence of the definition; q_(n-1) = 0"""
    n = len(coeffs)
    q, h = [0] * n, 0
    for i in range(n - 1, -1, -1):
        q[i] = h
        h = (coeffs[i] + z * h) % P
    return h, q


def direct(coeffs, z):
    """the same by direct summation: a(z) = sum a_i z^i, q_i = sum_(k > i) a_k z^(k - i - 1)"""
    n = len(coeffs)
    ev = sum(c * pow(z, i, P) for i, c in enumerate(coeffs)) % P
    return ev, [sum(coeffs[k] * pow(z, k - i - 1, P) for k in range(i + 1, n)) % P for i in range(n)]


def model(a, n, z, count=1, flags=0, how=horner):
    """te_msm_poly_divide on wire bytes -> (evals bytes, q bytes)"""
    vals, zs = decode(unpack(a, 32), flags), decode(unpack(z, 32), flags)
    evs, qs = [], []
    for k in range(count):
        ev, q = how(vals[k * n:(k + 1) * n], zs[0] if flags & SHARED_Z else zs[k])
        evs.append(ev)
        qs += q
    return pack(encode(evs, flags), 32), pack(encode(qs, flags), 32)


def closing_check(a, n, z, count, flags, evals, q):
    """q_(i-1) - z q_i = a_i on every element, with q_(-1) = a(z) and q_(n-1) = 0; everything canonical"""
    av, zs, ev, qv = decode(unpack(a, 32), flags), decode(unpack(z, 32), flags), unpack(evals, 32), unpack(q, 32)
    if max(ev + qv) >= P:
        return False
    ev, qv = decode(ev, flags), decode(qv, flags)
    for k in range(count):
        zk, c, w = zs[0] if flags & SHARED_Z else zs[k], av[k * n:(k + 1) * n], qv[k * n:(k + 1) * n]
        if w[n - 1] != 0:
            return False
        prev = ev[k]
        for i in range(n):
            if (prev - zk * w[i] - c[i]) % P:
                return False
            prev = w[i]
    return True


# ---- case lists -------------------------------------------------------------------------------------------------------------------
POINT_EXTREMES = (0, 1, P - 1, P, (1 << 256) - 1)                    # z; a random one joins them in points()


def lengths(T, squares):
    """n = 1, 2, 255, 256, 257, T - 1, T, T + 1, 2 T + 300 and -- squares -- T^2 - 1, T^2, T^2 + 1"""
    v = [1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T + 300]
    if squares:
        v += [T * T - 1, T * T, T * T + 1]
    return sorted(set(v))


@functools.lru_cache(maxsize=None)
def values(n, seed=0):
    """n raw 256-bit coefficients: the limb-class extremes of field_cases first (0, 1, p - 1, p, p + 1, 2^256 - 1, limb boundaries, ..),
    shuffled, then random residues and random full-width integers"""
    rnd = random.Random(0x901 + 1000003 * seed + n)
    ex = list(fc.extremes(fc.FIELD_P))
    rnd.shuffle(ex)
    v = ex[:n]
    while len(v) < n:
        v.append(rnd.randrange(P) if len(v) & 1 else rnd.randrange(1 << 256))
    return pack(v, 32)


def points(count, seed=0, which=None):
    """`count` raw 256-bit points: random, or -- which -- that extreme first"""
    rnd = random.Random(0x2E + 7919 * seed + count)
    v = [rnd.randrange(1 << 256) for _ in range(count)]
    if which is not None:
        v[0] = which
    return pack(v, 32)


@functools.lru_cache(maxsize=None)
def expected(n, count, flags, seed, which=None):
    """(a, z, evals, q) of a case, computed once and shared"""
    a = values(n * count, seed)
    z = points(1 if flags & SHARED_Z else count, seed, which)
    ev, q = model(a, n, z, count, flags)
    return a, z, ev, q
