"""Shared by tests/test_group_add_host.py and tests/test_gpu_group_add.py: the host shim of csrc/group_add.hip.hpp
(tests/csrc/groupaddcheck.cpp), the bigint models of te_msm_add* / te_msm_sum* on wire bytes, and the edge operands."""
import ctypes
import os
import subprocess

from oracle import model as m
from oracle import model377 as b
from oracle import oracle, oracle377

import test_scalar_mul_host as smh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUBTRACT, SHARED_B = 1, 2                       # TE_MSM_ADD_*
M_NO_NEGATE = 4                                 # the shim's deliberate mistake


def shim():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libgroupaddcheck.so"), os.path.join(d, "groupaddcheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("group_add.hip.hpp", "scalar_mul.hip.hpp", "from_x.hip.hpp", "check.hip.hpp", "fp.hpp", "fq377.hpp",
                                                         "field.hpp", "curve.hpp", "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    ci, cp, u64, u32 = ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32
    L.ga_add_points.argtypes = [ci, cp, cp, u64, ci, ci, cp]
    L.ga_sum_points.argtypes = [ci, cp, u64, u32, cp]
    L.ga_add_x_te.argtypes = [cp, cp, ci, cp]
    L.ga_check.argtypes = [ci, cp, ctypes.POINTER(ci)]
    return L


def point_bytes(curve):
    return 96 if curve == 1 else 64


def records(curve, raw):
    pb = point_bytes(curve)
    return [raw[i:i + pb] for i in range(0, len(raw), pb)]


# ---- the models, on wire records -------------------------------------------------------------------------------------------------
def decode(curve, rec):
    if curve == 1:
        return b.INF if rec == bytes(96) else b.xy_from_bytes(rec)
    return m.xy_from_bytes(rec)


def encode(curve, pt):
    return b.result_to_bytes(pt) if curve == 1 else m.points_to_bytes([pt])


def model_add(curve, ra, rb, subtract=False):
    mod = b if curve == 1 else m
    q = decode(curve, rb)
    return encode(curve, mod.add(decode(curve, ra), mod.neg(q) if subtract else q))


def model_add_all(curve, a, bb, subtract=False):
    ra, rb = records(curve, a), records(curve, bb)
    if len(rb) == 1:
        rb = rb * len(ra)
    return b"".join(model_add(curve, x, y, subtract) for x, y in zip(ra, rb))


def model_sum(curve, raw):
    mod = b if curve == 1 else m
    acc = b.INF if curve == 1 else (0, 1)
    for r in records(curve, raw):
        acc = mod.add(acc, decode(curve, r))
    return encode(curve, acc)


# ---- the shim's calls ------------------------------------------------------------------------------------------------------------
def shim_add(L, curve, a, bb, flags=0, mistake=0):
    pb = point_bytes(curve)
    n = len(a) // pb
    out = ctypes.create_string_buffer(max(1, pb * n))
    L.ga_add_points(curve, a, bb, n, flags, mistake, out)
    return out.raw[:pb * n]


def shim_sum(L, curve, raw, grid=1024):
    pb = point_bytes(curve)
    out = ctypes.create_string_buffer(pb)
    L.ga_sum_points(curve, raw, len(raw) // pb, grid, out)
    return out.raw[:pb]


# ---- operands --------------------------------------------------------------------------------------------------------------------
def te_points(seed, n):
    return oracle.gen_points(seed, n)


def bls_points(seed, n):
    return oracle377.gen_points(seed, n)


def te_edge_points():
    """every distinct point of te_edge_cases(), inputs and results: subgroup points and their multiples, O, T2, +-T4, G + T2 (order 2 L),
    G + T4 (4 L) and multiples of those"""
    seen = []
    for _, p, _, want in smh.te_edge_cases():
        for r in (p, want):
            if r not in seen:
                seen.append(r)
    return seen


def te_core_points():
    """(name, record): the identity, the points of order 2, 4, 2 L and 4 L, a subgroup point, its negative and another one"""
    sub = records(0, te_points(0xA16, 2))
    named = [("O", (0, 1))] + smh.te_torsion_points()
    out = [(nm, m.points_to_bytes([p])) for nm, p in named]
    return out + [("P", sub[0]), ("-P", m.points_to_bytes([m.neg(m.xy_from_bytes(sub[0]))])), ("Q", sub[1])]


def te_core_pairs():
    pts = te_core_points()
    return [("%s , %s" % (na, nb), ra, rb) for na, ra in pts for nb, rb in pts]


def bls_core_pairs():
    """(name, a, b): G1 points, negatives and the all-zero record (infinity) in either or both operands; P + P and P - P fall out of (P, P) and (P, -P)"""
    raw = records(1, bls_points(0x3E7, 2))
    neg = b.result_to_bytes(b.neg(b.xy_from_bytes(raw[0])))
    pts = [("P", raw[0]), ("-P", neg), ("Q", raw[1]), ("inf", bytes(96))]
    return [("%s , %s" % (na, nb), ra, rb) for na, ra in pts for nb, rb in pts]
