"""The record conversion of the Twisted-Edwards curve in three products (csrc/curve.hpp pnt_from_affine_raw) and the small-constant
product by d it closes with (csrc/fp.hpp fp_mul_d), compiled for the host by tests/csrc/convcheck.cpp -- the same limb code that
k_prep_points and k_part_scatter_prep run on gfx950 -- against bigints: residue, value bound and limb class."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 1 << 261            # device Montgomery radix: 9 limbs of 29 bits
NL, LB = 9, 29
LM = (1 << LB) - 1


@pytest.fixture(scope="module")
def cc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("convcheck") / "libconvcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "csrc", "convcheck.cpp")])
    L = ctypes.CDLL(so)
    L.cc_kd_q.restype = ctypes.c_uint32
    L.cc_kd_small.restype = ctypes.c_uint32
    L.cc_from_affine.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32)]
    return L


def lim(v):
    """class N: 8 limbs of 29 bits, the rest in the top limb"""
    return (ctypes.c_uint32 * NL)(*([(v >> (LB * i)) & LM for i in range(8)] + [v >> (LB * 8)]))


def val(ls):
    return sum(int(x) << (LB * i) for i, x in enumerate(ls))


def class_n(ls, top_bits):
    return all(int(x) <= LM for x in ls[:8]) and int(ls[8]) < 1 << top_bits


def test_small_constant_d_product(cc, model):
    """fp_mul_d: a * d as  3021 a - q p  with q estimated from a's top 32 bits (the pass of fp_mul_k2d with d * 2^50 = 2d * 2^49): the
    residue, the value bound (below 1.0001 p) and the limb class for random class-N operands below 2^254, for the range product
    outputs live in, and for the operands where 3021 a crosses a multiple of p (where the estimate is tightest)"""
    P, rnd = model.P, random.Random(3021)
    K = model.D
    assert K == 3021 == int(cc.cc_kd_small())
    assert int(cc.cc_kd_q()) == (K << 50) // ((P >> 222) + 1) < 1 << 32
    out = (ctypes.c_uint32 * NL)()

    def check(v):
        cc.cc_mul_d(lim(v), out)
        r = val(out)
        assert r % P == K * v % P, hex(v)
        assert 0 <= r < P + (P >> 13), hex(v)             # below 1.0002 p
        assert class_n(out, 22), hex(v)

    edge = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, (1 << 254) - 1, 1 << 253, (1 << 232) - 1, 1 << 232, (1 << 222) - 1, 1 << 222]
    for q in list(range(1, 12200, 61)) + [3020, 3021, 3022, 6041, 6042, 6043]:
        for d in (-2, -1, 0, 1, 2):                        # 3021 a just below, at and just above q p
            edge.append(max(0, (q * P + K - 1) // K + d))
    for v in edge:
        if v < 1 << 254:
            check(v)
    for _ in range(20000):
        check(rnd.randrange(1 << 254))
    for _ in range(5000):
        check(rnd.randrange(P + P // 8))


def test_record_conversion_in_three_products(cc, model):
    """pnt_from_affine_raw: ((y-x)/2, (y+x)/2, -d x y) in Montgomery form, each field of class N and below 2p (hm, hp < 1.07p, dt
    < 1.0001p), for canonical points, the neutral element and its negative, and non-canonical 256-bit coordinates"""
    P, D, rnd = model.P, model.D, random.Random(377)
    inv2 = pow(2, -1, P)
    out = (ctypes.c_uint32 * 27)()
    top = (1 << 256) - 1
    cases = [(0, 1), (0, P - 1), (1, 0), (P - 1, P - 1), (P, P), (top, top), (0, top), (top, 0), (P - 1, 1), (2 * P, 3 * P + 5)]
    cases += [(rnd.randrange(P), rnd.randrange(P)) for _ in range(4000)]
    cases += [(rnd.randrange(1 << 256), rnd.randrange(1 << 256)) for _ in range(2000)]
    for x, y in cases:
        cc.cc_from_affine(x.to_bytes(32, "little") + y.to_bytes(32, "little"), out)
        f = [out[9 * k:9 * k + 9] for k in range(3)]
        want = ((y - x) * inv2 * R % P, (y + x) * inv2 * R % P, -D * x * y * R % P)
        for k in range(3):
            v = val(f[k])
            assert v % P == want[k], (hex(x), hex(y), k)
            assert class_n(f[k], 24), (hex(x), hex(y), k)
            assert v < 2 * P, (hex(x), hex(y), k)
        assert val(f[0]) < P + P // 14 and val(f[1]) < P + P // 14
        assert val(f[2]) < P + (P >> 13)
