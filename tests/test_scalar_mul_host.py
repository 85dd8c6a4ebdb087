"""Batch scalar multiplication (te_msm_mul*, te_msm_mul_x): the product's per-lane code (csrc/scalar_mul.hip.hpp, compiled for the host
by tests/csrc/scalarmulcheck.cpp -- the functions k_scalar_mul and k_scalar_mul_affine run on gfx950) against the reference's known
answers and the bigint models, for both recodings (per-point signed windows, shared NAF), edge scalars, points outside the subgroup,
and the new names of the C header and the package."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

from oracle import model as m
from oracle import model377 as b
from oracle import oracle, oracle377

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = (1 << 256) - 1


@pytest.fixture(scope="module")
def sm():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libscalarmulcheck.so"), os.path.join(d, "scalarmulcheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("scalar_mul.hip.hpp", "from_x.hip.hpp", "check.hip.hpp", "fp.hpp", "fq377.hpp",
                                                         "field.hpp", "curve.hpp", "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.sm_mul.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_char_p]
    L.sm_naf.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.sm_mul_x_te.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    return L


def mul_te(sm, pts, ks, shared=False):
    """points (list of (x, y)), scalars (list, or one int when shared) -> list of (x, y)"""
    n = len(pts)
    sc = ks.to_bytes(32, "little") if shared else b"".join(k.to_bytes(32, "little") for k in ks)
    out = ctypes.create_string_buffer(max(1, 64 * n))
    sm.sm_mul(0, m.points_to_bytes(pts), sc, n, int(shared), out)
    return [m.xy_from_bytes(out.raw[64 * i:64 * i + 64]) for i in range(n)]


def mul_377(sm, pts, ks, shared=False):
    """points as wire bytes -> result bytes (96 a point; infinity as zeros)"""
    n = len(pts) // 96
    sc = ks.to_bytes(48, "little") if shared else b"".join(k.to_bytes(48, "little") for k in ks)
    out = ctypes.create_string_buffer(max(1, 96 * n))
    sm.sm_mul(1, pts, sc, n, int(shared), out)
    return out.raw[:96 * n]


def te_points(seed, n):
    raw = oracle.gen_points(seed, n)
    return [m.xy_from_bytes(raw[64 * i:64 * i + 64]) for i in range(n)]


def sqrt_minus_one():
    r = m.sqrt_mod_p(m.P - 1)
    assert r * r % m.P == m.P - 1
    return r


EDGE_TE = [0, 1, 2, m.L - 1, m.L, m.L + 1, 4 * m.L, b.R_ORDER, 1 << 255, TOP]
EDGE_377 = [0, 1, 2, b.R_ORDER - 1, b.R_ORDER, b.R_ORDER + 1, 2 * b.R_ORDER, 1 << 255, TOP, int("01" * 128, 2), int("10" * 128, 2)]


def digit_pattern_scalars():
    """2-bit signed windows take digits -2, -1, 0, 1: a scalar of one repeated window value u gives every digit u - 2 in every position;
    mixtures and alternations flip the sign from window to window; single bits and 2^256 - 2^i carry through the offset recoding"""
    ks = [int(format(u, "02b") * 128, 2) for u in range(4)]
    ks += [int("0110" * 64, 2), int("1001" * 64, 2), int("0011" * 64, 2), int("1100" * 64, 2), int("01" + "10" * 127, 2)]
    ks += [(1 << i) for i in (0, 1, 2, 3, 127, 254, 255)] + [(1 << 256) - (1 << i) for i in (1, 2, 128)]
    return ks


def te_torsion_points():
    """(name, point) outside the subgroup: T2 = (0, -1) of order 2, both T4 = (+-sqrt(-1), 0) of order 4, G + T2 (order 2 L), G + T4 (4 L)"""
    i4 = sqrt_minus_one()
    t2, t4a, t4b = (0, m.P - 1), (i4, 0), (m.P - i4, 0)
    g = (m.GX, m.GY)
    out = [("T2", t2), ("T4", t4a), ("-T4", t4b), ("G+T2", m.add(g, t2)), ("G+T4", m.add(g, t4a))]
    for _, p in out:
        assert m.on_curve(p)
    return out


def te_edge_cases(n_subgroup=4):
    """(name, point bytes, scalar, expected bytes): the cross product of every edge and digit-pattern scalar with subgroup points, O = (0, 1) and
    the torsion points, from the bigint model -- a few hundred elements, shared with the GPU tests"""
    pts = [("subgroup point %d" % i, p) for i, p in enumerate(te_points(0xA16, n_subgroup))] + [("O", (0, 1))] + te_torsion_points()
    ks = [("edge scalar %d" % i, k) for i, k in enumerate(EDGE_TE)] + [("digit pattern %d" % i, k) for i, k in enumerate(digit_pattern_scalars())]
    return [("%s x %s" % (kn, pn), m.points_to_bytes([p]), k, m.points_to_bytes([m.scalar_mul(k, p)])) for kn, k in ks for pn, p in pts]


def bls_edge_cases():
    """(name, points bytes, scalars, expected bytes) for n = 1, 7, 8, 9, 15, 16, 17, 19 -- every tail shape of the affine groups of 8 -- with the
    edge scalars in turn and scalars r or 0 placed so that infinity falls on the first slot, the last slot, a middle slot and a whole group"""
    r = b.R_ORDER
    out = []
    for n in (1, 7, 8, 9, 15, 16, 17, 19):
        raw = oracle377.gen_points(0x3E + n, n)
        pts = [b.xy_from_bytes(raw[96 * i:96 * i + 96]) for i in range(n)]
        plans = {"edge scalars": [EDGE_377[(i + n) % len(EDGE_377)] for i in range(n)],
                 "infinity first": [r if i == 0 else 1000 + i for i in range(n)],
                 "infinity last": [0 if i == n - 1 else 1000 + i for i in range(n)],
                 "infinity in the middle": [r if i == n // 2 or i % 8 == 3 else 1000 + i for i in range(n)],
                 "a whole group at infinity": [(0, r)[i & 1] if i < 8 else 1000 + i for i in range(n)],
                 "the last group at infinity": [2 * r if i >= 8 * ((n - 1) // 8) else 1000 + i for i in range(n)]}
        for what, ks in plans.items():
            out.append(("n = %d, %s" % (n, what), raw, ks, b"".join(b.result_to_bytes(b.scalar_mul(k, p)) for k, p in zip(ks, pts))))
    return out


# ---- Twisted-Edwards BLS12 -----------------------------------------------------------------------------------------------------
def test_reference_scalar_mul_kats(sm, kats):
    assert len(kats["scalar_mul"]) == 5
    pts = [(int(k["x"]), int(k["y"])) for k in kats["scalar_mul"]]
    ks = [int(k["k"]) for k in kats["scalar_mul"]]
    exp = [(int(k["rx"]), int(k["ry"])) for k in kats["scalar_mul"]]
    assert mul_te(sm, pts, ks) == exp
    for p, k, e in zip(pts, ks, exp):                  # the shared form, one point at a time
        assert mul_te(sm, [p], k, shared=True) == [e]


def test_reference_group_scalar_mul_x_kats(sm, kats):
    assert len(kats["group_scalar_mul_x"]) == 2
    for x, k, rx in kats["group_scalar_mul_x"]:
        out = ctypes.create_string_buffer(64)
        assert sm.sm_mul_x_te(int(x).to_bytes(32, "little"), int(k).to_bytes(32, "little"), out) == 0
        assert int.from_bytes(out.raw[:32], "little") == int(rx)


def test_random_points_and_scalars_per_point(sm):
    rnd = random.Random(0x5CA1)
    pts = te_points(0xA11, 300)
    ks = [rnd.getrandbits(256) for _ in range(300)]
    assert mul_te(sm, pts, ks) == [m.scalar_mul(k, p) for k, p in zip(ks, pts)]


def test_random_scalars_shared(sm):
    rnd = random.Random(0x5CA2)
    pts = te_points(0xA12, 19)                         # 19: groups of 8, 8 and 3 in the affine pass
    for k in [rnd.getrandbits(256) for _ in range(6)] + [rnd.getrandbits(253) for _ in range(3)]:
        assert mul_te(sm, pts, k, shared=True) == [m.scalar_mul(k, p) for p in pts], k


def test_edge_scalars_both_recodings(sm):
    pts = te_points(0xA13, len(EDGE_TE))
    assert mul_te(sm, pts, EDGE_TE) == [m.scalar_mul(k, p) for k, p in zip(EDGE_TE, pts)]
    for k in EDGE_TE:
        assert mul_te(sm, pts[:3], k, shared=True) == [m.scalar_mul(k, p) for p in pts[:3]], k
    assert mul_te(sm, pts[:2], [0, m.L]) == [(0, 1), (0, 1)]


def test_digit_patterns_hit_every_table_entry_and_sign(sm):
    # 2-bit signed windows take digits -2, -1, 0, 1: a scalar of one repeated window value u gives every digit u - 2 in every
    # position; mixtures and alternations flip the sign from window to window
    ks = digit_pattern_scalars()
    assert len(ks) == 19
    pts = te_points(0xA14, len(ks))
    assert mul_te(sm, pts, ks) == [m.scalar_mul(k, p) for k, p in zip(ks, pts)]
    for k in ks[:4]:
        assert mul_te(sm, pts[:2], k, shared=True) == [m.scalar_mul(k, p) for p in pts[:2]], k


def test_points_outside_the_subgroup(sm):
    t2, t4a, t4b, g2l, g4l = (p for _, p in te_torsion_points())       # g2l of order 2 L, g4l of order 4 L
    assert m.scalar_mul(4, t4a) == (0, 1) and m.scalar_mul(2, t4a) == t2
    assert m.scalar_mul(2 * m.L, g2l) == (0, 1) and m.scalar_mul(m.L, g2l) == t2
    pts = [t2, t4a, t4b, g2l, g4l]
    rnd = random.Random(0x5CA3)
    ks = EDGE_TE + [3, 5, 2 * m.L + 1, 4 * m.L - 1] + [rnd.getrandbits(256) for _ in range(6)]
    for p in pts:
        assert mul_te(sm, [p] * len(ks), ks) == [m.scalar_mul(k, p) for k in ks], p
        for k in ks:
            assert mul_te(sm, [p], k, shared=True) == [m.scalar_mul(k, p)], (p, k)


def test_shared_equals_per_point_with_the_scalar_repeated(sm):
    pts = te_points(0xA15, 17)
    for k in (TOP, 4 * m.L + 7, 12345):
        assert mul_te(sm, pts, k, shared=True) == mul_te(sm, pts, [k] * 17)


def naf_of(sm, curve, k):
    pos, neg = (ctypes.c_uint32 * 8)(), (ctypes.c_uint32 * 8)()
    top = sm.sm_naf(curve, k.to_bytes(32, "little"), pos, neg)
    val = sum(((pos[i // 32] >> (i % 32)) & 1) << i for i in range(256)) - sum(((neg[i // 32] >> (i % 32)) & 1) << i for i in range(256))
    digits = [((pos[i // 32] >> (i % 32)) & 1) - ((neg[i // 32] >> (i % 32)) & 1) for i in range(256)]
    return top, val, digits


def test_shared_naf_reduces_legally_and_is_non_adjacent(sm):
    rnd = random.Random(0x5CA4)
    for curve, order in ((0, 4 * m.L), (1, b.R_ORDER)):
        for k in [0, 1, 2, 3, order - 1, order, order + 1, 1 << 255, TOP] + [rnd.getrandbits(256) for _ in range(50)]:
            top, val, digits = naf_of(sm, curve, k)
            assert val == k % order, (curve, k)
            assert top == (max(i for i, d in enumerate(digits) if d) if val else -1)
            assert all(not (digits[i] and digits[i + 1]) for i in range(255)), (curve, k)
            assert top < 254


# ---- BLS12-377 G1 --------------------------------------------------------------------------------------------------------------
def test_bls377_random_points_and_scalars(sm):
    rnd = random.Random(0x377)
    n = 40
    raw = oracle377.gen_points(11, n)
    pts = [b.xy_from_bytes(raw[96 * i:96 * i + 96]) for i in range(n)]
    ks = [rnd.getrandbits(256) for _ in range(n)]
    assert mul_377(sm, raw, ks) == b"".join(b.result_to_bytes(b.scalar_mul(k, p)) for k, p in zip(ks, pts))
    for k in (ks[0], TOP):
        assert mul_377(sm, raw[:96 * 9], k, shared=True) == b"".join(b.result_to_bytes(b.scalar_mul(k, p)) for p in pts[:9])


def test_bls377_edge_scalars_and_infinity(sm):
    ks = EDGE_377
    assert len(ks) == 11 and ks[4] == b.R_ORDER
    raw = oracle377.gen_points(12, len(ks))
    pts = [b.xy_from_bytes(raw[96 * i:96 * i + 96]) for i in range(len(ks))]
    got = mul_377(sm, raw, ks)
    assert got == b"".join(b.result_to_bytes(b.scalar_mul(k, p)) for k, p in zip(ks, pts))
    assert got[:96] == bytes(96) and got[96 * 4:96 * 5] == bytes(96)       # [0] P and [r] P: the point at infinity as zeros
    for k in ks:
        assert mul_377(sm, raw[:96 * 3], k, shared=True) == b"".join(b.result_to_bytes(b.scalar_mul(k, p)) for p in pts[:3]), k


def test_bls377_infinity_among_finite_results_keeps_the_neighbours_right(sm):
    # infinity results in the middle of an affine group must not spoil the other inverses of the group
    raw = oracle377.gen_points(13, 16)
    pts = [b.xy_from_bytes(raw[96 * i:96 * i + 96]) for i in range(16)]
    ks = [(b.R_ORDER if i % 3 == 1 else 1000 + i) for i in range(16)]
    assert mul_377(sm, raw, ks) == b"".join(b.result_to_bytes(b.scalar_mul(k, p)) for k, p in zip(ks, pts))


def test_the_shared_edge_cases_on_the_host(sm):
    """the case builders the GPU tests import, through the host build: per-point scalars over the whole cross product, the shared form on one
    row of it, every BLS12-377 tail shape with infinity at the first, last and middle slots and over whole groups"""
    cases = te_edge_cases()
    assert 200 <= len(cases) <= 400
    pts = [m.xy_from_bytes(c[1]) for c in cases]
    got = mul_te(sm, pts, [c[2] for c in cases])
    for c, g in zip(cases, got):
        assert m.points_to_bytes([g]) == c[3], c[0]
    for name, raw, ks, want in bls_edge_cases():
        assert mul_377(sm, raw, ks) == want, name
        assert want.count(bytes(96)) >= (0 if "edge scalars" in name and len(ks) < 3 else 1), name


# ---- the public names -----------------------------------------------------------------------------------------------------------
NEW_FUNCS = ("te_msm_mul", "te_msm_mul_device", "te_msm_mul_x")


def test_header_declares_the_scalar_mul_entry_points(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name in NEW_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "te_msm.h"\n#include <stddef.h>\n'
                   "int (*f1)(te_ctx*, const uint8_t*, const uint8_t*, uint64_t, int, uint8_t*) = te_msm_mul;\n"
                   "int (*f2)(te_ctx*, const void*, const void*, uint64_t, int, void*) = te_msm_mul_device;\n"
                   "int (*f3)(te_ctx*, const uint8_t*, const uint8_t*, uint64_t, int, uint8_t*) = te_msm_mul_x;\n"
                   "int main(void) { return f1 && f2 && f3 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "use.o"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


def test_library_and_package_export_the_scalar_mul_entry_points(pkg):
    for meth in ("mul", "mul_device", "mul_x"):
        assert callable(getattr(pkg.MsmContext, meth, None)), meth
    r = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        pytest.skip("no nm")
    syms = set(re.findall(r"\bT\s+(\w+)", r.stdout.decode()))
    for name in NEW_FUNCS:
        assert name in syms, name


def test_node_module_exports_scalar_mul():
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    src = open(os.path.join(js, "compute_msm.js")).read()
    assert re.search(r"module\.exports\s*=\s*\{[^}]*\bscalarMul\b[^}]*\bscalarMulX\b", src)
    dts = open(os.path.join(js, "submission.d.ts")).read()
    assert "export declare const scalarMul: (points: Buffer, scalars: Buffer) => Buffer;" in dts
    assert "export declare const scalarMulX: (xs: Buffer, scalars: Buffer) => Buffer;" in dts
    addon = open(os.path.join(js, "addon.cc")).read()
    assert '{"scalarMul", ScalarMul}' in addon and '{"scalarMulX", ScalarMulX}' in addon
