"""Input-point validation (option "check_points", te_msm_check_points): the verdicts of the product's check code
(csrc/check.hip.hpp, compiled for the host by tests/csrc/pointcheck.cpp -- the same functions k_check_form / k_check_subgroup
run on gfx950) against the bigint models on every class of bad point, and the header's new names (plain C)."""
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


@pytest.fixture(scope="module")
def pc():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libpointcheck.so"), os.path.join(d, "pointcheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("check.hip.hpp", "fp.hpp", "fq377.hpp", "field.hpp", "curve.hpp",
                                                         "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.pc_check_te.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.pc_check_377.argtypes = [ctypes.c_char_p, ctypes.c_int]
    L.pc_code.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int]
    L.pc_code.restype = ctypes.c_uint64
    L.pc_decode.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
    return L


def sqrt_mod(a, p):
    """Tonelli-Shanks; None for a non-residue"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    mm, c, t, r = s, pow(z, q, p), pow(a, q, p), pow(a, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % p, i + 1
        bb = pow(c, 1 << (mm - i - 1), p)
        mm, c, t, r = i, bb * bb % p, t * bb * bb % p, r * bb % p
    return r


def te_bytes(x, y):
    return int(x).to_bytes(32, "little") + int(y).to_bytes(32, "little")


def b_bytes(x, y):
    return int(x).to_bytes(48, "little") + int(y).to_bytes(48, "little")


def te_bad_classes():
    """(name, point bytes, reason at level 2) -- each from the model; the reason is the first check the point fails"""
    P = m.xy_from_bytes(oracle.gen_points(5, 1)[:64])
    i4 = sqrt_mod(m.P - 1, m.P)                               # x^2 = -1: (x, 0) has order 4
    T2 = (0, m.P - 1)
    assert m.on_curve(T2) and m.on_curve((i4, 0)) and m.add((i4, 0), (i4, 0)) == T2
    PT = m.add(P, T2)
    assert m.on_curve(PT) and m.scalar_mul(m.L, PT) != m.ZERO
    return [("x+p", te_bytes(P[0] + m.P, P[1]), 1),
            ("y+p", te_bytes(P[0], P[1] + m.P), 1),
            ("y+1", te_bytes(P[0], (P[1] + 1) % m.P), 2),
            ("order2", te_bytes(*T2), 3),
            ("order4", te_bytes(i4, 0), 3),
            ("order4neg", te_bytes(m.P - i4, 0), 3),
            ("P+T2", te_bytes(*PT), 3)]


def bls_random_outside(seed):
    """a curve point from a random x with x^3 + 1 a square: outside G1 (the cofactor is huge)"""
    rng = random.Random(seed)
    while True:
        x = rng.randrange(b.Q)
        y = sqrt_mod(x ** 3 + 1, b.Q)
        if y:
            pt = (x, y)
            assert b.on_curve(pt) and b.scalar_mul(b.R_ORDER, pt) is not b.INF
            return pt


def bls_bad_classes():
    G = b.xy_from_bytes(oracle377.gen_points(5, 1)[:96])
    T2 = (b.Q - 1, 0)
    assert b.on_curve(T2)
    GT = b.add(G, T2)
    assert b.on_curve(GT) and b.scalar_mul(b.R_ORDER, GT) is not b.INF
    sqrt3 = sqrt_mod(3, b.Q)
    return [("x+q", b_bytes(G[0] + b.Q, G[1]), 1),
            ("y+q", b_bytes(G[0], G[1] + b.Q), 1),
            ("y+1", b_bytes(G[0], (G[1] + 1) % b.Q), 2),
            ("(-1,0)", b_bytes(*T2), 2),                              # on the curve, order 2: y = 0, the map is undefined
            ("infinity", bytes(96), 2),                               # 0 != 0^3 + 1
            ("w=0", b_bytes((-1 - sqrt3) % b.Q, 1), 2),               # x = -1 - sqrt(3) (either root), off the curve as well
            ("P+T2", b_bytes(*GT), 3),
            ("random", b_bytes(*bls_random_outside(11)), 3),
            ("random2", b_bytes(*bls_random_outside(12)), 3)]


def test_te_bad_classes(pc):
    for name, pt, reason in te_bad_classes():
        assert pc.pc_check_te(pt, 2) == reason, name
        assert pc.pc_check_te(pt, 1) == (reason if reason < 3 else 0), name


def test_bls377_bad_classes(pc):
    for name, pt, reason in bls_bad_classes():
        assert pc.pc_check_377(pt, 2) == reason, name
        assert pc.pc_check_377(pt, 1) == (reason if reason < 3 else 0), name


def test_valid_points_pass(pc, wasm_golden):
    from oracle.gen_golden import make_inputs
    seen = 0
    for g in wasm_golden:
        if g["n"] > 4096:
            continue
        pts, _ = make_inputs(g["seed"], min(g["n"], 64), g["mode"])
        for i in range(len(pts) // 64):
            assert pc.pc_check_te(pts[64 * i:64 * i + 64], 2) == 0, (g["name"], i)
            seen += 1
    assert seen > 200
    for pt in (te_bytes(m.GX, m.GY), te_bytes(*m.ZERO), te_bytes(0, 1)):
        assert pc.pc_check_te(pt, 2) == 0
    pts = oracle377.gen_points(3, 40)
    for i in range(40):
        assert pc.pc_check_377(pts[96 * i:96 * i + 96], 2) == 0, i
    assert pc.pc_check_377(b_bytes(b.GX, b.GY), 2) == 0


def test_verdicts_match_the_model_on_random_bytes(pc):
    """random curve points: the verdict equals the model's ([order] P == O), on both curves, and random words are rejected"""
    rng = random.Random(7)
    for _ in range(6):
        x = rng.randrange(m.P)
        y2 = (1 + x * x) * pow(1 - m.D * x * x, -1, m.P) % m.P          # -x^2 + y^2 = 1 + d x^2 y^2
        y = sqrt_mod(y2, m.P)
        if y is None:
            continue
        want = 0 if m.scalar_mul(m.L, (x, y)) == m.ZERO else 3
        assert pc.pc_check_te(te_bytes(x, y), 2) == want
    for _ in range(20):
        w = bytes(rng.getrandbits(8) for _ in range(64))
        assert pc.pc_check_te(w, 2) in (1, 2)
        w = bytes(rng.getrandbits(8) for _ in range(96))
        assert pc.pc_check_377(w, 2) in (1, 2)


def test_report_code_keeps_the_lowest_index_and_reason(pc):
    n = 1000
    codes = [pc.pc_code(n, i, r) for i, r in ((700, 1), (5, 3), (5, 2), (999, 2), (0 + 6, 1))]
    top = max(codes)
    idx, rs = ctypes.c_int64(), ctypes.c_int()
    pc.pc_decode(top, n, ctypes.byref(idx), ctypes.byref(rs))
    assert (idx.value, rs.value) == (5, 2)
    assert min(codes) > 0


def test_header_names_and_still_c(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    assert re.search(r"#define\s+TE_MSM_EPOINT\s+\(-5\)", hdr)
    for name in ("TE_MSM_POINT_NONCANONICAL", "TE_MSM_POINT_OFF_CURVE", "TE_MSM_POINT_NOT_IN_SUBGROUP",
                 "te_msm_check_points", "te_msm_check_points_device", '"check_points"', '"bad_point_index"', '"bad_point_reason"'):
        assert name in hdr, name
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "te_msm.h"\n#include <stddef.h>\n'
                   "int (*f1)(te_ctx*, const uint8_t*, uint64_t, int, int64_t*, int*) = te_msm_check_points;\n"
                   "int (*f2)(te_ctx*, const void*, uint64_t, int, int64_t*, int*) = te_msm_check_points_device;\n"
                   "int codes[] = {TE_MSM_EPOINT, TE_MSM_POINT_NONCANONICAL, TE_MSM_POINT_OFF_CURVE, TE_MSM_POINT_NOT_IN_SUBGROUP};\n"
                   "int main(void) { return codes[0] == -5 && f1 && f2 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "use.o"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
