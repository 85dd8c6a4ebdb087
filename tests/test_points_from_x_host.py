"""x-only points (te_msm_points_from_x*, te_msm_bind_points_x, te_msm_run_x): the product's recovery code (csrc/from_x.hip.hpp,
compiled for the host by tests/csrc/fromxcheck.cpp -- the same functions k_points_from_x runs on gfx950) against the reference's
getPointFromX known answers and the bigint models, on every class of bad x, and the new names of the C header and the package."""
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
def fx():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libfromxcheck.so"), os.path.join(d, "fromxcheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("from_x.hip.hpp", "check.hip.hpp", "fp.hpp", "fq377.hpp", "field.hpp", "curve.hpp",
                                                         "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    for f in (L.fx_from_x_te, L.fx_from_x_377, L.fx_sqrt_377):
        f.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
    L.fx_sqrt_ratio_te.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p]
    return L


def recover_te(fx, x):
    out = ctypes.create_string_buffer(64)
    r = fx.fx_from_x_te(int(x % (1 << 256)).to_bytes(32, "little"), out)
    return r, (int.from_bytes(out.raw[:32], "little"), int.from_bytes(out.raw[32:], "little"))


def recover_377(fx, x48: bytes):
    out = ctypes.create_string_buffer(96)
    r = fx.fx_from_x_377(x48, out)
    return r, (int.from_bytes(out.raw[:48], "little"), int.from_bytes(out.raw[48:], "little"))


def x377(x, larger=False, infinity=False, extra=0):
    v = x | (extra << 377) | (int(infinity) << 382) | (int(larger) << 383)
    return v.to_bytes(48, "little")


def te_y2(x):
    return (1 + x * x) * pow(1 - m.D * x * x, -1, m.P) % m.P


def is_qr(a, p):
    return a % p == 0 or pow(a, (p - 1) // 2, p) == 1


# ---- Twisted-Edwards BLS12 ---------------------------------------------------------------------------------------------------------
def test_reference_point_from_x_kats(fx, kats):
    assert len(kats["point_from_x"]) == 6
    for k in kats["point_from_x"]:
        x, y = int(k["x"]), int(k["y"])
        assert recover_te(fx, x) == (0, (x, y))


def test_recovery_gives_back_subgroup_points(fx):
    pts = oracle.gen_points(0xF00D, 1000) + oracle.gen_points_random(0xF00E, 1000)
    for i in range(2000):
        x, y = m.xy_from_bytes(pts[64 * i:64 * i + 64])
        assert recover_te(fx, x) == (0, (x, y)), i
    assert recover_te(fx, 0) == (0, (0, 1))
    assert recover_te(fx, m.GX) == (0, (m.GX, m.GY))


def test_bad_x_reasons(fx):
    for x in (m.P, m.P + 1, (1 << 256) - 1):
        assert recover_te(fx, x)[0] == 1, x
    rng = random.Random(3)
    nonres = [x for x in (rng.randrange(m.P) for _ in range(40)) if not is_qr(te_y2(x), m.P)][:6]
    assert len(nonres) >= 3
    for x in nonres:
        assert recover_te(fx, x)[0] == 2, x
    i4 = m.sqrt_mod_p(m.P - 1)
    T4 = (i4, 0)
    assert m.on_curve(T4) and m.add(T4, T4) == (0, m.P - 1)
    assert recover_te(fx, i4)[0] == 3 and recover_te(fx, m.P - i4)[0] == 3       # +-sqrt(-1): y = 0, order 4
    P = m.xy_from_bytes(oracle.gen_points(21, 1))
    for T in (T4, m.neg(T4)):                                                     # P + T4, P - T4
        PT = m.add(P, T)
        assert m.on_curve(PT) and m.scalar_mul(m.L, PT) != m.ZERO
        assert recover_te(fx, PT[0])[0] == 3


def test_order_two_shift_recovers_the_negated_point(fx):
    """P + T2 = (-x, -y): its x recovers -P = (-x, y), the point of the subgroup with that x (one chain, Q = T2: take -y)"""
    for seed in (31, 32, 33):
        P = m.xy_from_bytes(oracle.gen_points(seed, 1))
        PT = m.add(P, (0, m.P - 1))
        assert PT == ((-P[0]) % m.P, (-P[1]) % m.P)
        assert recover_te(fx, PT[0]) == (0, ((-P[0]) % m.P, P[1]))


def test_model_point_from_x_differs_only_outside_the_subgroup(fx):
    """getPointFromX (oracle.model.point_from_x) agrees wherever a subgroup point exists; on an order-4 coset it returns (x, -y) while
    the engine reports reason 3"""
    P = m.xy_from_bytes(oracle.gen_points(41, 1))
    assert recover_te(fx, P[0]) == (0, m.point_from_x(P[0]))
    PT = m.add(P, (m.sqrt_mod_p(m.P - 1), 0))
    assert m.point_from_x(PT[0])[0] == PT[0]                 # the reference answers something ...
    assert recover_te(fx, PT[0])[0] == 3                     # ... the engine refuses


# ---- square roots in both fields --------------------------------------------------------------------------------------------------
def two_adic_order(a, p):
    t, s = p - 1, 0
    while t % 2 == 0:
        t, s = t // 2, s + 1
    r, k = pow(a, t, p), 0
    while r != 1:
        r, k = r * r % p, k + 1
    return k, s


def smallest_nonresidue(p):
    z = 2
    while is_qr(z, p):
        z += 1
    return z


def test_sqrt_ratio_te_matches_the_model(fx):
    p = m.P
    z = smallest_nonresidue(p)
    rng = random.Random(5)
    cases = [(rng.randrange(1, p), rng.randrange(1, p)) for _ in range(60)]
    cases += [(z, 1), (z * z % p, 1), (pow(z, 3, p), 1), (1, 1), (p - 1, 1), (4, 1), (1, z)]
    assert two_adic_order(z * z % p, p) == (46, 47) and two_adic_order(z, p) == (47, 47)   # the uniform loop runs all 47 steps
    y = ctypes.create_string_buffer(32)
    for u, v in cases:
        qr = fx.fx_sqrt_ratio_te(u.to_bytes(32, "little"), v.to_bytes(32, "little"), y)
        r = u * pow(v, -1, p) % p
        got = int.from_bytes(y.raw, "little")
        assert got < p
        assert bool(qr) == is_qr(r, p), (u, v)
        if qr:
            want = m.sqrt_mod_p(r)
            assert got in (want, p - want), (u, v)
        else:
            assert got * got % p == z * r % p, (u, v)


def test_sqrt_377_matches_the_model(fx):
    q = b.Q
    z = smallest_nonresidue(q)
    rng = random.Random(6)
    cases = [rng.randrange(1, q) for _ in range(60)] + [z, z * z % q, pow(z, 3, q), 1, q - 1, 4]
    assert two_adic_order(z * z % q, q) == (45, 46) and two_adic_order(z, q) == (46, 46)
    y = ctypes.create_string_buffer(48)
    for u in cases:
        qr = fx.fx_sqrt_377(u.to_bytes(48, "little"), y)
        got = int.from_bytes(y.raw, "little")
        assert got < q
        assert bool(qr) == is_qr(u, q), u
        if qr:
            assert got * got % q == u, u
        else:
            assert got * got % q == z * u % q, u


# ---- BLS12-377 G1 ---------------------------------------------------------------------------------------------------------------
def test_bls377_flags_pick_the_root(fx):
    pts = oracle377.gen_points(9, 40) + b.points_to_bytes([b.G])
    for i in range(len(pts) // 96):
        x, y = b.xy_from_bytes(pts[96 * i:96 * i + 96])
        yl, ys = max(y, b.Q - y), min(y, b.Q - y)
        assert recover_377(fx, x377(x, larger=True)) == (0, (x, yl)), i
        assert recover_377(fx, x377(x, larger=False)) == (0, (x, ys)), i
        assert recover_377(fx, x377(x, larger=y > b.Q - y)) == (0, (x, y)), i


def test_bls377_bad_x_reasons(fx):
    G = b.G
    for extra in (1, 2, 4, 8, 16, 31):                                             # bits 377 .. 381
        assert recover_377(fx, x377(G[0], extra=extra))[0] == 1, extra
        assert recover_377(fx, x377(G[0], larger=True, infinity=True, extra=extra))[0] == 1, extra
    for x in (b.Q, b.Q + 1, (1 << 377) - 1):
        assert recover_377(fx, x377(x))[0] == 1, x
    assert recover_377(fx, x377(G[0], infinity=True))[0] == 2
    assert recover_377(fx, x377(0, infinity=True))[0] == 2
    assert recover_377(fx, bytes(47) + b"\x40")[0] == 2                           # the bare infinity flag
    rng = random.Random(8)
    nonres = [x for x in (rng.randrange(b.Q) for _ in range(40)) if not is_qr(x ** 3 + 1, b.Q)][:6]
    assert len(nonres) >= 3
    for x in nonres:
        assert recover_377(fx, x377(x))[0] == 2 and recover_377(fx, x377(x, larger=True))[0] == 2
    assert recover_377(fx, x377(b.Q - 1))[0] == 2 and recover_377(fx, x377(b.Q - 1, larger=True))[0] == 2   # x = -1: y = 0
    assert recover_377(fx, x377(0)) == (0, (0, 1)) and recover_377(fx, x377(0, larger=True)) == (0, (0, b.Q - 1))


def test_bls377_recovered_points_pass_the_form_check(fx):
    """a recovered point always passes check_form_377; outside G1 it still recovers (membership is option check_points = 2)"""
    rng = random.Random(10)
    seen = 0
    while seen < 12:
        x = rng.randrange(b.Q)
        if not is_qr(x ** 3 + 1, b.Q):
            continue
        r, (gx, gy) = recover_377(fx, x377(x))
        assert r == 0 and gx == x and b.on_curve((gx, gy)) and gy <= b.Q // 2
        seen += 1


# ---- the public names -----------------------------------------------------------------------------------------------------------
NEW_FUNCS = ("te_msm_points_from_x", "te_msm_points_from_x_device", "te_msm_bind_points_x", "te_msm_run_x")


def test_header_declares_the_x_only_entry_points(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    assert re.search(r"#define\s+TE_MSM_X_BYTES\s+32\b", hdr)
    assert re.search(r"#define\s+TE_MSM_X_BYTES_BLS12_377\s+48\b", hdr)
    for name in NEW_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "te_msm.h"\n#include <stddef.h>\n'
                   "int (*f1)(te_ctx*, const uint8_t*, uint64_t, uint8_t*, int64_t*, int*) = te_msm_points_from_x;\n"
                   "int (*f2)(te_ctx*, const void*, uint64_t, void*, int64_t*, int*) = te_msm_points_from_x_device;\n"
                   "int (*f3)(te_ctx*, const uint8_t*, uint64_t, te_bases**) = te_msm_bind_points_x;\n"
                   "int (*f4)(te_ctx*, const uint8_t*, const uint8_t*, uint64_t, uint8_t*) = te_msm_run_x;\n"
                   "int sizes[] = {TE_MSM_X_BYTES, TE_MSM_X_BYTES_BLS12_377};\n"
                   "int main(void) { return sizes[0] == 32 && f1 && f2 && f3 && f4 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "use.o"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


def test_library_and_package_export_the_x_only_entry_points(pkg):
    assert pkg.X_BYTES == 32 and pkg.X_BYTES_BLS12_377 == 48
    for meth in ("points_from_x", "points_from_x_device", "bind_points_x", "run_x"):
        assert callable(getattr(pkg.MsmContext, meth, None)), meth
    r = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        pytest.skip("no nm")
    syms = set(re.findall(r"\bT\s+(\w+)", r.stdout.decode()))
    for name in NEW_FUNCS:
        assert name in syms, name
