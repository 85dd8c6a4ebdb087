"""Batched group addition and point-set sums (te_msm_add*, te_msm_sum*): the product's per-lane code (csrc/group_add.hip.hpp, compiled for
the host by tests/csrc/groupaddcheck.cpp, the sum's block emulated as loops over its lanes) against the reference's known answers and the
bigint models; a deliberately wrong variant of the emulation, caught; a stand-alone sanitizer program; and the new names in the C header,
the library, the package and the addon."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

from oracle import model as m
from oracle import model377 as b

import group_add_cases as gc
import test_scalar_mul_host as smh

ROOT = gc.ROOT


@pytest.fixture(scope="module")
def ga():
    return gc.shim()


# ---- the reference's vectors ---------------------------------------------------------------------------------------------------------
def test_reference_add_groups_x_kats(ga, kats):
    """wasmFunctions.test.ts:28-40 through recover -> add -> x (two of the five are doublings)"""
    assert len(kats["add_groups_x"]) == 5
    doublings = 0
    for ax, bx, rx in kats["add_groups_x"]:
        out = ctypes.create_string_buffer(64)
        assert ga.ga_add_x_te(int(ax).to_bytes(32, "little"), int(bx).to_bytes(32, "little"), 0, out) == 0
        assert int.from_bytes(out.raw[:32], "little") == int(rx)
        doublings += ax == bx
    assert doublings == 2


# ---- Twisted-Edwards BLS12 -------------------------------------------------------------------------------------------------------------
def test_te_random_pairs_add_and_subtract(ga):
    a, bb = gc.te_points(0x6A1, 300), gc.te_points(0x6A2, 300)
    assert gc.shim_add(ga, 0, a, bb) == gc.model_add_all(0, a, bb)
    assert gc.shim_add(ga, 0, a, bb, gc.SUBTRACT) == gc.model_add_all(0, a, bb, subtract=True)
    assert gc.shim_add(ga, 0, a, bb[:64], gc.SHARED_B) == gc.model_add_all(0, a, bb[:64])
    assert gc.shim_add(ga, 0, a, bb[:64], gc.SHARED_B | gc.SUBTRACT) == gc.model_add_all(0, a, bb[:64], subtract=True)


def test_te_every_pair_of_the_edge_points(ga):
    """te_edge_cases() x te_edge_cases(), every distinct point of it with every other: the identity, order 2, 4, 2 L, 4 L, P + P, P - P"""
    pts = gc.te_edge_points()
    assert len(pts) >= 40 and m.points_to_bytes([(0, 1)]) in pts and m.points_to_bytes([(0, m.P - 1)]) in pts
    dec = [m.xy_from_bytes(r) for r in pts]
    a = b"".join(p for p in pts for _ in pts)
    bb = b"".join(pts) * len(pts)
    want = b"".join(m.points_to_bytes([m.add(p, q)]) for p in dec for q in dec)
    assert gc.shim_add(ga, 0, a, bb) == want
    few, dfew = pts[:60], dec[:60]                          # (every input point of the cases is among the first of them)
    a, bb = b"".join(p for p in few for _ in few), b"".join(few) * len(few)
    assert gc.shim_add(ga, 0, a, bb, gc.SUBTRACT) == b"".join(m.points_to_bytes([m.add(p, m.neg(q))]) for p in dfew for q in dfew)


def test_te_core_pairs_are_what_their_names_say(ga):
    for name, ra, rb in gc.te_core_pairs():
        assert gc.shim_add(ga, 0, ra, rb) == gc.model_add(0, ra, rb), name
        assert gc.shim_add(ga, 0, ra, rb, gc.SUBTRACT) == gc.model_add(0, ra, rb, subtract=True), name
    p = dict(gc.te_core_points())
    assert gc.shim_add(ga, 0, p["P"], p["-P"]) == p["O"] and gc.shim_add(ga, 0, p["P"], p["P"], gc.SUBTRACT) == p["O"]
    assert gc.shim_add(ga, 0, p["T4"], p["T4"]) == p["T2"] and gc.shim_add(ga, 0, p["T2"], p["T2"]) == p["O"]


# ---- BLS12-377 G1 ----------------------------------------------------------------------------------------------------------------------
def test_bls377_random_pairs_add_and_subtract(ga):
    a, bb = gc.bls_points(0x7A1, 60), gc.bls_points(0x7A2, 60)
    assert gc.shim_add(ga, 1, a, bb) == gc.model_add_all(1, a, bb)
    assert gc.shim_add(ga, 1, a, bb, gc.SUBTRACT) == gc.model_add_all(1, a, bb, subtract=True)
    assert gc.shim_add(ga, 1, a, bb[:96], gc.SHARED_B) == gc.model_add_all(1, a, bb[:96])


def test_bls377_edge_case_results_as_operands(ga):
    """the results of bls_edge_cases() -- G1 points with infinity at the first, last and middle slots and over whole groups -- added to each
    other reversed, to themselves (P + P) and subtracted from themselves (P - P)"""
    for name, _, _, want in smh.bls_edge_cases():
        recs = gc.records(1, want)
        rev = b"".join(reversed(recs))
        assert gc.shim_add(ga, 1, want, rev) == gc.model_add_all(1, want, rev), name
        assert gc.shim_add(ga, 1, want, want) == gc.model_add_all(1, want, want), name
        assert gc.shim_add(ga, 1, want, want, gc.SUBTRACT) == bytes(len(want)), name


def test_bls377_infinity_in_either_or_both_operands(ga):
    for name, ra, rb in gc.bls_core_pairs():
        assert gc.shim_add(ga, 1, ra, rb) == gc.model_add(1, ra, rb), name
        assert gc.shim_add(ga, 1, ra, rb, gc.SUBTRACT) == gc.model_add(1, ra, rb, subtract=True), name
    inf = bytes(96)
    assert gc.shim_add(ga, 1, inf, inf) == inf and gc.shim_add(ga, 1, inf, inf, gc.SUBTRACT) == inf


def test_the_zero_record_passes_these_calls_checks_only(ga):
    sub = ctypes.c_int(0)
    assert ga.ga_check(1, bytes(96), ctypes.byref(sub)) == 0 and sub.value == 1
    p = gc.bls_points(0x7A3, 1)
    assert ga.ga_check(1, p, ctypes.byref(sub)) == 0 and sub.value == 1
    bad = bytearray(p)
    bad[0] ^= 1
    assert ga.ga_check(1, bytes(bad), ctypes.byref(sub)) == 2
    t2 = m.points_to_bytes([(0, m.P - 1)])
    assert ga.ga_check(0, t2, ctypes.byref(sub)) == 0 and sub.value == 0
    assert ga.ga_check(0, bytes(64), ctypes.byref(sub)) == 2            # (0, 0) is not on the Twisted-Edwards curve


# ---- the affine pass at the edges of its groups of eight ------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_add_at_every_tail_shape_of_the_affine_groups_with_infinity_among_the_results(ga, curve):
    """n = 1, 7, 8, 9, 15, 16, 17: every tail of the groups of eight; every third pair is P - P, so the result is the identity -- on
    BLS12-377 the point at infinity: Z = 0 takes a stand-in in the group's product and comes out as zeros, the neighbours untouched"""
    gen = gc.bls_points if curve == 1 else gc.te_points
    pb = gc.point_bytes(curve)
    a = gen(0x51, 17)
    recs = gc.records(curve, a)
    bb = b"".join(r if i % 3 == 1 else recs[(i + 5) % 17] for i, r in enumerate(recs))
    want = gc.model_add_all(curve, a, bb, subtract=True)
    ident = bytes(96) if curve == 1 else m.points_to_bytes([(0, 1)])
    assert want[pb:2 * pb] == ident and want[:pb] != ident
    for n in (1, 7, 8, 9, 15, 16, 17):
        assert gc.shim_add(ga, curve, a[:pb * n], bb[:pb * n], gc.SUBTRACT) == want[:pb * n], n


# ---- the sum -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_sum_against_the_python_fold(ga, curve):
    gen = gc.bls_points if curve == 1 else gc.te_points
    pb = gc.point_bytes(curve)
    raw = gen(0x54, 257)
    for n in (0, 1, 2, 255, 256, 257):
        want = gc.model_sum(curve, raw[:pb * n])
        assert gc.shim_sum(ga, curve, raw[:pb * n]) == want, n
        assert gc.shim_sum(ga, curve, raw[:pb * n], grid=1) == want, n       # one block: every lane strides
    assert gc.shim_sum(ga, curve, b"") == (bytes(96) if curve == 1 else m.points_to_bytes([(0, 1)]))


@pytest.mark.parametrize("curve", [0, 1])
def test_sum_of_one_point_repeated_and_of_p_minus_p_alternating(ga, curve):
    gen = gc.bls_points if curve == 1 else gc.te_points
    mod = b if curve == 1 else m
    p = gen(0x55, 1)
    pt = gc.decode(curve, p)
    assert gc.shim_sum(ga, curve, p * 300) == gc.encode(curve, mod.scalar_mul(300, pt))
    neg = gc.encode(curve, mod.neg(pt))
    ident = bytes(96) if curve == 1 else m.points_to_bytes([(0, 1)])
    assert gc.shim_sum(ga, curve, (p + neg) * 150) == ident
    assert gc.shim_sum(ga, curve, (p + neg) * 150 + p) == p
    assert gc.shim_sum(ga, curve, (p + neg) * 150 + p, grid=2) == p


def test_sum_with_torsion_points_and_bls_infinity(ga):
    recs = [r for _, r in gc.te_core_points()] * 7 + gc.records(0, gc.te_points(0x56, 20))
    random.Random(0x57).shuffle(recs)
    raw = b"".join(recs)
    assert gc.shim_sum(ga, 0, raw) == gc.model_sum(0, raw)
    recs = gc.records(1, gc.bls_points(0x58, 30)) + [bytes(96)] * 5
    random.Random(0x59).shuffle(recs)
    raw = b"".join(recs)
    assert gc.shim_sum(ga, 1, raw) == gc.model_sum(1, raw)
    assert gc.shim_sum(ga, 1, bytes(96) * 9) == bytes(96)


# ---- a deliberate mistake: the variant of the emulation must be caught by the checks above ------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_b_not_negated_under_subtract_is_caught(ga, curve):
    gen = gc.bls_points if curve == 1 else gc.te_points
    a, bb = gen(0x5B, 5), gen(0x5C, 5)
    assert gc.shim_add(ga, curve, a, bb, gc.SUBTRACT, gc.M_NO_NEGATE) != gc.model_add_all(curve, a, bb, subtract=True)
    assert gc.shim_add(ga, curve, a, bb, gc.SUBTRACT, gc.M_NO_NEGATE) == gc.model_add_all(curve, a, bb)


# ---- sanitizers: a stand-alone program, nothing loaded into Python ---------------------------------------------------------------------------
def test_sanitizer_program_over_the_addition_and_the_sum():
    """tests/sanitize/san_group_add.cpp: its own main over the shim, built with -fsanitize=address,undefined; a sanitizer report aborts it"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tests", "sanitize")
    os.makedirs(os.path.join(d, "_build"), exist_ok=True)
    exe = os.path.join(d, "_build", "san_group_add")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(d, "san_group_add.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in out and "san_group_add: all checks passed" in out, out[-4000:]


# ---- the public names ---------------------------------------------------------------------------------------------------------------------
NEW_FUNCS = ("te_msm_add", "te_msm_add_device", "te_msm_add_x", "te_msm_sum", "te_msm_sum_device", "te_msm_sum_x")


def test_header_declares_the_group_add_entry_points(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name in NEW_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert re.search(r"#define\s+TE_MSM_ADD_SUBTRACT\s+1\b", hdr) and re.search(r"#define\s+TE_MSM_ADD_SHARED_B\s+2\b", hdr)
    assert "wasmFunctions.ts:112-119" in hdr and "wasmFunctions.ts:121-125" in hdr and '"bad_point_operand"' in hdr
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "te_msm.h"\n#include <stddef.h>\n'
                   "int (*f1)(te_ctx*, const uint8_t*, const uint8_t*, uint64_t, int, uint8_t*) = te_msm_add;\n"
                   "int (*f2)(te_ctx*, const void*, const void*, uint64_t, int, void*) = te_msm_add_device;\n"
                   "int (*f3)(te_ctx*, const uint8_t*, const uint8_t*, uint64_t, int, uint8_t*) = te_msm_add_x;\n"
                   "int (*f4)(te_ctx*, const uint8_t*, uint64_t, uint8_t*) = te_msm_sum;\n"
                   "int (*f5)(te_ctx*, const void*, uint64_t, uint8_t*) = te_msm_sum_device;\n"
                   "int (*f6)(te_ctx*, const uint8_t*, uint64_t, uint8_t*) = te_msm_sum_x;\n"
                   "int flags = TE_MSM_ADD_SUBTRACT | TE_MSM_ADD_SHARED_B;\n"
                   "int main(void) { return f1 && f2 && f3 && f4 && f5 && f6 && flags == 3 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "use.o"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


def test_library_and_package_export_the_group_add_entry_points(pkg):
    for meth in ("add", "add_device", "add_x", "sum", "sum_device", "sum_x"):
        assert callable(getattr(pkg.MsmContext, meth, None)), meth
    assert "operand" in pkg.MsmError(-5, "x", 0, 1, 1).__dict__
    r = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        pytest.skip("no nm")
    syms = set(re.findall(r"\bT\s+(\w+)", r.stdout.decode()))
    for name in NEW_FUNCS:
        assert name in syms, name


def test_node_module_exports_group_add():
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    src = open(os.path.join(js, "compute_msm.js")).read()
    exports = re.search(r"module\.exports\s*=\s*\{([^}]*)\}", src).group(1)
    dts = open(os.path.join(js, "submission.d.ts")).read()
    addon = open(os.path.join(js, "addon.cc")).read()
    for name in ("groupAdd", "groupAddX", "groupSum", "groupSumX"):
        assert re.search(r"\b%s\b" % name, exports), name
        assert "export declare const %s:" % name in dts, name
        assert '{"%s", %s}' % (name, name[0].upper() + name[1:]) in addon, name
