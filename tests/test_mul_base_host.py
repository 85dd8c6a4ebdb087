"""Fixed-base batch scalar multiplication (te_msm_bind_base, te_msm_mul_base*): the product's per-lane code and host-side table scalars
(csrc/mul_base.hip.hpp, compiled for the host by tests/csrc/mulbasecheck.cpp -- the functions k_mul_base and k_mul_base_entries run on
gfx950) against the Python restatement of the recoding and the bigint models:

  * the recoding for every W in 4..12, on the case scalars and 1 000 random ones;
  * every table entry at W = 4 and W = 8 for a subgroup point, G + T4 and a G1 point: the shim's table against the bigint model's, which
    is built by repeated addition; the table scalars j 2^(W i) mod (4 L | r) against Python; and the engine's route to the table (the
    scalar-multiplication chain over those scalars, the affine pass, the entry conversion) against the same bytes -- every entry at W = 4,
    every window's entries 0, 1, 2^(W-1) - 1, 2^(W-1) and a random one at W = 8 (the chain costs a millisecond an entry on the host);
  * the lane function over the full case list against m.scalar_mul / b.scalar_mul, byte for byte behind the affine group pass, at every
    W of the cases, through an accessor that counts every index outside the table (none allowed);
  * the Montgomery decode against k = a 2^-256 mod m;
  * four deliberate mistakes, each caught;
  * a stand-alone AddressSanitizer / UndefinedBehaviorSanitizer program over the same code (tests/sanitize/san_mul_base.cpp);
  * the new names in the C header, the library and the package."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

from oracle import model as m
from oracle import model377 as b
import mul_base_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def mb():
    return mc.shim()


def table_points():
    """(curve, name, wire bytes, point) of the three points whose tables are checked entry by entry"""
    sub, gt4 = mc.te_point("subgroup point 0"), mc.te_point("G+T4")
    _, raw, p377 = mc.bls_base_points()[0]
    return [(0, "subgroup point 0", m.points_to_bytes([sub]), sub), (0, "G+T4", m.points_to_bytes([gt4]), gt4), (1, "G1 point 0", raw, p377)]


def table_scalars(mb, curve, W):
    out = ctypes.create_string_buffer(mc.geometry(W)[2] * 32)
    mb.mbc_table_scalars(curve, W, out)
    return out.raw


def table_from_scalars(mb, curve, point_bytes, scalars32):
    n = len(scalars32) // 32
    out = ctypes.create_string_buffer(n * mc.SLOT)
    mb.mbc_table_from_scalars(curve, point_bytes, scalars32, n, out)
    return out.raw


def test_case_builder_prescriptions_hold():
    for W in mc.WINDOWS:
        cases = mc.prescribed(W)
        assert len(cases) == 9
        M, H, _ = mc.geometry(W)
        assert mc.recode(0, W) == [0] * M
        assert all(-H <= d < H for _, k in cases for d in mc.recode(k, W))
    assert mc.first_straddling_window(5) == 6 and mc.first_straddling_window(11) == 2 and mc.first_straddling_window(8) == 4
    assert 40 <= len(mc.case_scalars(0)) <= 60 and 40 <= len(mc.case_scalars(1)) <= 60


def test_geometry_and_offset_words(mb):
    for W in range(4, 13):
        M, H, E, C = ctypes.c_int(), ctypes.c_uint32(), ctypes.c_uint32(), (ctypes.c_uint32 * 9)()
        mb.mbc_geometry(W, ctypes.byref(M), ctypes.byref(H), ctypes.byref(E), C)
        assert (M.value, H.value, E.value) == mc.geometry(W)
        assert sum(w << (32 * j) for j, w in enumerate(C)) == mc.offset(W)
        assert W * M.value >= 258 and E.value * mc.SLOT == M.value * ((1 << (W - 1)) + 1) * 128


def test_recoding_for_every_window_width(mb):
    rnd = random.Random(0xD161)
    ks = [k for c in (0, 1) for _, k in mc.case_scalars(c)] + [rnd.getrandbits(256) for _ in range(1000)]
    for W in range(4, 13):
        M, H, _ = mc.geometry(W)
        d = (ctypes.c_int32 * M)()
        for k in ks:
            mb.mbc_digits(W, k.to_bytes(32, "little"), d)
            want = mc.recode(k, W)
            assert list(d) == want, (W, k)
            assert mc.value_of(want, W) == k and all(-H <= x < H for x in want) and want[-1] >= 0


def test_table_scalars_are_reduced_legally(mb):
    for curve, order in ((0, 4 * m.L), (1, b.R_ORDER)):
        for W in (4, 5, 8, 12):
            M, H, _ = mc.geometry(W)
            want = b"".join(((j << (W * i)) % order).to_bytes(32, "little") for i in range(M) for j in range(H + 1))
            assert table_scalars(mb, curve, W) == want, (curve, W)
            assert (H << (W * (M - 1))) >= 1 << 256                           # the top window reaches 2^256 and beyond: the reduction matters


@pytest.mark.parametrize("which", (0, 1, 2))
def test_every_table_entry_at_w4_and_w8(mb, which):
    rnd = random.Random(0x7AB)
    for curve, name, raw, p in table_points()[which:which + 1]:
        for W in (4, 8):
            M, H, E = mc.geometry(W)
            tab = mc.shim_table(curve, W, raw)
            want = mc.model_table(curve, W, p)
            assert len(tab) == E * mc.SLOT and len(want) == E
            for e in range(E):
                assert mc.entry_point(curve, tab[mc.SLOT * e:mc.SLOT * e + mc.SLOT]) == want[e], (name, W, divmod(e, H + 1))
            # the engine's route: its own scalars through the chain, the affine pass and the entry conversion
            sc = table_scalars(mb, curve, W)
            pick = list(range(E)) if W == 4 else sorted({i * (H + 1) + j for i in range(M) for j in (0, 1, H - 1, H, rnd.randrange(H + 1))})
            got = table_from_scalars(mb, curve, raw, b"".join(sc[32 * e:32 * e + 32] for e in pick))
            assert got == b"".join(tab[mc.SLOT * e:mc.SLOT * e + mc.SLOT] for e in pick), (name, W)


def test_entry_zero_is_the_neutral_element(mb):
    for curve, name, raw, p in table_points():
        M, H, E = mc.geometry(8)
        tab = mc.shim_table(curve, 8, raw)
        for i in range(M):
            slot = tab[mc.SLOT * i * (H + 1):mc.SLOT * i * (H + 1) + mc.SLOT]
            assert mc.entry_point(curve, slot) == (b.INF if curve else (0, 1)), (name, i)


@pytest.mark.parametrize("name", [n for n, _ in mc.te_base_points()])
def test_lane_over_the_full_case_list_te(mb, name):
    ks = [k for _, k in mc.case_scalars(0)]
    p = mc.te_point(name)
    raw = m.points_to_bytes([p])
    want = mc.te_expected(p, ks)
    assert mc.shim_mul(0, mc.DEFAULT_W, mc.shim_table(0, mc.DEFAULT_W, raw), ks) == want
    if name in ("subgroup point 1", "G+T4"):               # every width of the cases on a subgroup point and on the point of order 4 L
        for W in mc.WINDOWS:
            assert mc.shim_mul(0, W, mc.shim_table(0, W, raw), ks) == want, W


def test_lane_over_the_full_case_list_bls377(mb):
    ks = [k for _, k in mc.case_scalars(1)]
    for name, raw, p in mc.bls_base_points():
        want = mc.bls_expected(p, ks)
        assert want.count(bytes(96)) >= 3                  # 0, r, 2 r: infinity as zeros
        assert mc.shim_mul(1, mc.DEFAULT_W, mc.shim_table(1, mc.DEFAULT_W, raw), ks) == want, name
    _, raw, p = mc.bls_base_points()[1]
    for W in mc.WINDOWS:
        assert mc.shim_mul(1, W, mc.shim_table(1, W, raw), ks) == mc.bls_expected(p, ks), W


def test_bls377_infinity_inside_the_affine_groups(mb):
    _, raw, p = mc.bls_base_points()[0]
    tab = mc.shim_table(1, mc.DEFAULT_W, raw)
    for n in (1, 7, 8, 9, 17):
        for what, ks in mc.bls_infinity_plans(n):
            want = mc.bls_expected(p, ks)
            assert want.count(bytes(96)) >= 1
            assert mc.shim_mul(1, mc.DEFAULT_W, tab, ks) == want, (n, what)


def test_random_scalars_both_curves(mb):
    rnd = random.Random(0xF1BA)
    ks = [rnd.getrandbits(256) for _ in range(100)]
    p = mc.te_point("subgroup point 2")
    assert mc.shim_mul(0, 8, mc.shim_table(0, 8, m.points_to_bytes([p])), ks) == mc.te_expected(p, ks)
    _, raw, q = mc.bls_base_points()[0]
    assert mc.shim_mul(1, 8, mc.shim_table(1, 8, raw), ks[:40]) == mc.bls_expected(q, ks[:40])


def test_montgomery_scalars_are_decoded(mb):
    rnd = random.Random(0x3047)
    for curve in (0, 1):
        mod = mc.scalar_modulus(curve)
        ks = [0, 1, mod - 1, 12345] + [rnd.randrange(mod) for _ in range(12)]
        recs = [k * mc.R256 % mod for k in ks] + [mod, mc.TOP, 1, rnd.getrandbits(256)]       # any 256-bit record stands for its residue
        decoded = [mc.montgomery_decode(curve, a) for a in recs]
        assert decoded[:len(ks)] == ks
        if curve:
            _, raw, p = mc.bls_base_points()[0]
            want = mc.bls_expected(p, decoded)
        else:
            p = mc.te_point("subgroup point 0")
            raw, want = m.points_to_bytes([p]), mc.te_expected(p, decoded)
        for W in (8, mc.DEFAULT_W):
            tab = mc.shim_table(curve, W, raw)
            assert mc.shim_mul(curve, W, tab, recs, form=1) == want, (curve, W)
            assert mc.shim_mul(curve, W, tab, recs, form=0) != want


def test_deliberate_mistakes_are_caught(mb):
    """each mistake changes the answer on the case list (the shim's variants, or wrong inputs to the exact code); the unmodified run passes"""
    for curve in (0, 1):
        ks = [k for _, k in mc.case_scalars(curve)]
        if curve:
            _, raw, p = mc.bls_base_points()[0]
            want = mc.bls_expected(p, ks)
        else:
            p = mc.te_point("G+T4")                         # order 4 L: a scalar reduced mod anything smaller shows
            raw, want = m.points_to_bytes([p]), mc.te_expected(p, ks)
        W = 8
        M, H, E = mc.geometry(W)
        tab = mc.shim_table(curve, W, raw)
        assert mc.shim_mul(curve, W, tab, ks) == want
        caught = {}
        try:
            for variant, what in ((1, "a table off by one entry"), (2, "the sign dropped")):
                mb.mbc_set_variant(variant)
                caught[what] = mc.shim_mul(curve, W, tab, ks) != want
        finally:
            mb.mbc_set_variant(0)
        # the top window's scalars j 2^(W (M - 1)) cut to 256 bits instead of reduced mod the group's exponent
        sc = bytearray(table_scalars(mb, curve, W))
        top = (M - 1) * (H + 1)
        for j in range(H + 1):
            sc[32 * (top + j):32 * (top + j) + 32] = ((j << (W * (M - 1))) % mc.R256).to_bytes(32, "little")
        bad_top = table_from_scalars(mb, curve, raw, bytes(sc[32 * top:]))
        assert bad_top[:mc.SLOT] == tab[mc.SLOT * top:mc.SLOT * (top + 1)] and bad_top != tab[mc.SLOT * top:]   # (j = 0 alone stays below 2^256)
        caught["the top window's scalars not reduced"] = mc.shim_mul(curve, W, tab[:mc.SLOT * top] + bad_top, ks) != want
        caught["C of the wrong W"] = mc.shim_mul(curve, W, tab, ks, C=mc.offset(4)) != want
        assert mc.shim_mul(curve, W, tab, ks, C=mc.offset(W)) == want
        assert caught == {what: True for what in caught} and len(caught) == 4, (curve, caught)


def test_lane_code_under_address_and_undefined_behaviour_sanitizers():
    """tests/sanitize/san_mul_base.cpp: a stand-alone program (its own main, no Python) over the shim, built with
    -fsanitize=address,undefined; a sanitizer report aborts it"""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    d = os.path.join(ROOT, "tests", "sanitize")
    os.makedirs(os.path.join(d, "_build"), exist_ok=True)
    exe = os.path.join(d, "_build", "san_mul_base")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", exe, os.path.join(d, "san_mul_base.cpp")])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, env=env, timeout=300)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in out and "san_mul_base: all checks passed" in out, out[-4000:]


# ---- the public names ---------------------------------------------------------------------------------------------------------------
NEW_FUNCS = ("te_msm_bind_base", "te_msm_release_base", "te_msm_mul_base", "te_msm_mul_base_device", "te_msm_base_read")


def test_header_declares_the_fixed_base_entry_points(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name in NEW_FUNCS:
        assert re.search(r"\bint(64_t)?\s+%s\s*\(" % name, hdr), name
    assert "typedef struct te_base te_base;" in hdr
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "te_msm.h"\n#include <stddef.h>\n'
                   "int (*f1)(te_ctx*, const uint8_t*, te_base**) = te_msm_bind_base;\n"
                   "int (*f2)(te_ctx*, te_base*) = te_msm_release_base;\n"
                   "int (*f3)(te_ctx*, te_base*, const uint8_t*, uint64_t, uint8_t*) = te_msm_mul_base;\n"
                   "int (*f4)(te_ctx*, te_base*, const void*, uint64_t, void*) = te_msm_mul_base_device;\n"
                   "int64_t (*f5)(te_ctx*, const te_base*, int, uint32_t, uint32_t, uint32_t, void*, uint64_t, int*) = te_msm_base_read;\n"
                   "int main(void) { return f1 && f2 && f3 && f4 && f5 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "use.o"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


def test_library_and_package_export_the_fixed_base_entry_points(pkg):
    for meth in ("bind_base", "release_base", "mul_base", "mul_base_device", "base_read"):
        assert callable(getattr(pkg.MsmContext, meth, None)), meth
    assert hasattr(pkg, "Base")
    r = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    if r.returncode != 0:
        pytest.skip("no nm")
    syms = set(re.findall(r"\bT\s+(\w+)", r.stdout.decode()))
    for name in NEW_FUNCS:
        assert name in syms, name


def test_node_module_exports_the_fixed_base_calls():
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    src = open(os.path.join(js, "compute_msm.js")).read()
    assert re.search(r"module\.exports\s*=\s*\{[^}]*\bsetBase\b[^}]*\bscalarMulBase\b", src)
    dts = open(os.path.join(js, "submission.d.ts")).read()
    assert "export declare const setBase: (point: Buffer) => void;" in dts
    assert "export declare const scalarMulBase: (scalars: Buffer) => Buffer;" in dts
    addon = open(os.path.join(js, "addon.cc")).read()
    assert '{"setBase", SetBase}' in addon and '{"scalarMulBase", ScalarMulBase}' in addon
