"""Polynomial openings without a device: the per-lane code of csrc/poly.hip.hpp and the plan of csrc/poly_plan.hpp, compiled for the host
(tests/csrc/polycheck.cpp).  The model (the recurrence, in Python integers) is pinned to the definition by direct summation; the emulated
call equals the model byte for byte at chunk 1, 4 and the default, at every length around a lane row, a tile and a tile of tiles; the plan's
levels change where the test says; every index of the plan stays inside its allocation up to 2^30; refusals; five deliberate mistakes,
each caught; and the same emulation under sanitizers as a program of its own.  The same code runs on the device in tests/test_gpu_poly.py."""
import ctypes
import os
import re
import subprocess

import pytest

import poly_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = pc.P


@pytest.fixture(scope="module")
def L():
    return pc.shim()


@pytest.fixture(scope="module")
def chunks(L):
    return sorted({1, 4, pc.default_chunk(L)})


# ---- 1. the model -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64])
def test_model_equals_the_definition(n):
    for flags in (0, pc.MONTGOMERY, pc.SHARED_Z, pc.MONTGOMERY | pc.SHARED_Z):
        for which in pc.POINT_EXTREMES + (None,):
            a, z = pc.values(2 * n, seed=n), pc.points(1 if flags & pc.SHARED_Z else 2, n, which)
            got = pc.model(a, n, z, 2, flags)
            assert got == pc.model(a, n, z, 2, flags, how=pc.direct)
            assert pc.closing_check(a, n, z, 2, flags, *got)


def test_closing_check_tells_a_wrong_quotient():
    a, z, ev, q = pc.expected(64, 1, 0, 5)
    assert pc.closing_check(a, 64, z, 1, 0, ev, q)
    bad = bytearray(q)
    bad[32 * 10] ^= 1
    assert not pc.closing_check(a, 64, z, 1, 0, ev, bytes(bad))
    assert not pc.closing_check(a, 64, z, 1, 0, ev, q[:-32] + pc.pack([1], 32))
    assert not pc.closing_check(a, 64, z, 1, 0, pc.pack([(pc.unpack(ev, 32)[0] + 1) % P], 32), q)


# ---- 2. the emulated call against the model ---------------------------------------------------------------------------------------
def run_case(L, n, count, flags, chunk, seed, which=None):
    """with the quotient out of place and in place, evaluation only, and the quotient only"""
    a, z, ev, q = pc.expected(n, count, flags, seed, which)
    keep = bytes([0xA5])
    assert pc.emulate(L, a, n, z, count, flags, chunk)[:3] == (0, ev, q), ("out of place", n, count, flags, chunk)
    assert pc.emulate(L, a, n, z, count, flags, chunk, in_place=True)[:3] == (0, ev, q), ("in place", n, count, flags, chunk)
    assert pc.emulate(L, a, n, z, count, flags, chunk, quotient=False)[:3] == (0, ev, keep * len(a)), ("evaluation only", n, count, flags, chunk)
    assert pc.emulate(L, a, n, z, count, flags, chunk, evals=False)[:3] == (0, keep * (32 * count), q), ("quotient only", n, count, flags, chunk)


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("flags", [0, pc.MONTGOMERY, pc.SHARED_Z, pc.MONTGOMERY | pc.SHARED_Z])
def test_emulation_equals_the_model(L, chunks, count, flags):
    for chunk in chunks:
        T = pc.LANES * chunk
        for n in pc.lengths(T, squares=chunk == 1):
            if n > 4 * T and (count == 3) != bool(flags & pc.SHARED_Z):   # the squares: count 1 with a point each, count 3 with a shared one
                continue
            run_case(L, n, count, flags, chunk, seed=chunk)


@pytest.mark.parametrize("which", pc.POINT_EXTREMES)
def test_points_at_the_extremes(L, chunks, which):
    """z = 0, 1, p - 1, p, 2^256 - 1 as the first polynomial's point (and as the shared one), over one tile, a partly filled one and two levels"""
    for chunk in chunks:
        T = pc.LANES * chunk
        for n in (1, 257, T + 1, 2 * T + 300):
            for flags in (0, pc.MONTGOMERY | pc.SHARED_Z):
                run_case(L, n, 2, flags, chunk, seed=11, which=which)
    a0, z0, ev0, q0 = pc.expected(300, 1, 0, 3, 0)
    ap, zp, evp, qp = pc.expected(300, 1, 0, 3, P)
    assert a0 == ap and (ev0, q0) == (evp, qp)                       # z = 0 and z = p are one point
    assert pc.unpack(ev0, 32)[0] == pc.unpack(a0, 32)[0] % P


def test_coefficient_extremes_sit_in_the_first_tile():
    v = pc.unpack(pc.values(64), 32)
    assert {0, 1, P - 1, P, P + 1, (1 << 256) - 1} <= set(v)


def test_every_chunk_runs(L):
    """chunk is a run-time argument: every value from 1 to the largest, two levels and a partly filled last tile"""
    for chunk in range(1, pc.CHUNK_MAX + 1):
        n = pc.LANES * chunk + 77
        a, z, ev, q = pc.expected(n, 1, pc.MONTGOMERY, 21)
        assert pc.emulate(L, a, n, z, 1, pc.MONTGOMERY, chunk, in_place=True)[:3] == (0, ev, q), chunk
    assert pc.plan_info(L, 1000, chunk=pc.CHUNK_MAX + 1)["levels"] == 0      # refused by the plan; a call falls back to the default


def test_short_polynomials_fill_their_tiles(L):
    """a call runs at the chunk in force, but at no more than one tile needs to cover n: 2^10 coefficients at chunk 8 run at chunk 4"""
    for n, chunk, want in ((1, 8, 1), (256, 8, 1), (257, 8, 2), (1024, 8, 4), (1792, 8, 7), (1793, 8, 8), (2048, 8, 8), (2049, 8, 8), (1 << 30, 16, 16), (300, 1, 1)):
        assert L.poly_chunk_for(n, chunk) == want, (n, chunk)
    a, z, ev, q = pc.expected(1024, 3, 0, 77)
    assert pc.emulate(L, a, 1024, z, 3, 0, 8, in_place=True)[:3] == (0, ev, q)
    assert pc.emulate(L, a, 1024, z, 3, 0, 8, mistake=pc.M_LAST)[2] != q


# ---- 3. the plan ------------------------------------------------------------------------------------------------------------------
def test_levels_change_at_the_powers_of_the_tile(L, chunks):
    """1 level up to T, 2 up to T^2, 3 up to T^3, 4 above (chunk 1 alone gets there below 2^30: from 2^24 + 1)"""
    for chunk in chunks:
        T = pc.LANES * chunk
        for k in (1, 2, 3):
            if T ** k <= pc.MAX_N:
                assert pc.plan_info(L, T ** k, chunk=chunk)["levels"] == k, (chunk, k)
            if T ** k + 1 <= pc.MAX_N:
                info = pc.plan_info(L, T ** k + 1, chunk=chunk)
                assert info["levels"] == k + 1 and info["tiles"][-1] == 1 and info["n"][-1] == 2, (chunk, k)
    assert pc.plan_info(L, (1 << 24) + 1, chunk=1)["levels"] == 4 == pc.plan_info(L, pc.MAX_N, chunk=1)["levels"]
    assert pc.plan_info(L, pc.MAX_N, chunk=4)["levels"] == 3 == pc.plan_info(L, pc.MAX_N, chunk=pc.CHUNK_MAX)["levels"]


def test_the_deepest_recursion_runs_in_full(L):
    """At chunk 4 (T = 1024) no call up to 2^30 goes deeper than three levels, and T^2 + 1 -- run here in full against the model -- has
    three.  Chunk 1 reaches three levels at 65 537 (run in full above, in every form); its fourth needs 2^24 + 1 coefficients and is
    covered by the bounds replay alone: the levels are one loop over one kernel pair, whatever their number."""
    T = 1024
    n = T * T + 1
    assert pc.plan_info(L, n, chunk=4)["levels"] == 3 == max(pc.plan_info(L, m, chunk=4)["levels"] for m in (pc.MAX_N, pc.MAX_N - 1, T ** 3))
    a, z, ev, q = pc.expected(n, 1, 0, 4)
    assert pc.emulate(L, a, n, z, 1, 0, 4, in_place=True)[:3] == (0, ev, q)
    assert pc.plan_info(L, 65537, chunk=1)["levels"] == 3


def test_bounds_replay(L):
    """every global, scratch and LDS index, by arithmetic alone: n at the level boundaries +- 1 up to TE_MSM_POLY_MAX_N, count 1 .. 3"""
    checked = ctypes.c_uint64()
    for chunk in (1, 4, pc.default_chunk(L), pc.CHUNK_MAX):
        T = pc.LANES * chunk
        ns = {1, 2, 255, 256, 257, pc.MAX_N - 1, pc.MAX_N}
        for k in (1, 2, 3):
            ns |= {T ** k - 1, T ** k, T ** k + 1}
        for n in sorted(x for x in ns if 1 <= x <= pc.MAX_N):
            for count in (1, 2, 3) if n < pc.MAX_N // 2 else (1, 3):
                assert L.poly_replay(n, count, chunk, count == 2, ctypes.byref(checked)) == 0, (chunk, n, count)
                assert checked.value >= 2 * T + 4 * count * -(-n // T)
    assert L.poly_replay(pc.MAX_N + 1, 1, 1, 0, ctypes.byref(checked)) == pc.BOUNDS      # the plan refuses what the call refuses
    assert L.poly_replay(0, 1, 1, 0, ctypes.byref(checked)) == pc.BOUNDS


def test_scratch_is_about_a_record_a_tile(L):
    for chunk in (1, 8):
        T = pc.LANES * chunk
        for n, count in ((1, 1), (T, 3), (T + 1, 3), (1 << 20, 1), (1 << 24, 2)):
            info = pc.plan_info(L, n, count, chunk)
            assert info["records"] == count * sum(info["tiles"]) and info["records"] <= count * (-(-n // T) + -(-n // (T * T)) + 3)
            assert info["scratch_bytes"] == 32 * info["records"] + count * info["levels"] * 18 * 48
            assert info["lds_bytes"] == 4 * (256 * (8 * chunk + 4) + 256 * 9)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs(L):
    a, z = pc.values(16), pc.points(2)
    keep_q, keep_e = bytes([0xA5]) * len(a), bytes([0xA5]) * 64
    for kwargs, n, count, flags, why in (
            (dict(), 0, 2, 0, pc.POLY_BAD_N),
            (dict(), pc.MAX_N + 1, 2, 0, pc.POLY_BAD_N),
            (dict(), 8, 2, 4, pc.POLY_BAD_FLAGS),
            (dict(), 8, 2, -1, pc.POLY_BAD_FLAGS),
            (dict(null="a"), 8, 2, 0, pc.POLY_NULL),
            (dict(null="z"), 8, 2, 0, pc.POLY_NULL),
            (dict(evals=False, quotient=False), 8, 2, 0, pc.POLY_NO_OUTPUT),
            (dict(), 8, 2, 0, None)):
        rc, ev, q, reason = pc.emulate(L, a, n, z, count, flags, **kwargs)
        if why is None:
            assert rc == 0 and (ev, q) == pc.model(a, n, z, count, flags)       # ... and the same buffers are accepted when nothing is wrong
        else:
            assert (rc, reason, ev, q) == (pc.EINVAL, why, keep_e, keep_q), (n, count, flags, kwargs)
    src, zb, out, why = ctypes.create_string_buffer(a, len(a)), ctypes.create_string_buffer(z, len(z)), ctypes.create_string_buffer(keep_q, len(a)), ctypes.c_int()
    rc = L.poly_emulate(ctypes.addressof(src), 1 << 30, 1 << 30, ctypes.addressof(zb), 0, 0, 0, None, ctypes.addressof(out), ctypes.byref(why))      # count x n x 32 = 2^65
    assert (rc, why.value, out.raw) == (pc.EINVAL, pc.POLY_TOO_LARGE, keep_q)
    assert pc.emulate(L, b"", 8, b"", 0, 0, null="a")[0] == 0                   # count = 0 succeeds and touches nothing


# ---- 5. deliberate mistakes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", [pc.M_CARRY, pc.M_POINT, pc.M_FULL_TILE, pc.M_UNSHIFTED, pc.M_LAST])
def test_deliberate_mistakes_are_caught(L, mistake):
    for chunk, n, count in ((1, 2 * 256 + 300, 3), (4, 2 * 1024 + 300, 1)):
        a, z, ev, q = pc.expected(n, count, 0, 30 + mistake)
        assert pc.emulate(L, a, n, z, count, 0, chunk)[:3] == (0, ev, q)
        rc, gev, gq, _ = pc.emulate(L, a, n, z, count, 0, chunk, mistake=mistake)
        assert rc == 0 and (gev, gq) != (ev, q), (mistake, chunk)
        assert not pc.closing_check(a, n, z, count, 0, gev, gq), (mistake, chunk)


# ---- 6. the emulation under sanitizers: a program of its own ----------------------------------------------------------------------------
def test_emulation_under_sanitizers(tmp_path):
    exe = str(tmp_path / "san_poly")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "csrc", "san_poly.cpp")])      # (the runtimes linked in: the program's environment stays as it is)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "san_poly ok" in r.stdout, r.stdout[-2000:]


# ---- 7. the names -----------------------------------------------------------------------------------------------------------------
def test_names_in_header_and_package(pkg):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name, val in (("TE_MSM_POLY_MONTGOMERY", "1"), ("TE_MSM_POLY_SHARED_Z", "2"), ("TE_MSM_POLY_MAX_N", "(1ull << 30)"), ("TE_MSM_POLY_CHUNK", "%du" % pc.default_chunk(pc.shim()))):
        assert re.search(r"#define %s +%s(?![0-9])" % (name, re.escape(val)), hdr), name
    assert "te_msm_poly_divide(" in hdr and "te_msm_poly_divide_device(" in hdr
    assert (pkg.POLY_MONTGOMERY, pkg.POLY_SHARED_Z, pkg.POLY_MAX_N) == (pc.MONTGOMERY, pc.SHARED_Z, pc.MAX_N)
    assert callable(pkg.MsmContext.poly_divide) and callable(pkg.MsmContext.poly_divide_device)
