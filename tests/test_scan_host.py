"""Prefix sums and products without a device: the per-lane code of csrc/scan.hip.hpp and the plan of csrc/scan_plan.hpp, compiled for the
host (tests/csrc/scancheck.cpp).  The emulated call equals the model (Python integers, straight from the definition) byte for byte at chunk
1, 4 and the default and once at every chunk, at every length around a lane row, a tile and a tile of tiles, for both ops, modes and forms,
with and without a seed and each output, in place and out of place, and under SHARED_A; the extremes, zeros among a product's factors and
the sum's worst magnitude; every index of the plan stays inside its allocation up to 2^30; the documented intervals, replayed from the
plan's own reduction points; refusals; seven deliberate mistakes, each caught; and the same emulation under sanitizers as a program of its
own.  The same code runs on the device in tests/test_gpu_scan.py."""
import ctypes
import os
import re
import subprocess
from fractions import Fraction

import pytest

import scan_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = sc.P
KEEP = bytes([sc.FILL])


@pytest.fixture(scope="module")
def L():
    return sc.shim()


@pytest.fixture(scope="module")
def chunks(L):
    return sorted({1, 4, sc.default_chunk(L)})


# ---- 1. the model -----------------------------------------------------------------------------------------------------------------
def test_model_on_a_case_written_out():
    a = sc.pack([3, 5, 7, P + 2], 32)
    assert sc.model(sc.SUM, a, 4) == (sc.pack([3, 8, 15, 17], 32), sc.pack([17], 32))
    assert sc.model(sc.SUM, a, 4, flags=sc.EXCLUSIVE, init=sc.pack([10], 32)) == (sc.pack([10, 13, 18, 25], 32), sc.pack([27], 32))
    assert sc.model(sc.PRODUCT, a, 4) == (sc.pack([3, 15, 105, 210], 32), sc.pack([210], 32))
    assert sc.model(sc.PRODUCT, a, 2, 2, sc.EXCLUSIVE, sc.pack([2, P - 1], 32)) == (sc.pack([2, 6, P - 1, P - 7], 32), sc.pack([30, (7 * (P - 2)) % P], 32))
    g = sc.pack([3], 32)
    assert sc.model(sc.PRODUCT, g, 5, 1, sc.SHARED_A | sc.EXCLUSIVE) == (sc.pack([1, 3, 9, 27, 81], 32), sc.pack([243], 32))
    assert sc.model(sc.SUM, g, 3, 1, sc.SHARED_A, sc.pack([1], 32)) == (sc.pack([4, 7, 10], 32), sc.pack([10], 32))
    am = sc.pack([3 * sc.A % P, 5 * sc.A % P], 32)
    assert sc.model(sc.PRODUCT, am, 2, 1, sc.MONTGOMERY) == (sc.pack([3 * sc.A % P, 15 * sc.A % P], 32), sc.pack([15 * sc.A % P], 32))


# ---- 2. the emulated call against the model ---------------------------------------------------------------------------------------
def run_case(L, op, n, count, flags, chunk, seed, with_init=True, a=None):
    """out of place and in place, totals only, and out only"""
    if a is None:
        a, init, out, tot = sc.expected(op, n, count, flags, seed, with_init)
    else:
        init = sc.seeds(count, seed) if with_init else None
        out, tot = sc.model(op, a, n, count, flags, init)
    tag = (op, n, count, flags, chunk, with_init)
    assert sc.emulate(L, op, a, n, count, flags, chunk, init)[:3] == (0, out, tot), ("out of place",) + tag
    if not flags & sc.SHARED_A:
        assert sc.emulate(L, op, a, n, count, flags, chunk, init, in_place=True)[:3] == (0, out, tot), ("in place",) + tag
    assert sc.emulate(L, op, a, n, count, flags, chunk, init, want_out=False)[:3] == (0, KEEP * len(out), tot), ("totals only",) + tag
    assert sc.emulate(L, op, a, n, count, flags, chunk, init, want_totals=False)[:3] == (0, out, KEEP * (32 * count)), ("out only",) + tag


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("flags", sc.ALL_FLAGS)
@pytest.mark.parametrize("op", sc.OPS)
def test_emulation_equals_the_model(L, chunks, op, flags, count):
    for chunk in chunks:
        T = sc.LANES * chunk
        for n in sc.lengths(T, squares=chunk == 1):
            if n > 4 * T and (count == 3) != bool(flags & sc.MONTGOMERY):   # the squares: count 1 canonical, count 3 in the Montgomery form
                continue
            run_case(L, op, n, count, flags, chunk, seed=chunk, with_init=(n + count) % 2 == 0 or n > 4 * T)
    run_case(L, op, 300, count, flags, 0, seed=9, with_init=False)
    run_case(L, op, 2 * 256 + 300, count, flags, 1, seed=9, with_init=True)


@pytest.mark.parametrize("op", sc.OPS)
def test_every_chunk_runs(L, op):
    """chunk is a run-time argument: every value from 1 to the largest, two levels and a partly filled last tile"""
    for chunk in range(1, sc.CHUNK_MAX + 1):
        n = sc.LANES * chunk + 77
        flags = sc.MONTGOMERY | (sc.EXCLUSIVE if chunk & 1 else 0)
        a, init, out, tot = sc.expected(op, n, 1, flags, 21)
        assert sc.emulate(L, op, a, n, 1, flags, chunk, init, in_place=True)[:3] == (0, out, tot), chunk
    assert sc.plan_info(L, 1000, chunk=sc.CHUNK_MAX + 1)["levels"] == 0      # refused by the plan; a call falls back to the default


def test_the_deepest_recursion_runs_in_full(L):
    """At chunk 4 (T = 1024) no call up to 2^30 goes deeper than three levels, and T^2 + 1 -- run here in full against the model -- has
    three.  Chunk 1 reaches three levels at 65 537 (run in full above); its fourth needs 2^24 + 1 elements and is covered by the bounds
    replay alone: the levels are one loop over one kernel pair, whatever their number."""
    T = 1024
    n = T * T + 1
    assert sc.plan_info(L, n, chunk=4)["levels"] == 3 == max(sc.plan_info(L, x, chunk=4)["levels"] for x in (sc.MAX_N, sc.MAX_N - 1, T ** 3))
    for op, flags in ((sc.SUM, 0), (sc.PRODUCT, sc.EXCLUSIVE)):
        a, init, out, tot = sc.expected(op, n, 1, flags, 4)
        assert sc.emulate(L, op, a, n, 1, flags, 4, init, in_place=True)[:3] == (0, out, tot)
    assert sc.plan_info(L, 65537, chunk=1)["levels"] == 3


def test_short_vectors_fill_their_tiles(L):
    for n, chunk, want in ((1, 8, 1), (256, 8, 1), (257, 8, 2), (1024, 8, 4), (1792, 8, 7), (1793, 8, 8), (2048, 8, 8), (2049, 8, 8), (1 << 30, 16, 16), (300, 1, 1)):
        assert L.scan_chunk_for(n, chunk) == want, (n, chunk)


# ---- 3. values --------------------------------------------------------------------------------------------------------------------
def test_extremes_sit_in_the_first_tile():
    v = sc.unpack(sc.values(64), 32)
    assert {0, 1, P - 1, P, P + 1, (1 << 256) - 1} <= set(v)
    assert all(x % P for x in sc.unpack(sc.values(64, zero_free=True), 32))


@pytest.mark.parametrize("flags", [0, sc.MONTGOMERY | sc.EXCLUSIVE])
def test_extreme_records_and_seeds(L, chunks, flags):
    """0, 1, p - 1, p, p + 1, 2^256 - 1 as records (the sum's values() holds them all, zeros included) and each as the seed"""
    for chunk in chunks:
        T = sc.LANES * chunk
        for n in (257, T + 1):
            for e in (0, 1, P - 1, P, P + 1, (1 << 256) - 1):
                for op in sc.OPS:
                    a = sc.values(2 * n, 5, zero_free=op == sc.PRODUCT)
                    a = sc.with_record(sc.with_record(a, 3, e), n + n // 2, e) if e % P or op == sc.SUM else a
                    init = sc.pack([e, 7], 32)
                    out, tot = sc.model(op, a, n, 2, flags, init)
                    assert sc.emulate(L, op, a, n, 2, flags, chunk, init)[:3] == (0, out, tot), (chunk, n, e, op)


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_a_zero_among_the_factors(L, chunks, where):
    """a zero factor is an ordinary value: everything behind it is 0, everything in front is untouched, nothing inverts; 0 and p alike"""
    for chunk in chunks:
        T = sc.LANES * chunk
        for n in (2 * T + 300, 257):
            at = dict(first=0, middle=n // 2 + 1, last=n - 1)[where]
            for zero, flags in ((0, 0), (P, sc.EXCLUSIVE), (0, sc.MONTGOMERY | sc.EXCLUSIVE)):
                a = sc.with_record(sc.values(2 * n, 6, zero_free=True), n + at, zero)       # in the second vector of two
                run_case(L, sc.PRODUCT, n, 2, flags, chunk, seed=6, a=a)
                out, tot = sc.model(sc.PRODUCT, a, n, 2, flags, sc.seeds(2, 6))
                o, t = sc.unpack(out, 32), sc.unpack(tot, 32)
                assert t[0] != 0 and t[1] == 0 and all(o[:n + at])       # in front of the zero nothing is 0 ...
                assert not any(o[n + at + 1:])                          # ... and behind it everything is
                assert (o[n + at] == 0) == (not flags & sc.EXCLUSIVE)


def test_the_worst_magnitude_of_the_sum(L):
    """every record and the seed 2^256 - 1 over 2 T + 300 elements, at every chunk"""
    top = (1 << 256) - 1
    for chunk in range(1, sc.CHUNK_MAX + 1):
        n = 2 * sc.LANES * chunk + 300
        a, init = sc.pack([top] * n, 32), sc.pack([top], 32)
        for flags in (0, sc.EXCLUSIVE):
            want_tot = sc.pack([(n + 1) * top % P], 32)
            want_out = sc.pack([(i + (0 if flags else 1) + 1) * top % P for i in range(n)], 32)
            assert sc.emulate(L, sc.SUM, a, n, 1, flags, chunk, init)[:3] == (0, want_out, want_tot), (chunk, flags)
    a = sc.pack([top] * 3, 32)                                          # and as the one record of a shared vector, three levels at chunk 1
    n = 65537
    want = sc.pack([(i + 2) * top % P for i in range(n)] * 3, 32)
    assert sc.emulate(L, sc.SUM, a, n, 3, sc.SHARED_A, 1, sc.pack([top] * 3, 32))[:3] == (0, want, sc.pack([(n + 1) * top % P] * 3, 32))


# ---- 4. the plan ------------------------------------------------------------------------------------------------------------------
def test_levels_change_at_the_powers_of_the_tile(L, chunks):
    for chunk in chunks:
        T = sc.LANES * chunk
        for k in (1, 2, 3):
            if T ** k <= sc.MAX_N:
                assert sc.plan_info(L, T ** k, chunk=chunk)["levels"] == k, (chunk, k)
            if T ** k + 1 <= sc.MAX_N:
                info = sc.plan_info(L, T ** k + 1, chunk=chunk)
                assert info["levels"] == k + 1 and info["tiles"][-1] == 1 and info["n"][-1] == 2, (chunk, k)
    assert sc.plan_info(L, (1 << 24) + 1, chunk=1)["levels"] == 4 == sc.plan_info(L, sc.MAX_N, chunk=1)["levels"]
    assert sc.plan_info(L, sc.MAX_N, chunk=4)["levels"] == 3 == sc.plan_info(L, sc.MAX_N, chunk=sc.CHUNK_MAX)["levels"]


def test_bounds_replay(L):
    """every global, scratch and LDS index and every out record written once, by arithmetic alone: n at the level boundaries +- 1 up to
    TE_MSM_SCAN_MAX_N, count 1 .. 3 (count 2 under SHARED_A)"""
    checked = ctypes.c_uint64()
    for chunk in (1, 4, sc.default_chunk(L), sc.CHUNK_MAX):
        T = sc.LANES * chunk
        ns = {1, 2, 255, 256, 257, sc.MAX_N - 1, sc.MAX_N}
        for k in (1, 2, 3):
            ns |= {T ** k - 1, T ** k, T ** k + 1}
        for n in sorted(x for x in ns if 1 <= x <= sc.MAX_N):
            for count in (1, 2, 3) if n < sc.MAX_N // 2 else (1, 3):
                assert L.scan_replay(n, count, chunk, count == 2, ctypes.byref(checked)) == 0, (chunk, n, count)
                assert checked.value >= 2 * T + 4 * count * -(-n // T)
    assert L.scan_replay(sc.MAX_N + 1, 1, 1, 0, ctypes.byref(checked)) == sc.BOUNDS      # the plan refuses what the call refuses
    assert L.scan_replay(0, 1, 1, 0, ctypes.byref(checked)) == sc.BOUNDS


def test_scratch_is_about_a_record_a_tile(L):
    for chunk in (1, 8):
        T = sc.LANES * chunk
        for n, count in ((1, 1), (T, 3), (T + 1, 3), (1 << 20, 1), (1 << 24, 2)):
            info = sc.plan_info(L, n, count, chunk)
            assert info["records"] == count * (sum(info["tiles"]) + 1) and info["records"] <= count * (-(-n // T) + -(-n // (T * T)) + 4)
            assert info["scratch_bytes"] == 32 * info["records"]
            assert info["lds_bytes"] == 4 * (256 * (8 * chunk + 4) + 256 * 9) <= 160 * 1024


# ---- 5. the intervals of scan.hip.hpp's header, replayed from the plan's reduction points --------------------------------------------
R = Fraction(1 << 261, P)                  # in units of p: 438.8
RAW = Fraction(1 << 256, P)                # a 256-bit record: 13.72
R1 = Fraction((1 << 261) % P, P)           # R mod p: 0.79


def reduced(v):
    assert v < R, "a reduction's operand must be of class N below R"
    return v * R1 / R + 1


def stored(v):
    assert v < R, "9 limbs hold class N below R (a top limb below 2^29)"
    return v


def test_sum_intervals(L):
    pts = sc.reduction_points(L)
    for chunk in range(1, sc.CHUNK_MAX + 1):
        for level0 in (True, False):
            rec = RAW if level0 else Fraction(1)                         # scratch records are canonical
            lane = stored(chunk * rec)
            if pts["lane_total"]:
                lane = reduced(lane)
            v = lane
            for s in range(8):                                           # a tree / scan step doubles what a lane may hold
                v = stored(2 * v)
                if pts["steps"][s]:
                    v = reduced(v)
            for carry in (RAW, Fraction(1)):                             # a seed as given, or a scratch record
                t = stored(v + carry)
                assert reduced(t) < 2                                    # k_scan_totals' output: fo_words takes below 2 p
                h = reduced(t) if pts["prefix"] else t
                h = stored(h + chunk * rec)                              # the walk
                assert reduced(h) < 2
    assert pts["lane_total"] and pts["prefix"]                           # what the header documents
    with pytest.raises(AssertionError):                                  # ... and the bound does not hold without the lane's reduction
        stored(256 * 8 * RAW)


def test_product_intervals():
    out = RAW * 1 / R + 1                                                # a decoding product: a raw record x a canonical constant
    assert out < Fraction(104, 100)
    assert out * out / R + 1 < Fraction(101, 100)                        # a combine
    assert out * RAW / R + 1 < 2 and out < 2                             # encode with A = 2^256; internal words: fo_words takes below 2 p
    assert RAW < R and out < R                                           # every operand is of class N below R


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs(L):
    a = sc.values(16)
    keep_o, keep_t = KEEP * len(a), KEEP * 64
    for kwargs, op, n, count, flags, why in (
            (dict(), 2, 8, 2, 0, sc.SCAN_BAD_OP),
            (dict(), -1, 8, 2, 0, sc.SCAN_BAD_OP),
            (dict(), sc.SUM, 0, 2, 0, sc.SCAN_BAD_N),
            (dict(), sc.SUM, sc.MAX_N + 1, 2, 0, sc.SCAN_BAD_N),
            (dict(), sc.PRODUCT, 8, 2, 8, sc.SCAN_BAD_FLAGS),
            (dict(), sc.PRODUCT, 8, 2, -1, sc.SCAN_BAD_FLAGS),
            (dict(null_a=True), sc.SUM, 8, 2, 0, sc.SCAN_NULL),
            (dict(want_out=False, want_totals=False), sc.SUM, 8, 2, 0, sc.SCAN_NO_OUTPUT),
            (dict(in_place=True), sc.SUM, 8, 2, sc.SHARED_A, sc.SCAN_ALIAS),
            (dict(), sc.SUM, 8, 2, 0, None)):
        rc, out, tot, reason = sc.emulate(L, op, a, n, count, flags, out_len=len(a), **kwargs)
        if why is None:
            assert rc == 0 and (out, tot) == sc.model(op, a, n, count, flags)       # ... and the same buffers are accepted when nothing is wrong
        elif kwargs.get("in_place"):
            assert (rc, reason, out[:len(a)], tot) == (sc.EINVAL, why, a, keep_t)
        else:
            assert (rc, reason, out[:len(a)], tot) == (sc.EINVAL, why, keep_o, keep_t), (op, n, count, flags, kwargs)
    src, out, why = ctypes.create_string_buffer(a, len(a)), ctypes.create_string_buffer(keep_o, len(a)), ctypes.c_int()
    rc = L.scan_emulate(sc.SUM, ctypes.addressof(src), 1 << 30, 1 << 30, 0, 0, 0, None, None, ctypes.addressof(out), ctypes.byref(why))      # count x n x 32 = 2^65
    assert (rc, why.value, out.raw) == (sc.EINVAL, sc.SCAN_TOO_LARGE, keep_o)
    assert sc.emulate(L, sc.SUM, b"", 8, 0, 0, null_a=True)[0] == 0                 # count = 0 succeeds and touches nothing


# ---- 7. deliberate mistakes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake", [sc.M_CARRY, sc.M_UNSHIFTED, sc.M_NO_SEED, sc.M_SEED_EVERYWHERE, sc.M_ZERO_PAD, sc.M_NO_REDUCE, sc.M_INTERNAL_OUT])
def test_deliberate_mistakes_are_caught(L, mistake):
    op = sc.SUM if mistake == sc.M_NO_REDUCE else sc.PRODUCT
    ops = (op,) if mistake in (sc.M_NO_REDUCE, sc.M_ZERO_PAD, sc.M_INTERNAL_OUT) else sc.OPS
    for op in ops:
        for chunk, n, count in ((1, 2 * 256 + 300, 3), (4, 2 * 1024 + 300, 1)):
            if mistake == sc.M_NO_REDUCE:
                chunk, n = 8, 2 * 2048 + 300                                # the worst-case input
                a, init = sc.pack([(1 << 256) - 1] * (n * count), 32), sc.pack([(1 << 256) - 1] * count, 32)
                out, tot = sc.model(op, a, n, count, sc.EXCLUSIVE, init)
            else:
                a, init, out, tot = sc.expected(op, n, count, sc.EXCLUSIVE, 30 + mistake)
            assert sc.emulate(L, op, a, n, count, sc.EXCLUSIVE, chunk, init)[:3] == (0, out, tot)
            rc, gout, gtot, _ = sc.emulate(L, op, a, n, count, sc.EXCLUSIVE, chunk, init, mistake=mistake)
            assert rc == 0 and (gout, gtot) != (out, tot), (mistake, chunk, op)
            if mistake in (sc.M_NO_SEED, sc.M_INTERNAL_OUT, sc.M_NO_REDUCE):
                assert gout != out and gtot != tot, (mistake, chunk, op)
            elif mistake == sc.M_ZERO_PAD:
                assert gtot != tot, (mistake, chunk, op)                    # (the padding sits behind a vector's last element: only its total sees it)
            else:
                assert gout != out, (mistake, chunk, op)                    # (these leave the totals kernel alone)


# ---- 8. the emulation under sanitizers: a program of its own ----------------------------------------------------------------------------
def test_emulation_under_sanitizers(tmp_path):
    exe = str(tmp_path / "san_scan")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "csrc", "san_scan.cpp")])      # (the runtimes linked in: the program's environment stays as it is)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "san_scan ok" in r.stdout, r.stdout[-2000:]


# ---- 9. the names -----------------------------------------------------------------------------------------------------------------
def test_names_in_header_and_package(L, pkg):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    k = (ctypes.c_uint64 * 4)()
    L.scan_constants(k)
    assert [int(x) for x in k] == [sc.SUM, sc.PRODUCT, sc.MAX_N, sc.default_chunk(L)]
    for name, val in (("TE_MSM_SCAN_SUM", "0"), ("TE_MSM_SCAN_PRODUCT", "1"), ("TE_MSM_SCAN_MONTGOMERY", "1"), ("TE_MSM_SCAN_EXCLUSIVE", "2"), ("TE_MSM_SCAN_SHARED_A", "4"),
                      ("TE_MSM_SCAN_MAX_N", "(1ull << 30)"), ("TE_MSM_SCAN_CHUNK", "%du" % sc.default_chunk(L))):
        assert re.search(r"#define %s +%s(?![0-9])" % (name, re.escape(val)), hdr), name
    assert "te_msm_field_scan(" in hdr and "te_msm_field_scan_device(" in hdr
    assert (pkg.SCAN_SUM, pkg.SCAN_PRODUCT, pkg.SCAN_MONTGOMERY, pkg.SCAN_EXCLUSIVE, pkg.SCAN_SHARED_A, pkg.SCAN_MAX_N) == (sc.SUM, sc.PRODUCT, sc.MONTGOMERY, sc.EXCLUSIVE, sc.SHARED_A, sc.MAX_N)
    assert callable(pkg.MsmContext.field_scan) and callable(pkg.MsmContext.field_scan_device)
