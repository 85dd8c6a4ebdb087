"""Batched NTTs without a device: the per-lane code of csrc/ntt.hip.hpp and the plan of csrc/ntt_plan.hpp, compiled for the host
(tests/csrc/nttcheck.cpp).  The shim's textbook transform is pinned to Python integers; the emulated kernels equal it bit for bit at
every size up to the first one that runs the plan's largest number of passes; every index of the plan stays inside its allocation up
to 2^24; closed forms; refusals; and six deliberate mistakes, each caught.  The same code runs on the device in tests/test_gpu_ntt.py."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import ntt_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = nc.P


@pytest.fixture(scope="module")
def L():
    return nc.shim()


@pytest.fixture(scope="module")
def top(L):
    return nc.top_log_n(L)


def to_ints(raw):
    return nc.unpack(raw, 32)


# ---- 1. the root; the plan -------------------------------------------------------------------------------------------------------
def test_root_of_unity(L):
    w, order = ctypes.create_string_buffer(32), ctypes.c_uint32()
    L.ntt_root(ctypes.addressof(w), ctypes.byref(order))
    W = int.from_bytes(w.raw, "little")
    assert W == pow(22, (P - 1) >> 47, P) == 8065159656716812877374967518403273466521432693661810619979959746626482506078
    assert (P - 1) % (1 << 47) == 0 and (P - 1) % (1 << 48) != 0
    assert pow(W, 1 << 46, P) == P - 1 and pow(W, 1 << 47, P) == 1 and order.value == 47      # order exactly 2^47, by the shim's own squarings too


def test_plan_shape(L, top):
    """one pass up to the tile, the largest pass count first reached at or below 2^22, 2^24 reachable, small tables"""
    assert top <= 22
    for k in range(nc.MAX_LOG_N + 1):
        info = nc.plan_info(L, k)
        assert sum(info["r"]) == k and info["passes"] == max(1, len(info["r"])) and info["passes"] <= 3
        assert info["lds_bytes"] <= 64 << 10 and info["table_bytes"] <= 1 << 20
        assert (info["per_tile"] == 1024 >> k) if k <= 10 else (info["per_tile"] == 0 and min(info["r"]) >= 2 and max(info["r"]) <= 8)
        assert info["tmp_records"] == (0 if info["passes"] == 1 else 1 << k)


# ---- 2. the textbook transform against Python integers -----------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(0, 9))
def test_ref_equals_the_definition(L, log_n):
    a = nc.values(2 << log_n, seed=log_n)
    for flags in nc.FLAGS:
        for shift in nc.SHIFTS:
            assert nc.ref(L, a, log_n, 2, flags, shift) == nc.model(a, log_n, 2, flags, shift, transform=nc.naive), (flags, shift)


@pytest.mark.parametrize("log_n", range(9, 13))
def test_ref_equals_the_recursive_transform(L, log_n):
    a = nc.values(1 << log_n, seed=log_n)
    for flags in nc.FLAGS:
        for shift in nc.SHIFTS:
            assert nc.ref(L, a, log_n, 1, flags, shift) == nc.model(a, log_n, 1, flags, shift), (flags, shift)


def test_the_two_models_agree():
    v = to_ints(nc.values(64))
    v = [x % P for x in v]
    for inverse in (False, True):
        assert nc.naive(v, 6, inverse, 22) == nc.fast(v, 6, inverse, 22)


# ---- 3. the emulated kernels equal the textbook, bit for bit -----------------------------------------------------------------------
def test_top_size_is_the_first_of_three_passes(L, top):
    assert top == 17 and nc.plan_info(L, top)["passes"] == 3 and nc.plan_info(L, top - 1)["passes"] == 2


@pytest.mark.parametrize("log_n", range(0, 18))
def test_emulation_equals_ref(L, log_n):
    """count 1, 2, 3; every direction, form and shift at count 1, coming round over the sizes at 2 and 3; in place and out of place"""
    for count in (1, 2, 3):
        a = nc.values(count << log_n, seed=log_n)
        combos = [(f, s) for f in nc.FLAGS for s in nc.SHIFTS]
        if count > 1 or log_n > 13:                                 # (the large sizes take three of the twelve, different ones each)
            combos = [combos[(5 * log_n + 3 * k + count) % 12] for k in range(3 if count == 1 else 2 if log_n <= 13 else 1)]
        for k, (flags, shift) in enumerate(combos):
            want = nc.ref(L, a, log_n, count, flags, shift)
            assert nc.emulate(L, a, log_n, count, flags, shift, in_place=bool(k & 1))[:2] == (0, want), (log_n, count, flags, shift)


@pytest.mark.parametrize("log_n", range(0, 5))
def test_emulation_batch_counts_around_a_block(L, log_n):
    per_tile = nc.plan_info(L, log_n)["per_tile"]
    for k, count in enumerate(nc.batch_counts(per_tile)):
        flags, shift = nc.FLAGS[k % 4], nc.SHIFTS[k % 3]
        a = nc.values(count << log_n, seed=log_n)
        assert nc.emulate(L, a, log_n, count, flags, shift, in_place=bool(k & 1))[:2] == (0, nc.ref(L, a, log_n, count, flags, shift)), (log_n, count)


def test_emulation_in_pieces(L):
    """the piece loop (a device call reaches it above 2^24 elements): 5 (3) transforms in pieces of 2, at one, two and three passes"""
    for log_n, count in ((4, 5), (12, 5), (17, 3)):
        a = nc.values(count << log_n, seed=99)
        want = nc.ref(L, a, log_n, count, nc.INVERSE, 22)
        for in_place in (False, True) if log_n < 17 else (True,):
            assert nc.emulate(L, a, log_n, count, nc.INVERSE, 22, piece=2, in_place=in_place)[:2] == (0, want)


def test_raw_values_at_and_above_p(L):
    for log_n in (0, 2, 11):
        n = 1 << log_n
        raw = ([(1 << 256) - 1, P, P + 1, 0] * n)[:n]
        for flags in nc.FLAGS:
            a = nc.pack(raw, 32)
            want = nc.model(a, log_n, 1, flags, P + 22)
            assert nc.ref(L, a, log_n, 1, flags, P + 22) == want and nc.emulate(L, a, log_n, 1, flags, P + 22)[:2] == (0, want)
            assert all(x < P for x in to_ints(want))                # canonical outputs


# ---- 4. every index inside its allocation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n", range(0, nc.MAX_LOG_N + 1))
def test_bounds_replay(L, log_n):
    checked = ctypes.c_uint64()
    assert L.ntt_replay(log_n, 1, ctypes.byref(checked)) == 0
    assert checked.value >= 2048 + (2 << log_n)                     # at least: every slot of a tile stored and read, every record read and written


def test_bounds_replay_with_batches_and_pieces(L):
    checked = ctypes.c_uint64()
    for log_n, count in ((0, 1), (0, 1025), (3, 127), (3, 129), (10, 3), (11, 3), (17, 2), (23, 3)):
        assert L.ntt_replay(log_n, count, ctypes.byref(checked)) == 0, (log_n, count)


# ---- 5. closed forms, every output checked ----------------------------------------------------------------------------------------
CLOSED = (0, 1, 5, 10, 11, 13, 16, 17)


@pytest.mark.parametrize("log_n", CLOSED)
def test_all_ones_and_deltas(L, log_n):
    n, w = 1 << log_n, nc.omega(log_n)
    out = to_ints(nc.emulate(L, nc.pack([1] * n, 32), log_n)[1])
    assert out == [n % P] + [0] * (n - 1)
    k, s = (n - 1) | 1 if n > 1 else 0, 22
    k %= n
    delta = [0] * n
    delta[k] = 1
    out = to_ints(nc.emulate(L, nc.pack(delta, 32), log_n, shift=s)[1])
    sk, wk, t, want = pow(s, k, P), pow(w, k, P), 1, []
    for j in range(n):                                              # s^k w^(j k)
        want.append(sk * t % P)
        t = t * wk % P
    assert out == want


@pytest.mark.parametrize("log_n", CLOSED)
def test_geometric_sequence(L, log_n):
    """a_i = c^i: out[j] (c s w^j - 1) == (c s)^n - 1, at every j"""
    n, w, c, s = 1 << log_n, nc.omega(log_n), 0x1234567, 22
    a, t = [], 1
    for _ in range(n):
        a.append(t)
        t = t * c % P
    out = to_ints(nc.emulate(L, nc.pack(a, 32), log_n, shift=s)[1])
    rhs, x = (pow(c * s, n, P) - 1) % P, c * s % P
    for j in range(n):
        assert out[j] * (x - 1) % P == rhs, j
        x = x * w % P


@pytest.mark.parametrize("log_n", CLOSED)
def test_inverse_undoes_forward(L, log_n):
    a = nc.pack([v % P for v in to_ints(nc.values(2 << log_n, seed=7))], 32)
    for mont in (0, nc.MONTGOMERY):
        for shift in nc.SHIFTS if log_n < 16 else nc.SHIFTS[mont >> 1:mont + 1]:      # (the large sizes: plain without a shift, Montgomery with 22 and a raw one)
            rc, fwd, _ = nc.emulate(L, a, log_n, 2, mont, shift)
            assert rc == 0 and nc.emulate(L, fwd, log_n, 2, mont | nc.INVERSE, shift, in_place=True)[:2] == (0, a)


def test_convolution_theorem(L):
    rnd = random.Random(64)
    f, g = [rnd.randrange(P) for _ in range(32)], [rnd.randrange(P) for _ in range(32)]
    want = [0] * 64
    for i, x in enumerate(f):
        for j, y in enumerate(g):
            want[i + j] = (want[i + j] + x * y) % P
    ev = to_ints(nc.emulate(L, nc.pack(f + [0] * 32 + g + [0] * 32, 32), 6, 2)[1])
    prod = nc.pack([x * y % P for x, y in zip(ev[:64], ev[64:])], 32)
    assert to_ints(nc.emulate(L, prod, 6, 1, nc.INVERSE)[1]) == want


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output(L):
    a = nc.values(8)
    untouched = bytes([0xA5]) * len(a)
    NTT_BAD_LOG_N, NTT_BAD_FLAGS, NTT_TOO_LARGE, NTT_NULL, NTT_ZERO_SHIFT = range(1, 6)
    for log_n, count, flags, shift, why in ((25, 1, 0, None, NTT_BAD_LOG_N), (1 << 31, 1, 0, None, NTT_BAD_LOG_N), (3, 1, 4, None, NTT_BAD_FLAGS),
                                            (3, 1, 1 << 30, None, NTT_BAD_FLAGS), (3, 1, 0, 0, NTT_ZERO_SHIFT), (3, 1, nc.INVERSE, 0, NTT_ZERO_SHIFT),
                                            (3, 1, 0, P, NTT_ZERO_SHIFT), (3, 1, nc.INVERSE | nc.MONTGOMERY, 3 * P, NTT_ZERO_SHIFT), (24, 1 << 40, 0, None, NTT_TOO_LARGE)):
        assert nc.emulate(L, a, log_n, count, flags, shift) == (nc.EINVAL, untouched, why), (log_n, count, flags, shift)
    assert nc.emulate(L, a, 3, 1, null="a") == (nc.EINVAL, untouched, NTT_NULL)
    assert nc.emulate(L, a, 3, 1, null="out")[::2] == (nc.EINVAL, NTT_NULL)
    assert nc.emulate(L, a, 3, 0, null="a") == (0, untouched, 0)   # count = 0 succeeds and touches nothing
    assert nc.emulate(L, a, 3, 1)[0] == 0


# ---- 7. deliberate mistakes, each refused ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mistake,log_n,flags,shift", [
    (nc.M_ROOT, 3, 0, None), (nc.M_ROOT, 12, nc.INVERSE, None),
    (nc.M_SCALE, 5, nc.INVERSE, None), (nc.M_SCALE, 11, nc.INVERSE | nc.MONTGOMERY, 22),
    (nc.M_BITREV, 2, 0, None), (nc.M_BITREV, 17, 0, None),
    (nc.M_SHIFT_AFTER, 4, 0, 22), (nc.M_SHIFT_AFTER, 11, nc.INVERSE, 22),
    (nc.M_TWIDDLE, 11, 0, None), (nc.M_TWIDDLE, 17, nc.INVERSE, None),
    (nc.M_SPLIT, 13, 0, None), (nc.M_SPLIT, 17, 0, None),
])
def test_deliberate_mistakes_are_caught(L, mistake, log_n, flags, shift):
    a = nc.values(1 << log_n, seed=mistake)
    want = nc.ref(L, a, log_n, 1, flags, shift)
    assert nc.emulate(L, a, log_n, 1, flags, shift)[:2] == (0, want)
    rc, got, _ = nc.emulate(L, a, log_n, 1, flags, shift, mistake=mistake)
    assert rc == 0 and got != want
    if mistake == nc.M_TWIDDLE:                                     # one index in every twiddled pass: each spoils one line of every later pass, nothing else
        r = nc.plan_info(L, log_n)["r"]
        assert 0 < sum(x != y for x, y in zip(to_ints(got), to_ints(want))) <= sum(1 << sum(r[k:]) for k in range(1, len(r)))


# ---- 8. the same emulation under the sanitizers ----------------------------------------------------------------------------------------
def test_emulation_under_sanitizers(tmp_path):
    exe = str(tmp_path / "san_ntt")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "san_ntt.cpp")])
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, env=env)
    assert r.returncode == 0 and "san_ntt ok" in r.stdout, r.stdout[-2000:]


# ---- 9. the names ----------------------------------------------------------------------------------------------------------------------
def test_names_in_header_library_package_and_addon(pkg):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name, val in (("TE_MSM_NTT_INVERSE", "1"), ("TE_MSM_NTT_MONTGOMERY", "2"), ("TE_MSM_NTT_MAX_LOG_N", "24u")):
        assert re.search(r"#define %s +%s(?![0-9])" % (name, re.escape(val)), hdr), name
    assert str(nc.W) in hdr and "ntt_table_bytes" in hdr and "ntt_scratch_bytes" in hdr and "ntt_max_log_n" in hdr
    lib = ctypes.CDLL(pkg.library_path())
    assert hasattr(lib, "te_msm_ntt") and hasattr(lib, "te_msm_ntt_device")
    assert (pkg.NTT_INVERSE, pkg.NTT_MONTGOMERY, pkg.NTT_MAX_LOG_N) == (nc.INVERSE, nc.MONTGOMERY, nc.MAX_LOG_N)
    assert callable(pkg.MsmContext.ntt) and callable(pkg.MsmContext.ntt_device)
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    assert "te_msm_ntt" in open(os.path.join(js, "addon.cc")).read()
    assert re.search(r"\bntt\b", open(os.path.join(js, "compute_msm.js")).read()) and re.search(r"\bntt\b", open(os.path.join(js, "submission.d.ts")).read())
