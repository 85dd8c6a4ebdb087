"""MSMs over narrow scalars (options "scalar_bits", "scalar_record_bytes" = 8 / 16), without a GPU: the plan rule and the digit kernels'
load addresses, both from the HIP-free csrc/plan_arith.hpp compiled for the host by tests/csrc/narrowplan.cpp.

The rule, restated in Python integers: W = ceil((b + g) / c0) with g = 2 for signed digits and 0 for unsigned ones, and c = c0 (the
smallest size with that window count measured slower: DESIGN.md section 20).  A signed decomposition accepts exactly
s < 2^(cW) - sum_{w<W} 2^(cw + c - 1), an unsigned one s < 2^(cW): every b-bit scalar must lie below that limit."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32, u64 = ctypes.c_uint32, ctypes.c_uint64
DIG_BLOCK = 1024                      # TE_DIG_BLOCK: entries a block of the digit kernels covers (two per thread)
SIZES = (1, 2, 3, 1023, 1024, 1025, 2049)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("narrowplan") / "libnarrowplan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", so, os.path.join(ROOT, "tests", "csrc", "narrowplan.cpp")])
    L = ctypes.CDLL(so)
    L.np_windows.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int)] * 2
    L.np_windows.restype = None
    L.np_loads.argtypes = [u32, u32, u32, ctypes.c_int, ctypes.POINTER(u64), ctypes.POINTER(u32)]
    L.np_loads.restype = ctypes.c_int
    L.np_pair.argtypes = [u32, u32, ctypes.POINTER(u32), ctypes.POINTER(u32)]
    L.np_pair.restype = None
    return L


def windows(shim, c0, signed, bits):
    c, W = ctypes.c_int(), ctypes.c_int()
    shim.np_windows(c0, int(signed), bits, ctypes.byref(c), ctypes.byref(W))
    return c.value, W.value


def rule(c0, signed, b, g=None):
    g = (2 if signed else 0) if g is None else g
    return c0, -(-(b + g) // c0)


def limit(c, W, signed):
    """the first scalar the decomposition refuses"""
    return (1 << (c * W)) - (sum(1 << (c * w + c - 1) for w in range(W)) if signed else 0)


def rule_violations(plan_of):
    """every (b, c0, signed) at which plan_of breaks the contract: the rule's W, 4 <= c <= c0, 2^b <= limit"""
    bad = []
    for signed in (1, 0):
        for c0 in range(4, 17):
            for b in range(1, 257):
                c, W = plan_of(c0, signed, b)
                ok = W == rule(c0, signed, b)[1] and 4 <= c <= c0 and (1 << b) <= limit(c, W, signed)
                if not ok:
                    bad.append((b, c0, signed, c, W))
    return bad


def test_plan_rule_matches_the_integer_restatement(shim):
    assert rule_violations(lambda c0, signed, b: windows(shim, c0, signed, b)) == []
    for signed in (1, 0):
        for c0 in range(4, 17):
            for b in range(1, 257):
                assert windows(shim, c0, signed, b)[0] == c0, "the window size is kept"


def test_full_width_counts_are_unchanged(shim):
    for c0 in range(4, 17):
        today = {1: (255 + c0 - 1) // c0, 0: (256 + c0 - 1) // c0}
        for signed in (1, 0):
            assert windows(shim, c0, signed, 0) == (c0, today[signed]), "nothing declared: the plan is what it was"
            assert windows(shim, c0, signed, 253 if signed else 256) == (c0, today[signed])
    # a 64-bit MSM at n = 2^20 (16-bit windows) needs 5 windows where a full-width one runs 16, a 128-bit one 9
    assert windows(shim, 16, 1, 64) == (16, 5) and windows(shim, 16, 1, 128) == (16, 9)


def test_a_guard_of_one_bit_is_caught(shim):
    """cW = b + 1 does not admit every b-bit scalar: the checker must say so (the deliberate mistake g = 1)"""
    bad = rule_violations(lambda c0, signed, b: rule(c0, signed, b, g=1 if signed else 0))
    assert bad and all(signed == 1 for _, _, signed, _, _ in bad)
    assert any((1 << b) > limit(c, W, 1) for b, _, _, c, W in bad), "a b-bit scalar above the limit of a g = 1 plan"


# ---- the loads of the digit kernels ----------------------------------------------------------------------------------------------
def shim_loads(shim):
    def f(rec, i0, n, base16):
        at, by = (u64 * 6)(), (u32 * 6)()
        k = shim.np_loads(rec, i0, n, int(base16), at, by)
        return [(at[j], by[j]) for j in range(k)]
    return f


def unclamped_loads(rec, i0, n, base16):
    """the deliberate mistake: the second record of a pair is loaded without the clamp"""
    if rec == 8 and base16:
        return [(8 * i0, 16)]
    unit = min(rec, 16)
    ia = min(i0, n - 1)
    return [(rec * ia + 16 * k, unit) for k in range(rec // unit)] + [(rec * (i0 + 1) + 16 * k, unit) for k in range(rec // unit)]


def slices():
    """(record bytes, n, record offset of the slice in a 16-byte aligned packed buffer): lone calls start at 0, the MSMs of a batch call
    at sum lens[j] -- odd and even"""
    for rec in (8, 16, 32, 48):
        for n in SIZES:
            for off in (0, 1, 2, 7, 300, 1023):
                yield rec, n, off


def load_violations(loads):
    bad = []
    for rec, n, off in slices():
        base = off * rec                                     # byte address of the slice's first record (the buffer itself is 16-byte aligned)
        nst = (n + 7) & ~7
        blocks = (nst + DIG_BLOCK - 1) // DIG_BLOCK
        for i0 in range(0, blocks * DIG_BLOCK, 2):           # every thread of the grid loads, padding pairs included
            got = loads(rec, i0, n, base % 16 == 0)
            covered = set()
            for at, size in got:
                if at + size > n * rec or size not in (8, 16) or (size == 8 and rec != 8):
                    bad.append(("outside the slice", rec, n, off, i0, at, size))
                if (base + at) % size:
                    bad.append(("misaligned", rec, n, off, i0, at, size))
                covered.update(range(at, at + size))
            need = set()
            if i0 < n:
                need.update(range(rec * i0, rec * i0 + rec))
            if i0 + 1 < n:
                need.update(range(rec * (i0 + 1), rec * (i0 + 1) + rec))
            if not need <= covered:
                bad.append(("a record of the pair is not loaded", rec, n, off, i0))
    return bad


def test_every_load_lies_inside_its_slice_and_is_aligned(shim):
    assert load_violations(shim_loads(shim)) == []


def test_two_records_share_a_load_only_where_aligned_and_present(shim):
    loads = shim_loads(shim)
    assert loads(8, 0, 2, True) == [(0, 16)] and loads(8, 2, 5, True) == [(16, 16)]
    assert loads(8, 0, 2, False) == [(0, 8), (8, 8)], "an odd record offset of a batch call: 8-byte aligned only"
    assert loads(8, 2, 3, True) == [(16, 8), (16, 8)], "odd n: the last record is loaded alone"
    assert loads(16, 2, 3, True) == [(32, 16), (32, 16)]
    assert loads(32, 2, 3, True) == [(64, 16), (80, 16), (64, 16), (80, 16)]


def test_the_narrow_clamp_is_the_wide_one(shim):
    """pair_records(i0, n), which the narrow loads go through, is digits_block's own clamp: min(i0, n - 1) and min(i0 + 1, n - 1)"""
    ia, ib = u32(), u32()
    for n in SIZES:
        for i0 in range(0, ((n + 7) & ~7) + DIG_BLOCK, 2):
            shim.np_pair(i0, n, ctypes.byref(ia), ctypes.byref(ib))
            assert (ia.value, ib.value) == (min(i0, n - 1), min(i0 + 1, n - 1))


def test_an_unclamped_pair_load_is_caught():
    bad = load_violations(unclamped_loads)
    assert any(kind == "outside the slice" and n % 2 == 1 for kind, _, n, *_ in bad), "odd n: the unclamped second record lies outside"
    assert {rec for kind, rec, *_ in bad if kind == "outside the slice"} == {8, 16, 32, 48}


# ---- the public surface, as far as it shows without a device ----------------------------------------------------------------------
def test_header_and_documents_name_the_options():
    for rel in (("include", "te_msm.h"), ("README.md",), ("INTEGRATION.md",), ("DESIGN.md",)):
        text = open(os.path.join(ROOT, *rel)).read()
        assert "scalar_bits" in text and "scalar_record_bytes" in text, rel


def test_digit_kernels_have_the_narrow_instantiations():
    src = open(os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc", "kernels.hip.hpp")).read()
    assert "digits_block_narrow" in src and "te_plan::loads_of_pair" in src
    eng = open(os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc", "te_msm.hip")).read()
    assert "te_plan::windows_for" in eng and "num_windows_for" not in eng, "one statement of the rule"
