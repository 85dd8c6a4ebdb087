"""Fixed-base windows on the host (option "bind_fixed_base" = c in 16..21): csrc/fb_plan.hpp -- the plan's arithmetic and the digit
walk --, the two digit extractions of k_fb_digits as tests/csrc/fbcheck.cpp restates them line for line, and te_host::fixed_base_with /
fixed_base_to_affine, compared with the bigint model oracle/fixed_base.py, which is written from DESIGN.md and shares no code with them:
  * the walk of every scalar class of tests/fb_cases.py and 2000 seeded scalars per c: (row, lo, sign, carry) index for index, the entries'
    weights sum to the scalar, and the extra row holds exactly the top window's hb = 0 entries -- the one rule no MSM result can see;
  * the geometry at ragged, tiny and huge n and both "below 2^31" refusals at their thresholds;
  * the host tail on synthetic rows (random Z, absent rows, the neutral element as T), both accumulator forms, bit for bit;
  * a sequential replay of k_fb_digits and of the read range of the sort's first level: every index against the engine's buffer sizes,
    also with idx_base != 0 (which no caller passes today);
  * six deliberate mistakes switched into the shim are each caught by one of the checks above, and the single invariants (weight sum,
    extra-row membership, cap % 8) catch theirs without the comparison with the model in front of them.
The two "below 2^31" refusals are te_fb::bind_refused / msm_refused, which te_msm_bind_points and enqueue_fixed_base call."""
import ctypes
import os
import random
import subprocess

import pytest

import fb_cases
from oracle import fixed_base as fbm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS = list(fbm.C_RANGE)
R261 = 1 << 261
U32, U64 = ctypes.c_uint32, ctypes.c_uint64
GEO_KEYS = ("W", "rb", "rows", "reg", "cap", "chunks", "chunk_len", "CH", "S", "P", "logS", "seg_len")


@pytest.fixture(scope="module")
def fbc(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fbcheck") / "libfbcheck.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-o", so, os.path.join(ROOT, "tests", "csrc", "fbcheck.cpp")])
    lib = ctypes.CDLL(so)
    lib.fbc_geometry.argtypes = [U64, ctypes.c_int, U64, ctypes.POINTER(U64)]
    lib.fbc_walk.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_char_p, U32, U32, U32, ctypes.POINTER(U32)]
    lib.fbc_tail.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
    yield lib
    lib.fbc_set_variant(0)


def le32(ks):
    return b"".join(k.to_bytes(32, "little") for k in ks)


def header_geometry(fbc, n, c, n_table=None):
    o = (U64 * 26)()
    fbc.fbc_geometry(n, c, n if n_table is None else n_table, o)
    g = dict(zip(GEO_KEYS, (int(v) for v in o[:12])))
    g["half"] = [int(v) for v in o[12:22]]
    g["lds_bytes"] = int(o[22])
    return g, bool(o[23]), bool(o[24])


def shim_walk(fbc, ks, c, from_kernel, n_table=None, idx_base=0):
    """per scalar: ([(w, row, lo, sign, code, remap word)], carry) from csrc/fb_plan.hpp (from_kernel = 0) or from the restated text of
    k_fb_digits (1), whose two phases must name the same row"""
    n = len(ks)
    out = (U32 * (n * 18 * 6))()
    wmax = fbc.fbc_walk(from_kernel, c, le32(ks), n, n if n_table is None else n_table, idx_base, out)
    res = []
    for i in range(n):
        es, carry = [], False
        for w in range(wmax):
            kind, row, row_b, lo, code, word = out[(i * wmax + w) * 6:(i * wmax + w) * 6 + 6]
            if kind == 2:
                carry = True
            elif kind == 1:
                assert row == row_b, "phases A and B disagree on the row"
                es.append((w, row, lo, word >> 31, code, word & 0x7FFFFFFF))
        res.append((es, carry))
    return res


# ------------------------------------------------------------------ a. the walk
def all_walk_scalars(c):
    ks = [k for v in fb_cases.classes(c).values() for k in v] + fb_cases.refused(c) + fb_cases.randoms(c, 2000, 0xFB)
    ks += fb_cases.one_among_zeros(5, 3) + fb_cases.only_row(c, 8, fbm.regular_rows(c), 1) + fb_cases.only_row(c, 8, fbm.regular_rows(c) - 1, 2)
    return ks


def check_walk(fbc, c, coarse=True):
    """coarse = False leaves out the entry-for-entry comparison with the model: the invariants below it then have to bite on their own"""
    W, rb = fbm.windows(c), fbm.regular_rows(c)
    ks = all_walk_scalars(c)
    n = len(ks)
    seen_rows, seen_carry = set(), 0
    header, kernel = shim_walk(fbc, ks, c, 0), shim_walk(fbc, ks, c, 1)
    assert header == kernel, "csrc/fb_plan.hpp and the two extractions of k_fb_digits"
    for i, (k, (got, carry)) in enumerate(zip(ks, header)):
        want, wcarry = fbm.entries(k, c)
        if coarse:
            assert carry == (wcarry != 0), (c, hex(k))
        seen_carry += carry
        if carry:
            continue
        if coarse:
            assert [e[:4] for e in got] == want, (c, hex(k))
        # the entries' weights give the scalar back, as an integer: the extra row weighs like row 0, the code is lo + 1
        assert sum((-1 if sg else 1) * (((0 if row == rb else row) << 15) + code) << (c * w) for w, row, lo, sg, code, _ in got) == k, "the weights do not sum to the scalar %x (c = %d)" % (k, c)
        for w, row, lo, sg, code, word in got:
            assert row <= rb and lo < 1 << 15 and code == lo + 1 and word == w * n + i
            hb = (abs(fbm.walk(k, c)[0][w]) - 1) >> 15
            assert (row == rb) == (w == W - 1 and hb == 0), "the extra row holds the top window's hb = 0 entries and nothing else"
            seen_rows.add(row)
    assert seen_rows == set(range(rb + 1)) and seen_carry == len(fb_cases.refused(c))


@pytest.mark.parametrize("c", CS)
def test_walk_matches_the_model_index_for_index(fbc, c):
    fbc.fbc_set_variant(0)
    check_walk(fbc, c)


def test_acceptance_thresholds_come_from_the_walk():
    for c in CS:
        top = fbm.largest_accepted(c)
        assert fbm.walk(top, c)[1] == 0 and top < 1 << 256
        nxt = fbm.smallest_refused(c)
        if nxt is None:
            assert top == (1 << 256) - 1 and fbm.windows(c) * c - 1 >= 256          # every 256-bit scalar is walked
        else:
            assert nxt == top + 1 and fbm.walk(nxt, c)[1] != 0 and c in (16, 17)
        for name, ks in fb_cases.classes(c).items():
            assert ks, (c, name)
        assert ("top window hb != 0" in fb_cases.classes(c)) == (c in (17, 20))     # where the top window holds 17 bits below 2^256


# ------------------------------------------------------------------ b. the geometry
def _largest_n_below(c):
    return ((1 << 31) - 1) // fbm.windows(c)                # the largest n with W n < 2^31


def check_geometry(fbc, c, coarse=True):
    for n in (1, 2, 7, 8, 9, 255, 4096, 4097, 70001, 1 << 20, 1 << 22, _largest_n_below(c), _largest_n_below(c) + 1):
        g, bind_no, msm_no = header_geometry(fbc, n, c)
        want = fbm.geometry(n, c)
        if coarse:
            assert g == want, (c, n, {k: (g[k], want[k]) for k in g if g[k] != want[k]})
        assert g["cap"] % 8 == 0, "cap is no multiple of 8"
        assert g["cap"] >= max(g["reg"], n) and g["chunk_len"] % 4096 == 0 and g["CH"] * g["chunk_len"] >= g["cap"]
        assert g["lds_bytes"] <= 64 * 1024 and g["rows"] <= fbm.ROW_FILL_WORDS
        assert g["seg_len"] in (16, 32, 64) and 1 <= g["CH"] <= g["chunks"] <= 256
        assert bind_no == fbm.bind_refused(c, n) == (n > _largest_n_below(c)), (c, n)
        assert msm_no == fbm.msm_refused(n, c, n), (c, n)


@pytest.mark.parametrize("c", CS)
def test_geometry_matches_the_model(fbc, c):
    fbc.fbc_set_variant(0)
    check_geometry(fbc, c)


def test_refusals_fall_where_the_code_says(fbc):
    """bind: W n_table >= 2^31; an MSM: rows x cap >= 2^31 (the digit and remap rows are indexed with 31 bits) or the table's bound"""
    fbc.fbc_set_variant(0)
    for c in CS:
        nmax = _largest_n_below(c)
        assert not header_geometry(fbc, 1, c, nmax)[1] and header_geometry(fbc, 1, c, nmax + 1)[1]
        assert not header_geometry(fbc, 1, c, nmax)[2] and header_geometry(fbc, 1, c, nmax + 1)[2]
        # rows x cap: the smallest n (over a table that is itself within its bound) at which the MSM is refused, by bisection on the model
        lo, hi = 1, nmax
        if not fbm.msm_refused(hi, c, 1):
            continue
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if fbm.msm_refused(mid, c, 1) else (mid + 1, hi)
        for n in (lo - 1, lo):
            g, _, no = header_geometry(fbc, n, c, 1)
            assert no == (n == lo) == (g["rows"] * g["cap"] >= 1 << 31), (c, n)


# ------------------------------------------------------------------ c. the host tail
def _row_bytes(model, rng, pts5):
    """720 bytes: five extended points (X, Y, Z, T) = (x Z, y Z, Z, x y Z), nine 29-bit limbs each, Montgomery form R = 2^261"""
    P = model.P
    out = b""
    for x, y in pts5:
        z = rng.randrange(2, P)
        for v in (x * z, y * z, z, x * y * z):
            m = v * R261 % P
            out += b"".join(((m >> (29 * j)) & 0x1FFFFFFF).to_bytes(4, "little") for j in range(9))
    assert len(out) == 720 and any(out)
    return out


def _tail_cases(model, rb):
    rng = random.Random(0x7A11 + rb)
    pool = model.gen_points(0x7A11, 8)

    def rnd():
        return model.scalar_mul(rng.randrange(1, model.L), pool[rng.randrange(8)])
    rows = rb + 1
    full = {r: [rnd() for _ in range(5)] for r in range(rows)}
    yield "all rows", full
    yield "extra row only", {rb: full[rb]}
    yield "row rb-1 only", {rb - 1: full[rb - 1]}
    yield "row 0 absent", {r: v for r, v in full.items() if r != 0}
    yield "all absent", {}
    neutral = dict(full)
    neutral[rb - 1] = [model.ZERO] + full[rb - 1][1:]
    yield "T neutral", neutral


def check_tail(fbc, model, rb, forms=(0, 1, 2)):
    c = 16 + rb.bit_length() - 1
    assert fbm.regular_rows(c) == rb
    have_ifma = bool(fbc.fbc_have_ifma())
    for name, rows in _tail_cases(model, rb):
        rng = random.Random(rb)
        blob = b"".join(_row_bytes(model, rng, rows[r]) if r in rows else bytes(720) for r in range(rb + 1))
        want = model.points_to_bytes([fbm.tail(model, rows, c)])
        if name == "all absent":
            assert want == model.points_to_bytes([(0, 1)])
        for form in forms:
            out = ctypes.create_string_buffer(64)
            rc = fbc.fbc_tail(form, blob, rb + 1, rb, 15, out)
            if rc == -1:
                assert form == 1 and not have_ifma
                continue
            assert out.raw == want, (rb, name, form)
    return have_ifma


@pytest.mark.parametrize("rb", [1, 2, 4, 8, 16, 32])
def test_host_tail_on_synthetic_rows(fbc, model, rb):
    fbc.fbc_set_variant(0)
    if not check_tail(fbc, model, rb):
        print("no AVX-512 IFMA on this CPU: fixed_base_with<IfmaAcc> was not run")


# ------------------------------------------------------------------ d. the bounds replay
def replay_cases(c):
    """(name, scalars) of every case the GPU tests run or could run, small enough for a sequential replay"""
    cl = fb_cases.classes(c)
    rb = fbm.regular_rows(c)
    for name, ks in cl.items():
        yield name, ks
    yield "every class among random scalars, n = 300", fb_cases.mixed(c, 300, 3)[0]
    yield "every class among random scalars, n = 4097", fb_cases.mixed(c, 4097, 4)[0]
    yield "one among zeros", fb_cases.one_among_zeros(257, 256)
    yield "extra row only", fb_cases.only_row(c, 700, rb, 5)
    yield "row rb-1 only", fb_cases.only_row(c, 700, rb - 1, 6)
    yield "all equal", [cl["digits +max"][0]] * 3000


def check_replay(c, ks, name, idx_base=0, n_table=None):
    r = fbm.replay(ks, c, n_table=n_table, idx_base=idx_base)
    assert not r["violations"], (c, name, r["violations"][:4])
    assert not r["carry"]
    # what the replay wrote is the model's bucket membership, entry for entry
    n, nt = len(ks), len(ks) if n_table is None else n_table
    want = {}
    for i, k in enumerate(ks):
        for w, row, lo, sg in fbm.entries(k, c)[0]:
            want.setdefault(row, []).append((lo + 1, (w * nt + idx_base + i) | (sg << 31)))
    cap = r["geometry"]["cap"]
    for row, fill in enumerate(r["fill"]):
        assert fill == len(want.get(row, [])), (c, name, row)
        if fill <= cap:
            assert sorted(r["written"][row].values()) == sorted(want.get(row, [])), (c, name, row)
    assert r["fallback"] == any(f > cap for f in r["fill"])
    return r


@pytest.mark.parametrize("c", CS)
def test_bounds_replay_of_the_digit_kernel_and_the_first_scatter(c):
    for name, ks in replay_cases(c):
        r = check_replay(c, ks, name)
        if name in ("extra row only", "row rb-1 only"):
            only = fbm.regular_rows(c) - (name != "extra row only")
            assert r["fill"][only] > 0 and sum(r["fill"]) == r["fill"][only], (c, name)
        assert r["fallback"] == (name == "all equal" and c >= 17), (c, name)      # (c = 16: one regular row, sized for all 15 n entries)
        # a launch that covers a slice of a larger table: idx_base != 0 (no caller passes it today)
        n = len(ks)
        check_replay(c, ks, name + ", idx_base", idx_base=1000, n_table=n + 1000)
        check_replay(c, ks, name + ", idx_base at the table's end", idx_base=5 * n, n_table=6 * n)
    # ... and past the table's end the replay reports it
    top = 1 << (c * (fbm.windows(c) - 1))
    bad = fbm.replay([top, top], c, n_table=2, idx_base=1)
    assert any("outside the table" in v for v in bad["violations"])
    bad = fbm.replay([1, 1], c, n_table=2, idx_base=1)            # (a lower window's word stays inside: it names the next table's record)
    assert any("alias the next table" in v for v in bad["violations"])


def test_row_fill_at_the_capacity_boundary_in_the_replay():
    """the cases of tests/test_gpu_fixed_base_stages.py: fill = cap - 1, cap, cap + 1 in one regular row"""
    for c, n, row in ((19, 5000, 3), (20, 5000, 15)):
        cap = fbm.geometry(n, c)["cap"]
        for fill in (cap - 1, cap, cap + 1):
            r = check_replay(c, fb_cases.fill_case(c, n, row, fill), "fill")
            assert r["fill"][row] == fill and r["fallback"] == (fill > cap)
        # the extra row takes one entry per scalar at most: n < cap for every n, it cannot overflow
        assert n < cap
        r = check_replay(c, fb_cases.only_row(c, n, fbm.regular_rows(c), 9), "extra row full")
        assert r["fill"][-1] == n and not r["fallback"] and sum(r["fill"][:-1]) == 0


# ------------------------------------------------------------------ e. the checks bite
def test_deliberate_mistakes_in_the_shim_are_caught(fbc, model):
    """variant -> the check that must fail (tests/csrc/fbcheck.cpp)"""
    table = {
        1: lambda: check_walk(fbc, 20),                    # the extra-row rule dropped: ONLY the walk check sees it
        2: lambda: check_walk(fbc, 16),                    # sign lost in neg
        3: lambda: check_walk(fbc, 17),                    # code lo instead of lo + 1
        4: lambda: check_geometry(fbc, 18),                # half missing the top window
        5: lambda: check_tail(fbc, model, 4, forms=(0,)),  # U summed down to r = 2
        6: lambda: check_geometry(fbc, 19),                # cap not rounded to 8
    }
    try:
        for v, check in table.items():
            fbc.fbc_set_variant(v)
            with pytest.raises(AssertionError):
                check()
        fbc.fbc_set_variant(4)                             # the walk sees the missing half bit as well
        with pytest.raises(AssertionError):
            check_walk(fbc, 21)
        # the invariants on their own, without the entry-for-entry comparison that fires first above
        for v, c, check, message in ((1, 20, check_walk, "extra row holds"), (1, 16, check_walk, "extra row holds"), (2, 16, check_walk, "weights do not sum"),
                                     (3, 17, check_walk, "weights do not sum"), (4, 21, check_walk, "weights do not sum"), (6, 19, check_geometry, "multiple of 8")):
            fbc.fbc_set_variant(v)
            with pytest.raises(AssertionError, match=message):
                check(fbc, c, coarse=False)
        # U down to r = 2 drops the term 1 x T_1: invisible with one regular row (U is empty), visible from two on
        fbc.fbc_set_variant(5)
        check_tail(fbc, model, 1, forms=(0,))
        with pytest.raises(AssertionError):
            check_tail(fbc, model, 2, forms=(0,))
    finally:
        fbc.fbc_set_variant(0)
    check_walk(fbc, 20)
    check_geometry(fbc, 19)
