"""Sparse matrix-vector products without a device: the per-lane code of csrc/spmv.hip.hpp and the plan of csrc/spmv_plan.hpp, compiled for
the host (tests/csrc/spmvcheck.cpp).  The emulated call equals the model (Python integers, the definition itself) byte for byte at chunk
1, 4 and the default over every row structure; what a bind lays down -- row ids and the transpose -- equals a model; every index of the
plan stays inside its allocation up to 2^33 entries and 2^31 rows; the limb and value bounds of everything stored, by interval
arithmetic; refusals; six deliberate mistakes, each caught; and the same emulation under sanitizers as a program of its own.  The same
code runs on the device in tests/test_gpu_spmv.py."""
import ctypes
import os
import re
import subprocess

import pytest

import spmv_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = sc.P
ALL_M = (0, sc.MATRIX_MONTGOMERY)
ALL_X = (0, sc.SPMV_MONTGOMERY)


@pytest.fixture(scope="module")
def L():
    return sc.shim()


@pytest.fixture(scope="module")
def chunks(L):
    return sorted({1, 4, sc.default_chunk(L)})


# ---- 1. the model -----------------------------------------------------------------------------------------------------------------
def test_model_on_a_matrix_done_by_hand():
    """[[2, 0, 3], [0, 0, 0], [p - 1, 1, 1 (twice)]] x (5, 7, 11): a repeated column is summed, an empty row is 0"""
    M = sc.Matrix(3, 3, (2, 0, 4), lambda r, i, e: (0, 2, 0, 1, 2, 2)[e], lambda r, i, e: (2, 3, P - 1, 1, 1, 1)[e])
    x = sc.pack([5, 7, 11], 32)
    assert sc.unpack(sc.model(M, x), 32) == [43, 0, (-5 + 7 + 22) % P]
    y = sc.pack([1, 100, 10000], 32)
    assert sc.unpack(sc.model(M, y, flags=sc.SPMV_TRANSPOSE), 32) == [(2 - 10000) % P, 10000, 3 + 20000]
    a = sc.A
    xm = sc.pack([5 * a % P, 7 * a % P, 11 * a % P], 32)
    assert sc.unpack(sc.model(M, xm, flags=sc.SPMV_MONTGOMERY), 32) == [43 * a % P, 0, 24 * a % P]


# ---- 2. the emulated call against the model ---------------------------------------------------------------------------------------
def run_case(L, name, chunk, count, mflags, flags, seed=0, mistake=0):
    T = sc.LANES * chunk
    M, x, want = sc.expected(name, T, chunk, count, mflags, flags, seed)
    rc, got, _, _ = sc.emulate(L, M, x, count, mflags | (sc.MATRIX_TRANSPOSE if flags & sc.SPMV_TRANSPOSE else 0), flags, chunk, mistake)
    return rc, got, want


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("transpose", [0, sc.SPMV_TRANSPOSE])
def test_emulation_equals_the_model(L, chunks, count, transpose):
    for chunk in chunks:
        for turn, name in enumerate(sc.structures(sc.LANES * chunk, chunk)):
            mflags, xflags = ALL_M[turn & 1], ALL_X[(turn >> 1) & 1]
            rc, got, want = run_case(L, name, chunk, count, mflags, xflags | transpose)
            assert rc == 0 and got == want, (name, chunk, count, mflags, xflags, transpose)


def test_the_four_forms(L, chunks):
    for chunk in chunks:
        for mflags in ALL_M:
            for xflags in ALL_X:
                for name in ("tail_shorts_head", "dense_column"):
                    for tr in (0, sc.SPMV_TRANSPOSE):
                        rc, got, want = run_case(L, name, chunk, 2, mflags, xflags | tr, seed=3)
                        assert rc == 0 and got == want, (name, chunk, mflags, xflags, tr)


def test_worst_magnitude(L):
    """one full-tile row, every value and every x 2^256 - 1, at every chunk: the largest sums the scan holds"""
    for chunk in range(1, sc.CHUNK_MAX + 1):
        M, x = sc.worst(sc.LANES * chunk)
        for mflags in ALL_M:
            rc, got, _, _ = sc.emulate(L, M, x, 1, mflags, 0, chunk)
            assert rc == 0 and got == sc.model(M, x, 1, mflags, 0), (chunk, mflags)


def test_values_hold_the_extremes():
    M = sc.structure("nnz:%d" % 257, 256, 1)
    assert set(sc.EXTREMES) <= set(M.val) and set(sc.EXTREMES) <= set(sc.unpack(sc.vector(97, 1), 32))


# ---- 3. what a bind lays down; the plan ----------------------------------------------------------------------------------------------
def test_row_ids_and_transpose_equal_the_model(L):
    for name in ("nnz:600", "descending_and_repeated_columns", "dense_column", "empties", "one_column", "one_row:300"):
        M = sc.structure(name, 256, 1)
        row, t_ptr, t_col, t_row, t_val = sc.sides(L, M)
        want_ptr, want_col, want_val = M.transposed()
        assert row == M.row_of(), name
        assert (t_ptr, t_col, t_val) == (want_ptr, want_col, want_val), name
        assert t_row == [c for c in range(M.cols) for _ in range(want_ptr[c + 1] - want_ptr[c])], name


def test_tiles_are_cut_by_position(L, chunks):
    for chunk in chunks:
        T = sc.LANES * chunk
        for rows, nnz, count in ((1, 0, 1), (1000, 0, 2), (1, T, 1), (5, T + 1, 3), (1 << 20, 4 << 20, 1), (1, 1 << 24, 1), (1 << 22, 1 << 24, 2)):
            info = sc.plan_info(L, rows, 7, nnz, count, chunk)
            assert info["T"] == T and info["tiles"] == -(-nnz // T) and info["row_blocks"] == -(-rows // 256)
            assert info["per"] == max(info["tiles"], info["row_blocks"])
            assert info["frag_records"] == 2 * count * info["tiles"] and info["scratch_bytes"] == 32 * info["frag_records"]
            assert info["lds_bytes"] == 4 * 256 * ((9 * chunk) | 1) and info["side_bytes"] == 40 * nnz + 8 * (rows + 1)
    assert sc.plan_info(L, 10, 10, 10, chunk=sc.CHUNK_MAX + 1)["T"] == 0      # refused by the plan; a call falls back to the default
    assert sc.plan_info(L, 10, 10, 10, chunk=sc.CHUNK_MAX)["lds_bytes"] + 1024 <= 160 * 1024


def test_bounds_replay(L):
    """every global, scratch and LDS index, by arithmetic alone: up to 2^33 entries and 2^31 rows and columns"""
    checked = ctypes.c_uint64()
    for chunk in (1, 4, sc.default_chunk(L), sc.CHUNK_MAX):
        T = sc.LANES * chunk
        for rows, cols, nnz, count in ((1, 1, 0, 1), (1, 1, 1, 3), (300, 7, T - 1, 2), (300, 7, T, 2), (300, 7, T + 1, 2), (sc.MAX_DIM, sc.MAX_DIM, 1 << 33, 1),
                                       (sc.MAX_DIM - 1, 3, (1 << 33) - 1, 3), (3, sc.MAX_DIM, (1 << 32) + 1, 5), (1 << 20, 1 << 20, 4 << 20, 3)):
            if chunk == 1 and nnz > 1 << 32 and count > 1:
                count = 1
            assert L.spmv_replay(rows, cols, nnz, count, chunk, ctypes.byref(checked)) == 0, (chunk, rows, cols, nnz, count)
            assert checked.value >= 2 * T + 3 * -(-nnz // T)
    for rows, cols, nnz, count in ((0, 1, 0, 1), (1, 0, 0, 1), (sc.MAX_DIM + 1, 1, 0, 1), (1, sc.MAX_DIM + 1, 0, 1), (1, 1, 0, 0), (sc.MAX_DIM, 1, 0, 1 << 29)):
        assert L.spmv_replay(rows, cols, nnz, count, 8, ctypes.byref(checked)) == sc.BOUNDS      # the plan refuses what the call refuses


# ---- 4. limbs and values of everything stored: interval arithmetic (as tests/test_limb_bounds_te.py) -------------------------------------
LB, NL = 29, 9
LM = (1 << LB) - 1
R = 1 << (LB * NL)


class B:
    """limbs 0 .. 7 up to lim, the top limb up to top, the value up to val (an integer)"""

    def __init__(self, lim, top, val):
        self.lim, self.top, self.val = lim, top, val


def N(val):
    return B(LM, val >> (LB * (NL - 1)), val)


def add_norm(a, b):
    lim, top = a.lim + b.lim, a.top + b.top
    assert lim < 1 << 32 and top + (lim >> LB) + 1 < 1 << 32         # fe_add then fe_norm
    return N(a.val + b.val)


def mul(a, b):
    ma, mb = max(a.lim, a.top), max(b.lim, b.top)
    assert NL * ma * mb + (NL - 1) * LM * LM + LM < 1 << 64, "column overflow"
    return N(a.val * b.val // R + P)


def reduce(a):
    return mul(a, N(R % P))


def out(a):
    r = reduce(a)
    assert r.val < 2 * P, "fo_words subtracts p once"
    return r


def scan_bounds(info, chunk, with_reduction=True):
    """the largest value a lane holds behind every step of k_spmv_tile's scan, and what the closed runs are"""
    t = mul(N(P - 1), N((1 << 256) - 1))                           # a product: v R mod p (canonical) times any 256-bit record
    assert t.val < 1.04 * P
    lane = N(0)
    for _ in range(chunk):
        lane = add_norm(lane, t)
    v, stored = lane, lane
    for s in range(info["scan_steps"]):
        stored = max(stored, v, key=lambda b: b.val)               # what the scan area holds at this step
        v = add_norm(v, v)
        if with_reduction and s == info["scan_reduce"]:
            assert v.val < R
            v = reduce(v)
    return lane, v, stored


def test_limb_and_value_bounds(L):
    info = sc.plan_info(L, 1, 1, 1)
    assert info["scan_steps"] == 8 and 256 == 1 << info["scan_steps"]
    for chunk in range(1, sc.CHUNK_MAX + 1):
        lane, v, stored = scan_bounds(info, chunk)
        assert 2 * lane.val < 33 * P and stored.val < 264 * P < R and 10 * v.val < 237 * P      # 16.5 p, 264 p, 23.7 p: the figures of spmv.hip.hpp and DESIGN.md section 24
        out(v)                                                     # a closed tail
        out(add_norm(lane, v))                                     # a closed head: the lane's first run and the lane before's value
        assert 10 * add_norm(lane, v).val < 402 * P
    # k_spmv_rows: kRowFold canonical fragments on a reduced value, a reduction, and one behind every step of the tree
    acc = reduce(N(33 * P))
    for _ in range(info["row_fold"]):
        acc = add_norm(acc, N(P - 1))
    assert acc.val < 33.1 * P
    acc = reduce(acc)
    for _ in range(info["scan_steps"]):
        acc = reduce(add_norm(acc, acc))
    out(acc)


def test_the_scan_needs_its_reduction(L):
    """without it the eight steps reach 256 x 4.125 p at the default chunk: past R, where a product with R mod p no longer comes out below 2 p"""
    info = sc.plan_info(L, 1, 1, 1)
    _, v, _ = scan_bounds(info, sc.default_chunk(L), with_reduction=False)
    assert v.val > R
    with pytest.raises(AssertionError):
        out(v)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output(L):
    M = sc.structure("nnz:600", 256, 1)
    x = sc.vector(M.cols, 1)
    keep = bytes([0xA5]) * (32 * M.rows)
    bad_ptr0 = (1).to_bytes(8, "little") + M.ptr_bytes[8:]
    down = M.ptr_bytes[:8 * 5] + (0).to_bytes(8, "little") + M.ptr_bytes[8 * 6:]
    bad_col = bytearray(M.col_bytes)
    for at in (77, 300):
        bad_col[4 * at:4 * at + 4] = (M.cols + at).to_bytes(4, "little")
    for kwargs, mflags, flags, why in (
            (dict(dims=(0, M.cols)), 0, 0, sc.SPMV_BAD_DIMS),
            (dict(dims=(M.rows, 0)), 0, 0, sc.SPMV_BAD_DIMS),
            (dict(dims=(sc.MAX_DIM + 1, M.cols)), 0, 0, sc.SPMV_BAD_DIMS),
            (dict(dims=(M.rows, sc.MAX_DIM + 1)), 0, 0, sc.SPMV_BAD_DIMS),
            (dict(ptr=bad_ptr0), 0, 0, sc.SPMV_BAD_PTR),
            (dict(ptr=down), 0, 0, sc.SPMV_BAD_PTR),
            (dict(col=bytes(bad_col)), 0, 0, sc.SPMV_BAD_INDEX),
            (dict(null="ptr"), 0, 0, sc.SPMV_NULL),
            (dict(null="col"), 0, 0, sc.SPMV_NULL),
            (dict(null="vals"), 0, 0, sc.SPMV_NULL),
            (dict(), 4, 0, sc.SPMV_BAD_FLAGS),
            (dict(), 0, 4, sc.SPMV_BAD_FLAGS),
            (dict(), 0, -1, sc.SPMV_BAD_FLAGS),
            (dict(), 0, sc.SPMV_TRANSPOSE, sc.SPMV_NO_TRANSPOSE),
            (dict(null="x"), 0, 0, sc.SPMV_NULL),
            (dict(null="out"), 0, 0, sc.SPMV_NULL),
            (dict(), 0, 0, None)):
        rc, got, reason, bad = sc.emulate(L, M, x, 1, mflags, flags, **kwargs)
        if why is None:
            assert rc == 0 and got == sc.model(M, x)                 # ... and the same buffers are accepted when nothing is wrong
            continue
        assert (rc, reason) == (sc.EINVAL, why), (kwargs, mflags, flags)
        if kwargs.get("null") != "out" and "dims" not in kwargs:
            assert got == bytes([0xA5]) * len(got) and len(got) >= 32, (kwargs, mflags, flags)      # (flags -1 holds TRANSPOSE: the output would be cols records)
        if why == sc.SPMV_BAD_INDEX:
            assert bad == 77                                         # the lowest position
    square = sc.Matrix(4, 4, (1, 1, 1, 1), lambda r, i, e: r, lambda r, i, e: 3)
    xs = sc.vector(4, 2)
    rc, got, reason, _ = sc.emulate(L, square, xs, 1, 0, 0, in_place=True)
    assert (rc, reason, got) == (sc.EINVAL, sc.SPMV_IN_PLACE, xs)
    rc, _, reason, _ = sc.emulate(L, M, x, 1 << 60, 0, 0)            # count x rows x 32 beyond 64 bits
    assert (rc, reason) == (sc.EINVAL, sc.SPMV_TOO_LARGE)
    assert sc.emulate(L, M, b"", 0, 0, 0, null="x")[:2] == (0, b"")   # count = 0 succeeds and touches nothing


# ---- 6. deliberate mistakes -------------------------------------------------------------------------------------------------------
def test_a_head_fragment_in_the_wrong_row_is_caught(L, chunks):
    for chunk in chunks:
        for count in (1, 3):                                          # (the first long row takes the head fragment that belongs to the second)
            rc, got, want = run_case(L, "tail_shorts_head", chunk, count, 0, 0, mistake=sc.M_HEAD_ROW)
            assert rc == 0 and got != want, (chunk, count)


def test_an_unwritten_empty_row_is_caught(L, chunks):
    for chunk in chunks:
        for name in ("empties", "empties_at_tile_boundary"):
            rc, got, want = run_case(L, name, chunk, 1, 0, 0, mistake=sc.M_EMPTY)
            assert rc == 0 and got != want and bytes([0xA5]) * 32 in got, (chunk, name)


def test_a_scan_without_segment_flags_is_caught(L, chunks):
    for chunk in chunks:
        for name in ("chunk_rows", "ones:%d" % (sc.LANES * chunk + 9)):
            rc, got, want = run_case(L, name, chunk, 1, 0, 0, mistake=sc.M_NO_FLAGS)
            assert rc == 0 and got != want, (chunk, name)


def test_a_scan_without_its_reduction_is_caught(L):
    """the worst-case input at the default chunk and at the largest: the row's sum passes R and comes out wrong"""
    for chunk in (sc.default_chunk(L), sc.CHUNK_MAX):
        M, x = sc.worst(sc.LANES * chunk)
        want = sc.model(M, x)
        assert sc.emulate(L, M, x, 1, 0, 0, chunk)[:2] == (0, want)
        rc, got, _, _ = sc.emulate(L, M, x, 1, 0, 0, chunk, mistake=sc.M_NO_REDUCE)
        assert rc == 0 and got != want, chunk


@pytest.mark.parametrize("mistake", [sc.M_UNSTABLE, sc.M_OFF_BY_ONE])
def test_a_wrong_counting_sort_is_caught(L, mistake):
    M = sc.structure("dense_column", 256, 1)
    want_ptr, want_col, want_val = M.transposed()
    _, t_ptr, t_col, _, t_val = sc.sides(L, M, mistake)
    assert (t_ptr, t_col, t_val) != (want_ptr, want_col, want_val)
    if mistake == sc.M_OFF_BY_ONE:                                   # ... and the product with it is wrong (an unstable sort only reorders a sum)
        x = sc.vector(M.rows, 5)
        rc, got, _, _ = sc.emulate(L, M, x, 1, sc.MATRIX_TRANSPOSE, sc.SPMV_TRANSPOSE, 1, mistake)
        assert rc == 0 and got != sc.model(M, x, 1, 0, sc.SPMV_TRANSPOSE)


# ---- 7. the emulation under sanitizers: a program of its own ----------------------------------------------------------------------------
def test_emulation_under_sanitizers(tmp_path):
    exe = str(tmp_path / "san_spmv")
    subprocess.check_call(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-o", exe, os.path.join(ROOT, "tests", "csrc", "san_spmv.cpp")])      # (the runtimes linked in: the program's environment stays as it is)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    assert r.returncode == 0 and "san_spmv ok" in r.stdout, r.stdout[-2000:]


# ---- 8. the names -----------------------------------------------------------------------------------------------------------------
def test_names_in_header_and_package(pkg):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name, val in (("TE_MSM_MATRIX_MONTGOMERY", "1"), ("TE_MSM_MATRIX_TRANSPOSE", "2"), ("TE_MSM_SPMV_MONTGOMERY", "1"), ("TE_MSM_SPMV_TRANSPOSE", "2"),
                      ("TE_MSM_SPMV_CHUNK", "%du" % sc.default_chunk(sc.shim()))):
        assert re.search(r"#define %s +%s(?![0-9])" % (name, re.escape(val)), hdr), name
    for fn in ("te_msm_bind_matrix", "te_msm_release_matrix", "te_msm_matrix_shape", "te_msm_spmv", "te_msm_spmv_device"):
        assert fn + "(" in hdr
    assert (pkg.MATRIX_MONTGOMERY, pkg.MATRIX_TRANSPOSE, pkg.SPMV_MONTGOMERY, pkg.SPMV_TRANSPOSE) == (1, 2, 1, 2)
    for method in ("bind_matrix", "release_matrix", "spmv", "spmv_device"):
        assert callable(getattr(pkg.MsmContext, method))
