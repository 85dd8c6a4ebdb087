"""Shared by tests/test_spmv_host.py and tests/test_gpu_spmv.py: the host shim of csrc/spmv.hip.hpp (tests/csrc/spmvcheck.cpp), the model of
te_msm_spmv in Python integers -- out[k rows + r] = sum_e vals[e] x[k cols + col[e]] mod p, the definition itself -- and the case lists.
Expected values never come from a kernel of the library."""
import ctypes
import functools
import os
import random
import subprocess

import field_cases as fc
from oracle import model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = m.P
A = 1 << 256
TOP = A - 1
MATRIX_MONTGOMERY, MATRIX_TRANSPOSE = 1, 2                          # TE_MSM_MATRIX_*
SPMV_MONTGOMERY, SPMV_TRANSPOSE = 1, 2                              # TE_MSM_SPMV_*
LANES = 256
CHUNK_MAX = 16
MAX_DIM = 1 << 31
EINVAL = -1
BOUNDS = -100
SPMV_BAD_DIMS, SPMV_BAD_FLAGS, SPMV_BAD_PTR, SPMV_BAD_INDEX, SPMV_NULL, SPMV_NO_TRANSPOSE, SPMV_IN_PLACE, SPMV_TOO_LARGE = range(1, 9)
M_HEAD_ROW, M_EMPTY, M_NO_FLAGS, M_NO_REDUCE, M_UNSTABLE, M_OFF_BY_ONE = range(1, 7)      # the shim's deliberate mistakes
pack, unpack = fc.pack, fc.unpack
EXTREMES = (0, 1, P - 1, P, TOP)


def shim():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libspmvcheck.so"), os.path.join(d, "spmvcheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("spmv.hip.hpp", "spmv_plan.hpp", "plan_arith.hpp", "field_ops.hip.hpp", "scalar_mul.hip.hpp", "from_x.hip.hpp",
                                                         "check.hip.hpp", "fp.hpp", "fq377.hpp", "field.hpp", "curve.hpp", "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    ci, vp, u64, u32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.spmv_emulate.argtypes = [u64, u64, vp, vp, vp, ci, vp, u64, ci, u32, ci, vp, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_int64)]
    L.spmv_emulate.restype = ci
    L.spmv_sides.argtypes = [u64, u64, vp, vp, vp, ci, vp, vp, vp, vp, vp]
    L.spmv_sides.restype = ci
    L.spmv_replay.argtypes = [u64, u64, u64, u64, u32, ctypes.POINTER(u64)]
    L.spmv_replay.restype = ci
    L.spmv_plan_info.argtypes = [u64, u64, u64, u64, u32, ctypes.POINTER(u64)]
    return L


def plan_info(L, rows, cols, nnz, count=1, chunk=0):
    out = (ctypes.c_uint64 * 16)()
    L.spmv_plan_info(rows, cols, nnz, count, chunk or default_chunk(L), out)
    keys = ("T", "tiles", "row_blocks", "per", "frag_records", "scratch_bytes", "lds_bytes", "chunk_default", "chunk_max", "scan_reduce", "row_fold", "side_bytes", "scan_steps")
    return dict(zip(keys, (int(v) for v in out)))


def default_chunk(L):
    out = (ctypes.c_uint64 * 16)()
    L.spmv_plan_info(1, 1, 0, 1, 1, out)
    return int(out[7])


# ---- matrices ---------------------------------------------------------------------------------------------------------------------
class Matrix:
    """a CSR matrix as the C-ABI takes it: row_ptr (uint64), col_idx (uint32), vals (32-byte records), all as bytes, and as lists"""

    def __init__(self, rows, cols, lens, col_of, val_of):
        self.rows, self.cols = rows, cols
        self.ptr = [0]
        for n in lens:
            self.ptr.append(self.ptr[-1] + n)
        self.nnz = self.ptr[-1]
        self.col, self.val = [], []
        for r, n in enumerate(lens):
            for i in range(n):
                e = len(self.col)
                self.col.append(col_of(r, i, e))
                self.val.append(val_of(r, i, e))
        self.ptr_bytes = b"".join(v.to_bytes(8, "little") for v in self.ptr)
        self.col_bytes = b"".join(v.to_bytes(4, "little") for v in self.col)
        self.val_bytes = pack(self.val, 32)

    def row_of(self):
        return [r for r in range(self.rows) for _ in range(self.ptr[r + 1] - self.ptr[r])]

    def transposed(self):
        """(t_ptr, t_col, t_val): the transpose as CSR, a column's entries in the order of the stream -- a stable sort by column"""
        order = sorted(range(self.nnz), key=lambda e: self.col[e])       # (sorted is stable)
        rows = self.row_of()
        t_ptr = [0] * (self.cols + 1)
        for c in self.col:
            t_ptr[c + 1] += 1
        for c in range(self.cols):
            t_ptr[c + 1] += t_ptr[c]
        return t_ptr, [rows[e] for e in order], [self.val[e] for e in order]


def values(seed):
    """a value or x record by position: the extremes 0, 1, p - 1, p, 2^256 - 1 among random residues and random full-width integers"""
    rnd = random.Random(0x5A + 7919 * seed)
    pool = list(EXTREMES) + [rnd.randrange(P) for _ in range(40)] + [rnd.randrange(A) for _ in range(40)]
    rnd.shuffle(pool)
    return lambda *at: pool[(at[-1] * 31 + 7) % len(pool)]


def vector(n, seed):
    f = values(100 + seed)
    return pack([f(i) for i in range(n)], 32)


def random_lens(nnz, seed):
    """row lengths that sum to nnz: mostly 0 .. 5, now and then a long one"""
    rnd = random.Random(0x77 + seed + 1000003 * nnz)
    lens = []
    left = nnz
    while left > 0:
        n = rnd.choice((0, 1, 1, 2, 3, 4, 5, 5, 37, 300)) if rnd.random() < 0.97 else rnd.randrange(1, 900)
        n = min(n, left)
        lens.append(n)
        left -= n
    return lens or [0]


@functools.lru_cache(maxsize=None)
def structure(name, T, chunk, seed=0):
    """the row structures of the issue, by name, as a Matrix"""
    rnd = random.Random(0xC5 + seed)
    cols = 97
    col_of = lambda r, i, e: (e * 13 + r) % cols                                  # noqa: E731
    if name.startswith("nnz:"):
        lens = random_lens(int(name[4:]), seed)
    elif name.startswith("ones:"):
        lens = [1] * int(name[5:])
    elif name.startswith("one_row:"):
        lens = [int(name[8:])]
    elif name == "chunk_rows":
        lens = [chunk - 1, chunk, chunk + 1] * (T // (3 * chunk) + 3)
    elif name.startswith("row_ends:"):                                            # a row ending one before / at / one after a tile's last entry
        lens = [5, T - 5 + int(name[9:]) - 1, 1, 1, 1, 2, 3]
    elif name == "empties":
        lens = [0, 0, 3, 0, 0, 0, 5, 2, 1, 0, 0]
    elif name == "empties_at_tile_boundary":
        lens = [T - 3, 3, 0, 0, 0, 7, 0, T - 7, 0, 0, 4]
    elif name == "tail_shorts_head":                                              # tile 1: the tail of a long row, whole short rows, the head of another long row
        lens = [T + T // 2, 3, 1, 0, 5, 2, T, 4]
    elif name == "tile_inside_a_row":
        lens = [3, 3 * T + 10, 2]
    elif name == "descending_and_repeated_columns":
        lens = [6, 1, 9, 0, 4] * 12
        col_of = lambda r, i, e: (cols - 1 - i // 2) if r % 2 else (5 if i % 3 else 90 - i)      # noqa: E731
    elif name == "one_column":
        lens, cols = random_lens(T + 70, seed), 1
        col_of = lambda r, i, e: 0                                                # noqa: E731
    elif name == "dense_column":                                                  # the constant's column in every row: one row of the transpose holds them all
        lens = [1 + rnd.randrange(4) for _ in range(T // 2)]
        col_of = lambda r, i, e: 0 if i == 0 else 1 + (e * 13 + r) % (cols - 1)    # noqa: E731
    else:
        raise KeyError(name)
    return Matrix(len(lens), cols, tuple(lens), col_of, values(seed + len(lens)))


def structures(T, chunk):
    names = ["nnz:%d" % n for n in sorted({0, 1, 255, 256, 257, T - 1, T, T + 1, 2 * T + 300})]
    names += ["ones:%d" % (T + 9), "one_row:%d" % (2 * T + 300), "one_row:%d" % T, "chunk_rows", "row_ends:0", "row_ends:1", "row_ends:2", "empties", "empties_at_tile_boundary",
              "tail_shorts_head", "tile_inside_a_row", "descending_and_repeated_columns", "one_column", "dense_column"]
    return names


@functools.lru_cache(maxsize=None)
def worst(T):
    """one full-tile row, every value and every x 2^256 - 1: the largest sums the scan sees"""
    return Matrix(1, 4, (T,), lambda r, i, e: e % 4, lambda *at: TOP), pack([TOP] * 4, 32)


# ---- the model: Python integers ---------------------------------------------------------------------------------------------------
def decode(v, mont):
    ia = pow(A, -1, P)
    return [x * ia % P for x in v] if mont else [x % P for x in v]


def encode(v, mont):
    return [x * A % P for x in v] if mont else [x % P for x in v]


def model(M, x, count=1, mflags=0, flags=0):
    """te_msm_spmv on wire bytes -> out bytes, straight from the definition (TRANSPOSE: the definition on the transposed matrix)"""
    vals, xs = decode(M.val, mflags & MATRIX_MONTGOMERY), decode(unpack(x, 32), flags & SPMV_MONTGOMERY)
    tr = bool(flags & SPMV_TRANSPOSE)
    n_in, n_out = (M.rows, M.cols) if tr else (M.cols, M.rows)
    assert len(xs) == count * n_in
    rows = M.row_of()
    out = [0] * (count * n_out)
    for k in range(count):
        for e in range(M.nnz):
            r, c = (M.col[e], rows[e]) if tr else (rows[e], M.col[e])
            out[k * n_out + r] += vals[e] * xs[k * n_in + c]
    return pack(encode([v % P for v in out], flags & SPMV_MONTGOMERY), 32)


@functools.lru_cache(maxsize=None)
def expected(name, T, chunk, count, mflags, flags, seed=0):
    """(matrix, x, out) of a named case, computed once and shared"""
    M = structure(name, T, chunk, seed)
    x = vector(count * (M.rows if flags & SPMV_TRANSPOSE else M.cols), seed + count)
    return M, x, model(M, x, count, mflags, flags)


def emulate(L, M, x, count=1, mflags=0, flags=0, chunk=0, mistake=0, fill=0xA5, null=None, in_place=False, dims=None, ptr=None, col=None):
    """(rc, out bytes, reason, bad position): spmv_emulate; out starts as `fill` bytes"""
    rows, cols = dims or (M.rows, M.cols)
    n_out = cols if flags & SPMV_TRANSPOSE else rows
    size = max(1, 32 * min(count, 8) * min(n_out, 1 << 20))
    keep = lambda b: ctypes.create_string_buffer(bytes(b), max(1, len(b)))            # noqa: E731
    bp, bc, bv, bx = keep(ptr or M.ptr_bytes), keep(col or M.col_bytes), keep(M.val_bytes), keep(x)
    out = bx if in_place else ctypes.create_string_buffer(bytes([fill]) * size, size)
    why, bad = ctypes.c_int(), ctypes.c_int64(-1)
    arg = lambda name, b: None if null == name else ctypes.addressof(b)               # noqa: E731
    rc = L.spmv_emulate(rows, cols, arg("ptr", bp), arg("col", bc), arg("vals", bv), mflags, arg("x", bx), count, flags, chunk, mistake, arg("out", out),
                        ctypes.byref(why), ctypes.byref(bad))
    return rc, out.raw[:32 * count * n_out], why.value, bad.value


def sides(L, M, mistake=0):
    """(row, t_ptr, t_col, t_row, t_val) as the shim's bind lays them down"""
    row = (ctypes.c_uint32 * max(1, M.nnz))()
    t_ptr = (ctypes.c_uint64 * (M.cols + 1))()
    t_col, t_row = (ctypes.c_uint32 * max(1, M.nnz))(), (ctypes.c_uint32 * max(1, M.nnz))()
    t_val = ctypes.create_string_buffer(max(1, 32 * M.nnz))
    assert L.spmv_sides(M.rows, M.cols, M.ptr_bytes, M.col_bytes, M.val_bytes, mistake, row, t_ptr, t_col, t_row, t_val) == 0
    return list(row)[:M.nnz], list(t_ptr), list(t_col)[:M.nnz], list(t_row)[:M.nnz], unpack(t_val.raw[:32 * M.nnz], 32)
