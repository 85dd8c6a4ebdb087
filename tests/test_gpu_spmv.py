"""Sparse matrix-vector products on the GPU (te_msm_bind_matrix, te_msm_spmv*; include/te_msm.h "sparse matrices"): byte-equal to the model in
Python integers (tests/spmv_cases.py: the definition itself) over every size and row structure at chunk 1 (T = 256) and at the default
chunk, count 1 and 3, the four combinations of the Montgomery flags, the transpose, the device form between guard bands and the host
form on one and two slices; the worst magnitude; refusals with the output compared untouched; the lifetimes of the options; the Python
methods and the Node function; and the use it is for -- Az, Bz, Cz of a satisfiable R1CS to the quotient's coefficients and their MSM
without leaving the device."""
import ctypes
import os
import random

import pytest

import field_cases as fc
import ntt_cases as nc
import spmv_cases as sc

pytestmark = pytest.mark.gpu

PAT = 0xAB
BAND = 1 << 12
P = sc.P
ALL_M = (0, sc.MATRIX_MONTGOMERY)
ALL_X = (0, sc.SPMV_MONTGOMERY)


@pytest.fixture(scope="module")
def L():
    return sc.shim()


@pytest.fixture(scope="module")
def one(pkg):
    with pkg.MsmContext((0,)) as c:
        yield c


@pytest.fixture(scope="module")
def two(pkg):
    with pkg.MsmContext((0, 0)) as c:
        yield c


def _dev(buf):
    import torch
    return torch.frombuffer(bytearray(buf or b"\0"), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def bind(c, M, mflags=0):
    h = ctypes.c_void_p()
    rc = c._L.te_msm_bind_matrix(c._h, M.rows, M.cols, M.ptr_bytes, M.col_bytes or None, M.val_bytes or None, mflags, ctypes.byref(h))
    assert rc == 0, c.last_error() if hasattr(c, "last_error") else rc
    return h


def release(c, h):
    assert c._L.te_msm_release_matrix(c._h, h) == 0


def on_device(c, h, x, n_out, count=1, flags=0):
    """te_msm_spmv_device -> (status, out bytes); out starts as a pattern and lies between two guard bands, which must stay as they were"""
    import torch
    dx = _dev(x)
    size = 32 * count * n_out
    whole = torch.full((2 * BAND + max(1, size),), PAT, dtype=torch.uint8, device="cuda")
    _sync()
    rc = c._L.te_msm_spmv_device(c._h, h, dx.data_ptr(), count, flags, whole.data_ptr() + BAND)
    got = bytes(whole.cpu().numpy())
    assert got[:BAND] == bytes([PAT]) * BAND and got[BAND + size:] == bytes([PAT]) * (len(got) - BAND - size), "a guard band was written"
    assert bytes(dx.cpu().numpy())[:len(x)] == x
    return rc, got[BAND:BAND + size]


def on_host(c, h, x, n_out, count=1, flags=0):
    size = 32 * count * n_out
    out = ctypes.create_string_buffer(bytes([PAT]) * max(1, size), max(1, size))
    rc = c._L.te_msm_spmv(c._h, h, x, count, flags, out)
    return rc, out.raw[:size]


def check_structure(c, run, name, chunk, count, mflags, xflags, both_sides=True):
    T = sc.LANES * chunk
    M = sc.structure(name, T, chunk)
    h = bind(c, M, mflags | sc.MATRIX_TRANSPOSE)
    try:
        for tr in (0, sc.SPMV_TRANSPOSE) if both_sides else (0,):
            M, x, want = sc.expected(name, T, chunk, count, mflags, xflags | tr)
            assert run(c, h, x, M.cols if tr else M.rows, count, xflags | tr) == (0, want), (name, chunk, count, mflags, xflags, tr)
    finally:
        release(c, h)


# ---- 1. every size, row structure, count and form, against the model --------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("chunk", [0, 1])
def test_device_form_over_every_structure(one, L, monkeypatch, chunk, count):
    if chunk:
        monkeypatch.setenv("TE_MSM_SPMV_CHUNK", str(chunk))
    chunk = chunk or sc.default_chunk(L)
    assert one.get_option("spmv_chunk") == chunk
    for turn, name in enumerate(sc.structures(sc.LANES * chunk, chunk)):
        check_structure(one, on_device, name, chunk, count, ALL_M[turn & 1], ALL_X[(turn >> 1) & 1])


@pytest.mark.parametrize("chunk", [0, 1])
def test_the_four_forms(one, L, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("TE_MSM_SPMV_CHUNK", str(chunk))
    chunk = chunk or sc.default_chunk(L)
    for mflags in ALL_M:
        for xflags in ALL_X:
            for name in ("tail_shorts_head", "dense_column"):
                check_structure(one, on_device, name, chunk, 2, mflags, xflags)


def test_worst_magnitude(one, L, monkeypatch):
    """one full-tile row, every value and every x 2^256 - 1"""
    for chunk in (sc.default_chunk(L), 1, sc.CHUNK_MAX):
        monkeypatch.setenv("TE_MSM_SPMV_CHUNK", str(chunk))
        M, x = sc.worst(sc.LANES * chunk)
        h = bind(one, M)
        assert on_device(one, h, x, 1) == (0, sc.model(M, x)), chunk
        release(one, h)


def test_every_chunk_runs(one, monkeypatch):
    for chunk in range(1, sc.CHUNK_MAX + 1):
        monkeypatch.setenv("TE_MSM_SPMV_CHUNK", str(chunk))
        check_structure(one, on_device, "tail_shorts_head", chunk, 1, 0, 0)
    monkeypatch.setenv("TE_MSM_SPMV_CHUNK", "17")                    # outside 1 .. 16: the default
    assert one.get_option("spmv_chunk") == sc.default_chunk(sc.shim())


@pytest.mark.parametrize("chunk", [0, 1])
def test_host_form_on_one_and_two_slices(one, two, L, monkeypatch, chunk):
    """three vectors: slices of two and one on a context of two devices"""
    if chunk:
        monkeypatch.setenv("TE_MSM_SPMV_CHUNK", str(chunk))
    chunk = chunk or sc.default_chunk(L)
    for turn, name in enumerate(("nnz:%d" % (2 * sc.LANES * chunk + 300), "tail_shorts_head", "empties", "dense_column", "nnz:0")):
        for c in (one, two):
            check_structure(c, on_host, name, chunk, 3, ALL_M[turn & 1], ALL_X[(turn >> 1) & 1])


def test_python_methods(pkg, one):
    M = sc.structure("tail_shorts_head", 256, 1)
    x = sc.vector(2 * M.cols, 4)
    mat = one.bind_matrix(M.rows, M.cols, M.ptr, M.col, M.val, transpose=True)
    assert (mat.rows, mat.cols, mat.nnz) == (M.rows, M.cols, M.nnz)
    r, k, z = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    assert one._L.te_msm_matrix_shape(mat._h, ctypes.byref(r), ctypes.byref(k), ctypes.byref(z)) == 0 and (r.value, k.value, z.value) == (M.rows, M.cols, M.nnz)
    assert one.spmv(mat, x, count=2) == sc.model(M, x, 2)
    y = sc.vector(M.rows, 5)
    assert one.spmv(mat, y, transpose=True, montgomery=True) == sc.model(M, y, 1, 0, sc.SPMV_TRANSPOSE | sc.SPMV_MONTGOMERY)
    assert one.spmv(mat, b"", count=0) == b""
    import torch
    dx, dout = _dev(x), torch.zeros(32 * 2 * M.rows, dtype=torch.uint8, device="cuda")
    _sync()
    one.spmv_device(mat, dx.data_ptr(), 2, dout.data_ptr())
    assert bytes(dout.cpu().numpy()) == sc.model(M, x, 2)
    with pytest.raises(pkg.MsmError):
        one.spmv(mat, x[:-32], count=2)
    mat.release()
    with pytest.raises(pkg.MsmError):
        one.spmv(mat, x, count=2)
    packed = one.bind_matrix(M.rows, M.cols, M.ptr_bytes, M.col_bytes, M.val_bytes)
    with pytest.raises(pkg.MsmError):
        one.spmv(packed, y, transpose=True)
    packed.release()
    assert (pkg.MATRIX_MONTGOMERY, pkg.MATRIX_TRANSPOSE, pkg.SPMV_MONTGOMERY, pkg.SPMV_TRANSPOSE) == (1, 2, 1, 2)


# ---- 2. refusals; the options' lifetimes -------------------------------------------------------------------------------------------
def test_bind_refusals(two):
    c = two
    M = sc.structure("nnz:600", 256, 1)
    h = ctypes.c_void_p()

    def try_bind(rows=M.rows, cols=M.cols, ptr=M.ptr_bytes, col=M.col_bytes, val=M.val_bytes, flags=0):
        rc = c._L.te_msm_bind_matrix(c._h, rows, cols, ptr, col, val, flags, ctypes.byref(h))
        assert (rc == 0) == bool(h.value)
        return rc
    before = c.get_option("matrix_bytes")
    bad_col = bytearray(M.col_bytes)
    for at in (77, 300):
        bad_col[4 * at:4 * at + 4] = (M.cols + at).to_bytes(4, "little")
    assert try_bind(rows=0) == sc.EINVAL and try_bind(cols=0) == sc.EINVAL
    assert try_bind(rows=sc.MAX_DIM + 1) == sc.EINVAL and try_bind(cols=sc.MAX_DIM + 1) == sc.EINVAL
    assert try_bind(ptr=(1).to_bytes(8, "little") + M.ptr_bytes[8:]) == sc.EINVAL
    assert try_bind(ptr=M.ptr_bytes[:40] + bytes(8) + M.ptr_bytes[48:]) == sc.EINVAL
    assert try_bind(col=bytes(bad_col)) == sc.EINVAL and c.get_option("bad_index_position") == 77
    assert try_bind(ptr=None) == sc.EINVAL and try_bind(col=None) == sc.EINVAL and try_bind(val=None) == sc.EINVAL
    assert try_bind(flags=4) == sc.EINVAL and try_bind(flags=-1) == sc.EINVAL
    assert c.get_option("matrix_bytes") == before
    assert try_bind() == 0                                            # the context is usable
    x = sc.vector(M.cols, 1)
    assert on_device(c, h, x, M.rows) == (0, sc.model(M, x))
    release(c, h)
    assert c._L.te_msm_release_matrix(c._h, h) == sc.EINVAL          # released once


def test_call_refusals_leave_the_output(two):
    import torch
    c = two
    M = sc.Matrix(40, 40, tuple([3] * 40), lambda r, i, e: (r + 7 * i) % 40, sc.values(9))
    x = sc.vector(2 * 40, 1)
    size = 32 * 2 * 40
    untouched = (sc.EINVAL, bytes([PAT]) * size)
    h, ht = bind(c, M), bind(c, M, sc.MATRIX_TRANSPOSE)
    for flags in (4, 1 << 16, -1):
        assert on_device(c, h, x, 40, 2, flags) == untouched and on_host(c, h, x, 40, 2, flags) == untouched, flags
    assert on_device(c, h, x, 40, 2, sc.SPMV_TRANSPOSE) == untouched and on_host(c, h, x, 40, 2, sc.SPMV_TRANSPOSE) == untouched
    assert on_device(c, ht, x, 40, 2, sc.SPMV_TRANSPOSE) == (0, sc.model(M, x, 2, 0, sc.SPMV_TRANSPOSE))
    assert on_device(c, None, x, 40, 2) == untouched and on_host(c, None, x, 40, 2) == untouched                        # no matrix
    dx, dout = _dev(x), torch.full((size,), PAT, dtype=torch.uint8, device="cuda")
    _sync()
    host = ctypes.create_string_buffer(x, len(x))                   # a buffer on no device of the context
    call = c._L.te_msm_spmv_device
    assert call(c._h, h, None, 2, 0, dout.data_ptr()) == sc.EINVAL and call(c._h, h, dx.data_ptr(), 2, 0, None) == sc.EINVAL
    assert call(c._h, h, dx.data_ptr(), 2, 0, dx.data_ptr()) == sc.EINVAL                                               # never in place
    assert call(c._h, h, ctypes.addressof(host), 2, 0, dout.data_ptr()) == sc.EINVAL and call(c._h, h, dx.data_ptr(), 2, 0, ctypes.addressof(host)) == sc.EINVAL
    assert call(c._h, h, dx.data_ptr(), 1 << 60, 0, dout.data_ptr()) == sc.EINVAL                                       # count x rows x 32 beyond 64 bits
    assert c._L.te_msm_spmv(c._h, h, None, 2, 0, host) == sc.EINVAL and c._L.te_msm_spmv(c._h, h, host, 2, 0, host) == sc.EINVAL
    if torch.cuda.device_count() > 1:                               # d_x and d_out on two devices
        with torch.cuda.device(1):
            far = torch.full((size,), PAT, dtype=torch.uint8, device="cuda:1")
            torch.cuda.synchronize()
        assert call(c._h, h, dx.data_ptr(), 2, 0, far.data_ptr()) == sc.EINVAL
        assert bytes(far.cpu().numpy()) == bytes([PAT]) * size
    assert bytes(dx.cpu().numpy()) == x and host.raw == x and bytes(dout.cpu().numpy()) == bytes([PAT]) * size
    assert call(c._h, h, None, 0, 0, None) == 0 and c._L.te_msm_spmv(c._h, h, None, 0, 0, None) == 0                    # count = 0
    assert bytes(dout.cpu().numpy()) == bytes([PAT]) * size
    assert on_device(c, h, x, 40, 2) == (0, sc.model(M, x, 2))      # the context is usable
    release(c, h)
    release(c, ht)


def test_option_lifetimes(pkg, L):
    chunk = sc.default_chunk(L)
    T = sc.LANES * chunk
    M = sc.structure("tail_shorts_head", T, chunk)
    x, x3 = sc.vector(M.cols, 1), sc.vector(3 * M.cols, 3)
    side = lambda rows: 40 * M.nnz + 8 * (rows + 1)                   # noqa: E731
    with pkg.MsmContext((0, 0)) as c:
        assert c.get_option("matrix_bytes") == 0 and c.get_option("spmv_scratch_bytes") == 0
        h = bind(c, M)
        assert c.get_option("matrix_bytes") == 2 * side(M.rows) == 2 * sc.plan_info(L, M.rows, M.cols, M.nnz)["side_bytes"]
        ht = bind(c, M, sc.MATRIX_TRANSPOSE)
        assert c.get_option("matrix_bytes") == 2 * (2 * side(M.rows) + side(M.cols))
        assert on_device(c, h, x, M.rows) == (0, sc.model(M, x))
        small = c.get_option("spmv_scratch_bytes")
        assert small == sc.plan_info(L, M.rows, M.cols, M.nnz, 1)["scratch_bytes"] == 64 * -(-M.nnz // T)
        assert on_device(c, h, x3, M.rows, 3) == (0, sc.model(M, x3, 3))
        grown = c.get_option("spmv_scratch_bytes")
        assert grown == 3 * small
        assert on_device(c, h, x, M.rows) == (0, sc.model(M, x)) and c.get_option("spmv_scratch_bytes") == grown      # grown on use, kept
        c.trim(0)
        assert c.get_option("spmv_scratch_bytes") == 0 and c.get_option("matrix_bytes") == 2 * (2 * side(M.rows) + side(M.cols))
        assert on_device(c, ht, x, M.rows) == (0, sc.model(M, x)) and c.get_option("spmv_scratch_bytes") == small
        release(c, ht)
        assert c.get_option("matrix_bytes") == 2 * side(M.rows)
        release(c, h)
        assert c.get_option("matrix_bytes") == 0
        bind(c, M, sc.MATRIX_TRANSPOSE)                              # left bound: te_msm_destroy frees it


# ---- 3. the chain the feature exists for ----------------------------------------------------------------------------------------------
def test_r1cs_to_the_quotient_and_its_msm(pkg):
    """A satisfiable R1CS of 2^10 constraints: random sparse A and B with the constant's column in every row, C with one entry a row
    chosen so that (Cz)_i = (Az)_i (Bz)_i.  z stays on the device: Az, Bz, Cz by te_msm_spmv_device, inverse NTTs, coset NTTs,
    (ab - c) / (g^n - 1) by te_msm_field_op_device, the coset inverse NTT -- the quotient's coefficients, equal to the Python-integer
    model, and their MSM over a bound set equal to the oracle's."""
    import torch
    from oracle import oracle377
    log_n, n, g = 10, 1 << 10, 22
    rnd = random.Random(0x51C5)
    z = [1] + [rnd.randrange(1, P) for _ in range(n - 1)]

    def sparse():
        lens = [2 + rnd.randrange(4) for _ in range(n)]
        return sc.Matrix(n, n, tuple(lens), lambda r, i, e: 0 if i == 0 else rnd.randrange(1, n), lambda r, i, e: rnd.choice((1, P - 1, rnd.randrange(P))))
    mA, mB = sparse(), sparse()
    zb = sc.pack(z, 32)
    az, bz = sc.unpack(sc.model(mA, zb), 32), sc.unpack(sc.model(mB, zb), 32)
    ccol = [1 + rnd.randrange(n - 1) for _ in range(n)]
    mC = sc.Matrix(n, n, tuple([1] * n), lambda r, i, e: ccol[r], lambda r, i, e: az[r] * bz[r] * pow(z[ccol[r]], -1, P) % P)
    cz = sc.unpack(sc.model(mC, zb), 32)
    assert cz == [a * b % P for a, b in zip(az, bz)]
    # the model of the quotient: (a(X) b(X) - c(X)) / (X^n - 1) through the coset g H, in Python integers
    on_coset = [nc.fast(nc.fast(v, log_n, inverse=True), log_n, s=g) for v in (az, bz, cz)]
    zh_inv = pow(pow(g, n, P) - 1, -1, P)
    quot = nc.fast([(a * b - c) * zh_inv % P for a, b, c in zip(*on_coset)], log_n, inverse=True, s=g)
    assert quot[n - 1] == 0                                          # degree n - 2: the system is satisfied
    pts = oracle377.gen_points(29, n)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        c.set_option("scalar_record_bytes", 32)
        bases = c.bind_points(pts)
        mats = [c.bind_matrix(m.rows, m.cols, m.ptr_bytes, m.col_bytes, m.val_bytes) for m in (mA, mB, mC)]
        dz = _dev(zb)
        abc = torch.zeros(3 * 32 * n, dtype=torch.uint8, device="cuda")
        _sync()
        at = [abc.data_ptr() + k * 32 * n for k in range(3)]
        for k in range(3):
            c.spmv_device(mats[k], dz.data_ptr(), 1, at[k])
        c.ntt_device(at[0], log_n, 3, at[0], inverse=True)
        c.ntt_device(at[0], log_n, 3, at[0], shift=g)
        c.field_op_device(pkg.FIELD_MUL, at[0], at[1], n, at[0])
        c.field_op_device(pkg.FIELD_SUB, at[0], at[2], n, at[0])
        dinv = _dev(sc.pack([zh_inv], 32))
        _sync()
        c.field_op_device(pkg.FIELD_MUL, at[0], dinv.data_ptr(), n, at[0], shared_b=True)
        c.ntt_device(at[0], log_n, 1, at[0], inverse=True, shift=g)
        got = bytes(abc.cpu().numpy())[:32 * n]
        msm = c.run_scalars_device(bases, at[0])
        for mat in mats:
            mat.release()
        bases.release()
    assert got == sc.pack(quot, 32)
    assert msm == oracle377.msm(pts, sc.pack(quot, 48), threads=2)


# ---- the Node function -------------------------------------------------------------------------------------------------------------
def test_node_spmv(pkg, tmp_path):
    import json
    import shutil
    import subprocess
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not installed on this box")
    js = os.path.join(fc.ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists("/usr/include/node/node_api.h") and not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        pytest.skip("no N-API addon and no node headers to build it")
    if not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        subprocess.check_call(["make", "-C", js, "-s"])
    M = sc.structure("tail_shorts_head", 256, 1)
    x, y = sc.vector(2 * M.cols, 4), sc.vector(M.rows, 5)
    for name, data in (("ptr", M.ptr_bytes), ("col", M.col_bytes), ("val", M.val_bytes), ("x", x), ("y", y)):
        (tmp_path / (name + ".bin")).write_bytes(data)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
const rd = (n) => fs.readFileSync(process.argv[2] + '/' + n + '.bin');
(async () => {
  const out = {};
  const rows = Number(process.argv[3]), cols = Number(process.argv[4]);
  const id = await m.bindMatrix(rows, cols, rd('ptr'), rd('col'), rd('val'), {transpose: true});
  out.a = (await m.spmv(id, rd('x'), {count: 2})).toString('hex');
  out.t = (await m.spmv(id, rd('y'), {transpose: true, montgomery: true})).toString('hex');
  await m.spmv(id, rd('x'), {count: 3}).then(() => { out.short = 'resolved'; }, (e) => { out.short = String(e.message); });
  await m.spmv(id + 99, rd('x'), {count: 2}).then(() => { out.none = 'resolved'; }, (e) => { out.none = String(e.message); });
  await m.bindMatrix(0, cols, rd('ptr'), rd('col'), rd('val')).then(() => { out.bad = 'resolved'; }, (e) => { out.bad = String(e.message); });
  m.releaseMatrix(id);
  await m.spmv(id, rd('x'), {count: 2}).then(() => { out.gone = 'resolved'; }, (e) => { out.gone = String(e.message); });
  console.log(JSON.stringify(out));
})();
"""
    r = subprocess.run([node, "-e", script, js, str(tmp_path), str(M.rows), str(M.cols)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert bytes.fromhex(out["a"]) == sc.model(M, x, 2) and bytes.fromhex(out["t"]) == sc.model(M, y, 1, 0, sc.SPMV_TRANSPOSE | sc.SPMV_MONTGOMERY)
    assert "resolved" not in (out["short"], out["none"], out["bad"], out["gone"]), out
