"""Batched NTTs on the GPU (te_msm_ntt*; include/te_msm.h "batched NTTs"): byte-equal to the textbook transform of the host shim
(tests/csrc/nttcheck.cpp, itself pinned to Python integers in tests/test_ntt_host.py) at every size up to the first one that runs the
plan's largest number of passes, both directions, both forms, with and without a shift, device and host form, one and two slices, in
place and out of place; the batch counts that leave a block partly filled; 2^24 and a buffer past 2^32 bytes by closed forms; refusals;
the table's lifetime; and the use it is for -- evaluations to coefficients to an MSM without leaving the device."""
import ctypes
import functools
import os
import random

import pytest

import field_cases as fc
import ntt_cases as nc

pytestmark = pytest.mark.gpu

PAT = 0xAB
P = nc.P


@pytest.fixture(scope="module")
def L():
    return nc.shim()


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


def _shift(shift):
    return None if shift is None else int(shift).to_bytes(32, "little")


def on_device(c, a, log_n, count=1, flags=0, shift=None, in_place=False):
    """te_msm_ntt_device -> (status, output bytes); out of place, the output starts as a pattern"""
    import torch
    da = _dev(a)
    dout = da if in_place else torch.full((max(1, len(a)),), PAT, dtype=torch.uint8, device="cuda")
    _sync()
    rc = c._L.te_msm_ntt_device(c._h, da.data_ptr(), log_n, count, flags, _shift(shift), dout.data_ptr())
    return rc, bytes(dout.cpu().numpy())[:len(a)]


def on_host(c, a, log_n, count=1, flags=0, shift=None, in_place=False):
    src = ctypes.create_string_buffer(bytes(a), max(1, len(a)))
    out = src if in_place else ctypes.create_string_buffer(bytes([PAT]) * max(1, len(a)), max(1, len(a)))
    rc = c._L.te_msm_ntt(c._h, ctypes.addressof(src), log_n, count, flags, _shift(shift), ctypes.addressof(out))
    return rc, out.raw[:len(a)]


@functools.lru_cache(maxsize=None)
def _case(log_n, count, flags, shift):
    """(input, what ntt_ref makes of it): computed once, shared by the tests"""
    a = nc.values(count << log_n, seed=log_n)
    return a, nc.ref(nc.shim(), a, log_n, count, flags, shift)


def _top():
    return nc.top_log_n(nc.shim())


# ---- 1. every size, direction, form and shift, against the textbook ----------------------------------------------------------------
@pytest.mark.parametrize("flags", nc.FLAGS)
@pytest.mark.parametrize("log_n", range(0, 18))
def test_device_form_matches_ref(one, L, log_n, flags):
    assert _top() == 17                                             # the range above: 0 .. the first size of three passes
    for k, shift in enumerate(nc.SHIFTS):
        a, want = _case(log_n, 1, flags, shift)
        assert on_device(one, a, log_n, 1, flags, shift, in_place=bool((k + flags + log_n) & 1)) == (0, want), (log_n, flags, shift)


@pytest.mark.parametrize("log_n", range(0, 18))
def test_host_form_on_one_and_two_slices(one, two, L, log_n):
    """three transforms: slices of two and one on a context of two devices; every flag and shift comes round over the sizes"""
    for step in (0, 1):
        flags, shift = nc.FLAGS[(log_n + step) % 4], nc.SHIFTS[(log_n + 2 * step) % 3]
        a, want = _case(log_n, 3, flags, shift)
        assert on_host(one, a, log_n, 3, flags, shift, in_place=bool(step)) == (0, want), (log_n, flags, shift)
        assert on_host(two, a, log_n, 3, flags, shift, in_place=not step) == (0, want), (log_n, flags, shift)
        assert on_device(one, a, log_n, 3, flags, shift, in_place=bool(step)) == (0, want), (log_n, flags, shift)


@pytest.mark.parametrize("log_n", range(0, 5))
def test_batch_counts_around_a_block(one, L, log_n):
    per_tile = nc.plan_info(L, log_n)["per_tile"]
    assert per_tile == 1024 >> log_n
    for k, count in enumerate(nc.batch_counts(per_tile)):
        flags, shift = nc.FLAGS[k % 4], nc.SHIFTS[k % 3]
        a, want = _case(log_n, count, flags, shift)
        assert on_device(one, a, log_n, count, flags, shift, in_place=bool(k & 1)) == (0, want), (log_n, count)
        if count in (per_tile + 1, 1000):
            assert on_host(one, a, log_n, count, flags, shift) == (0, want), (log_n, count)


def test_python_methods(pkg, one, L):
    a, want = _case(6, 2, nc.INVERSE | nc.MONTGOMERY, 22)
    assert one.ntt(a, 6, count=2, inverse=True, montgomery=True, shift=22) == want
    assert one.ntt(a, 6, count=2, inverse=True, montgomery=True, shift=(22).to_bytes(32, "little")) == want
    assert one.ntt(b"", 3, count=0) == b""
    da = _dev(a)
    _sync()
    one.ntt_device(da.data_ptr(), 6, 2, da.data_ptr(), inverse=True, montgomery=True, shift=22)
    assert bytes(da.cpu().numpy()) == want
    with pytest.raises(pkg.MsmError):
        one.ntt(a, 6, count=2, shift=0)
    with pytest.raises(pkg.MsmError):
        one.ntt(a, 7, count=2)
    assert (pkg.NTT_INVERSE, pkg.NTT_MONTGOMERY, pkg.NTT_MAX_LOG_N) == (1, 2, 24) and one.get_option("ntt_max_log_n") == 24


# ---- 2. the largest size ----------------------------------------------------------------------------------------------------------
def _records(n):
    import torch
    return torch.zeros((n, 4), dtype=torch.int64, device="cuda")    # n records of 32 bytes, little-endian words of 64 bits


def test_largest_size_by_closed_forms(one, L):
    import torch
    log_n, n = 24, 1 << 24
    assert nc.plan_info(L, log_n)["passes"] == 3
    a, out = _records(n), torch.full((n, 4), -1, dtype=torch.int64, device="cuda")
    a[:, 0] = 1
    _sync()
    assert one._L.te_msm_ntt_device(one._h, a.data_ptr(), log_n, 1, 0, None, out.data_ptr()) == 0
    want = _records(n)
    want[0, 0] = n
    assert torch.equal(out, want)                                   # all ones -> n delta_0, in full
    del want, out
    k = n - 12345                                                   # odd and large
    a.zero_()
    a[k, 0] = 1
    delta = a.clone()
    _sync()
    assert one._L.te_msm_ntt_device(one._h, a.data_ptr(), log_n, 1, 0, None, a.data_ptr()) == 0
    rnd = random.Random(24)
    js = sorted(set(nc.tile_corners(L, log_n)) | {0, 1, n - 1, n // 2} | {rnd.randrange(n) for _ in range(4096)})[:4200]
    assert len(js) >= 4096
    got = a[torch.tensor(js, device="cuda")].cpu().numpy().tobytes()
    w = nc.omega(log_n)
    assert got == nc.pack([pow(w, j * k % n, P) for j in js], 32)   # delta_k -> w^(j k)
    assert one._L.te_msm_ntt_device(one._h, a.data_ptr(), log_n, 1, nc.INVERSE, None, a.data_ptr()) == 0
    assert torch.equal(a, delta)                                    # and back, exactly, in full


def test_buffer_past_4_gib(one, L):
    """129 transforms of 2^20 in place: 129 * 2^25 bytes.  Zeros stay zeros; the all-ones transform at the far end becomes n delta_0"""
    import torch
    log_n, n, count = 20, 1 << 20, 129
    assert count * n * 32 > 1 << 32 and nc.plan_info(L, log_n)["piece"] < count
    a = _records(count * n)
    a[(count - 1) * n:, 0] = 1
    _sync()
    assert one._L.te_msm_ntt_device(one._h, a.data_ptr(), log_n, count, 0, None, a.data_ptr()) == 0
    assert int(a[(count - 1) * n, 0]) == n
    a[(count - 1) * n, 0] = 0
    assert not bool(a.any())


# ---- 3. refusals; the tables' lifetime -----------------------------------------------------------------------------------------------
def test_refusals_leave_the_output(two):
    a = nc.values(8)
    untouched = (nc.EINVAL, bytes([PAT]) * len(a))
    c = two
    for log_n, flags, shift in ((25, 0, None), (1 << 20, 0, None), (3, 4, None), (3, 1 << 16, None), (3, 0, 0), (3, nc.INVERSE, 0), (3, 0, P), (3, nc.INVERSE, P),
                                (3, nc.MONTGOMERY, 2 * P)):
        assert on_device(c, a, log_n, 1, flags, shift) == untouched, (log_n, flags, shift)
        assert on_host(c, a, log_n, 1, flags, shift) == untouched, (log_n, flags, shift)
    da = _dev(a)
    _sync()
    host = ctypes.create_string_buffer(a, len(a))                   # a buffer on no device of the context
    assert c._L.te_msm_ntt_device(c._h, da.data_ptr(), 3, 1, 0, None, ctypes.addressof(host)) == nc.EINVAL
    assert c._L.te_msm_ntt_device(c._h, ctypes.addressof(host), 3, 1, 0, None, da.data_ptr()) == nc.EINVAL
    assert c._L.te_msm_ntt_device(c._h, None, 3, 1, 0, None, da.data_ptr()) == nc.EINVAL
    assert c._L.te_msm_ntt_device(c._h, da.data_ptr(), 3, 1, 0, None, None) == nc.EINVAL
    assert c._L.te_msm_ntt(c._h, None, 3, 1, 0, None, host) == nc.EINVAL and c._L.te_msm_ntt(c._h, host, 3, 1, 0, None, None) == nc.EINVAL
    assert bytes(da.cpu().numpy()) == a and host.raw == a
    assert c._L.te_msm_ntt_device(c._h, None, 3, 0, 0, None, None) == 0 and c._L.te_msm_ntt(c._h, None, 3, 0, 0, None, None) == 0      # count = 0
    assert on_device(c, a, 3, 1, 0, None)[0] == 0                  # the context is usable


def test_tables_and_scratch_are_made_on_first_use_and_trimmed(pkg, L):
    a, want = _case(5, 1, 0, None)
    with pkg.MsmContext((0,)) as c:
        assert c.get_option("ntt_table_bytes") == 0
        assert on_device(c, a, 5, 1) == (0, want)
        held = c.get_option("ntt_table_bytes")
        assert held == nc.plan_info(L, 5)["table_bytes"] == 2 * 4096 * 48
        assert on_device(c, a, 5, 1, 0, 22)[0] == 0 and c.get_option("ntt_table_bytes") == held      # a shift's tables are the call's own
        assert c.get_option("ntt_scratch_bytes") == 0               # one pass: no buffer between passes
        b, want_b = _case(12, 3, 0, None)
        assert on_device(c, b, 12, 3) == (0, want_b) and c.get_option("ntt_scratch_bytes") == nc.plan_info(L, 12, 3)["tmp_records"] * 32 == 3 * 32 << 12
        assert on_device(c, b[:32 << 12], 12, 1)[0] == 0 and c.get_option("ntt_scratch_bytes") == 3 * 32 << 12      # grown on use, kept
        c.trim(0)
        assert c.get_option("ntt_table_bytes") == 0 and c.get_option("ntt_scratch_bytes") == 0
        assert on_device(c, a, 5, 1) == (0, want) and c.get_option("ntt_table_bytes") == held
        assert on_device(c, b, 12, 3) == (0, want_b)


# ---- 4. the chain the feature exists for ----------------------------------------------------------------------------------------------
def _poly_and_evals(log_n, seed):
    rnd = random.Random(seed)
    coeffs = [rnd.randrange(P) for _ in range(1 << log_n)]
    return coeffs, nc.fast(coeffs, log_n)                           # evaluations over the domain, in Python integers


@pytest.mark.parametrize("montgomery", [0, 1])
def test_evaluations_to_coefficients_to_an_msm_bls12_377(pkg, montgomery):
    """evaluations in device memory -> ntt_device(inverse) -> te_msm_run_scalars_device over a bound set, 32-byte records: the commitment
    to the polynomial, equal to the oracle's MSM over the Python coefficients; nothing crosses the link in between"""
    from oracle import oracle377
    log_n, n = 10, 1 << 10
    coeffs, evals = _poly_and_evals(log_n, 0x4B5A)
    pts = oracle377.gen_points(13, n)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        c.set_option("scalar_record_bytes", 32)
        c.set_option("scalars_montgomery", montgomery)
        bases = c.bind_points(pts)
        d = _dev(nc.pack([v * nc.A % P for v in evals] if montgomery else evals, 32))
        _sync()
        c.ntt_device(d.data_ptr(), log_n, 1, d.data_ptr(), inverse=True, montgomery=bool(montgomery))
        got = c.run_scalars_device(bases, d.data_ptr())
        bases.release()
    assert got == oracle377.msm(pts, nc.pack(coeffs, 48), threads=2)


def test_evaluations_to_coefficients_to_an_msm_twisted_edwards(pkg):
    """the same on the Twisted-Edwards curve, whose base field p is: the coefficients, canonical integers below p, are its MSM's scalars
    (its scalar field is another modulus, so only the canonical form chains there)"""
    from oracle import oracle
    log_n, n = 10, 1 << 10
    coeffs, evals = _poly_and_evals(log_n, 0x7E)
    pts = oracle.gen_points(17, n)
    with pkg.MsmContext((0,)) as c:
        bases = c.bind_points(pts)
        d = _dev(nc.pack(evals, 32))
        _sync()
        c.ntt_device(d.data_ptr(), log_n, 1, d.data_ptr(), inverse=True)
        got = c.run_scalars_device(bases, d.data_ptr())
        bases.release()
    assert got == oracle.msm(pts, nc.pack(coeffs, 32), threads=2)


def test_polynomial_product_by_pointwise_multiplication(pkg, one):
    """two polynomials of degree < 128 -> forward (n = 256, both in one call) -> field_op_device(MUL) -> inverse == the schoolbook product"""
    import torch
    rnd = random.Random(256)
    f, g = [rnd.randrange(P) for _ in range(128)], [rnd.randrange(P) for _ in range(128)]
    want = [0] * 256
    for i, x in enumerate(f):
        for j, y in enumerate(g):
            want[i + j] = (want[i + j] + x * y) % P
    d = _dev(nc.pack(f + [0] * 128 + g + [0] * 128, 32))
    prod = torch.empty(32 * 256, dtype=torch.uint8, device="cuda")
    _sync()
    one.ntt_device(d.data_ptr(), 8, 2, d.data_ptr())
    one.field_op_device(pkg.FIELD_MUL, d.data_ptr(), d.data_ptr() + 32 * 256, 256, prod.data_ptr())
    one.ntt_device(prod.data_ptr(), 8, 1, prod.data_ptr(), inverse=True)
    assert bytes(prod.cpu().numpy()) == nc.pack(want, 32)


# ---- the Node function -------------------------------------------------------------------------------------------------------------
def test_node_ntt(pkg, tmp_path):
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
    a, fwd = _case(7, 3, 0, 22)
    _, inv = _case(7, 3, nc.INVERSE | nc.MONTGOMERY, None)
    (tmp_path / "a.bin").write_bytes(a)
    (tmp_path / "s.bin").write_bytes((22).to_bytes(32, "little"))
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
(async () => {
  const a = fs.readFileSync(process.argv[2]), s = fs.readFileSync(process.argv[3]), out = {};
  out.fwd = (await m.ntt(a, 7, {count: 3, shift: s})).toString('hex');
  out.inv = (await m.ntt(a, 7, {count: 3, inverse: true, montgomery: true})).toString('hex');
  out.empty = (await m.ntt(Buffer.alloc(0), 7, {count: 0})).length;
  await m.ntt(a, 25).then(() => { out.bad = 'resolved'; }, (e) => { out.bad = String(e.message); });
  await m.ntt(a, 7, {count: 3, shift: Buffer.alloc(32)}).then(() => { out.zero = 'resolved'; }, (e) => { out.zero = String(e.message); });
  console.log(JSON.stringify(out));
})();
"""
    r = subprocess.run([node, "-e", script, js, str(tmp_path / "a.bin"), str(tmp_path / "s.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert bytes.fromhex(out["fwd"]) == fwd and bytes.fromhex(out["inv"]) == inv and out["empty"] == 0
    assert "te_msm error -1" in out["bad"] and "te_msm error -1" in out["zero"], out
