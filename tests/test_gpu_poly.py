"""Polynomial openings on the GPU (te_msm_poly_divide*; include/te_msm.h "polynomial openings"): byte-equal to the model in Python integers
(tests/poly_cases.py: the recurrence itself) at every length around a lane row, a tile and a tile of tiles, at the default chunk and at
chunk 1 (three levels at 65 537), both forms, one point each and a shared one, device and host form, one and two slices, in place and out
of place; evaluation only and quotient only; refusals; the scratch buffer's lifetime; and the use it is for -- evaluations to coefficients
to the witness polynomial to its MSM without leaving the device."""
import ctypes
import functools
import os
import random

import pytest

import field_cases as fc
import ntt_cases as nc
import poly_cases as pc

pytestmark = pytest.mark.gpu

PAT = 0xAB
P = pc.P
ALL_FLAGS = (0, pc.MONTGOMERY, pc.SHARED_Z, pc.MONTGOMERY | pc.SHARED_Z)


@pytest.fixture(scope="module")
def L():
    return pc.shim()


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


def on_device(c, a, n, z, count=1, flags=0, in_place=False, quotient=True, evals=True):
    """te_msm_poly_divide_device -> (status, evals bytes, q bytes); the outputs start as a pattern (in place: q is a)"""
    import torch
    da = _dev(a)
    dq = da if in_place else torch.full((max(1, len(a)),), PAT, dtype=torch.uint8, device="cuda")
    ev = ctypes.create_string_buffer(bytes([PAT]) * max(1, 32 * count), max(1, 32 * count))
    _sync()
    rc = c._L.te_msm_poly_divide_device(c._h, da.data_ptr(), n, count, z, flags, ev if evals else None, dq.data_ptr() if quotient else None)
    return rc, ev.raw[:32 * count], bytes(dq.cpu().numpy())[:len(a)]


def on_host(c, a, n, z, count=1, flags=0, in_place=False, quotient=True, evals=True):
    src = ctypes.create_string_buffer(bytes(a), max(1, len(a)))
    q = src if in_place else ctypes.create_string_buffer(bytes([PAT]) * max(1, len(a)), max(1, len(a)))
    ev = ctypes.create_string_buffer(bytes([PAT]) * max(1, 32 * count), max(1, 32 * count))
    rc = c._L.te_msm_poly_divide(c._h, ctypes.addressof(src), n, count, z, flags, ev if evals else None, ctypes.addressof(q) if quotient else None)
    return rc, ev.raw[:32 * count], q.raw[:len(a)]


def check_case(c, run, n, count, flags, seed, which=None, turn=0):
    """the call against the model: with the quotient (in place or out of place by turn), and -- every other turn -- one output alone"""
    a, z, ev, q = pc.expected(n, count, flags, seed, which)
    keep_q, keep_e = bytes([PAT]) * len(a), bytes([PAT]) * (32 * count)
    assert run(c, a, n, z, count, flags, in_place=bool(turn & 1)) == (0, ev, q), (n, count, flags, turn)
    if turn & 2:
        assert run(c, a, n, z, count, flags, quotient=False) == (0, ev, keep_q), ("evaluation only", n, count, flags)
    else:
        assert run(c, a, n, z, count, flags, evals=False, in_place=not turn & 1) == (0, keep_e, q), ("quotient only", n, count, flags)


# ---- 1. every length, count, form and point, against the model ------------------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_device_form_at_the_default_chunk(one, L, count, flags):
    chunk = pc.default_chunk(L)
    assert one.get_option("poly_chunk") == chunk
    for turn, n in enumerate(pc.lengths(pc.LANES * chunk, squares=False)):
        check_case(one, on_device, n, count, flags, seed=chunk, turn=turn + count)


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("flags", ALL_FLAGS)
def test_device_form_at_chunk_1_up_to_three_levels(one, L, monkeypatch, count, flags):
    monkeypatch.setenv("TE_MSM_POLY_CHUNK", "1")
    assert one.get_option("poly_chunk") == 1 and pc.plan_info(L, 65537, chunk=1)["levels"] == 3
    for turn, n in enumerate(pc.lengths(pc.LANES, squares=True)):
        if n > 4 * pc.LANES and (count == 3) != bool(flags & pc.SHARED_Z):       # the squares: count 1 with a point each, count 3 with a shared one
            continue
        check_case(one, on_device, n, count, flags, seed=1, turn=turn + count)


@pytest.mark.parametrize("chunk", [0, 1, 4])
def test_host_form_on_one_and_two_slices(one, two, L, monkeypatch, chunk):
    """three polynomials: slices of two and one on a context of two devices, so that a slice boundary falls between polynomials"""
    if chunk:
        monkeypatch.setenv("TE_MSM_POLY_CHUNK", str(chunk))
    T = pc.LANES * (chunk or pc.default_chunk(L))
    for turn, n in enumerate(pc.lengths(T, squares=False)):
        flags = ALL_FLAGS[turn % 4]
        check_case(one, on_host, n, 3, flags, seed=chunk or pc.default_chunk(L), turn=turn)
        check_case(two, on_host, n, 3, flags, seed=chunk or pc.default_chunk(L), turn=turn + 1)


@pytest.mark.parametrize("which", pc.POINT_EXTREMES)
def test_points_at_the_extremes(one, L, monkeypatch, which):
    for chunk in (0, 1):
        if chunk:
            monkeypatch.setenv("TE_MSM_POLY_CHUNK", "1")
        T = pc.LANES * (chunk or pc.default_chunk(L))
        for turn, n in enumerate((1, 257, T + 1, 2 * T + 300)):
            for flags in (0, pc.MONTGOMERY | pc.SHARED_Z):
                check_case(one, on_device, n, 2, flags, seed=11, which=which, turn=turn)


def test_every_chunk_runs(one, monkeypatch):
    for chunk in range(1, pc.CHUNK_MAX + 1):
        monkeypatch.setenv("TE_MSM_POLY_CHUNK", str(chunk))
        n = pc.LANES * chunk + 77
        a, z, ev, q = pc.expected(n, 1, pc.MONTGOMERY, 21)
        assert on_device(one, a, n, z, 1, pc.MONTGOMERY, in_place=True) == (0, ev, q), chunk
    monkeypatch.setenv("TE_MSM_POLY_CHUNK", "17")                    # outside 1 .. 16: the default
    assert one.get_option("poly_chunk") == pc.default_chunk(pc.shim())


def test_python_methods(pkg, one):
    a, z, ev, q = pc.expected(300, 2, pc.MONTGOMERY, 8)
    assert one.poly_divide(a, 300, z, count=2, montgomery=True) == (ev, q)
    assert one.poly_divide(a, 300, pc.unpack(z, 32), count=2, montgomery=True, quotient=False) == (ev, None)
    a1, z1, ev1, q1 = pc.expected(300, 2, pc.SHARED_Z, 8)
    assert one.poly_divide(a1, 300, pc.unpack(z1, 32)[0], count=2, shared_z=True) == (ev1, q1)
    assert one.poly_divide(b"", 5, b"", count=0) == (b"", b"")
    da = _dev(a)
    _sync()
    assert one.poly_divide_device(da.data_ptr(), 300, 2, z, da.data_ptr(), montgomery=True) == ev
    assert bytes(da.cpu().numpy()) == q
    with pytest.raises(pkg.MsmError):
        one.poly_divide(a, 299, z, count=2)
    with pytest.raises(pkg.MsmError):
        one.poly_divide(a, 300, z[:32], count=2)
    assert (pkg.POLY_MONTGOMERY, pkg.POLY_SHARED_Z, pkg.POLY_MAX_N) == (1, 2, 1 << 30)


# ---- 2. evaluation only writes nothing but the scratch buffer ------------------------------------------------------------------------
def test_evaluation_only_leaves_device_memory_alone(one, L):
    """the coefficients sit between two guard bands in one allocation; with d_q NULL every byte of it is as it was"""
    import torch
    n, count = 2 * pc.LANES * pc.default_chunk(L) + 300, 3
    a, z, ev, _ = pc.expected(n, count, 0, 40)
    band = 1 << 16
    whole = torch.full((2 * band + len(a),), PAT, dtype=torch.uint8, device="cuda")
    whole[band:band + len(a)] = _dev(a)
    before = whole.clone()
    out = ctypes.create_string_buffer(32 * count)
    _sync()
    assert one._L.te_msm_poly_divide_device(one._h, whole.data_ptr() + band, n, count, z, 0, out, None) == 0
    assert out.raw == ev and torch.equal(whole, before)
    assert one.get_option("poly_scratch_bytes") >= pc.plan_info(L, n, count)["scratch_bytes"]


# ---- 3. refusals; the scratch buffer's lifetime ------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs(two):
    import torch
    c = two
    a, z = pc.values(16), pc.points(2)
    untouched = (pc.EINVAL, bytes([PAT]) * 64, bytes([PAT]) * len(a))
    for n, flags in ((0, 0), (pc.MAX_N + 1, 0), (8, 4), (8, 1 << 16)):
        assert on_device(c, a, n, z, 2, flags) == untouched, (n, flags)
        assert on_host(c, a, n, z, 2, flags) == untouched, (n, flags)
    assert on_device(c, a, 8, None, 2, 0) == untouched and on_host(c, a, 8, None, 2, 0) == untouched                  # a NULL z
    assert on_device(c, a, 8, z, 2, 0, quotient=False, evals=False)[0] == pc.EINVAL                                # both outputs NULL
    assert on_host(c, a, 8, z, 2, 0, quotient=False, evals=False)[0] == pc.EINVAL
    da, dq = _dev(a), torch.full((len(a),), PAT, dtype=torch.uint8, device="cuda")
    _sync()
    host = ctypes.create_string_buffer(a, len(a))                   # a buffer on no device of the context
    ev = ctypes.create_string_buffer(bytes([PAT]) * 64, 64)
    assert c._L.te_msm_poly_divide_device(c._h, da.data_ptr(), 8, 2, z, 0, ev, ctypes.addressof(host)) == pc.EINVAL
    assert c._L.te_msm_poly_divide_device(c._h, ctypes.addressof(host), 8, 2, z, 0, ev, dq.data_ptr()) == pc.EINVAL
    assert c._L.te_msm_poly_divide_device(c._h, ctypes.addressof(host), 8, 2, z, 0, ev, None) == pc.EINVAL
    assert c._L.te_msm_poly_divide_device(c._h, None, 8, 2, z, 0, ev, dq.data_ptr()) == pc.EINVAL
    assert c._L.te_msm_poly_divide_device(c._h, da.data_ptr(), 1 << 30, 1 << 30, z, 0, ev, dq.data_ptr()) == pc.EINVAL      # count x n x 32 = 2^65
    if torch.cuda.device_count() > 1:                               # d_a and d_q on two devices
        with torch.cuda.device(1):
            far = torch.full((len(a),), PAT, dtype=torch.uint8, device="cuda:1")
            torch.cuda.synchronize()
        assert c._L.te_msm_poly_divide_device(c._h, da.data_ptr(), 8, 2, z, 0, ev, far.data_ptr()) == pc.EINVAL
        assert bytes(far.cpu().numpy()) == bytes([PAT]) * len(a)
    assert c._L.te_msm_poly_divide(c._h, None, 8, 2, z, 0, ev, host) == pc.EINVAL
    assert bytes(da.cpu().numpy()) == a and host.raw == a and ev.raw == bytes([PAT]) * 64 and bytes(dq.cpu().numpy()) == bytes([PAT]) * len(a)
    assert c._L.te_msm_poly_divide_device(c._h, None, 8, 0, None, 0, ev, None) == 0 and c._L.te_msm_poly_divide(c._h, None, 8, 0, None, 0, None, host) == 0      # count = 0
    assert ev.raw == bytes([PAT]) * 64 and host.raw == a
    assert on_device(c, a, 8, z, 2, 0)[1:] == pc.model(a, 8, z, 2, 0)      # the context is usable


def test_scratch_grows_on_use_and_is_trimmed(pkg, L):
    chunk = pc.default_chunk(L)
    n = 2 * pc.LANES * chunk + 300
    a, z, ev, q = pc.expected(n, 1, 0, chunk)
    a3, z3, ev3, q3 = pc.expected(n, 3, 0, chunk)
    with pkg.MsmContext((0,)) as c:
        assert c.get_option("poly_scratch_bytes") == 0
        assert on_device(c, a, n, z) == (0, ev, q)
        small = c.get_option("poly_scratch_bytes")
        assert small == pc.plan_info(L, n, 1)["scratch_bytes"] == 32 * 4 + 2 * 18 * 48
        assert on_device(c, a3, n, z3, 3) == (0, ev3, q3)
        grown = c.get_option("poly_scratch_bytes")
        assert grown == pc.plan_info(L, n, 3)["scratch_bytes"] > small
        assert on_device(c, a, n, z) == (0, ev, q) and c.get_option("poly_scratch_bytes") == grown      # grown on use, kept
        c.trim(0)
        assert c.get_option("poly_scratch_bytes") == 0
        assert on_device(c, a3, n, z3, 3, in_place=True) == (0, ev3, q3) and c.get_option("poly_scratch_bytes") == grown


# ---- 4. the chain the feature exists for ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", [0, 1])
def test_evaluations_to_the_opening_msm_bls12_377(pkg, montgomery):
    """evaluations in device memory -> ntt_device(inverse) -> poly_divide_device in place -> te_msm_run_scalars_device over the first n - 1
    records against a bound set of n - 1 points: the opening's witness commitment, equal to the oracle's MSM over the model's quotient.
    Nothing but z, a(z) and the MSM result crosses the link."""
    from oracle import oracle377
    log_n, n = 12, 1 << 12
    rnd = random.Random(0x0BE + montgomery)
    coeffs = [rnd.randrange(P) for _ in range(n)]
    evals = nc.fast(coeffs, log_n)
    z = rnd.randrange(P)
    az, quot = pc.horner(coeffs, z)
    pts = oracle377.gen_points(23, n - 1)
    wire = (lambda v: [x * pc.A % P for x in v]) if montgomery else (lambda v: v)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        c.set_option("scalar_record_bytes", 32)
        c.set_option("scalars_montgomery", montgomery)
        bases = c.bind_points(pts)
        d = _dev(pc.pack(wire(evals), 32))
        _sync()
        c.ntt_device(d.data_ptr(), log_n, 1, d.data_ptr(), inverse=True, montgomery=bool(montgomery))
        got_az = c.poly_divide_device(d.data_ptr(), n, 1, wire([z]), d.data_ptr(), montgomery=bool(montgomery))
        got = c.run_scalars_device(bases, d.data_ptr())
        bases.release()
    assert got_az == pc.pack(wire([az]), 32)
    assert got == oracle377.msm(pts, pc.pack(quot[:n - 1], 48), threads=2)


# ---- the Node function -------------------------------------------------------------------------------------------------------------
def test_node_poly_divide(pkg, tmp_path):
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
    a, z, ev, q = pc.expected(300, 3, pc.MONTGOMERY, 8)
    a1, z1, ev1, _ = pc.expected(300, 3, pc.SHARED_Z, 8)
    assert a1 == a
    (tmp_path / "a.bin").write_bytes(a)
    (tmp_path / "z.bin").write_bytes(z)
    (tmp_path / "z1.bin").write_bytes(z1)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
(async () => {
  const a = fs.readFileSync(process.argv[2]), z = fs.readFileSync(process.argv[3]), z1 = fs.readFileSync(process.argv[4]), out = {};
  const r = await m.polyDivide(a, 300, z, {count: 3, montgomery: true});
  out.evals = r.evals.toString('hex'); out.quotient = r.quotient.toString('hex');
  const e = await m.polyDivide(a, 300, z1, {count: 3, sharedZ: true, quotient: false});
  out.evals1 = e.evals.toString('hex'); out.none = e.quotient === null;
  await m.polyDivide(a, 0, z, {count: 3}).then(() => { out.bad = 'resolved'; }, (x) => { out.bad = String(x.message); });
  await m.polyDivide(a, 300, z1, {count: 3}).then(() => { out.short = 'resolved'; }, (x) => { out.short = String(x.message); });
  console.log(JSON.stringify(out));
})();
"""
    r = subprocess.run([node, "-e", script, js, str(tmp_path / "a.bin"), str(tmp_path / "z.bin"), str(tmp_path / "z1.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert bytes.fromhex(out["evals"]) == ev and bytes.fromhex(out["quotient"]) == q and bytes.fromhex(out["evals1"]) == ev1 and out["none"] is True
    assert out["bad"] != "resolved" and out["short"] != "resolved", out
