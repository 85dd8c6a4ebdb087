"""Prefix sums and products on the GPU (te_msm_field_scan*; include/te_msm.h "prefix sums and products"): byte-equal to the model in Python
integers (tests/scan_cases.py: the definition itself) at every length around a lane row, a tile and a tile of tiles, at the default chunk
and at chunk 1 (three levels at 65 537), both ops, modes and forms, with and without seeds, shared and not, device and host form, one and two
slices, in place and out of place, between guard bands; totals only and out only; refusals; the scratch buffer's lifetime; and the two uses
it is for -- a grand product from its factors to the MSM over its coefficients, and the powers of tau into an SRS -- without leaving the
device."""
import ctypes
import os
import random

import pytest

from oracle import model as m
import field_cases as fc
import mul_base_cases as mc
import ntt_cases as nc
import scan_cases as sc

pytestmark = pytest.mark.gpu

PAT = 0xAB
BAND = 4096
P = sc.P


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


def on_device(c, op, a, n, count=1, flags=0, init=None, in_place=False, want_out=True, want_totals=True):
    """te_msm_field_scan_device -> (status, out bytes, totals bytes); out lies between two guard bands of one allocation and totals between
    two of a host buffer, all a pattern at the start (in place: out is a, between its bands), and the bands are as they were"""
    import torch
    out_len = 32 * count * n
    size = max(len(a), out_len) if in_place else out_len
    whole = torch.full((2 * BAND + max(1, size),), PAT, dtype=torch.uint8, device="cuda")
    da = whole[BAND:] if in_place else _dev(a)
    if in_place:
        whole[BAND:BAND + len(a)] = _dev(a)
    tot = ctypes.create_string_buffer(bytes([PAT]) * (64 + 32 * count), 64 + 32 * count)
    _sync()
    rc = c._L.te_msm_field_scan_device(c._h, op, da.data_ptr(), n, count, flags, init, ctypes.addressof(tot) + 32 if want_totals else None,
                                       whole.data_ptr() + BAND if want_out else None)
    got = bytes(whole.cpu().numpy())
    band = bytes([PAT]) * BAND
    assert got[:BAND] == band and got[BAND + size:] == band, "a guard band of out changed"
    assert tot.raw[:32] == bytes([PAT]) * 32 == tot.raw[32 + 32 * count:], "a guard band of totals changed"
    return rc, got[BAND:BAND + out_len], tot.raw[32:32 + 32 * count]


def on_host(c, op, a, n, count=1, flags=0, init=None, in_place=False, want_out=True, want_totals=True):
    out_len = 32 * count * n
    src = ctypes.create_string_buffer(bytes(a), max(1, len(a)))
    out = src if in_place else ctypes.create_string_buffer(bytes([PAT]) * max(1, out_len), max(1, out_len))
    tot = ctypes.create_string_buffer(bytes([PAT]) * max(1, 32 * count), max(1, 32 * count))
    rc = c._L.te_msm_field_scan(c._h, op, ctypes.addressof(src), n, count, flags, init, tot if want_totals else None, ctypes.addressof(out) if want_out else None)
    return rc, out.raw[:out_len], tot.raw[:32 * count]


def check_case(c, run, op, n, count, flags, seed, turn=0):
    """the call against the model: both outputs (in place or out of place by turn; a seed or none by turn), and one output alone"""
    with_init = bool(turn & 4) or n > 4096
    a, init, out, tot = sc.expected(op, n, count, flags, seed, with_init)
    keep_o, keep_t = bytes([PAT]) * len(out), bytes([PAT]) * (32 * count)
    in_place = bool(turn & 1) and not flags & sc.SHARED_A
    assert run(c, op, a, n, count, flags, init, in_place=in_place) == (0, out, tot), (op, n, count, flags, turn)
    if turn & 2:
        assert run(c, op, a, n, count, flags, init, want_out=False) == (0, keep_o, tot), ("totals only", op, n, count, flags)
    else:
        assert run(c, op, a, n, count, flags, init, want_totals=False, in_place=not in_place and not flags & sc.SHARED_A) == (0, out, keep_t), ("out only", op, n, count, flags)


# ---- 1. every length, count, op, mode, form and seed, against the model -----------------------------------------------------------------
@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("flags", sc.ALL_FLAGS)
@pytest.mark.parametrize("op", sc.OPS)
def test_device_form_at_the_default_chunk(one, L, op, flags, count):
    chunk = sc.default_chunk(L)
    assert one.get_option("scan_chunk") == chunk
    for turn, n in enumerate(sc.lengths(sc.LANES * chunk, squares=False)):
        check_case(one, on_device, op, n, count, flags, seed=chunk, turn=turn + count)


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("flags", sc.ALL_FLAGS)
@pytest.mark.parametrize("op", sc.OPS)
def test_device_form_at_chunk_1_up_to_three_levels(one, L, monkeypatch, op, flags, count):
    monkeypatch.setenv("TE_MSM_SCAN_CHUNK", "1")
    assert one.get_option("scan_chunk") == 1 and sc.plan_info(L, 65537, chunk=1)["levels"] == 3
    for turn, n in enumerate(sc.lengths(sc.LANES, squares=True)):
        if n > 4 * sc.LANES and (count == 3) != bool(flags & sc.MONTGOMERY):     # the squares: count 1 canonical, count 3 in the Montgomery form
            continue
        check_case(one, on_device, op, n, count, flags, seed=1, turn=turn + count)


@pytest.mark.parametrize("chunk", [0, 1])
@pytest.mark.parametrize("op", sc.OPS)
def test_host_form_on_one_and_two_slices(one, two, L, monkeypatch, op, chunk):
    """three vectors: slices of two and one on a context of two devices, so that a slice boundary falls between vectors"""
    if chunk:
        monkeypatch.setenv("TE_MSM_SCAN_CHUNK", str(chunk))
    T = sc.LANES * (chunk or sc.default_chunk(L))
    for turn, n in enumerate(sc.lengths(T, squares=False)):
        flags = sc.ALL_FLAGS[turn % 8]
        check_case(one, on_host, op, n, 3, flags, seed=chunk or sc.default_chunk(L), turn=turn)
        check_case(two, on_host, op, n, 3, flags, seed=chunk or sc.default_chunk(L), turn=turn + 5)


@pytest.mark.parametrize("op", sc.OPS)
def test_every_chunk_runs(one, monkeypatch, op):
    for chunk in range(1, sc.CHUNK_MAX + 1):
        monkeypatch.setenv("TE_MSM_SCAN_CHUNK", str(chunk))
        n = sc.LANES * chunk + 77
        flags = sc.MONTGOMERY | (sc.EXCLUSIVE if chunk & 1 else 0)
        a, init, out, tot = sc.expected(op, n, 1, flags, 21)
        assert on_device(one, op, a, n, 1, flags, init, in_place=True) == (0, out, tot), chunk
    monkeypatch.setenv("TE_MSM_SCAN_CHUNK", "17")                    # outside 1 .. 16: the default
    assert one.get_option("scan_chunk") == sc.default_chunk(sc.shim())


def test_zeros_and_the_worst_sum(one, L):
    """a zero factor at the first, a middle and the last position of a product; every record and the seed 2^256 - 1 in a sum"""
    T = sc.LANES * sc.default_chunk(L)
    n = 2 * T + 300
    for at in (0, n // 2 + 1, n - 1):
        a = sc.with_record(sc.values(2 * n, 6, zero_free=True), n + at, P if at else 0)
        init = sc.seeds(2, 6)
        for flags in (0, sc.MONTGOMERY | sc.EXCLUSIVE):
            out, tot = sc.model(sc.PRODUCT, a, n, 2, flags, init)
            assert on_device(one, sc.PRODUCT, a, n, 2, flags, init) == (0, out, tot), (at, flags)
    top = (1 << 256) - 1
    a, init = sc.pack([top] * n, 32), sc.pack([top], 32)
    want = sc.pack([(i + 2) * top % P for i in range(n)], 32)
    assert on_device(one, sc.SUM, a, n, 1, 0, init, in_place=True) == (0, want, sc.pack([(n + 1) * top % P], 32))


def test_python_methods(pkg, one):
    a, init, out, tot = sc.expected(sc.PRODUCT, 300, 2, sc.MONTGOMERY | sc.EXCLUSIVE, 8)
    assert one.field_scan(sc.PRODUCT, a, 300, count=2, init=init, montgomery=True, exclusive=True) == (out, tot)
    assert one.field_scan(sc.PRODUCT, a, 300, count=2, init=sc.unpack(init, 32), montgomery=True, exclusive=True, out=False) == (None, tot)
    a1, _, out1, tot1 = sc.expected(sc.SUM, 300, 2, sc.SHARED_A, 8, False)
    assert one.field_scan(sc.SUM, a1, 300, count=2, shared_a=True, totals=False) == (out1, None)
    assert one.field_scan(sc.SUM, b"", 5, count=0) == (b"", b"")
    da = _dev(a)
    _sync()
    assert one.field_scan_device(sc.PRODUCT, da.data_ptr(), 300, 2, da.data_ptr(), init=init, montgomery=True, exclusive=True) == (da.data_ptr(), tot)
    assert bytes(da.cpu().numpy()) == out
    with pytest.raises(pkg.MsmError):
        one.field_scan(sc.SUM, a, 299, count=2)
    with pytest.raises(pkg.MsmError):
        one.field_scan(sc.SUM, a, 300, count=2, init=init[:32])
    with pytest.raises(pkg.MsmError):
        one.field_scan(7, a, 300, count=2)
    assert (pkg.SCAN_SUM, pkg.SCAN_PRODUCT, pkg.SCAN_MONTGOMERY, pkg.SCAN_EXCLUSIVE, pkg.SCAN_SHARED_A, pkg.SCAN_MAX_N) == (0, 1, 1, 2, 4, 1 << 30)


# ---- 2. totals only writes nothing but the scratch buffer ---------------------------------------------------------------------------
def test_totals_only_leaves_device_memory_alone(one, L):
    """the vectors sit between two guard bands in one allocation; with d_out NULL every byte of it is as it was"""
    import torch
    n, count = 2 * sc.LANES * sc.default_chunk(L) + 300, 3
    for op in sc.OPS:
        a, init, _, tot = sc.expected(op, n, count, 0, 40)
        band = 1 << 16
        whole = torch.full((2 * band + len(a),), PAT, dtype=torch.uint8, device="cuda")
        whole[band:band + len(a)] = _dev(a)
        before = whole.clone()
        got = ctypes.create_string_buffer(32 * count)
        _sync()
        assert one._L.te_msm_field_scan_device(one._h, op, whole.data_ptr() + band, n, count, 0, init, got, None) == 0
        assert got.raw == tot and torch.equal(whole, before)
    assert one.get_option("scan_scratch_bytes") >= sc.plan_info(L, n, count)["scratch_bytes"]


# ---- 3. refusals; the scratch buffer's lifetime ------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs(two):
    import torch
    c = two
    a = sc.values(16)
    keep_o, keep_t = bytes([PAT]) * len(a), bytes([PAT]) * 64

    def _raw(run, op, n, flags):
        """the call on buffers of len(a) bytes and 64 of totals -> (status, totals bytes); out is as it was"""
        da, do = _dev(a), torch.full((len(a),), PAT, dtype=torch.uint8, device="cuda")
        tot = ctypes.create_string_buffer(keep_t, 64)
        _sync()
        if run is on_device:
            rc = c._L.te_msm_field_scan_device(c._h, op, da.data_ptr(), n, 2, flags, None, tot, do.data_ptr())
            assert bytes(do.cpu().numpy()) == keep_o
        else:
            src, out = ctypes.create_string_buffer(a, len(a)), ctypes.create_string_buffer(keep_o, len(a))
            rc = c._L.te_msm_field_scan(c._h, op, ctypes.addressof(src), n, 2, flags, None, tot, ctypes.addressof(out))
            assert out.raw == keep_o
        return rc, tot.raw

    for run in (on_device, on_host):
        for op, n, flags in ((2, 8, 0), (-1, 8, 0), (sc.SUM, 0, 0), (sc.PRODUCT, sc.MAX_N + 1, 0), (sc.SUM, 8, 8), (sc.PRODUCT, 8, 1 << 16)):
            assert _raw(run, op, n, flags) == (sc.EINVAL, keep_t), (run.__name__, op, n, flags)
        assert run(c, sc.SUM, a, 8, 2, 0, None, want_out=False, want_totals=False)[0] == sc.EINVAL                     # both outputs NULL
    da, do = _dev(a), torch.full((len(a),), PAT, dtype=torch.uint8, device="cuda")
    _sync()
    host = ctypes.create_string_buffer(a, len(a))                   # a buffer on no device of the context
    tot = ctypes.create_string_buffer(keep_t, 64)
    f = c._L.te_msm_field_scan_device
    assert f(c._h, sc.SUM, da.data_ptr(), 8, 2, 0, None, tot, ctypes.addressof(host)) == sc.EINVAL
    assert f(c._h, sc.SUM, ctypes.addressof(host), 8, 2, 0, None, tot, do.data_ptr()) == sc.EINVAL
    assert f(c._h, sc.SUM, ctypes.addressof(host), 8, 2, 0, None, tot, None) == sc.EINVAL
    assert f(c._h, sc.SUM, None, 8, 2, 0, None, tot, do.data_ptr()) == sc.EINVAL
    assert f(c._h, sc.SUM, da.data_ptr(), 1 << 30, 1 << 30, 0, None, tot, do.data_ptr()) == sc.EINVAL      # count x n x 32 = 2^65
    assert f(c._h, sc.SUM, da.data_ptr(), 8, 2, sc.SHARED_A, None, tot, da.data_ptr()) == sc.EINVAL        # aliasing under SHARED_A
    if torch.cuda.device_count() > 1:                               # d_a and d_out on two devices
        with torch.cuda.device(1):
            far = torch.full((len(a),), PAT, dtype=torch.uint8, device="cuda:1")
            torch.cuda.synchronize()
        assert f(c._h, sc.SUM, da.data_ptr(), 8, 2, 0, None, tot, far.data_ptr()) == sc.EINVAL
        assert bytes(far.cpu().numpy()) == keep_o
    assert c._L.te_msm_field_scan(c._h, sc.SUM, None, 8, 2, 0, None, tot, host) == sc.EINVAL
    assert bytes(da.cpu().numpy()) == a and host.raw == a and tot.raw == keep_t and bytes(do.cpu().numpy()) == keep_o
    assert f(c._h, sc.SUM, None, 8, 0, 0, None, tot, None) == 0 and c._L.te_msm_field_scan(c._h, sc.SUM, None, 8, 0, 0, None, None, host) == 0      # count = 0
    assert tot.raw == keep_t and host.raw == a
    assert on_device(c, sc.PRODUCT, a, 8, 2, 0)[1:] == sc.model(sc.PRODUCT, a, 8, 2, 0)      # the context is usable


def test_scratch_grows_on_use_and_is_trimmed(pkg, L):
    chunk = sc.default_chunk(L)
    n = 2 * sc.LANES * chunk + 300
    a, init, out, tot = sc.expected(sc.SUM, n, 1, 0, chunk)
    a3, init3, out3, tot3 = sc.expected(sc.SUM, n, 3, 0, chunk)
    with pkg.MsmContext((0,)) as c:
        assert c.get_option("scan_scratch_bytes") == 0
        assert on_device(c, sc.SUM, a, n, 1, 0, init) == (0, out, tot)
        small = c.get_option("scan_scratch_bytes")
        assert small == sc.plan_info(L, n, 1)["scratch_bytes"] == 32 * 5
        assert on_device(c, sc.SUM, a3, n, 3, 0, init3) == (0, out3, tot3)
        grown = c.get_option("scan_scratch_bytes")
        assert grown == sc.plan_info(L, n, 3)["scratch_bytes"] > small
        assert on_device(c, sc.SUM, a, n, 1, 0, init) == (0, out, tot) and c.get_option("scan_scratch_bytes") == grown      # grown on use, kept
        c.trim(0)
        assert c.get_option("scan_scratch_bytes") == 0
        assert on_device(c, sc.SUM, a3, n, 3, 0, init3, in_place=True) == (0, out3, tot3) and c.get_option("scan_scratch_bytes") == grown


# ---- 4. the chains the feature exists for ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("montgomery", [0, 1])
def test_grand_product_to_its_msm_bls12_377(pkg, montgomery):
    """f random and g a permutation of it: f + gamma and g + gamma (field_op_device ADD, shared), 1 / (g + gamma) (INV), the ratios (MUL), their
    exclusive running product z (field_scan_device) -- equal to the model, closing at 1, and not at 1 once one element of g is changed --
    then z's coefficients (ntt_device inverse) and their MSM over a bound set, equal to the oracle's.  Nothing but gamma, the total and the
    MSM result crosses the link."""
    from oracle import oracle377
    log_n, n = 10, 1 << 10
    rnd = random.Random(0x6AD + montgomery)
    f = [rnd.randrange(P) for _ in range(n)]
    g = list(f)
    rnd.shuffle(g)
    gamma = rnd.randrange(P)
    wire = (lambda v: [x * sc.A % P for x in v]) if montgomery else (lambda v: v)
    mont = bool(montgomery)
    z = [1]
    for i in range(n - 1):
        z.append(z[-1] * (f[i] + gamma) * pow(g[i] + gamma, -1, P) % P)
    coeffs = nc.fast(z, log_n, inverse=True)
    pts = oracle377.gen_points(29, n)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        c.set_option("scalar_record_bytes", 32)
        c.set_option("scalars_montgomery", montgomery)
        bases = c.bind_points(pts)
        dgamma = _dev(sc.pack(wire([gamma]), 32))

        def grand_product(gs):
            df, dg = _dev(sc.pack(wire(f), 32)), _dev(sc.pack(wire(gs), 32))
            _sync()
            c.field_op_device(pkg.FIELD_ADD, df.data_ptr(), dgamma.data_ptr(), n, df.data_ptr(), shared_b=True, montgomery=mont)
            c.field_op_device(pkg.FIELD_ADD, dg.data_ptr(), dgamma.data_ptr(), n, dg.data_ptr(), shared_b=True, montgomery=mont)
            c.field_op_device(pkg.FIELD_INV, dg.data_ptr(), None, n, dg.data_ptr(), montgomery=mont)
            c.field_op_device(pkg.FIELD_MUL, df.data_ptr(), dg.data_ptr(), n, df.data_ptr(), montgomery=mont)
            _, total = c.field_scan_device(pkg.SCAN_PRODUCT, df.data_ptr(), n, 1, df.data_ptr(), montgomery=mont, exclusive=True)
            return df, total

        dz, total = grand_product(g)
        assert bytes(dz.cpu().numpy()) == sc.pack(wire(z), 32)
        assert total == sc.pack(wire([1]), 32)                       # g is a permutation of f
        c.ntt_device(dz.data_ptr(), log_n, 1, dz.data_ptr(), inverse=True, montgomery=mont)
        got = c.run_scalars_device(bases, dz.data_ptr())
        bad = list(g)
        bad[n // 3] = (bad[n // 3] + 1) % P
        _, total_bad = grand_product(bad)
        assert total_bad != sc.pack(wire([1]), 32)
        bases.release()
    assert got == oracle377.msm(pts, sc.pack(coeffs, 48), threads=2)


@pytest.mark.parametrize("curve", [0, 1])
def test_powers_of_tau_into_an_srs(pkg, curve):
    """SHARED_A | EXCLUSIVE product of tau = tau^0 .. tau^(n-1) on the device, fed to te_msm_mul_base_device: the same bytes as te_msm_mul_base
    over host-computed powers.  The scan writes 32-byte records: it feeds the Twisted-Edwards curve's scalars and BLS12-377's at
    "scalar_record_bytes" = 32.  BLS12-377's default 48-byte scalar records do not agree with them and are not a case here: a caller sets
    the option, as the MSMs over device scalars do."""
    import torch
    n = 300
    tau = random.Random(0x7A0 + curve).randrange(P)
    powers = [pow(tau, i, P) for i in range(n)]
    raw = mc.bls_base_points()[0][1] if curve else m.points_to_bytes([mc.te_point("subgroup point 0")])
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        if curve:
            c.set_option("scalar_record_bytes", 32)
        base = c.bind_base(raw)
        want = c.mul_base(base, sc.pack(powers, 32))
        dtau = _dev(sc.pack([tau], 32))
        dpow = torch.full((32 * n,), PAT, dtype=torch.uint8, device="cuda")
        dout = torch.full((len(want),), PAT, dtype=torch.uint8, device="cuda")
        _sync()
        _, total = c.field_scan_device(pkg.SCAN_PRODUCT, dtau.data_ptr(), n, 1, dpow.data_ptr(), exclusive=True, shared_a=True)
        assert bytes(dpow.cpu().numpy()) == sc.pack(powers, 32) and total == sc.pack([pow(tau, n, P)], 32)
        c.mul_base_device(base, dpow.data_ptr(), n, dout.data_ptr())
        assert bytes(dout.cpu().numpy()) == want
        c.release_base(base)


# ---- the Node function -------------------------------------------------------------------------------------------------------------
def test_node_field_scan(pkg, tmp_path):
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
    a, init, out, tot = sc.expected(sc.PRODUCT, 300, 3, sc.MONTGOMERY | sc.EXCLUSIVE, 8)
    a1, _, out1, tot1 = sc.expected(sc.SUM, 300, 3, sc.SHARED_A, 8, False)
    (tmp_path / "a.bin").write_bytes(a)
    (tmp_path / "init.bin").write_bytes(init)
    (tmp_path / "a1.bin").write_bytes(a1)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
(async () => {
  const a = fs.readFileSync(process.argv[2]), init = fs.readFileSync(process.argv[3]), a1 = fs.readFileSync(process.argv[4]), res = {};
  const r = await m.fieldScan('product', a, 300, {count: 3, init, montgomery: true, exclusive: true});
  res.out = r.out.toString('hex'); res.totals = r.totals.toString('hex');
  const e = await m.fieldScan('sum', a1, 300, {count: 3, sharedA: true, out: false});
  res.totals1 = e.totals.toString('hex'); res.none = e.out === null;
  await m.fieldScan('sum', a, 0, {count: 3}).then(() => { res.bad = 'resolved'; }, (x) => { res.bad = String(x.message); });
  await m.fieldScan('max', a, 300, {count: 3}).then(() => { res.op = 'resolved'; }, (x) => { res.op = String(x.message); });
  console.log(JSON.stringify(res));
})();
"""
    r = subprocess.run([node, "-e", script, js, str(tmp_path / "a.bin"), str(tmp_path / "init.bin"), str(tmp_path / "a1.bin")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    res = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert bytes.fromhex(res["out"]) == out and bytes.fromhex(res["totals"]) == tot and bytes.fromhex(res["totals1"]) == tot1 and res["none"] is True
    assert res["bad"] != "resolved" and res["op"] != "resolved", res
