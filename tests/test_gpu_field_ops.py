"""Batched field arithmetic on the GPU (te_msm_field_op*; include/te_msm.h): byte-equal to the host shim and to Python integers on both
fields and in both forms, host and device buffers; the inversion block at every tile and chain edge for every chain length; failures with
the lowest index, the output untouched; in place; argument errors; a context of two slices; and the use it is for -- products of
Montgomery-form scalars handed to an MSM without leaving the device."""
import ctypes
import os

import pytest

import field_cases as fc

pytestmark = pytest.mark.gpu

PAT = 0xAB
FORMS = [0, fc.MONTGOMERY]


@pytest.fixture(scope="module")
def L():
    return fc.shim()


def _dev(buf):
    import torch
    return torch.frombuffer(bytearray(buf or b"\0"), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def on_device(c, field, op, a, bb=None, flags=0, out="new"):
    """te_msm_field_op_device; out: "new" (a buffer pre-filled with a pattern), "a" or "b" (in place).  (status, output bytes, index, reason)"""
    import torch
    n = len(a) // fc.nbytes(field)
    da, db = _dev(a), _dev(bb) if bb is not None else None
    dout = {"new": torch.full((max(1, len(a)),), PAT, dtype=torch.uint8, device="cuda"), "a": da, "b": db}[out]
    _sync()
    rc = c._L.te_msm_field_op_device(c._h, field, op, da.data_ptr(), db.data_ptr() if db is not None else None, n, flags, dout.data_ptr())
    got = bytes(dout.cpu().numpy())[:len(a)]
    return rc, got, c.get_option("bad_field_index") if rc == fc.EFIELD else -1, c.get_option("bad_field_reason") if rc == fc.EFIELD else 0


def on_host(c, field, op, a, bb=None, flags=0):
    n = len(a) // fc.nbytes(field)
    out = ctypes.create_string_buffer(bytes([PAT]) * max(1, len(a)), max(1, len(a)))
    rc = c._L.te_msm_field_op(c._h, field, op, bytes(a), None if bb is None else bytes(bb), n, flags, out)
    return rc, out.raw[:len(a)], c.get_option("bad_field_index") if rc == fc.EFIELD else -1, c.get_option("bad_field_reason") if rc == fc.EFIELD else 0


def both_match(c, L, field, op, a, bb=None, flags=0):
    """device and host forms against the shim and the model: status, bytes (untouched on a failure), index, reason"""
    want = fc.model_op(field, op, a, bb, flags)
    want = (want[0], want[1] if want[0] == 0 else bytes([PAT]) * len(a), want[2], want[3])
    sh = fc.shim_op(L, field, op, a, bb, flags, fill=PAT)
    assert sh == want
    assert on_device(c, field, op, a, bb, flags) == want
    assert on_host(c, field, op, a, bb, flags) == want


# ---- 1. every op, both fields, both forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("field", fc.FIELDS)
def test_map_ops_match_shim_and_model(pkg, L, field, flags):
    a, bb = fc.binary_operands(field)
    eb = fc.nbytes(field)
    with pkg.MsmContext((0,)) as c:
        for op in (fc.ADD, fc.SUB, fc.MUL):
            both_match(c, L, field, op, a, bb, flags)
            both_match(c, L, field, op, a, bb[5 * eb:6 * eb], flags | fc.SHARED_B)
        for op in (fc.DOUBLE, fc.NEG, fc.SQUARE):
            both_match(c, L, field, op, fc.unary_operands(field), None, flags)


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("field", fc.FIELDS)
def test_inv_pow_sqrt_match_shim_and_model(pkg, L, field, flags):
    p, eb = fc.modulus(field), fc.nbytes(field)
    with pkg.MsmContext((0,)) as c:
        both_match(c, L, field, fc.INV, fc.unary_operands(field), None, flags | fc.ZERO_OK)
        both_match(c, L, field, fc.INV, fc.nonzero_operands(field), None, flags)
        a, e = fc.pow_operands(field)
        both_match(c, L, field, fc.POW, a, e, flags)
        for x in (17, 0, (1 << 256) - 1):
            both_match(c, L, field, fc.POW, fc.unary_operands(field), fc.pack([x], 32), flags | fc.SHARED_B)
        A = 1 << (8 * eb)
        squares, _ = fc.sqrt_inputs(field)
        both_match(c, L, field, fc.SQRT, fc.pack([v * A % p if flags else v for v in squares], eb), None, flags)


def test_python_methods(pkg):
    with pkg.MsmContext((0,)) as c:
        p = fc.modulus(fc.FIELD_P)
        a, bb = fc.pack([3, p - 1, p + 2], 32), fc.pack([5, 2, 7], 32)
        assert c.field_op(pkg.FIELD_MUL, a, bb) == fc.pack([15, p - 2, 14], 32)
        assert c.field_op(pkg.FIELD_POW, a, fc.pack([17], 32), shared_b=True) == fc.pack([pow(3, 17, p), p - 1, pow(2, 17, p)], 32)
        assert c.field_op(pkg.FIELD_SQRT, fc.pack([4, 0], 32)) == fc.pack([2, 0], 32)
        assert c.field_op(pkg.FIELD_INV, fc.pack([0, 2], 32), zero_ok=True) == fc.pack([0, (p + 1) // 2], 32)
        q = fc.modulus(fc.FIELD_Q377)
        assert c.field_op(pkg.FIELD_NEG, fc.pack([1], 48), field=pkg.FIELD_Q377) == fc.pack([q - 1], 48)
        with pytest.raises(pkg.MsmError) as e:
            c.field_op(pkg.FIELD_INV, fc.pack([1, 2, 0, 0], 32))
        assert (e.value.code, e.value.index, e.value.reason) == (pkg.EFIELD, 2, pkg.FIELD_ZERO)
        with pytest.raises(pkg.MsmError) as e:
            c.field_op(pkg.FIELD_SQRT, fc.pack([4, 11], 32))
        assert (e.value.code, e.value.index, e.value.reason) == (pkg.EFIELD, 1, pkg.FIELD_NOT_SQUARE)
        da = _dev(a)
        _sync()
        c.field_op_device(pkg.FIELD_DOUBLE, da.data_ptr(), None, 3, da.data_ptr())
        assert bytes(da.cpu().numpy()) == fc.pack([6, p - 2, 4], 32)
        assert c.get_option("field_inv_group") in fc.GROUPS


# ---- 2. the inversion block, through the C-ABI ---------------------------------------------------------------------------------------
@pytest.fixture
def inv_group():
    """the chain length of the calls that follow (TE_MSM_FIELD_INV_GROUP, read by every call), put back afterwards"""
    keep = os.environ.get("TE_MSM_FIELD_INV_GROUP")

    def choose(g):
        os.environ["TE_MSM_FIELD_INV_GROUP"] = str(g)
    yield choose
    if keep is None:
        os.environ.pop("TE_MSM_FIELD_INV_GROUP", None)
    else:
        os.environ["TE_MSM_FIELD_INV_GROUP"] = keep


@pytest.mark.parametrize("group", fc.GROUPS)
def test_inversion_block_shapes(pkg, inv_group, group):
    inv_group(group)
    with pkg.MsmContext((0,)) as c:
        for n in fc.inv_sizes(group):
            a = fc.pack(fc.inv_values(fc.FIELD_P, n, group, zeros=False), 32)
            assert on_device(c, fc.FIELD_P, fc.INV, a)[:2] == fc.model_op(fc.FIELD_P, fc.INV, a)[:2]
            z = fc.pack(fc.inv_values(fc.FIELD_P, n, group), 32)
            assert on_device(c, fc.FIELD_P, fc.INV, z, None, fc.ZERO_OK)[:2] == fc.model_op(fc.FIELD_P, fc.INV, z, None, fc.ZERO_OK)[:2]
            assert on_device(c, fc.FIELD_P, fc.INV, z, None, fc.ZERO_OK, out="a")[:2] == fc.model_op(fc.FIELD_P, fc.INV, z, None, fc.ZERO_OK)[:2]
            if n >= 256 * group:
                assert on_device(c, fc.FIELD_P, fc.INV, z) == (fc.EFIELD, bytes([PAT]) * len(z), 3, fc.ZERO)       # several zeros: the lowest


@pytest.mark.parametrize("field,flags", [(fc.FIELD_Q377, 0), (fc.FIELD_Q377, fc.MONTGOMERY), (fc.FIELD_P, fc.MONTGOMERY)])
def test_inversion_block_other_field_and_form(pkg, inv_group, field, flags):
    for group in (8, 16):
        inv_group(group)
        n = 2 * 256 * group + 300
        a = fc.pack(fc.inv_values(field, n, group), fc.nbytes(field))
        with pkg.MsmContext((0, 0)) as c:
            want = fc.model_op(field, fc.INV, a, None, flags | fc.ZERO_OK)[:2]
            assert on_device(c, field, fc.INV, a, None, flags | fc.ZERO_OK)[:2] == want
            assert on_host(c, field, fc.INV, a, None, flags | fc.ZERO_OK)[:2] == want


# ---- 3. failures ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", fc.FIELDS)
@pytest.mark.parametrize("ids", [(0,), (0, 0)])
def test_failures_report_the_lowest_index_and_leave_the_output(pkg, field, ids):
    p, eb, n = fc.modulus(field), fc.nbytes(field), 300
    _, z, _ = fc.root_of_unity(field)
    good = [pow(7 + i, 2, p) for i in range(n)]                     # non-zero squares
    with pkg.MsmContext(ids) as c:
        assert c.get_option("bad_field_index") == -1 and c.get_option("bad_field_reason") == 0
        for op, bad_value, reason in ((fc.INV, p, fc.ZERO), (fc.SQRT, z, fc.NOT_SQUARE)):
            for where in ((0,), (151,), (n - 1,), (200, 77)):
                v = list(good)
                for k in where:
                    v[k] = bad_value
                a = fc.pack(v, eb)
                want = (fc.EFIELD, bytes([PAT]) * len(a), min(where), reason)
                assert on_device(c, field, op, a) == want, (op, where)
                assert on_host(c, field, op, a) == want, (op, where)
                assert "field element %d" % min(where) in c._L.te_msm_last_error(c._h).decode()
            ok = fc.pack(good, eb)                                  # the context is usable: the next call succeeds
            assert on_device(c, field, op, ok)[:2] == fc.model_op(field, op, ok)[:2]
            assert on_host(c, field, op, ok)[:2] == fc.model_op(field, op, ok)[:2]


# ---- 4. in place ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field", fc.FIELDS)
def test_in_place(pkg, field):
    p, eb, n = fc.modulus(field), fc.nbytes(field), 300
    a = fc.pack([pow(5 + i, 2, p) for i in range(n)], eb)
    bb = fc.pack([(1 << (8 * eb)) - 1 - i for i in range(n)], eb)
    e = fc.pack([(3 << 254) + i for i in range(n)], 32)
    with pkg.MsmContext((0,)) as c:
        for flags in FORMS:
            assert on_device(c, field, fc.MUL, a, bb, flags, out="a")[:2] == fc.model_op(field, fc.MUL, a, bb, flags)[:2]
            assert on_device(c, field, fc.MUL, a, bb, flags, out="b")[:2] == fc.model_op(field, fc.MUL, a, bb, flags)[:2]
            assert on_device(c, field, fc.INV, a, None, flags, out="a")[:2] == fc.model_op(field, fc.INV, a, None, flags)[:2]
            assert on_device(c, field, fc.POW, a, e, flags, out="a")[:2] == fc.model_op(field, fc.POW, a, e, flags)[:2]
        assert on_device(c, field, fc.SQRT, a, None, 0, out="a")[:2] == fc.model_op(field, fc.SQRT, a)[:2]
        if field == fc.FIELD_P:                                     # exponents and results of one size
            assert on_device(c, field, fc.POW, a, e, 0, out="b")[:2] == fc.model_op(field, fc.POW, a, e)[:2]
        else:                                                       # 32-byte exponents under 48-byte results: refused, nothing written
            rc, got, _, _ = on_device(c, field, fc.POW, a, e + bytes(16 * n), 0, out="b")
            assert rc == -1 and got[:32 * n] == e


# ---- 5. argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_output(pkg):
    a, bb = fc.pack([1, 2, 3, 4], 32), fc.pack([5, 6, 7, 8], 32)
    untouched = (-1, bytes([PAT]) * len(a), -1, 0)
    with pkg.MsmContext((0, 0)) as c:
        for field, op, b_, flags in ((2, fc.ADD, bb, 0), (-1, fc.ADD, bb, 0), (0, 9, None, 0), (0, -1, None, 0), (0, fc.ADD, bb, 8), (0, fc.ADD, bb, 1 << 16),
                                     (0, fc.NEG, bb, 0), (0, fc.INV, None, fc.SHARED_B), (0, fc.MUL, bb, fc.ZERO_OK), (0, fc.SQRT, None, fc.ZERO_OK),
                                     (0, fc.MUL, None, 0)):
            assert on_device(c, field, op, a, b_, flags) == untouched, (field, op, flags)
            assert on_host(c, field, op, a, b_, flags) == untouched, (field, op, flags)
        da, db = _dev(a), _dev(bb)
        _sync()
        host = ctypes.create_string_buffer(bb, len(bb))             # an operand that is on no device of the context
        assert c._L.te_msm_field_op_device(c._h, 0, fc.ADD, da.data_ptr(), ctypes.addressof(host), 4, 0, da.data_ptr()) == -1
        assert c._L.te_msm_field_op_device(c._h, 0, fc.ADD, da.data_ptr(), db.data_ptr(), 4, 0, ctypes.addressof(host)) == -1
        assert bytes(da.cpu().numpy()) == a and host.raw == bb
        assert c._L.te_msm_field_op_device(c._h, 0, fc.ADD, None, None, 0, 0, None) == 0          # n = 0: a no-op
        assert c._L.te_msm_field_op(c._h, 0, fc.ADD, None, None, 0, 0, None) == 0
        assert c.field_op(pkg.FIELD_ADD, b"", b"") == b""
        assert c._L.te_msm_field_op(c._h, 0, fc.ADD, a, bb, 1 << 31, 0, None) == -1


# ---- 6. two slices ----------------------------------------------------------------------------------------------------------------
def test_two_slices_equal_one_and_keep_the_callers_device(pkg):
    import torch
    field, eb = fc.FIELD_P, 32
    a, bb = fc.binary_operands(field)
    a, bb = a[:eb * (len(a) // eb // 2 * 2 - 1)], bb[:eb * (len(a) // eb // 2 * 2 - 1)]      # an odd count: slices of unequal length
    with pkg.MsmContext((0,)) as one, pkg.MsmContext((0, 0)) as two:
        before = torch.cuda.current_device()
        for op, b_, flags in ((fc.MUL, bb, fc.MONTGOMERY), (fc.SUB, bb, 0), (fc.INV, None, fc.ZERO_OK), (fc.POW, bb, 0), (fc.ADD, bb[:eb], fc.SHARED_B)):
            want = on_host(one, field, op, a, b_, flags)
            assert want[0] == 0 and on_host(two, field, op, a, b_, flags) == want
        assert on_host(two, field, op, a[:eb], bb[:eb], fc.SHARED_B)[0] == 0       # one element: one slice
        assert torch.cuda.current_device() == before


# ---- 7. the use it is for ------------------------------------------------------------------------------------------------------------
def test_products_feed_an_msm_without_leaving_the_device(pkg):
    """BLS12-377: scalars a_i b_i made by te_msm_field_op_device(FIELD_P, MUL, MONTGOMERY) from a native prover's residues go straight to
    te_msm_run_scalars_device under "scalars_montgomery" = 1 and 32-byte records; the MSM equals the oracle's over the products"""
    import random
    import torch
    from oracle import oracle377
    n, r = 300, fc.modulus(fc.FIELD_P)
    rnd = random.Random(0x377)
    av, bv = [rnd.randrange(r) for _ in range(n)], [rnd.randrange(r) for _ in range(n)]
    A = 1 << 256
    pts = oracle377.gen_points(11, n)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        c.set_option("scalar_record_bytes", 32)
        c.set_option("scalars_montgomery", 1)
        bases = c.bind_points(pts)
        da, db = _dev(fc.pack([v * A % r for v in av], 32)), _dev(fc.pack([v * A % r for v in bv], 32))
        dk = torch.empty(32 * n, dtype=torch.uint8, device="cuda")
        _sync()
        c.field_op_device(pkg.FIELD_MUL, da.data_ptr(), db.data_ptr(), n, dk.data_ptr(), montgomery=True)
        got = c.run_scalars_device(bases, dk.data_ptr())
        bases.release()
    assert got == oracle377.msm(pts, fc.pack([x * y % r for x, y in zip(av, bv)], 48), threads=2)


# ---- the Node function -------------------------------------------------------------------------------------------------------------
def test_node_field_op(pkg, tmp_path):
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
    p, n = fc.modulus(fc.FIELD_P), 300
    a = fc.pack([pow(3 + i, 2, p) for i in range(n)], 32)
    bb = fc.pack([(1 << 256) - 1 - 5 * i for i in range(n)], 32)
    aq = fc.pack([(1 << 384) - 1 - i for i in range(n)], 48)
    bad = a[:32 * 123] + fc.pack([p], 32) + a[32 * 124:]
    files = {"a.bin": a, "b.bin": bb, "aq.bin": aq, "bad.bin": bad, "e17.bin": fc.pack([17], 32)}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
const [a, b, aq, bad, e17] = process.argv.slice(2).map((f) => fs.readFileSync(f));
(async () => {
  const out = {}, F = m.FIELD_OPS;
  out.mul = (await m.fieldOp(F.mul, a, b)).toString('hex');
  out.mulm = (await m.fieldOp(F.mul, a, b, {montgomery: true})).toString('hex');
  out.pow17 = (await m.fieldOp(F.pow, a, e17, {sharedB: true})).toString('hex');
  out.sqrt = (await m.fieldOp(F.sqrt, a, null)).toString('hex');
  out.invq = (await m.fieldOp(F.inv, aq, null, {field: 1})).toString('hex');
  out.zero_ok = (await m.fieldOp(F.inv, bad, null, {zeroOk: true})).toString('hex');
  out.empty = (await m.fieldOp(F.add, Buffer.alloc(0), Buffer.alloc(0))).length;
  await m.fieldOp(F.inv, bad).then(() => { out.bad = 'resolved'; }, (e) => { out.bad = String(e.message); out.i = e.index; out.r = e.reason; });
  await m.fieldOp(F.neg, a, b).then(() => { out.arg = 'resolved'; }, (e) => { out.arg = String(e.message); });
  console.log(JSON.stringify(out));
})();
"""
    r = subprocess.run([node, "-e", script, js] + [str(tmp_path / f) for f in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert bytes.fromhex(out["mul"]) == fc.model_op(fc.FIELD_P, fc.MUL, a, bb)[1]
    assert bytes.fromhex(out["mulm"]) == fc.model_op(fc.FIELD_P, fc.MUL, a, bb, fc.MONTGOMERY)[1]
    assert bytes.fromhex(out["pow17"]) == fc.model_op(fc.FIELD_P, fc.POW, a, files["e17.bin"], fc.SHARED_B)[1]
    assert bytes.fromhex(out["sqrt"]) == fc.model_op(fc.FIELD_P, fc.SQRT, a)[1]
    assert bytes.fromhex(out["invq"]) == fc.model_op(fc.FIELD_Q377, fc.INV, aq)[1]
    assert bytes.fromhex(out["zero_ok"]) == fc.model_op(fc.FIELD_P, fc.INV, bad, None, fc.ZERO_OK)[1]
    assert out["empty"] == 0
    assert "te_msm error -6" in out["bad"] and (out["i"], out["r"]) == (123, fc.ZERO), out
    assert "te_msm error -1" in out["arg"], out
