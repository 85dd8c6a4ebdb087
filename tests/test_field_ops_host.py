"""Batched field arithmetic without a device: the per-lane code of csrc/field_ops.hip.hpp, compiled for the host (tests/csrc/fieldopscheck.cpp),
against the reference's own answers (tests/golden/field_ops_wasm_golden.json), against Python integers on both fields, and -- the
inversion block -- at every tile and chain edge.  The same arithmetic runs on the device in tests/test_gpu_field_ops.py."""
import ctypes
import json
import os
import re
import subprocess

import pytest

import field_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
FORMS = [0, fc.MONTGOMERY]


@pytest.fixture(scope="module")
def L():
    return fc.shim()


@pytest.fixture(scope="module")
def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "field_ops_wasm_golden.json")))


def same(L, field, op, a, bb=None, flags=0, group=16):
    """the shim and the model agree: status, bytes, failing index and reason"""
    got, want = fc.shim_op(L, field, op, a, bb, flags, group), fc.model_op(field, op, a, bb, flags)
    assert got[0] == want[0] and got[2:] == want[2:], (got[0], got[2:], want[0], want[2:])
    if want[0] == 0:
        assert got[1] == want[1]
    else:
        assert got[1] == bytes([0xA5]) * len(a)                     # untouched
    return got


# ---- 1. the reference's own answers ----------------------------------------------------------------------------------------------
def test_reference_goldens(L, golden):
    p = int(golden["modulus"])
    assert p == fc.modulus(fc.FIELD_P)
    seen = {}
    for c in golden["cases"]:
        op = fc.OPS[c["op"]]
        a = fc.pack([int(c["a"])], 32)
        bb = fc.pack([int(c["b"])], 32) if "b" in c else None
        rc, out, bad, why = fc.shim_op(L, fc.FIELD_P, op, a, bb)
        seen[c["op"]] = seen.get(c["op"], 0) + 1
        if c["out"] == "traps":
            assert (rc, bad) == (fc.EFIELD, 0) and why == (fc.ZERO if op == fc.INV else fc.NOT_SQUARE), c
            continue
        assert rc == 0, c
        r, want = int.from_bytes(out, "little"), int(c["out"])
        if op == fc.SQRT:                                           # the reference's sign has no rule: either root, ours the smaller
            assert want in (r, (p - r) % p) and r * r % p == int(c["a"]) % p and r <= (p - 1) // 2, c
        else:
            assert r == want, c
    assert all(seen[k] >= 40 for k in ("add", "sub", "mul", "double", "inv", "pow", "sqrt")), seen


def test_golden_holds_the_named_cases(golden):
    p = int(golden["modulus"])
    by = {(c["op"], c["a"], c.get("b")): c["out"] for c in golden["cases"]}
    assert by[("inv", "0", None)] == "traps" and by[("sqrt", "11", None)] == "traps"
    assert by[("pow", "0", "0")] == "1" and by[("sqrt", "0", None)] == "0"
    assert by[("sqrt", "4", None)] == str(p - 2)                    # ... which is why the engine fixes its own rule
    assert any(c["a"] == str(p + 1) and c["op"] == "double" and c["out"] == "2" for c in golden["cases"])
    for e in (0, 1, 17, p - 2, p - 1):
        assert any(c["op"] == "pow" and c["b"] == str(e) for c in golden["cases"])


# ---- 2. Python integers, both fields, both forms ------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("field", fc.FIELDS)
def test_binary_ops_on_the_extremes(L, field, flags):
    a, bb = fc.binary_operands(field)
    eb = fc.nbytes(field)
    for op in (fc.ADD, fc.SUB, fc.MUL):
        same(L, field, op, a, bb, flags)
        for k in (0, 3, 5, len(bb) // eb - 1):                      # one b for every i
            same(L, field, op, a, bb[k * eb:(k + 1) * eb], flags | fc.SHARED_B)


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("field", fc.FIELDS)
def test_unary_ops_on_the_extremes(L, field, flags):
    a = fc.unary_operands(field)
    for op in (fc.DOUBLE, fc.NEG, fc.SQUARE):
        same(L, field, op, a, None, flags)
    same(L, field, fc.INV, a, None, flags | fc.ZERO_OK)
    same(L, field, fc.INV, fc.nonzero_operands(field), None, flags)
    assert same(L, field, fc.INV, a, None, flags)[2:] == (0, fc.ZERO)      # the first extreme is 0


def test_outputs_are_canonical_and_inputs_stand_for_residues(L):
    for field in fc.FIELDS:
        p, eb = fc.modulus(field), fc.nbytes(field)
        a = fc.pack([p, p + 1, (1 << (8 * eb)) - 1], eb)
        out = fc.unpack(same(L, field, fc.ADD, a, fc.pack([1], eb), fc.SHARED_B)[1], eb)
        assert out == [1, 2, (1 << (8 * eb)) % p] and all(x < p for x in out)


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("field", fc.FIELDS)
def test_pow_windows_and_shared_exponents(L, field, flags):
    a, e = fc.pow_operands(field)
    same(L, field, fc.POW, a, e, flags)
    bases = fc.unary_operands(field)
    for x in fc.pow_exponents(field):
        same(L, field, fc.POW, bases, fc.pack([x], 32), flags | fc.SHARED_B)
    one = fc.unpack(fc.model_op(field, fc.POW, fc.pack([0], fc.nbytes(field)), fc.pack([0], 32), flags)[1], fc.nbytes(field))
    assert one == [(1 << (8 * fc.nbytes(field))) % fc.modulus(field) if flags else 1]       # 0^0 = 1


@pytest.mark.parametrize("flags", FORMS)
@pytest.mark.parametrize("field", fc.FIELDS)
def test_sqrt_at_every_two_adic_depth(L, field, flags):
    p, eb = fc.modulus(field), fc.nbytes(field)
    A = 1 << (8 * eb)
    store = (lambda v: v * A % p) if flags else (lambda v: v)
    squares, others = fc.sqrt_inputs(field)
    rc, out, _, _ = same(L, field, fc.SQRT, fc.pack([store(v) for v in squares], eb), None, flags)
    assert rc == 0
    for v, r in zip(squares, fc.unpack(out, eb)):
        r = r * pow(A, -1, p) % p if flags else r
        assert r * r % p == v and r <= (p - 1) // 2
    for k, v in enumerate(others):                                  # every non-square alone, and all at once
        assert same(L, field, fc.SQRT, fc.pack([store(v)], eb), None, flags)[2:] == (0, fc.NOT_SQUARE), k
    mixed = fc.pack([store(v) for v in squares[:5] + others[3:] + squares[5:]], eb)
    assert same(L, field, fc.SQRT, mixed, None, flags)[2:] == (5, fc.NOT_SQUARE)


# ---- 3. the inversion block -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", fc.GROUPS)
def test_inversion_block_shapes(L, group):
    for n in fc.inv_sizes(group):
        a = fc.pack(fc.inv_values(fc.FIELD_P, n, group, zeros=False), 32)
        same(L, fc.FIELD_P, fc.INV, a, None, 0, group)
        z = fc.pack(fc.inv_values(fc.FIELD_P, n, group), 32)
        got = same(L, fc.FIELD_P, fc.INV, z, None, fc.ZERO_OK, group)
        if n >= 256 * group:
            assert fc.unpack(got[1], 32)[6::256][:group] == [0] * group          # the chain of zeros
            assert same(L, fc.FIELD_P, fc.INV, z, None, 0, group)[2:] == (3, fc.ZERO)        # several zeros: the lowest


@pytest.mark.parametrize("field,flags", [(fc.FIELD_Q377, 0), (fc.FIELD_Q377, fc.MONTGOMERY), (fc.FIELD_P, fc.MONTGOMERY)])
def test_inversion_block_other_field_and_form(L, field, flags):
    for group in (8, 16):
        n = 2 * 256 * group + 300
        same(L, field, fc.INV, fc.pack(fc.inv_values(field, n, group), fc.nbytes(field)), None, flags | fc.ZERO_OK, group)


def test_in_place(L):
    for field in fc.FIELDS:
        eb = fc.nbytes(field)
        a = fc.pack(fc.inv_values(field, 256 * 8 + 5, 8), eb)
        for op, flags in ((fc.INV, fc.ZERO_OK), (fc.SQUARE, 0), (fc.NEG, 0)):
            assert fc.shim_op(L, field, op, a, None, flags, 8, in_place=True)[1] == fc.model_op(field, op, a, None, flags)[1]


# ---- 4. deliberate mistakes are caught ---------------------------------------------------------------------------------------------
def test_deliberate_mistakes_are_caught(L):
    f, eb, g = fc.FIELD_P, 32, 8
    n = 256 * g + 1
    a = fc.pack(fc.inv_values(f, n, g, zeros=False), eb)
    want = fc.model_op(f, fc.INV, a)[1]
    assert fc.shim_op(L, f, fc.INV, a, None, 0, g)[1] == want
    assert fc.shim_op(L, f, fc.INV, a, None, 0, g, fc.M_WALK)[1] != want
    z = fc.pack(fc.inv_values(f, n, g), eb)
    want = fc.model_op(f, fc.INV, z, None, fc.ZERO_OK)[1]
    assert fc.shim_op(L, f, fc.INV, z, None, fc.ZERO_OK, g)[1] == want
    assert fc.shim_op(L, f, fc.INV, z, None, fc.ZERO_OK, g, fc.M_ZERO)[1] != want
    four = fc.pack([4], eb)
    assert fc.shim_op(L, f, fc.SQRT, four)[1] == fc.pack([2], eb)
    assert fc.shim_op(L, f, fc.SQRT, four, None, 0, 16, fc.M_LARGER)[1] == fc.pack([fc.modulus(f) - 2], eb)
    three, e = fc.pack([3], eb), fc.pack([fc.modulus(f) + 5], 32)
    for flags in (0, fc.SHARED_B):
        assert fc.shim_op(L, f, fc.POW, three, e, flags)[1] == fc.pack([3 ** 6], eb)      # 3^(p + 5) = 3^(p - 1) 3^6
        assert fc.shim_op(L, f, fc.POW, three, e, flags, 16, fc.M_REDUCE)[1] == fc.pack([3 ** 5], eb)


# ---- 5. the same code under the sanitizers, as a program of its own --------------------------------------------------------------------
def test_field_ops_under_sanitizers(tmp_path):
    exe = str(tmp_path / "san_field")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "csrc", "san_field.cpp")])
    env = {k: v for k, v in os.environ.items() if k != "LD_PRELOAD"}
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, env=env)
    assert r.returncode == 0 and "san_field ok" in r.stdout, r.stdout[-2000:]


# ---- 6. the names -------------------------------------------------------------------------------------------------------------------
def test_names_in_header_library_package_and_addon(pkg):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name, val in (("TE_MSM_EFIELD", "(-6)"), ("TE_MSM_FIELD_P", "0"), ("TE_MSM_FIELD_Q377", "1"), ("TE_MSM_FIELD_SHARED_B", "1"),
                      ("TE_MSM_FIELD_MONTGOMERY", "2"), ("TE_MSM_FIELD_ZERO_OK", "4"), ("TE_MSM_FIELD_ZERO", "1"), ("TE_MSM_FIELD_NOT_SQUARE", "2")):
        assert re.search(r"#define %s +%s(?![0-9])" % (name, re.escape(val)), hdr), name
    for k, name in enumerate(("ADD", "SUB", "MUL", "DOUBLE", "NEG", "SQUARE", "INV", "POW", "SQRT")):
        assert re.search(r"#define TE_MSM_FIELD_%s +%d\b" % (name, k), hdr) and getattr(pkg, "FIELD_" + name) == k
    assert "field_ops_cost.txt" in hdr and "bad_field_index" in hdr and "field_inv_group" in hdr
    lib = ctypes.CDLL(pkg.library_path())
    assert hasattr(lib, "te_msm_field_op") and hasattr(lib, "te_msm_field_op_device")
    assert (pkg.EFIELD, pkg.FIELD_P, pkg.FIELD_Q377, pkg.FIELD_ZERO, pkg.FIELD_NOT_SQUARE) == (-6, 0, 1, 1, 2)
    assert callable(pkg.MsmContext.field_op) and callable(pkg.MsmContext.field_op_device)
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    assert "fieldOp" in open(os.path.join(js, "addon.cc")).read() and "fieldOp" in open(os.path.join(js, "submission.d.ts")).read()
    g = re.search(r"#define TE_MSM_FIELD_INV_GROUP +(\d+)u", hdr)
    assert g and int(g.group(1)) in fc.GROUPS
