"""Fixed-base batch scalar multiplication on the GPU (te_msm_bind_base, te_msm_mul_base[_device], te_msm_base_read; include/te_msm.h):
[k_i] P byte for byte against the bigint models on both curves, host and device forms, every window width of the cases; the table entry
for entry against the host build of the same code; against te_msm_mul over the point replicated; 1, 2 and 4 device contexts; BLS12-377
infinity inside the affine groups; Montgomery scalars; every error with the output untouched; lifetime of the table.  Every case list
is cleared by the host shim (tests/csrc/mulbasecheck.cpp, whose table accessor counts indices outside the table) before it goes to the
device."""
import ctypes
import json
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from oracle import model as m
from oracle import model377 as b
from oracle import oracle
import mul_base_cases as mc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PB = {0: 64, 1: 96}
SB = {0: 32, 1: 48}
EINVAL, EPOINT = -1, -5
PIECE = 1 << 18                     # a device multiplies in pieces of 2^18 scalars (points.hip, kMulPiece)


def _dev(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _ctx(pkg, curve, ids=(0,), W=None, level=0):
    c = pkg.MsmContext(ids)
    c.set_option("curve", curve)
    c.set_option("check_points", level)
    if W is not None:
        c.set_option("mul_base_window", W)
    return c


def base_of(curve, i=0):
    """(wire bytes, model point) of a base point: a subgroup point / a G1 point"""
    if curve:
        _, raw, p = mc.bls_base_points()[i]
        return raw, p
    p = mc.te_point("subgroup point %d" % i)
    return m.points_to_bytes([p]), p


def expected(curve, p, ks):
    return mc.bls_expected(p, ks) if curve else mc.te_expected(p, ks)


def cleared(curve, W, raw, ks, want, form=0):
    """the host build of the lane code gives `want` over the same table and scalars, and asked for no entry outside the table"""
    assert mc.shim_mul(curve, W, mc.shim_table(curve, W, raw), ks, form=form) == want
    return want


def mul_device(c, base, sc, n, curve):
    import torch
    ds = _dev(sc or b"\0")
    dout = torch.full((max(1, PB[curve] * n),), 0xAB, dtype=torch.uint8, device="cuda")
    _sync()
    c.mul_base_device(base, ds.data_ptr(), n, dout.data_ptr())
    return bytes(dout.cpu().numpy())


def rand_ints(seed, n):
    raw = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(n)]


# ---- sizes and forms ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_sizes_host_and_device_forms(pkg, curve):
    raw, p = base_of(curve)
    ks_all = mc.padded_scalars(curve, 300, 0x51 + curve)
    want_all = cleared(curve, mc.DEFAULT_W, raw, ks_all, expected(curve, p, ks_all))
    pb = PB[curve]
    with _ctx(pkg, curve) as c:
        base = c.bind_base(raw)
        assert base.window == mc.DEFAULT_W
        for n in (0, 1, 2, 63, 64, 65, 255, 256, 257, 300):
            sc = mc.scalar_bytes(curve, ks_all[:n])
            assert c.mul_base(base, sc) == want_all[:pb * n], n
            got = mul_device(c, base, sc, n, curve)
            if n == 0:
                assert got == b"\xab"                      # n = 0 leaves the output untouched
                out = ctypes.create_string_buffer(b"\xab" * pb, pb)
                assert c._L.te_msm_mul_base(c._h, base._h, sc, 0, out) == 0 and out.raw == b"\xab" * pb
            else:
                assert got == want_all[:pb * n], n
        c.release_base(base)


# ---- the case list ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in mc.te_base_points()])
def test_full_case_list_per_base_point_te(pkg, name):
    ks = [k for _, k in mc.case_scalars(0)]
    sc = mc.scalar_bytes(0, ks)
    p = mc.te_point(name)
    raw = m.points_to_bytes([p])
    want = cleared(0, mc.DEFAULT_W, raw, ks, mc.te_expected(p, ks))
    with _ctx(pkg, 0) as c:
        base = c.bind_base(raw)
        assert base.window == mc.DEFAULT_W
        assert c.mul_base(base, sc) == want
        assert mul_device(c, base, sc, len(ks), 0) == want
        c.release_base(base)


def test_full_case_list_per_base_point_bls377(pkg):
    ks = [k for _, k in mc.case_scalars(1)]
    sc = mc.scalar_bytes(1, ks)
    with _ctx(pkg, 1) as c:
        for name, raw, p in mc.bls_base_points():
            want = cleared(1, mc.DEFAULT_W, raw, ks, mc.bls_expected(p, ks))
            base = c.bind_base(raw)
            assert c.mul_base(base, sc) == want, name
            assert mul_device(c, base, sc, len(ks), 1) == want, name
            c.release_base(base)


@pytest.mark.parametrize("W", [4, 5, 8, 11, 12])
@pytest.mark.parametrize("curve", [0, 1])
def test_case_list_at_other_window_widths(pkg, curve, W):
    raw, p = base_of(curve, 1)
    ks = mc.padded_scalars(curve, 300, 0x300)               # (one list for every W: the model answers it once)
    want = cleared(curve, W, raw, ks, expected(curve, p, ks))
    sc = mc.scalar_bytes(curve, ks)
    with _ctx(pkg, curve, W=W) as c:
        base = c.bind_base(raw)
        assert base.window == W
        assert c.mul_base(base, sc) == want
        assert mul_device(c, base, sc, 300, curve) == want


def test_torsion_base_at_other_window_widths(pkg):
    p = mc.te_point("G+T4")
    raw = m.points_to_bytes([p])
    ks = mc.padded_scalars(0, 300, 0x7044)
    sc = mc.scalar_bytes(0, ks)
    for W in (4, 8):
        want = cleared(0, W, raw, ks, mc.te_expected(p, ks))
        with _ctx(pkg, 0, W=W) as c:
            assert c.mul_base(c.bind_base(raw), sc) == want, W


# ---- against the existing kernel ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_equals_te_msm_mul_over_the_point_replicated(pkg, curve):
    n = 4099
    raw, _ = base_of(curve)
    ks = rand_ints(0x4099 + curve, n)
    sc = mc.scalar_bytes(curve, ks)
    with _ctx(pkg, curve) as c:
        base = c.bind_base(raw)
        got = c.mul_base(base, sc)
        assert got == c.mul(raw * n, sc)
        assert mul_device(c, base, sc, n, curve) == got


def test_one_scalar_past_the_piece_boundary(pkg):
    """te_msm_mul_base_device walks its scalars in pieces: the second turn of that loop, one scalar long"""
    import torch
    n = PIECE + 1
    raw, p = base_of(0)
    sc = np.random.default_rng(0x9BA5E).integers(0, 256, size=(n, 32), dtype=np.uint8).tobytes()
    rnd = random.Random(0x9BA5E)
    idx = sorted(set([0, PIECE - 2, PIECE - 1, PIECE] + rnd.sample(range(n), 40)))
    with _ctx(pkg, 0) as c:
        base = c.bind_base(raw)
        assert base.window == mc.DEFAULT_W
        got = mul_device(c, base, sc, n, 0)
        assert len(got) == 64 * n
        ks = [int.from_bytes(sc[32 * i:32 * i + 32], "little") for i in idx]
        want = mc.te_expected(p, ks)
        for j, i in enumerate(idx):
            assert got[64 * i:64 * i + 64] == want[64 * j:64 * j + 64], i
        dp, ds = _dev(raw * n), _dev(sc)
        dout = torch.full((64 * n,), 0xAB, dtype=torch.uint8, device="cuda")
        _sync()
        c.mul_device(dp.data_ptr(), ds.data_ptr(), n, dout.data_ptr())
        assert bytes(dout.cpu().numpy()) == got


# ---- the table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [4, 8])
@pytest.mark.parametrize("curve", [0, 1])
def test_table_entry_for_entry(pkg, curve, W):
    raw, _ = base_of(curve)
    M, H, E = mc.geometry(W)
    want = mc.shim_table(curve, W, raw)
    with _ctx(pkg, curve, ids=(0, 0), W=W) as c:
        base = c.bind_base(raw)
        for di in (0, 1):
            got = b""
            for i in range(M):
                eb, part = c.base_read(base, i, 0, H + 1, di)
                assert eb == mc.SLOT and len(part) == (H + 1) * mc.SLOT
                got += part
            assert got == want, di
        assert c.base_read(base, M - 1, H, 1)[1] == want[-mc.SLOT:]
        with pytest.raises(pkg.MsmError):
            c.base_read(base, M, 0, 1)
        with pytest.raises(pkg.MsmError):
            c.base_read(base, 0, H, 2)


# ---- several devices ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_device_lists_give_the_same_bytes(pkg, curve):
    raw, p = base_of(curve)
    ks = mc.padded_scalars(curve, 301, 0xD3)
    want = cleared(curve, mc.DEFAULT_W, raw, ks, expected(curve, p, ks))
    sc = mc.scalar_bytes(curve, ks)
    for ids in ((0,), (0, 0), (0, 0, 0, 0)):
        with _ctx(pkg, curve, ids=ids) as c:
            base = c.bind_base(raw)
            assert c.get_option("mul_base_bytes") == len(ids) * mc.geometry(mc.DEFAULT_W)[2] * mc.SLOT
            assert c.mul_base(base, sc) == want, ids
            assert c.mul_base(base, sc[:SB[curve] * 3]) == want[:PB[curve] * 3], ids     # fewer scalars than devices
            assert mul_device(c, base, sc, 301, curve) == want, ids


# ---- BLS12-377 infinity ---------------------------------------------------------------------------------------------------------------
def test_bls377_infinity_slots(pkg):
    raw, p = base_of(1)
    with _ctx(pkg, 1) as c:
        base = c.bind_base(raw)
        for n in (1, 7, 8, 9, 17):
            for what, ks in mc.bls_infinity_plans(n):
                want = cleared(1, mc.DEFAULT_W, raw, ks, mc.bls_expected(p, ks))
                assert want.count(bytes(96)) >= 1
                sc = mc.scalar_bytes(1, ks)
                assert c.mul_base(base, sc) == want, (n, what)
                assert mul_device(c, base, sc, n, 1) == want, (n, what)


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def _untouched_host(c, base_handle, sc, n, pb):
    out = ctypes.create_string_buffer(b"\xab" * (pb * n), pb * n)
    rc = c._L.te_msm_mul_base(c._h, base_handle, sc, n, out)
    assert out.raw == b"\xab" * (pb * n)
    return rc


def _untouched_device(c, base_handle, sc, n, pb):
    import torch
    ds = _dev(sc)
    dout = torch.full((pb * n,), 0xAB, dtype=torch.uint8, device="cuda")
    _sync()
    rc = c._L.te_msm_mul_base_device(c._h, base_handle, ds.data_ptr(), n, dout.data_ptr())
    assert bytes(dout.cpu().numpy()) == b"\xab" * (pb * n)
    return rc


def test_bad_points_at_bind(pkg):
    g = (m.GX, m.GY)
    good = m.points_to_bytes([g])
    off = m.points_to_bytes([(g[0], (g[1] + 1) % m.P)])
    assert not m.on_curve(m.xy_from_bytes(off))
    gt4 = mc.te_point("G+T4")
    gt4_raw = m.points_to_bytes([gt4])
    ks = [k for _, k in mc.case_scalars(0)][:12]
    sc = mc.scalar_bytes(0, ks)
    with _ctx(pkg, 0, level=1) as c:
        keep = c.bind_base(good)
        before = c.get_option("mul_bases_bound")
        assert before == 1
        with pytest.raises(pkg.MsmError) as e:
            c.bind_base(off)
        assert (e.value.code, e.value.index, e.value.reason) == (EPOINT, 0, pkg.POINT_OFF_CURVE)
        h = ctypes.c_void_p(0x1234)
        assert c._L.te_msm_bind_base(c._h, off, ctypes.byref(h)) == EPOINT and not h.value       # no handle
        assert c.get_option("mul_bases_bound") == before
        assert c.mul_base(c.bind_base(gt4_raw), sc) == mc.te_expected(gt4, ks)                    # on the curve: level 1 passes it
        c.set_option("check_points", 2)
        bound = c.get_option("mul_bases_bound")
        with pytest.raises(pkg.MsmError) as e:
            c.bind_base(gt4_raw)
        assert (e.value.code, e.value.index, e.value.reason) == (EPOINT, 0, pkg.POINT_NOT_IN_SUBGROUP)
        assert c.get_option("mul_bases_bound") == bound
        c.set_option("check_points", 0)
        want = cleared(0, mc.DEFAULT_W, gt4_raw, ks, mc.te_expected(gt4, ks))
        assert c.mul_base(c.bind_base(gt4_raw), sc) == want                                       # level 0 binds it, and is exact
        assert c.mul_base(keep, sc) == mc.te_expected(g, ks)                                      # the context is still usable


def test_wrong_curve_released_handle_and_null_pointers(pkg):
    raw, p = base_of(0)
    ks = [k for _, k in mc.case_scalars(0)][:9]
    sc, sc377 = mc.scalar_bytes(0, ks), mc.scalar_bytes(1, ks)
    with _ctx(pkg, 0) as c:
        base = c.bind_base(raw)
        h = base._h
        want = mc.te_expected(p, ks)
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)                                             # a handle of the other curve
        assert _untouched_host(c, h, sc377, 9, 96) == EINVAL
        assert _untouched_device(c, h, sc377, 9, 96) == EINVAL
        c.set_option("curve", pkg.CURVE_TE_BLS12)
        assert c.mul_base(base, sc) == want
        # null pointers with n > 0
        out = ctypes.create_string_buffer(64 * 9)
        assert c._L.te_msm_mul_base(c._h, h, None, 9, out) == EINVAL
        assert c._L.te_msm_mul_base(c._h, h, sc, 9, None) == EINVAL
        assert c._L.te_msm_mul_base_device(c._h, h, None, 9, None) == EINVAL
        assert c._L.te_msm_mul_base(c._h, None, sc, 9, out) == EINVAL
        # device buffers that are not on a device of the context: host memory
        host_sc = ctypes.create_string_buffer(sc, len(sc))
        host_out = ctypes.create_string_buffer(b"\xab" * (64 * 9), 64 * 9)
        rc = c._L.te_msm_mul_base_device(c._h, h, ctypes.cast(host_sc, ctypes.c_void_p), 9, ctypes.cast(host_out, ctypes.c_void_p))
        assert rc == EINVAL and host_out.raw == b"\xab" * (64 * 9)
        assert c.mul_base(base, sc) == want
        # a released handle
        other = c.bind_base(raw)
        c.release_base(base)
        assert c.get_option("mul_bases_bound") == 1
        assert _untouched_host(c, h, sc, 9, 64) == EINVAL
        assert _untouched_device(c, h, sc, 9, 64) == EINVAL
        assert c._L.te_msm_release_base(c._h, h) == EINVAL
        assert c.mul_base(other, sc) == want                                                      # still usable


# ---- Montgomery scalars ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_montgomery_scalars(pkg, curve):
    raw, p = base_of(curve)
    mod = mc.scalar_modulus(curve)
    ks = [0, 1, mod - 1] + [k % mod for k in rand_ints(0x3047 + curve, 70)]
    recs = [k * mc.R256 % mod for k in ks] + [mod, mc.TOP] + rand_ints(0x3048, 8)               # any 256-bit record stands for its residue
    decoded = [mc.montgomery_decode(curve, a) for a in recs]
    want = cleared(curve, mc.DEFAULT_W, raw, recs, expected(curve, p, decoded), form=1)
    canonical = cleared(curve, mc.DEFAULT_W, raw, recs, expected(curve, p, recs))
    sc = mc.scalar_bytes(curve, recs)
    with _ctx(pkg, curve) as c:
        base = c.bind_base(raw)
        c.set_option("scalars_montgomery", 1)
        assert c.mul_base(base, sc) == want
        assert mul_device(c, base, sc, len(recs), curve) == want
        with pytest.raises(pkg.MsmError):
            c.mul(raw * len(recs), sc)                                                            # te_msm_mul* keep refusing the option
        c.set_option("scalars_montgomery", 0)
        assert c.mul_base(base, sc) == canonical
        assert mul_device(c, base, sc, len(recs), curve) == canonical


# ---- lifetime ---------------------------------------------------------------------------------------------------------------------------
def test_table_memory_is_counted_and_given_back(pkg):
    raw, _ = base_of(0)
    raw377, _ = base_of(1)
    with _ctx(pkg, 0, ids=(0, 0)) as c:
        assert c.get_option("mul_base_bytes") == 0 and c.get_option("mul_bases_bound") == 0
        total, held = 0, []
        for W in (4, 8, 10):
            c.set_option("mul_base_window", W)
            assert c.get_option("mul_base_window") == W
            M, H, E = mc.geometry(W)
            assert E == M * ((1 << (W - 1)) + 1)
            held.append(c.bind_base(raw))
            total += 2 * E * 128
            assert c.get_option("mul_base_bytes") == total and c.get_option("mul_bases_bound") == len(held)
        assert c.get_option("bases_bound") == 0 and c.get_option("bases_bytes") == 0              # not folded into the MSM's bound sets
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        b377 = c.bind_base(raw377)
        assert c.get_option("mul_base_bytes") == total + 2 * mc.geometry(10)[2] * 128
        c.release_base(b377)
        c.set_option("curve", pkg.CURVE_TE_BLS12)
        for h in held:
            c.release_base(h)
        assert c.get_option("mul_base_bytes") == 0 and c.get_option("mul_bases_bound") == 0
        for W in (3, 13):
            with pytest.raises(pkg.MsmError):
                c.set_option("mul_base_window", W)


def test_destroy_with_a_handle_still_bound(pkg):
    raw, p = base_of(0)
    ks = [5, 7]
    for _ in range(3):
        c = _ctx(pkg, 0, ids=(0, 0), W=12)
        base = c.bind_base(raw)
        assert c.get_option("mul_base_bytes") == 2 * mc.geometry(12)[2] * 128
        assert c.mul_base(base, mc.scalar_bytes(0, ks)) == mc.te_expected(p, ks)
        c.close()                                                                                  # te_msm_destroy frees the tables on both devices
    with _ctx(pkg, 0) as c:                                                                        # and the process goes on
        assert c.get_option("mul_bases_bound") == 0
        assert c.mul_base(c.bind_base(raw), mc.scalar_bytes(0, ks)) == mc.te_expected(p, ks)


def test_calling_threads_device_is_left_alone(pkg):
    import torch
    raw, _ = base_of(0)
    before = torch.cuda.current_device()
    with _ctx(pkg, 0, ids=(0, 0)) as c:
        base = c.bind_base(raw)
        c.mul_base(base, bytes(32 * 5))
        mul_device(c, base, bytes(32 * 5), 5, 0)
        c.base_read(base, 0, 0, 1, 1)
        c.release_base(base)
    assert torch.cuda.current_device() == before


# ---- Node -------------------------------------------------------------------------------------------------------------------------------
def test_node_scalar_mul_base(pkg, tmp_path):
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not installed on this box")
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists("/usr/include/node/node_api.h") and not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        pytest.skip("no N-API addon and no node headers to build it")
    if not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        subprocess.check_call(["make", "-C", js, "-s"])
    n = 257
    point = oracle.gen_points(23, 1)
    sc = oracle.gen_scalars(23, n)
    for name, data in (("p.bin", point), ("pn.bin", point * n), ("s.bin", sc)):
        (tmp_path / name).write_bytes(data)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
const [p, pn, sc] = process.argv.slice(2).map((f) => fs.readFileSync(f));
const out = {};
try { m.scalarMulBase(sc); out.unbound = 'returned'; } catch (e) { out.unbound = String(e.message); }
m.setBase(p);
out.base = m.scalarMulBase(sc).toString('hex');
out.again = m.scalarMulBase(sc).toString('hex');
out.mul = m.scalarMul(pn, sc).toString('hex');
console.log(JSON.stringify(out));
"""
    files = [str(tmp_path / f) for f in ("p.bin", "pn.bin", "s.bin")]
    r = subprocess.run([node, "-e", script, js] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.stdout.strip(), r.stderr.decode()
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert out["base"] == out["mul"] and out["again"] == out["mul"] and len(out["base"]) == 2 * 64 * n
    assert "setBase" in out["unbound"]
    with _ctx(pkg, 0) as c:
        assert bytes.fromhex(out["base"]) == c.mul_base(c.bind_base(point), sc)
