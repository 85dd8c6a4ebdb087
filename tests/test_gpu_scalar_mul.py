"""Batch scalar multiplication on the GPU (te_msm_mul[_device], te_msm_mul_x; include/te_msm.h): [k_i] P_i byte for byte against the
bigint models on both curves, both scalar modes, host and device buffers; the whole array pinned through the MSM against the 24
WASM goldens (the reference's own Address.msm); the reference's known answers; shared = per-point with the scalar repeated, mul_x =
points_from_x + mul; 1, 2 and 4 device contexts give the same bytes; bad points and bad x report the lowest index and its reason
through every entry point with the output untouched."""
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
from oracle import oracle, oracle377
from oracle.gen_golden import make_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOP = (1 << 256) - 1
SIZES = {0: (64, 32, 32), 1: (96, 48, 48)}          # point, scalar record, x-only bytes
PIECE = 1 << 18                     # a device multiplies in pieces of 2^18 points (points.hip, kMulPiece)


def _dev(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _ctx(pkg, curve, level=0, ids=(0,)):
    c = pkg.MsmContext(ids)
    c.set_option("curve", curve)
    c.set_option("check_points", level)
    return c


def rand_scalars(seed, n, curve):
    """n uniformly random 256-bit scalars in the curve's record format (BLS12-377: 48-byte records, top 16 bytes zero)"""
    raw = np.random.default_rng(seed).integers(0, 256, size=(n, 32), dtype=np.uint8)
    if curve == 1:
        raw = np.concatenate([raw, np.zeros((n, 16), dtype=np.uint8)], axis=1)
    return raw.tobytes()


def scalar_at(sc, i, curve):
    sb = SIZES[curve][1]
    return int.from_bytes(sc[sb * i:sb * i + 32], "little")


def expect(curve, pts, i, k):
    """the model's [k] P_i as result bytes"""
    pb = SIZES[curve][0]
    if curve == 1:
        return b.result_to_bytes(b.scalar_mul(k, b.xy_from_bytes(pts[pb * i:pb * i + pb])))
    return m.points_to_bytes([m.scalar_mul(k, m.xy_from_bytes(pts[pb * i:pb * i + pb]))])


def xs_of(pts: bytes, curve: int) -> bytes:
    """x-only form (te_msm_points_from_x's): TE the 32-byte x; BLS12-377 the 48-byte x with bit 7 of byte 47 for the larger root"""
    pb, xb = (96, 48) if curve == 1 else (64, 32)
    a = np.frombuffer(pts, dtype=np.uint8).reshape(-1, pb)
    xs = a[:, :xb].copy()
    if curve == 1:
        half = (b.Q - 1) // 2
        ys = a[:, 48:].tobytes()
        larger = np.fromiter((int.from_bytes(ys[48 * i:48 * i + 48], "little") > half for i in range(len(a))), dtype=bool, count=len(a))
        xs[larger, 47] |= 0x80
    return xs.tobytes()


def mul_device(c, pts, sc, n, shared):
    import torch
    dp, ds = _dev(pts or b"\0"), _dev(sc)
    dout = torch.full((max(1, len(pts)),), 0xAB, dtype=torch.uint8, device="cuda")
    _sync()
    c.mul_device(dp.data_ptr(), ds.data_ptr(), n, dout.data_ptr(), shared=shared)
    return bytes(dout.cpu().numpy())[:len(pts)]


# ---- small n, both curves, both modes, host and device buffers --------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_small_n_byte_equal_to_the_model(pkg, curve):
    pb, sb, _ = SIZES[curve]
    with _ctx(pkg, curve) as c:
        for n in (0, 1, 2, 63, 64, 65, 257):
            pts, _ = pkg.synth_inputs(0x5CA + n, n, scalars=False, curve=curve) if n else (b"", None)
            sc = rand_scalars(n, n, curve)
            exp = b"".join(expect(curve, pts, i, scalar_at(sc, i, curve)) for i in range(n))
            assert c.mul(pts, sc) == exp, n
            if n:
                assert mul_device(c, pts, sc, n, False) == exp, n
            k = TOP - n
            one = k.to_bytes(sb, "little")
            exp_s = b"".join(expect(curve, pts, i, k) for i in range(n))
            assert c.mul(pts, one) == exp_s, n
            if n:
                assert mul_device(c, pts, one, n, True) == exp_s, n


@pytest.mark.parametrize("curve", [0, 1])
def test_identity_results(pkg, curve):
    pb, sb, _ = SIZES[curve]
    order = b.R_ORDER if curve == 1 else m.L
    ident = bytes(96) if curve == 1 else m.points_to_bytes([(0, 1)])
    with _ctx(pkg, curve) as c:
        pts, _ = pkg.synth_inputs(77, 5, scalars=False, curve=curve)
        sc = b"".join(k.to_bytes(sb, "little") for k in (0, order, 2 * order, 1, 0))
        got = c.mul(pts, sc)
        for i in (0, 1, 2, 4):
            assert got[pb * i:pb * i + pb] == ident, i
        assert got[pb * 3:pb * 4] == pts[pb * 3:pb * 4]
        assert c.mul(pts, bytes(sb)) == ident * 5
        assert c.mul(pts, order.to_bytes(sb, "little")) == ident * 5


# ---- large n: sampled against the model ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,logn", [(0, 16), (0, 20), (0, 22), (1, 16), (1, 20)])
def test_large_n_sampled(pkg, curve, logn):
    n = 1 << logn
    pb, sb, _ = SIZES[curve]
    pts, _ = pkg.synth_inputs(0xB16 + logn, n, scalars=False, curve=curve)
    sc = rand_scalars(logn, n, curve)
    rnd = random.Random(logn)
    idx = sorted(set([0, 1, n // 2, n - 2, n - 1] + rnd.sample(range(n), 507) + ([PIECE - 1, PIECE, PIECE + 1, 2 * PIECE] if logn >= 20 else [])))
    with _ctx(pkg, curve) as c:
        got = c.mul(pts, sc)
        assert len(got) == pb * n
        for i in idx:
            assert got[pb * i:pb * i + pb] == expect(curve, pts, i, scalar_at(sc, i, curve)), i
        k = rnd.getrandbits(256)
        got_s = c.mul(pts, k.to_bytes(sb, "little"))
        for i in idx[:64]:
            assert got_s[pb * i:pb * i + pb] == expect(curve, pts, i, k), i
        if logn == 16:
            assert mul_device(c, pts, sc, n, False) == got


# ---- pinned through the MSM ------------------------------------------------------------------------------------------------------------
def test_msm_of_the_products_equals_every_wasm_golden(pkg, wasm_golden):
    """sum_i [k_i] P_i == Address.msm's answer: te_msm_run over mul's output with every scalar 1"""
    seen = set()
    with _ctx(pkg, 0) as c:
        for g in wasm_golden:
            pts, sc = make_inputs(g["seed"], g["n"], g["mode"])
            prod = c.mul(pts, sc)
            ones = (1).to_bytes(32, "little") * g["n"]
            assert m.xy_from_bytes(c.run(prod, ones)) == (int(g["x"]), int(g["y"])), g["name"]
            seen.add(g["n"])
    assert len(wasm_golden) == 24 and max(seen) == 1 << 20


def test_bls377_msm_of_the_products_equals_the_msm(pkg):
    with _ctx(pkg, 1) as c:
        for n in (1000, 1 << 16):
            pts, sc = pkg.synth_inputs(0x377 + n, n, curve=1)
            ones = (1).to_bytes(48, "little") * n
            assert c.run(c.mul(pts, sc), ones) == c.run(pts, sc), n


# ---- the reference's known answers on the device -----------------------------------------------------------------------------------
def test_reference_kats_on_the_device(pkg, kats):
    with _ctx(pkg, 0) as c:
        ks = kats["scalar_mul"]
        pts = m.points_to_bytes([(int(k["x"]), int(k["y"])) for k in ks])
        sc = b"".join(int(k["k"]).to_bytes(32, "little") for k in ks)
        want = m.points_to_bytes([(int(k["rx"]), int(k["ry"])) for k in ks])
        assert c.mul(pts, sc) == want
        assert mul_device(c, pts, sc, len(ks), False) == want
        for i, k in enumerate(ks):
            assert c.mul(pts[64 * i:64 * i + 64], int(k["k"]).to_bytes(32, "little")) == want[64 * i:64 * i + 64]
        g = kats["group_scalar_mul_x"]
        xs = b"".join(int(x).to_bytes(32, "little") for x, _, _ in g)
        sc = b"".join(int(k).to_bytes(32, "little") for _, k, _ in g)
        got = c.mul_x(xs, sc)
        assert [int.from_bytes(got[64 * i:64 * i + 32], "little") for i in range(len(g))] == [int(r) for _, _, r in g]
        for i, (x, k, r) in enumerate(g):                 # shared: one group at a time
            got = c.mul_x(xs[32 * i:32 * i + 32], int(k).to_bytes(32, "little"))
            assert int.from_bytes(got[:32], "little") == int(r)


# ---- modes and paths agree -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_shared_equals_per_point_and_mul_x_equals_from_x_then_mul(pkg, curve):
    pb, sb, _ = SIZES[curve]
    n = 5000
    pts, _ = pkg.synth_inputs(0x5A5 + curve, n, scalars=False, curve=curve)
    with _ctx(pkg, curve) as c:
        for k in (TOP, 1 << 255, 123456789):
            one = k.to_bytes(sb, "little")
            assert c.mul(pts, one) == c.mul(pts, one * n), k
        sc = rand_scalars(99, n, curve)
        xs = xs_of(pts, curve)
        assert c.points_from_x(xs) == pts
        assert c.mul_x(xs, sc) == c.mul(pts, sc)
        assert c.mul_x(xs, sc[:sb]) == c.mul(pts, sc[:sb])


@pytest.mark.parametrize("curve", [0, 1])
def test_one_two_and_four_devices_give_identical_bytes(pkg, curve):
    pb, sb, _ = SIZES[curve]
    n = 3001
    pts, _ = pkg.synth_inputs(0xD1 + curve, n, scalars=False, curve=curve)
    sc = rand_scalars(7, n, curve)
    xs = xs_of(pts, curve)
    outs = []
    for ids in ((0,), (0, 0), (0, 0, 0, 0)):
        with _ctx(pkg, curve, ids=ids) as c:
            outs.append((c.mul(pts, sc), c.mul(pts, sc[:sb]), c.mul_x(xs, sc)))
    assert outs[0] == outs[1] == outs[2]
    assert outs[0][0][:pb] == expect(curve, pts, 0, scalar_at(sc, 0, curve))


# ---- bad points --------------------------------------------------------------------------------------------------------------------------
def _with_bad(buf, width, at):
    a = bytearray(buf)
    for i, rec in at:
        a[width * i:width * i + width] = rec
    return bytes(a)


def _off_curve(curve, pts, i):
    pb = SIZES[curve][0]
    p = bytearray(pts[pb * i:pb * i + pb])
    p[pb // 2] ^= 1                                       # y's low bit: off the curve
    return bytes(p)


def _outside_subgroup(curve):
    if curve == 1:
        # a point of y^2 = x^3 + 1 outside G1: x = 2 gives y = 3 (order 6 over the rationals, so not of order r)
        return b.le48(2) + b.le48(3)
    g2l = m.add((m.GX, m.GY), (0, m.P - 1))               # order 2 L
    return m.points_to_bytes([g2l])


def _raw_mul(c, fn, src, sc, n, shared, out_len):
    out = ctypes.create_string_buffer(b"\xab" * out_len, out_len)
    rc = fn(c._h, src, sc, n, int(shared), out)
    return rc, out.raw


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("ids", [(0,), (0, 0), (0, 0, 0, 0)])
def test_bad_points_report_the_lowest_index_output_untouched(pkg, curve, ids):
    pb, sb, xb = SIZES[curve]
    n = 1000                                             # 4 slices of 250, 2 of 500: the bad indices fall in several slices
    pts, _ = pkg.synth_inputs(0xBAD + curve, n, scalars=False, curve=curve)
    sc = rand_scalars(5, n, curve)
    cases = [
        (1, [(700, _off_curve(curve, pts, 700)), (300, _off_curve(curve, pts, 300))], 300, 2),
        (1, [(999, _off_curve(curve, pts, 999))], 999, 2),
        (2, [(820, _outside_subgroup(curve)), (260, _outside_subgroup(curve))], 260, 3),
        (2, [(600, _outside_subgroup(curve)), (610, _off_curve(curve, pts, 610))], 600, 3),
    ]
    for level, at, lowest, reason in cases:
        bad = _with_bad(pts, pb, at)
        with _ctx(pkg, curve, level, ids) as c:
            for shared in (False, True):
                s = sc[:sb] if shared else sc
                rc, out = _raw_mul(c, c._L.te_msm_mul, bad, s, n, shared, pb * n)
                assert rc == pkg.EPOINT and out == b"\xab" * (pb * n), (level, at)
                assert (c.get_option("bad_point_index"), c.get_option("bad_point_reason")) == (lowest, reason)
                with pytest.raises(pkg.MsmError) as e:
                    c.mul(bad, s)
                assert (e.value.index, e.value.reason) == (lowest, reason)
            if ids == (0,):
                import torch
                dp, ds = _dev(bad), _dev(sc)
                dout = torch.full((pb * n,), 0xAB, dtype=torch.uint8, device="cuda")
                _sync()
                with pytest.raises(pkg.MsmError) as e:
                    c.mul_device(dp.data_ptr(), ds.data_ptr(), n, dout.data_ptr())
                assert (e.value.index, e.value.reason) == (lowest, reason)
                assert bytes(dout.cpu().numpy()) == b"\xab" * (pb * n)
            assert c.mul(pts, sc) == c.mul(pts, sc)      # the context stays usable
            assert c.mul(pts[:pb], sc[:sb]) == expect(curve, pts, 0, scalar_at(sc, 0, curve))


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("ids", [(0,), (0, 0, 0, 0)])
def test_bad_x_reports_the_lowest_index_output_untouched(pkg, curve, ids):
    pb, sb, xb = SIZES[curve]
    n = 1000
    pts, _ = pkg.synth_inputs(0xBADF + curve, n, scalars=False, curve=curve)
    xs = xs_of(pts, curve)
    sc = rand_scalars(6, n, curve)
    noncanon = (b.Q if curve == 1 else m.P).to_bytes(xb, "little")
    bad = _with_bad(xs, xb, [(900, noncanon), (420, noncanon)])
    with _ctx(pkg, curve, 0, ids) as c:
        for shared in (False, True):
            s = sc[:sb] if shared else sc
            rc, out = _raw_mul(c, c._L.te_msm_mul_x, bad, s, n, shared, pb * n)
            assert rc == pkg.EPOINT and out == b"\xab" * (pb * n)
            assert (c.get_option("bad_point_index"), c.get_option("bad_point_reason")) == (420, 1)
            with pytest.raises(pkg.MsmError) as e:
                c.mul_x(bad, s)
            assert (e.value.index, e.value.reason) == (420, 1)
        assert c.mul_x(xs, sc) == c.mul(pts, sc)         # still usable
    if curve == 1:
        # a recovered point outside G1 is check_points level 2's to report: x = 2 recovers (2, +-3)
        bad2 = _with_bad(xs, xb, [(777, b.le48(2))])
        with _ctx(pkg, curve, 2, ids) as c:
            with pytest.raises(pkg.MsmError) as e:
                c.mul_x(bad2, sc)
            assert (e.value.index, e.value.reason) == (777, 3)


def test_bad_arguments(pkg):
    with _ctx(pkg, 0) as c:
        pts, _ = pkg.synth_inputs(1, 4, scalars=False)
        with pytest.raises(pkg.MsmError):
            c.mul(pts, bytes(32 * 3))                    # neither one scalar nor n
        import torch
        dp = _dev(pts)
        _sync()
        host_sc = ctypes.create_string_buffer(32 * 4)
        rc = c._L.te_msm_mul_device(c._h, dp.data_ptr(), ctypes.cast(host_sc, ctypes.c_void_p), 4, 0, dp.data_ptr())
        assert rc == -1                                  # the scalars are not on the device
        assert c.mul(b"", bytes(32)) == b""


# ---- Node -------------------------------------------------------------------------------------------------------------------------------
def test_node_scalar_mul(pkg, tmp_path):
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not installed on this box")
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists("/usr/include/node/node_api.h") and not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        pytest.skip("no N-API addon and no node headers to build it")
    if not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        subprocess.check_call(["make", "-C", js, "-s"])
    n = 2000
    pts, sc = oracle.gen_points(21, n), oracle.gen_scalars(21, n)
    xs = xs_of(pts, 0)
    badx = _with_bad(xs, 32, [(1500, m.P.to_bytes(32, "little")), (1234, m.P.to_bytes(32, "little"))])
    badp = _with_bad(pts, 64, [(1700, _off_curve(0, pts, 1700))])
    k = TOP.to_bytes(32, "little")
    for name, data in (("p.bin", pts), ("s.bin", sc), ("x.bin", xs), ("badx.bin", badx), ("badp.bin", badp), ("k.bin", k)):
        (tmp_path / name).write_bytes(data)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
const [pts, sc, xs, badx, badp, k] = process.argv.slice(2).map((f) => fs.readFileSync(f));
const out = {};
out.mul = m.scalarMul(pts, sc).toString('hex');
out.shared = m.scalarMul(pts, k).toString('hex');
out.mulx = m.scalarMulX(xs, sc).toString('hex');
try { m.scalarMulX(badx, sc); out.badx = 'returned'; } catch (e) { out.badx = String(e.message); out.xi = e.index; out.xr = e.reason; }
m.setCheckPoints(1);
try { m.scalarMul(badp, sc); out.badp = 'returned'; } catch (e) { out.badp = String(e.message); out.pi = e.index; out.pr = e.reason; }
m.setCheckPoints(0);
console.log(JSON.stringify(out));
"""
    files = [str(tmp_path / f) for f in ("p.bin", "s.bin", "x.bin", "badx.bin", "badp.bin", "k.bin")]
    r = subprocess.run([node, "-e", script, js] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    with _ctx(pkg, 0) as c:
        want = c.mul(pts, sc)
        assert bytes.fromhex(out["mul"]) == want and bytes.fromhex(out["mulx"]) == want
        assert bytes.fromhex(out["shared"]) == c.mul(pts, k)
    for i in (0, 1999):
        assert want[64 * i:64 * i + 64] == expect(0, pts, i, scalar_at(sc, i, 0))
    assert "te_msm error -5" in out["badx"] and (out["xi"], out["xr"]) == (1234, 1), out
    assert "te_msm error -5" in out["badp"] and (out["pi"], out["pr"]) == (1700, 2), out
