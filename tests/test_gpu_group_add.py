"""Batched group addition and point-set sums on the GPU (te_msm_add*, te_msm_sum*; include/te_msm.h): byte-equal to the bigint models on
both curves, host and device buffers, one to four slices; in place; shared B; the edge pairs of the host test; BLS12-377 infinity in and
out; a call one pair past the piece boundary; sums against the closed form of a chain point buffer and against the MSM over all-ones
scalars; bad points and bad x with the failing operand; the Node functions."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import chain_msm
from oracle import model as m
from oracle import model377 as b

import group_add_cases as gc

pytestmark = pytest.mark.gpu

ROOT = gc.ROOT
COUNTS = (1, 8, 9, 255, 256, 257, 2047, 2048, 2049)
IDS = [(0,), (0, 0), (0, 0, 0, 0)]
PAT = 0xAB


def _dev(buf):
    import torch
    return torch.frombuffer(bytearray(buf or b"\0"), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _ctx(pkg, curve, level=0, ids=(0,)):
    c = pkg.MsmContext(ids)
    c.set_option("curve", curve)
    c.set_option("check_points", level)
    return c


def add_device(c, a, bb, n, subtract=False, shared_b=False, out="new"):
    """out: "new" (a buffer pre-filled with a pattern), "a" or "b" (in place); returns the output bytes"""
    import torch
    da, db = _dev(a), _dev(bb)
    dout = {"new": torch.full((max(1, len(a)),), PAT, dtype=torch.uint8, device="cuda"), "a": da, "b": db}[out]
    _sync()
    c.add_device(da.data_ptr(), db.data_ptr(), n, dout.data_ptr(), subtract=subtract, shared_b=shared_b)
    return bytes(dout.cpu().numpy())[:len(a)]


_OPERANDS = {}


def operands(pkg, curve):
    """(a, b, model a + b, model a - b) over max(COUNTS) pairs, computed once: every count is a prefix"""
    if curve not in _OPERANDS:
        n = max(COUNTS)
        a, _ = pkg.synth_inputs(0x6AD + curve, n, scalars=False, curve=curve)
        bb, _ = pkg.synth_inputs(0x6AE + curve, n, scalars=False, curve=curve)
        _OPERANDS[curve] = (a, bb, gc.model_add_all(curve, a, bb), gc.model_add_all(curve, a, bb, subtract=True))
    return _OPERANDS[curve]


# ---- add and subtract against the models ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("ids", IDS)
def test_add_and_subtract_match_the_model_at_every_count(pkg, curve, ids):
    pb = gc.point_bytes(curve)
    a, bb, want_add, want_sub = operands(pkg, curve)
    with _ctx(pkg, curve, 0, ids) as c:
        assert c.add(b"", b"") == b""
        for n in COUNTS:
            A, B = a[:pb * n], bb[:pb * n]
            s = c.add(A, B)
            assert s == want_add[:pb * n], n
            assert c.add(A, B, subtract=True) == want_sub[:pb * n], n
            assert c.add(s, B, subtract=True) == A, n                      # (A + B) - B == A, byte for byte
            assert add_device(c, A, B, n) == s, n
            assert add_device(c, A, B, n, subtract=True) == want_sub[:pb * n], n
            assert add_device(c, A, B, n, out="a") == s and add_device(c, A, B, n, out="b") == s, n       # in place: d_out = d_a, d_out = d_b
            assert add_device(c, s, B, n, subtract=True, out="a") == A, n
            if n > 1:
                one = B[:pb]
                assert c.add(A, one) == c.add(A, one * n), n               # shared B against B replicated
                assert add_device(c, A, one, n, shared_b=True) == c.add(A, one * n), n
                assert add_device(c, A, one, n, subtract=True, shared_b=True) == c.add(A, one * n, subtract=True), n
        out = ctypes.create_string_buffer(a[:pb * 300], pb * 300)          # the host form with out == a
        assert c._L.te_msm_add(c._h, out, bb[:pb * 300], 300, 0, out) == 0 and out.raw == want_add[:pb * 300]


@pytest.mark.parametrize("curve", [0, 1])
def test_edge_pairs_at_the_first_a_middle_and_the_last_index_of_300(pkg, curve):
    pb = gc.point_bytes(curve)
    a, bb, want_add, want_sub = operands(pkg, curve)
    pairs = gc.bls_core_pairs() if curve == 1 else gc.te_core_pairs()
    with _ctx(pkg, curve) as c:
        for k in range(0, len(pairs), 3):
            A, B = bytearray(a[:pb * 300]), bytearray(bb[:pb * 300])
            wa, ws = bytearray(want_add[:pb * 300]), bytearray(want_sub[:pb * 300])
            for at, (_, ra, rb) in zip((0, 157, 299), pairs[k:k + 3]):
                A[pb * at:pb * at + pb], B[pb * at:pb * at + pb] = ra, rb
                wa[pb * at:pb * at + pb], ws[pb * at:pb * at + pb] = gc.model_add(curve, ra, rb), gc.model_add(curve, ra, rb, subtract=True)
            names = [p[0] for p in pairs[k:k + 3]]
            assert add_device(c, bytes(A), bytes(B), 300) == bytes(wa), names
            assert add_device(c, bytes(A), bytes(B), 300, subtract=True) == bytes(ws), names
        assert c.add(bytes(A), bytes(B)) == bytes(wa)


def test_bls377_infinity_at_every_position_of_a_lanes_group_of_eight(pkg):
    a, bb, want_add, _ = operands(pkg, 1)
    n, inf = 24, bytes(96)
    with _ctx(pkg, 1) as c:
        for pos in range(8):
            A, B = bytearray(a[:96 * n]), bytearray(bb[:96 * n])
            A[96 * pos:96 * pos + 96] = inf                               # O + B
            B[96 * (8 + pos):96 * (9 + pos)] = inf                        # A + O
            A[96 * (16 + pos):96 * (17 + pos)] = inf                      # O + O
            B[96 * (16 + pos):96 * (17 + pos)] = inf
            want = gc.model_add_all(1, bytes(A), bytes(B))
            assert want[96 * (16 + pos):96 * (17 + pos)] == inf and want[96 * pos:96 * pos + 96] == bytes(B[96 * pos:96 * pos + 96])
            assert add_device(c, bytes(A), bytes(B), n) == want, pos
            same = add_device(c, bytes(A), bytes(A), n, subtract=True)    # P - P: every slot infinity
            assert same == inf * n, pos
            assert add_device(c, same, bytes(B), n) == bytes(B), pos      # ... and accepted again: no host fix-up in a chain


@pytest.mark.parametrize("curve", [0, 1])
def test_chained_sum_of_add_matches_the_model(pkg, curve):
    pb = gc.point_bytes(curve)
    a, bb, want_add, _ = operands(pkg, curve)
    n = 300
    import torch
    with _ctx(pkg, curve) as c:
        da, db = _dev(a[:pb * n]), _dev(bb[:pb * n])
        _sync()
        c.add_device(da.data_ptr(), db.data_ptr(), n, da.data_ptr())
        assert c.sum_device(da.data_ptr(), n) == gc.model_sum(curve, want_add[:pb * n])
        c.add_device(da.data_ptr(), da.data_ptr(), n, da.data_ptr(), subtract=True)       # acc - acc: all identity
        assert c.sum_device(da.data_ptr(), n) == (bytes(96) if curve == 1 else m.points_to_bytes([(0, 1)]))


def test_add_one_pair_past_the_piece_boundary(pkg):
    """te_msm_add_device cuts a call into pieces of "group_add_piece" pairs that share one projective buffer: n = piece + 1 runs a whole piece
    and a piece of one pair.  Twisted-Edwards (the cut is the same code on both curves).  Operands: 4099 points tiled over the array at two
    different phases, so every pair near the boundary is a different pair."""
    import torch
    with _ctx(pkg, 0) as c:
        piece = c.get_option("group_add_piece")
        n = piece + 1
        k = 4099
        base, _ = pkg.synth_inputs(0x6B0, k, scalars=False, curve=0)
        t = torch.frombuffer(bytearray(base), dtype=torch.uint8).cuda().view(k, 64)
        idx = torch.arange(n, device="cuda")
        da = t[idx % k].contiguous()
        db = t[(idx * 7 + 3) % k].contiguous()
        dout = torch.empty_like(da)
        _sync()
        c.add_device(da.data_ptr(), db.data_ptr(), n, dout.data_ptr())
        got = dout.cpu().numpy()
        rng = np.random.default_rng(0x6B1)
        near = [i for i in range(piece - 300, n)] + [int(i) for i in rng.integers(0, n, size=512)]
        recs = gc.records(0, base)
        for i in near:
            assert got[i].tobytes() == gc.model_add(0, recs[i % k], recs[(i * 7 + 3) % k]), i
        c.add_device(dout.data_ptr(), db.data_ptr(), n, dout.data_ptr(), subtract=True)    # (A + B) - B, in place, over the whole array
        assert np.array_equal(dout.cpu().numpy(), da.cpu().numpy())


# ---- sums ---------------------------------------------------------------------------------------------------------------------------------
def closed_form(curve, pts, n):
    """sum_{i < n} P_i = n P_0 + n (n - 1) / 2 (P_1 - P_0) for a chain point buffer"""
    mod = b if curve == 1 else m
    if n == 0:
        return bytes(96) if curve == 1 else m.points_to_bytes([(0, 1)])
    pb = gc.point_bytes(curve)
    p0 = gc.decode(curve, pts[:pb])
    if n == 1:
        return gc.encode(curve, p0)
    d = mod.add(gc.decode(curve, pts[pb:2 * pb]), mod.neg(p0))
    return gc.encode(curve, mod.add(mod.scalar_mul(n, p0), mod.scalar_mul(n * (n - 1) // 2, d)))


@pytest.mark.parametrize("curve", [0, 1])
def test_sum_against_the_closed_form_of_a_chain(pkg, curve):
    pb = gc.point_bytes(curve)
    with _ctx(pkg, curve) as c:
        edge = c.get_option("group_sum_grid") * 256                       # the stage-1 grid bound x its block: above it lanes stride
        assert edge == 1024 * 256
        nmax = edge + 1
        pts, _ = pkg.synth_inputs(0x6B2 + curve, nmax, scalars=False, curve=curve)
        chain_msm.check_chain(curve, pts, chain_msm.sample_indices(nmax, 16, seed=3))
        dp = _dev(pts)
        _sync()
        for n in (0, 1, 2, 255, 256, 257, edge - 1, edge, edge + 1):
            assert c.sum_device(dp.data_ptr(), n) == closed_form(curve, pts, n), n
        for n in (0, 1, 2, 255, 256, 257):
            assert c.sum(pts[:pb * n]) == closed_form(curve, pts, n), n
            assert closed_form(curve, pts, n) == gc.model_sum(curve, pts[:pb * n]), n
    for ids in IDS[1:]:
        with _ctx(pkg, curve, 0, ids) as c:
            for n in (1, 2, 3, 257, 5000):
                assert c.sum(pts[:pb * n]) == closed_form(curve, pts, n), (ids, n)


@pytest.mark.parametrize("curve", [0, 1])
def test_sum_equals_the_msm_over_all_ones_scalars(pkg, curve):
    n, sb = 300, 48 if curve == 1 else 32
    pts, _ = pkg.synth_inputs(0x6B4 + curve, n, scalars=False, curve=curve)
    ones = (1).to_bytes(sb, "little") * n
    with _ctx(pkg, curve) as c:
        dp, ds = _dev(pts), _dev(ones)
        _sync()
        assert c.sum_device(dp.data_ptr(), n) == c.run_device(dp.data_ptr(), ds.data_ptr(), n)


# ---- errors ---------------------------------------------------------------------------------------------------------------------------------
def _off_curve(curve, rec):
    p = bytearray(rec)
    p[len(p) // 2] ^= 1                                                   # y's low bit
    return bytes(p)


def _outside_subgroup(curve):
    if curve == 1:
        return b.le48(2) + b.le48(3)                                      # on y^2 = x^3 + 1, of order 6
    return m.points_to_bytes([m.add((m.GX, m.GY), (0, m.P - 1))])         # order 2 L


def _put(buf, pb, at, rec):
    r = bytearray(buf)
    r[pb * at:pb * at + pb] = rec
    return bytes(r)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("ids", IDS)
def test_bad_points_name_index_reason_and_operand_output_untouched(pkg, curve, ids):
    pb = gc.point_bytes(curve)
    n = 1000
    a, bb = operands(pkg, curve)[0][:pb * n], operands(pkg, curve)[1][:pb * n]
    for level, reason in ((1, 2), (2, 3)):
        bad = (lambda rec: _off_curve(curve, rec)) if level == 1 else (lambda rec: _outside_subgroup(curve))
        with _ctx(pkg, curve, level, ids) as c:
            assert c.get_option("bad_point_operand") == -1
            for at in (0, n - 1):
                A, B = _put(a, pb, at, bad(a[pb * at:pb * at + pb])), _put(bb, pb, at, bad(bb[pb * at:pb * at + pb]))
                for pa, pbuf, operand in ((A, bb, 0), (a, B, 1), (A, B, 0)):          # in a alone, in b alone, in both: a is named first
                    out = ctypes.create_string_buffer(bytes([PAT]) * (pb * n), pb * n)
                    assert c._L.te_msm_add(c._h, pa, pbuf, n, 0, out) == pkg.EPOINT
                    assert out.raw == bytes([PAT]) * (pb * n)
                    assert (c.get_option("bad_point_index"), c.get_option("bad_point_reason"), c.get_option("bad_point_operand")) == (at, reason, operand)
                    with pytest.raises(pkg.MsmError) as e:
                        c.add(pa, pbuf, subtract=True)
                    assert (e.value.index, e.value.reason, e.value.operand) == (at, reason, operand)
                    if ids == (0,):
                        import torch
                        da, db = _dev(pa), _dev(pbuf)
                        dout = torch.full((pb * n,), PAT, dtype=torch.uint8, device="cuda")
                        _sync()
                        with pytest.raises(pkg.MsmError) as e:
                            c.add_device(da.data_ptr(), db.data_ptr(), n, dout.data_ptr())
                        assert (e.value.index, e.value.reason, e.value.operand) == (at, reason, operand)
                        assert bytes(dout.cpu().numpy()) == bytes([PAT]) * (pb * n)
                with pytest.raises(pkg.MsmError) as e:
                    c.sum(A)
                assert (e.value.index, e.value.reason, e.value.operand) == (at, reason, 0)
                if ids == (0,):
                    da = _dev(A)
                    _sync()
                    with pytest.raises(pkg.MsmError) as e:
                        c.sum_device(da.data_ptr(), n)
                    assert (e.value.index, e.value.reason, e.value.operand) == (at, reason, 0)
            A = _put(_put(a, pb, 700, bad(a[:pb])), pb, 300, bad(a[:pb]))              # the lowest index of several, b's lower than a's
            B = _put(bb, pb, 120, bad(bb[:pb]))
            with pytest.raises(pkg.MsmError) as e:
                c.add(A, B)
            assert (e.value.index, e.value.operand) == (120, 1)
            with pytest.raises(pkg.MsmError) as e:
                c.add(A, bb)
            assert (e.value.index, e.value.operand) == (300, 0)
            with pytest.raises(pkg.MsmError) as e:
                c.add(a, bad(bb[:pb]))                                                 # a failing shared b: index 0, operand 1
            assert (e.value.index, e.value.operand) == (0, 1)
            assert c.add(a, bb) == operands(pkg, curve)[2][:pb * n]                    # the context stays usable
            if curve == 1:
                inf = _put(a, pb, 5, bytes(96))                                        # the zero record passes both levels in these calls
                assert c.add(inf, bb)[96 * 5:96 * 6] == bb[96 * 5:96 * 6]
                assert c.check_points(inf, level) == (5, 2)                            # ... and only in these


def xs_of(pts, curve):
    """x-only form (te_msm_points_from_x's): TE the 32-byte x; BLS12-377 the 48-byte x with bit 7 of byte 47 for the larger root"""
    pb, xb = (96, 48) if curve == 1 else (64, 32)
    arr = np.frombuffer(pts, dtype=np.uint8).reshape(-1, pb)
    xs = arr[:, :xb].copy()
    if curve == 1:
        half = (b.Q - 1) // 2
        ys = arr[:, 48:].tobytes()
        larger = np.fromiter((int.from_bytes(ys[48 * i:48 * i + 48], "little") > half for i in range(len(arr))), dtype=bool, count=len(arr))
        xs[larger, 47] |= 0x80
    return xs.tobytes()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("ids", [(0,), (0, 0, 0, 0)])
def test_x_only_forms_and_bad_x(pkg, curve, ids, kats):
    pb, xb = gc.point_bytes(curve), 48 if curve == 1 else 32
    n = 600
    a, bb, want_add, want_sub = (v[:pb * n] for v in operands(pkg, curve))
    ax, bx = xs_of(a, curve), xs_of(bb, curve)
    noncanon = (b.Q if curve == 1 else m.P).to_bytes(xb, "little")
    with _ctx(pkg, curve, 0, ids) as c:
        assert c.add_x(ax, bx) == want_add and c.add_x(ax, bx, subtract=True) == want_sub
        assert c.add_x(ax, bx[:xb]) == c.add(a, bb[:pb])
        assert c.sum_x(ax) == c.sum(a) == gc.model_sum(curve, a)
        assert c.sum_x(b"") == (bytes(96) if curve == 1 else m.points_to_bytes([(0, 1)]))
        if curve == 0:
            for x1, x2, rx in kats["add_groups_x"]:                        # the reference's vectors through the device
                got = c.add_x(int(x1).to_bytes(32, "little"), int(x2).to_bytes(32, "little"))
                assert int.from_bytes(got[:32], "little") == int(rx)
        for at in (0, n - 1):
            badx_a, badx_b = _put(ax, xb, at, noncanon), _put(bx, xb, at, noncanon)
            for pa, pbuf, operand in ((badx_a, bx, 0), (ax, badx_b, 1), (badx_a, badx_b, 0)):
                out = ctypes.create_string_buffer(bytes([PAT]) * (pb * n), pb * n)
                assert c._L.te_msm_add_x(c._h, pa, pbuf, n, 0, out) == pkg.EPOINT and out.raw == bytes([PAT]) * (pb * n)
                assert (c.get_option("bad_point_index"), c.get_option("bad_point_reason"), c.get_option("bad_point_operand")) == (at, 1, operand)
            with pytest.raises(pkg.MsmError) as e:
                c.sum_x(badx_a)
            assert (e.value.index, e.value.reason, e.value.operand) == (at, 1, 0)
        if curve == 1:
            with pytest.raises(pkg.MsmError) as e:                         # infinity is refused by the x-only forms (points_from_x's rule)
                c.sum_x(_put(ax, xb, 9, bytes(47) + b"\x40"))
            assert (e.value.index, e.value.reason) == (9, 2)
        assert c.add_x(ax, bx) == want_add                                 # still usable
    if curve == 1:
        with _ctx(pkg, curve, 2, ids) as c:                                # a recovered point outside G1 is check_points level 2's to report
            with pytest.raises(pkg.MsmError) as e:
                c.add_x(ax, _put(bx, xb, 77, b.le48(2)))
            assert (e.value.index, e.value.reason, e.value.operand) == (77, 3, 1)


def test_bad_arguments(pkg):
    import torch
    with _ctx(pkg, 0) as c:
        a, bb = operands(pkg, 0)[0][:64 * 4], operands(pkg, 0)[1][:64 * 4]
        out = ctypes.create_string_buffer(64 * 4)
        for flags in (4, 8, 1 << 16, -1):
            assert c._L.te_msm_add(c._h, a, bb, 4, flags, out) == -1       # unknown flag bits: TE_MSM_EINVAL
        with pytest.raises(pkg.MsmError):
            c.add(a, bb[:64 * 3])                                          # neither one point nor n
        da, db = _dev(a), _dev(bb)
        _sync()
        assert c._L.te_msm_add_device(c._h, da.data_ptr(), db.data_ptr(), 4, 4, da.data_ptr()) == -1
        host = ctypes.create_string_buffer(bb, 64 * 4)                     # an operand that is not on the context's device
        assert c._L.te_msm_add_device(c._h, da.data_ptr(), ctypes.cast(host, ctypes.c_void_p), 4, 0, da.data_ptr()) == -1
        assert c._L.te_msm_sum_device(c._h, ctypes.cast(host, ctypes.c_void_p), 4, out) == -1
        assert bytes(da.cpu().numpy()) == a
    if torch.cuda.device_count() > 1:
        with pkg.MsmContext((0, 1)) as c:
            da, db = _dev(a), torch.frombuffer(bytearray(bb), dtype=torch.uint8).to("cuda:1")
            torch.cuda.synchronize(0), torch.cuda.synchronize(1)
            assert c._L.te_msm_add_device(c._h, da.data_ptr(), db.data_ptr(), 4, 0, da.data_ptr()) == -1


# ---- Node -------------------------------------------------------------------------------------------------------------------------------------
def test_node_group_add_and_sum(pkg, tmp_path, kats):
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not installed on this box")
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists("/usr/include/node/node_api.h") and not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        pytest.skip("no N-API addon and no node headers to build it")
    if not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        subprocess.check_call(["make", "-C", js, "-s"])
    n = 600
    a, bb, want_add, want_sub = (v[:64 * n] for v in operands(pkg, 0))
    kx = [[int(v).to_bytes(32, "little") for v in k] for k in kats["add_groups_x"]]
    files = {"a.bin": a, "b.bin": bb, "ax.bin": b"".join(k[0] for k in kx), "bx.bin": b"".join(k[1] for k in kx),
             "bad.bin": _put(bb, 64, 421, _off_curve(0, bb[:64]))}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
const [a, b, ax, bx, bad] = process.argv.slice(2).map((f) => fs.readFileSync(f));
const out = {};
out.add = m.groupAdd(a, b).toString('hex');
out.sub = m.groupAdd(a, b, {subtract: true}).toString('hex');
out.shared = m.groupAdd(a, b.subarray(0, 64)).toString('hex');
out.addx = m.groupAddX(ax, bx).toString('hex');
out.sum = m.groupSum(a).toString('hex');
out.sumx = m.groupSumX(ax).toString('hex');
out.empty = m.groupSum(Buffer.alloc(0)).toString('hex');
m.setCheckPoints(1);
try { m.groupAdd(a, bad); out.bad = 'returned'; } catch (e) { out.bad = String(e.message); out.i = e.index; out.r = e.reason; out.o = e.operand; }
m.setCheckPoints(0);
console.log(JSON.stringify(out));
"""
    r = subprocess.run([node, "-e", script, js] + [str(tmp_path / f) for f in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert bytes.fromhex(out["add"]) == want_add and bytes.fromhex(out["sub"]) == want_sub
    assert bytes.fromhex(out["shared"]) == gc.model_add_all(0, a, bb[:64])
    addx = bytes.fromhex(out["addx"])
    assert [int.from_bytes(addx[64 * i:64 * i + 32], "little") for i in range(5)] == [int(k[2]) for k in kats["add_groups_x"]]
    assert bytes.fromhex(out["sum"]) == gc.model_sum(0, a)
    with _ctx(pkg, 0) as c:
        assert bytes.fromhex(out["sumx"]) == c.sum_x(files["ax.bin"])
    assert bytes.fromhex(out["empty"]) == m.points_to_bytes([(0, 1)])
    assert "te_msm error -5" in out["bad"] and (out["i"], out["r"], out["o"]) == (421, 2, 1), out
