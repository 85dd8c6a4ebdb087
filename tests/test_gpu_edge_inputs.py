"""The product's own kernels on the edge classes of their inputs, through the C-ABI (te_msm_points_from_x[_device], te_msm_mul[_device],
te_msm_mul_x): what the host tests feed the g++ build of from_x.hip.hpp and scalar_mul.hip.hpp -- the points of order 2 and 4 and their
cosets, x = 0, +-sqrt(-1), x = q - 1, every reserved flag bit, an x whose y^2 has each 2-adic order 0 .. 46, the edge and digit-pattern
scalars, infinity in every position of an affine group -- run here through k_points_from_x, k_scalar_mul and k_scalar_mul_affine with
their own register allocation.  The classes come from the builders of tests/test_points_from_x_host.py and tests/test_scalar_mul_host.py,
their expected bytes and reasons from the bigint models.  Every input is data the API is specified to accept or to reject with a code."""
import ctypes
import functools
import random

import pytest

from oracle import model as m
from oracle import model377 as b
from oracle import oracle, oracle377
from test_points_from_x_host import bls_x_classes, te_x_classes
from test_scalar_mul_host import EDGE_377, EDGE_TE, bls_edge_cases, digit_pattern_scalars, te_edge_cases, te_torsion_points

pytestmark = pytest.mark.gpu

N = 300
SIZES = {0: (64, 32, 32), 1: (96, 48, 48)}          # point, scalar record, x-only bytes


def _dev(buf):
    import torch
    return torch.frombuffer(bytearray(buf), dtype=torch.uint8).cuda()


def _sync():
    import torch
    torch.cuda.synchronize()


def _ctx(pkg, curve, ids=(0,)):
    c = pkg.MsmContext(ids)
    c.set_option("curve", curve)
    c.set_option("check_points", 0)
    return c


@functools.lru_cache(maxsize=None)
def _valid(curve):
    """300 valid x-coordinates and their points"""
    from test_gpu_points_from_x import xs_of
    pts = oracle377.gen_points(0xED6E, N) if curve == 1 else oracle.gen_points(0xED6E, N)
    return xs_of(pts, curve), pts


def _classes(curve, fq377check):
    if curve == 0:
        return te_x_classes()
    from test_oracle_bls377 import _edwards_consts
    return bls_x_classes(_edwards_consts(fq377check)[0])


def _place(buf, width, at, rec):
    a = bytearray(buf)
    a[width * at:width * at + width] = rec
    return bytes(a)


def _from_x_host(pkg, c, xs, n, pb):
    out = ctypes.create_string_buffer(b"\x5a" * (pb * n), pb * n)
    fb, why = ctypes.c_int64(-7), ctypes.c_int(-7)
    rc = pkg.binding._lib().te_msm_points_from_x(c._h, xs, n, out, ctypes.byref(fb), ctypes.byref(why))
    return rc, fb.value, why.value, out.raw


def _from_x_device(pkg, c, xs, n, pb):
    import torch
    dx, dout = _dev(xs), torch.full((pb * n,), 0x5a, dtype=torch.uint8, device="cuda")
    _sync()
    fb, why = ctypes.c_int64(-7), ctypes.c_int(-7)
    rc = pkg.binding._lib().te_msm_points_from_x_device(c._h, dx.data_ptr(), n, dout.data_ptr(), ctypes.byref(fb), ctypes.byref(why))
    return rc, fb.value, why.value, bytes(dout.cpu().numpy())


@pytest.mark.parametrize("curve", [0, 1])
def test_every_rejected_x_class_alone_at_the_first_a_middle_and_the_last_index(pkg, fq377check, curve):
    """each rejected class alone among 300 valid x-coordinates: its index and its reason, the output buffer untouched, through the host and
    the device entry point"""
    pb, _, xb = SIZES[curve]
    xs, _ = _valid(curve)
    rejected = [cl for cl in _classes(curve, fq377check) if isinstance(cl[2], int)]
    assert {r for _, _, r in rejected} == ({1, 2, 3} if curve == 0 else {1, 2})
    failures = []
    with _ctx(pkg, curve) as c:
        for name, x, reason in rejected:
            for at in (0, N // 2, N - 1):
                bx = _place(xs, xb, at, x)
                for entry, fn in (("points_from_x", _from_x_host), ("points_from_x_device", _from_x_device)):
                    rc, idx, why, out = fn(pkg, c, bx, N, pb)
                    if (rc, idx, why) != (pkg.EPOINT, at, reason) or out != b"\x5a" * (pb * N):
                        failures.append("%s: class '%s' at index %d: code %d, index %d, reason %d (expected reason %d)%s"
                                        % (entry, name, at, rc, idx, why, reason, "" if out == b"\x5a" * (pb * N) else ", output written"))
    assert not failures, "\n".join(failures[:20])


@pytest.mark.parametrize("curve", [0, 1])
def test_every_accepted_edge_x_returns_the_models_bytes(pkg, fq377check, curve):
    """the accepted classes in one buffer of 300 -- rotated so that each of the first, a middle and the last index holds one -- among valid x"""
    pb, _, xb = SIZES[curve]
    xs, pts = _valid(curve)
    accepted = [cl for cl in _classes(curve, fq377check) if not isinstance(cl[2], int)]
    assert len(accepted) >= (2 + 6 + 3 + 10 if curve == 0 else 3 * 41 + 2)
    if curve == 0:
        assert sum(1 for cl in accepted if cl[0].startswith("y^2 of 2-adic order")) >= 10
    with _ctx(pkg, curve) as c:
        for shift in (0, N // 2, N - len(accepted)):
            slots = [(shift + j) % N for j in range(len(accepted))]
            bx, want = bytearray(xs), bytearray(pts)
            for at, (_, x, pt) in zip(slots, accepted):
                bx[xb * at:xb * at + xb] = x
                want[pb * at:pb * at + pb] = pt
            for entry, fn in (("points_from_x", _from_x_host), ("points_from_x_device", _from_x_device)):
                rc, idx, why, out = fn(pkg, c, bytes(bx), N, pb)
                assert rc == 0, "%s: code %d at index %d, reason %d: class '%s'" % (entry, rc, idx, why, dict(zip(slots, accepted)).get(idx, ("a valid x",))[0])
                for at, (name, _, pt) in zip(slots, accepted):
                    assert out[pb * at:pb * at + pb] == pt, "%s: class '%s' at index %d" % (entry, name, at)
                assert out == bytes(want), entry


@pytest.mark.parametrize("curve", [0, 1])
def test_several_classes_in_one_buffer_the_lowest_index_wins(pkg, fq377check, curve):
    pb, _, xb = SIZES[curve]
    xs, _ = _valid(curve)
    rejected = [cl for cl in _classes(curve, fq377check) if isinstance(cl[2], int)]
    rnd = random.Random(0xC1A55 + curve)
    with _ctx(pkg, curve) as c:
        for trial in range(6):
            picks = rnd.sample(rejected, 5)
            slots = sorted(rnd.sample(range(N), 5))
            rnd.shuffle(picks)
            bx = xs
            for at, (_, x, _) in zip(slots, picks):
                bx = _place(bx, xb, at, x)
            for entry, fn in (("points_from_x", _from_x_host), ("points_from_x_device", _from_x_device)):
                rc, idx, why, out = fn(pkg, c, bx, N, pb)
                assert (rc, idx, why) == (pkg.EPOINT, slots[0], picks[0][2]), "%s: classes %s at %s" % (entry, [p[0] for p in picks], slots)
                assert out == b"\x5a" * (pb * N)
        assert c.points_from_x(xs) == _valid(curve)[1]                        # the context stays usable


# ---- scalar multiplication ------------------------------------------------------------------------------------------------------------
def _mul_device(c, pts, sc, n, shared):
    import torch
    dp, ds = _dev(pts), _dev(sc)
    dout = torch.full((len(pts),), 0xAB, dtype=torch.uint8, device="cuda")
    _sync()
    c.mul_device(dp.data_ptr(), ds.data_ptr(), n, dout.data_ptr(), shared=shared)
    return bytes(dout.cpu().numpy())


@functools.lru_cache(maxsize=None)
def _te_cases():
    return te_edge_cases()


def _report(cases, got, want, pb, what):
    bad = [cases[i][0] for i in range(len(cases)) if got[pb * i:pb * i + pb] != want[pb * i:pb * i + pb]]
    assert not bad, "%s: %d of %d differ from the model: %s" % (what, len(bad), len(cases), "; ".join(bad[:8]))


def test_te_edge_scalars_times_edge_points_per_point(pkg):
    """every scalar of EDGE_TE and every digit pattern x subgroup points, O, T2, both T4, G + T2, G + T4, one scalar per point: the model's
    bytes from te_msm_mul and te_msm_mul_device; the first 255, 256 and 257 of them again (the last block full, and one lane past it)"""
    cases = _te_cases()
    assert len(cases) == (len(EDGE_TE) + len(digit_pattern_scalars())) * (4 + 1 + 5) and len(cases) > 257
    pts, sc, want = (b"".join(cs[1] for cs in cases), b"".join(cs[2].to_bytes(32, "little") for cs in cases), b"".join(cs[3] for cs in cases))
    with _ctx(pkg, 0) as c:
        _report(cases, c.mul(pts, sc), want, 64, "mul")
        _report(cases, _mul_device(c, pts, sc, len(cases), False), want, 64, "mul_device")
        for n in (255, 256, 257):
            _report(cases[:n], c.mul(pts[:64 * n], sc[:32 * n]), want[:64 * n], 64, "mul, n = %d" % n)


def test_te_edge_scalars_shared(pkg):
    """each edge and digit-pattern scalar as the shared scalar over the ten edge points (reduced mod 4 L on the host: the cofactor part counts)"""
    cases = _te_cases()
    per = 10
    with _ctx(pkg, 0) as c:
        for j in range(0, len(cases), per):
            row = cases[j:j + per]
            k = row[0][2]
            assert all(cs[2] == k for cs in row)
            pts, want = b"".join(cs[1] for cs in row), b"".join(cs[3] for cs in row)
            _report(row, c.mul(pts, k.to_bytes(32, "little")), want, 64, "mul, shared")
            if j % (3 * per) == 0:
                _report(row, _mul_device(c, pts, k.to_bytes(32, "little"), per, True), want, 64, "mul_device, shared")


def test_te_mul_x_on_the_accepted_edge_x_equals_from_x_then_mul(pkg):
    accepted = [cl for cl in te_x_classes() if not isinstance(cl[2], int)]
    xs, pts = b"".join(cl[1] for cl in accepted), b"".join(cl[2] for cl in accepted)
    ks = (EDGE_TE + digit_pattern_scalars()) * (len(accepted) // 29 + 1)
    sc = b"".join(k.to_bytes(32, "little") for k in ks[:len(accepted)])
    with _ctx(pkg, 0) as c:
        assert c.points_from_x(xs) == pts
        want = c.mul(pts, sc)
        got = c.mul_x(xs, sc)
        _report(accepted, got, want, 64, "mul_x against points_from_x then mul")
        model = b"".join(m.points_to_bytes([m.scalar_mul(k, m.xy_from_bytes(cl[2]))]) for k, cl in zip(ks, accepted))
        _report(accepted, got, model, 64, "mul_x")
        one = (m.L + 1).to_bytes(32, "little")
        assert c.mul_x(xs, one) == pts, "mul_x, shared scalar L + 1: the recovered points lie in the subgroup"


def test_te_one_and_four_devices_give_the_same_bytes(pkg):
    cases = _te_cases()
    pts, sc = b"".join(cs[1] for cs in cases), b"".join(cs[2].to_bytes(32, "little") for cs in cases)
    tors = b"".join(m.points_to_bytes([p]) for _, p in te_torsion_points())
    outs = []
    for ids in ((0,), (0, 0, 0, 0)):
        with _ctx(pkg, 0, ids) as c:
            outs.append((c.mul(pts, sc), c.mul(tors, (4 * m.L - 1).to_bytes(32, "little"))))
    assert outs[0] == outs[1]
    assert outs[0][0] == b"".join(cs[3] for cs in cases)


@functools.lru_cache(maxsize=None)
def _bls_cases():
    return bls_edge_cases()


def test_bls377_every_tail_shape_with_infinity_in_every_position(pkg):
    """n = 1, 7, 8, 9, 15, 16, 17, 19 with the edge scalars and with r or 0 placed so that infinity falls on the first, the last and a middle
    slot of an affine group, on a whole group and on the tail group: the model's bytes, the neighbours of every infinity included"""
    cases = _bls_cases()
    assert {len(cs[2]) for cs in cases} == {1, 7, 8, 9, 15, 16, 17, 19}
    with _ctx(pkg, 1) as c:
        for name, raw, ks, want in cases:
            sc = b"".join(k.to_bytes(48, "little") for k in ks)
            assert c.mul(raw, sc) == want, "mul: " + name
            if "middle" in name or "edge" in name:
                assert _mul_device(c, raw, sc, len(ks), False) == want, "mul_device: " + name


def test_bls377_shared_and_per_point_agree_on_the_edge_scalars(pkg):
    with _ctx(pkg, 1) as c:
        for n in (1, 8, 9, 19):
            raw = oracle377.gen_points(0x3E + n, n)
            pts = [b.xy_from_bytes(raw[96 * i:96 * i + 96]) for i in range(n)]
            for j, k in enumerate(EDGE_377):
                one = k.to_bytes(48, "little")
                got = c.mul(raw, one)
                assert got == c.mul(raw, one * n), "n = %d, edge scalar %d" % (n, j)
                if n == 9:
                    assert got == b"".join(b.result_to_bytes(b.scalar_mul(k, p)) for p in pts), "n = 9, edge scalar %d" % j
