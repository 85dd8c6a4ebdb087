"""Montgomery-form inputs on the GPU (include/te_msm.h: options "scalars_montgomery", read when a call starts, and "points_montgomery",
read at bind time).  Every result is compared bit for bit with oracle.msm / oracle377.msm over the CANONICAL points and the scalars decoded
in Python (k = a * 2^-256 mod m); nothing expected comes from the engine.  One-GPU box: contexts of two "devices" name GPU 0 twice.

Two places where a case is built otherwise than its one-line description suggests, with the reason:
  * the fixed-base fallback: a "bind_fixed_base" = 16 set has ONE regular row, sized for every entry of the MSM, so no scalar vector can
    overflow it -- that set is checked for running the fixed-base windows (fallbacks stay 0), and the all-equal vector takes its fallback
    on a second set with c = 19 (eight regular rows), where thirteen equal digits land in one of them.
  * "te_msm_run does not decode points": the group law is only associative on the curve, so no oracle has an answer for off-curve bytes.
    The test therefore passes bytes B that ARE points when read as canonical integers -- and that are, like any bytes, the Montgomery
    encoding of something else (B * 2^-256).  te_msm_run with the option set must equal the oracle over B as canonical integers."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import model as m
from oracle import oracle, oracle377
from test_point_checks_host import bls_bad_classes, te_bad_classes

pytestmark = pytest.mark.gpu

L_TE = 2111115437357092606062206234695386632838870926408408195193685246394721360383
R_377 = 8444461749428370424248824938781546531375899335154063827935233455917409239041
P = R_377
Q = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
MOD = {0: L_TE, 1: R_377}                     # scalar field of the curve in force
FIELD = {0: P, 1: Q}                          # base field
COORD = {0: 32, 1: 48}                        # bytes of one coordinate
SIZES = {0: (64, 32, 64), 1: (96, 48, 96)}    # point, scalar record, result bytes
ORA = {0: oracle, 1: oracle377}
RA = 1 << 256
EINVAL, ESCALAR, EPOINT = -1, -3, -5
SHAPES = (1, 2, 3, 1023, 1024, 1025, 4097, 1 << 14)
NP = 4097                                     # every scalar path


def _dev(buf):
    import torch
    t = torch.frombuffer(bytearray(buf) if len(buf) else bytearray(16), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def edge_values(mod):
    """the edge values of tests/test_scalar_form_host.py, the all-0xff record first"""
    single = [0xffffffff << (32 * j) for j in range(8)]
    all_but_one = [(RA - 1) ^ (0xffffffff << (32 * j)) for j in range(8)]
    return [RA - 1, mod, RA % mod, mod + 1, mod - 1, 1, 0] + single + all_but_one


def record(curve, a):
    return a.to_bytes(32, "little") + bytes(SIZES[curve][1] - 32)


@functools.lru_cache(maxsize=None)
def scalars(curve, n, seed=1):
    """(Montgomery-form records, the records of the decoded canonical k): as many edge values as fit, then seeded random k < m encoded,
    every fourth of them as an encoding >= m (a + j m below 2^256)"""
    mod = MOD[curve]
    rng = np.random.default_rng(1000 * seed + 10 * n + curve)
    vals = edge_values(mod)[:n]
    raw = rng.bytes(32 * max(0, n - len(vals)))
    for i in range(n - len(vals)):
        a = int.from_bytes(raw[32 * i:32 * i + 32], "little") % mod * RA % mod
        if i % 4 == 1:
            a += (1 + i % 7) * mod
            assert mod <= a < RA
        vals.append(a)
    rinv = pow(RA, -1, mod)
    return b"".join(record(curve, a) for a in vals), b"".join(record(curve, a * rinv % mod) for a in vals)


@functools.lru_cache(maxsize=None)
def points(curve, n=1 << 14):
    return ORA[curve].gen_points(4242 + curve, n)


def msm(curve, pts, sc):
    if curve == 1:
        return oracle377.msm(pts, sc, c=16 if len(sc) // 48 >= 1024 else 8, threads=16)
    return oracle.msm(pts, sc, threads=16)


@functools.lru_cache(maxsize=None)
def want_prefix(curve, n, seed=1):
    """the oracle over the first n canonical points and the decoded scalars of scalars(curve, n, seed)"""
    return msm(curve, points(curve)[:SIZES[curve][0] * n], scalars(curve, n, seed)[1])


def encode_points(curve, pts, plus=None):
    """every coordinate x -> x * R_a mod p (32 bytes) / mod q (48 bytes); plus: {coordinate index: multiples of the modulus added}"""
    cb, f = COORD[curve], FIELD[curve]
    ra = 1 << (8 * cb)
    out = bytearray()
    for i in range(len(pts) // cb):
        v = int.from_bytes(pts[cb * i:cb * i + cb], "little") * ra % f + (plus or {}).get(i, 0) * f
        out += v.to_bytes(cb, "little")
    return bytes(out)


def ctx_for(pkg, curve, ids=(0,), scalars_mont=1):
    c = pkg.MsmContext(ids)
    c.set_option("curve", curve)
    c.set_option("scalars_montgomery", scalars_mont)
    return c


def identity(curve):
    return bytes(32) + (1).to_bytes(32, "little") if curve == 0 else bytes(96)


# ---- the options themselves ------------------------------------------------------------------------------------------------------------
def test_options_default_to_zero_and_take_0_or_1(pkg):
    with pkg.MsmContext((0,)) as c:
        for key in ("scalars_montgomery", "points_montgomery"):
            assert c.get_option(key) == 0
            for v in (1, 0):
                c.set_option(key, v)
                assert c.get_option(key) == v
            for v in (-1, 2):
                with pytest.raises(pkg.MsmError) as e:
                    c.set_option(key, v)
                assert e.value.code == EINVAL


# ---- shapes: the two-scalars-per-thread step, the block boundary, both digit forms, a forced window size -----------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_shapes_digit_forms_and_window_bits(pkg, curve):
    pb = SIZES[curve][0]
    with ctx_for(pkg, curve) as c:
        for n in SHAPES:
            sc, _ = scalars(curve, n)
            assert sc[:32] == b"\xff" * 32, "the all-0xff record leads every vector"
            want = want_prefix(curve, n)
            for signed in (1, 0):
                c.set_option("signed_digits", signed)
                for wb in (0, 7):
                    c.set_option("window_bits", wb)
                    assert c.run(points(curve)[:pb * n], sc) == want, (n, signed, wb)
        # the same bytes read canonically: the all-0xff record trips the final carry under signed digits -- the option is what decodes it
        c.set_option("signed_digits", 1)
        c.set_option("window_bits", 0)
        c.set_option("scalars_montgomery", 0)
        with pytest.raises(pkg.MsmError) as e:
            c.run(points(curve)[:pb * 3], scalars(curve, 3)[0])
        assert e.value.code == ESCALAR
        c.set_option("scalars_montgomery", 1)
        assert c.run(points(curve)[:pb * 3], scalars(curve, 3)[0]) == want_prefix(curve, 3)


# ---- every scalar path at n = 4097 ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_every_scalar_path(pkg, curve):
    import torch
    pb, sb, _ = SIZES[curve]
    n = NP
    pts = points(curve)[:pb * n]
    sc, _ = scalars(curve, n)
    want = want_prefix(curve, n)
    dp, ds = _dev(pts), _dev(sc)
    with ctx_for(pkg, curve) as c:
        assert c.run(pts, sc) == want
        assert c.run_device(dp.data_ptr(), ds.data_ptr(), n) == want
        ts = [c.submit(pts, sc), c.submit_async(pts, sc), c.submit_device(dp.data_ptr(), ds.data_ptr(), n)]
        assert [c.collect(t) for t in ts] == [want] * 3
        b = c.bind_points(pts)
        for chunks in (1, 3):
            c.set_option("scalar_chunks", chunks)
            assert c.run_scalars(b, sc) == want, chunks
            assert c.run_scalars_device(b, ds.data_ptr()) == want, chunks
        c.set_option("scalar_chunks", 0)
        ts = [c.submit_scalars(b, sc), c.submit_scalars_device(b, ds.data_ptr())]
        assert [c.collect(t) for t in ts] == [want] * 2
        # batch over prefixes: one shared ragged sequence, then every MSM alone
        lens = (0, 1, 5, 4097, 300)
        bufs = [scalars(curve, L, seed=2 + i)[0] for i, L in enumerate(lens)]
        wants = [identity(curve) if L == 0 else want_prefix(curve, L, seed=2 + i) for i, L in enumerate(lens)]
        packed = _dev(b"".join(bufs))
        for small_max in (1 << 15, 0):
            c.set_option("batch_small_max", small_max)
            assert c.run_scalars_batch(b, bufs) == wants, small_max
            assert c.run_scalars_batch_device(b, packed.data_ptr(), lens) == wants, small_max
        c.set_option("batch_small_max", 1 << 15)
        # indexed subset: repeats, more entries than the set has points
        mi = n + 300
        idx = np.random.default_rng(5 + curve).integers(0, n, size=mi).astype("<u4")
        assert len(np.unique(idx)) < mi
        si, si_dec = scalars(curve, mi, seed=9)
        gathered = np.frombuffer(pts, dtype=np.uint8).reshape(-1, pb)[idx.astype(np.int64)].tobytes()
        want_idx = msm(curve, gathered, si_dec)
        di, dsi = _dev(idx.tobytes()), _dev(si)
        assert c.run_scalars_indexed(b, idx, si) == want_idx
        assert c.run_scalars_indexed_device(b, di.data_ptr(), dsi.data_ptr(), mi) == want_idx
        ts = [c.submit_scalars_indexed(b, idx, si), c.submit_scalars_indexed_device(b, di.data_ptr(), dsi.data_ptr(), mi)]
        assert [c.collect(t) for t in ts] == [want_idx] * 2
        c.release_points(b)
        # the window-sharded building block and its host tail
        cw, W = c.plan(n)
        part = torch.zeros(W * c.row_bytes, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        c.partial_device(dp.data_ptr(), ds.data_ptr(), n, part.data_ptr())
        c.partial_wait(0)
        assert c.finalize(part.cpu().numpy().tobytes(), cw, W) == want


@pytest.mark.parametrize("curve", [0, 1])
def test_two_devices_point_and_window_shards(pkg, curve):
    pb = SIZES[curve][0]
    n = NP
    pts = points(curve)[:pb * n]
    sc, _ = scalars(curve, n)
    want = want_prefix(curve, n)
    dp, ds = _dev(pts), _dev(sc)
    with ctx_for(pkg, curve, ids=(0, 0)) as c:
        c.set_option("host_shard_min", 1)
        assert c.run(pts, sc) == want                                         # point shards
        assert c.run_device(dp.data_ptr(), ds.data_ptr(), n) == want          # window shards
        b = c.bind_points(pts)
        assert c.run_scalars(b, sc) == want
        assert c.run_scalars_device(b, ds.data_ptr()) == want
        ts = [c.submit_scalars(b, sc), c.submit_async(pts, sc), c.submit_scalars_device(b, ds.data_ptr())]
        assert [c.collect(t) for t in reversed(ts)] == [want] * 3
        c.release_points(b)


def test_fixed_base_sets_and_their_fallback(pkg):
    n = NP
    pts = points(0)[:64 * n]
    sc, _ = scalars(0, n)
    want = want_prefix(0, n)
    ds = _dev(sc)
    # thirteen equal 19-bit digits 0x2345: every entry of every window but the top one lands in regular row 0 of a c = 19 table
    k = sum(0x2345 << (19 * w) for w in range(13))
    assert k < L_TE
    same = record(0, k * RA % L_TE) * n
    want_same = oracle.msm(pts, record(0, k) * n, threads=16)
    with ctx_for(pkg, 0) as c:
        c.set_option("bind_fixed_base", 16)
        fb16 = c.bind_points(pts)
        c.set_option("bind_fixed_base", 19)
        fb19 = c.bind_points(pts)
        c.set_option("bind_fixed_base", 0)
        assert c.run_scalars(fb16, sc) == want and c.run_scalars_device(fb16, ds.data_ptr()) == want
        ts = [c.submit_scalars(fb16, sc), c.submit_scalars_device(fb16, ds.data_ptr())]
        assert [c.collect(t) for t in ts] == [want] * 2
        assert c.run_scalars(fb19, sc) == want
        assert c.get_option("fixed_base_fallbacks") == 0, "the fixed-base windows did not run"
        assert c.run_scalars(fb16, same) == want_same
        assert c.get_option("fixed_base_fallbacks") == 0                      # (one regular row: nothing to overflow)
        assert c.run_scalars(fb19, same) == want_same
        assert c.get_option("fixed_base_fallbacks") == 1
        # the fallback of a TICKET runs at its collect: with the form the ticket was submitted with, whatever the option says by then
        t = c.submit_scalars(fb19, same)
        c.set_option("scalars_montgomery", 0)
        assert c.collect(t) == want_same
        assert c.get_option("fixed_base_fallbacks") == 2
        c.release_points(fb16)
        c.release_points(fb19)


# ---- tickets carry the form they were submitted with -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_tickets_keep_their_form(pkg, curve):
    pb = SIZES[curve][0]
    n = NP
    pts = points(curve)[:pb * n]
    enc, dec = scalars(curve, n)
    plain = ORA[curve].gen_scalars(77, n)
    want_mont, want_plain = want_prefix(curve, n), msm(curve, pts, plain)
    assert msm(curve, pts, dec) == want_mont
    dp, de, dpl = _dev(pts), _dev(enc), _dev(plain)
    with ctx_for(pkg, curve) as c:
        b = c.bind_points(pts)
        forms = [lambda s, d: c.submit(pts, s), lambda s, d: c.submit_async(pts, s), lambda s, d: c.submit_device(dp.data_ptr(), d.data_ptr(), n),
                 lambda s, d: c.submit_scalars(b, s), lambda s, d: c.submit_scalars_device(b, d.data_ptr())]
        for f in forms:
            c.set_option("scalars_montgomery", 1)
            t_on = f(enc, de)
            c.set_option("scalars_montgomery", 0)
            t_off = f(plain, dpl)
            c.set_option("scalars_montgomery", 1)                              # flipped again before either is collected
            assert c.collect(t_off) == want_plain and c.collect(t_on) == want_mont
        c.release_points(b)


# ---- BLS12-377 records: bytes 32..47 must be zero ---------------------------------------------------------------------------------------------
def test_curve1_record_with_a_high_byte_is_escalar(pkg):
    n = 300
    pts = points(1)[:96 * n]
    sc = bytearray(scalars(1, n)[0])
    with ctx_for(pkg, 1) as c:
        for signed in (1, 0):
            c.set_option("signed_digits", signed)
            assert c.run(pts, bytes(sc)) == want_prefix(1, n)
            bad = bytearray(sc)
            bad[48 * 200 + 40] = 1
            out = ctypes.create_string_buffer(b"\xab" * 96, 96)
            assert c._L.te_msm_run(c._h, pts, bytes(bad), n, out) == ESCALAR
            assert out.raw == b"\xab" * 96, "output touched"
        assert c.run(pts, bytes(sc)) == want_prefix(1, n)


# ---- calls that are not MSM-scalar paths refuse the option -----------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_mul_and_run_x_are_refused_with_the_output_untouched(pkg, curve):
    pb, sb, _ = SIZES[curve]
    n = 50
    pts = points(curve)[:pb * n]
    sc = scalars(curve, n)[0]
    xb = pkg.X_BYTES_BLS12_377 if curve else pkg.X_BYTES
    xs = b"".join(pts[pb * i:pb * i + COORD[curve]] for i in range(n))
    assert len(xs) == xb * n
    dp, ds = _dev(pts), _dev(sc)
    import torch
    dout = torch.full((pb * n,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with ctx_for(pkg, curve) as c:
        for fn, args in ((c._L.te_msm_mul, (pts, sc, n, 0)), (c._L.te_msm_mul_x, (xs, sc, n, 0)), (c._L.te_msm_mul, (pts, sc[:sb], n, 1))):
            out = ctypes.create_string_buffer(b"\xab" * (pb * n), pb * n)
            assert fn(c._h, *args, out) == EINVAL
            assert out.raw == b"\xab" * (pb * n)
            assert b"scalars_montgomery" in c._L.te_msm_last_error(c._h)
        out = ctypes.create_string_buffer(b"\xab" * 96, 96)
        assert c._L.te_msm_run_x(c._h, xs, sc, n, out) == EINVAL and out.raw == b"\xab" * 96
        assert c._L.te_msm_mul_device(c._h, dp.data_ptr(), ds.data_ptr(), n, 0, dout.data_ptr()) == EINVAL
        torch.cuda.synchronize()
        assert bool((dout == 0xAB).all())
        # the context stays usable, and the calls work again without the option
        assert c.run(pts, sc) == want_prefix(curve, n)
        c.set_option("scalars_montgomery", 0)
        dec = scalars(curve, n)[1]
        got = c.mul(pts, dec)
        assert got[:pb] == ORA[curve].scalar_mul(pts[:pb], int.from_bytes(dec[:32], "little"))


# ---- points bound from Montgomery coordinates ---------------------------------------------------------------------------------------------------
def record_residues(curve, raw, rec_bytes, count):
    """the coordinates of `count` bound records as residues mod p / q (29-bit limbs in u32 words)"""
    nl, f = (9, P) if curve == 0 else (14, Q)
    coords = 3 if rec_bytes in (128, 168) else 4
    w = np.frombuffer(raw, dtype="<u4").reshape(count, rec_bytes // 4)
    return [[sum(int(w[i, nl * k + j]) << (29 * j) for j in range(nl)) % f for k in range(coords)] for i in range(count)]


@pytest.mark.parametrize("curve,affine", [(0, 1), (1, 1), (1, 0)])
def test_sets_bound_from_montgomery_coordinates(pkg, curve, affine):
    pb, sb, _ = SIZES[curve]
    with ctx_for(pkg, curve, scalars_mont=0) as c:
        c.set_option("bind_affine", affine)
        for n in (1, 255, 4097):
            pts = points(curve)[:pb * n]
            # every fifth coordinate as a non-canonical encoding (+ p, + 2 p ...: below 2^256 / 2^384 for any residue)
            menc = encode_points(curve, pts, plus={i: 1 + i % 3 for i in range(0, 2 * n, 5)})
            sc = ORA[curve].gen_scalars(31 + n, n)
            want = msm(curve, pts, sc)
            b0 = c.bind_points(pts)
            b1 = c.bind_points(menc, montgomery=True)
            assert c.get_option("points_montgomery") == 0, "the keyword lasts for the call"
            c.set_option("points_montgomery", 1)
            dm = _dev(menc)
            b2 = c.bind_points_device(dm.data_ptr(), n)
            c.set_option("points_montgomery", 0)
            lens = [n, 1, max(1, n // 3)]
            idx = np.random.default_rng(n).integers(0, n, size=n + 7).astype("<u4")
            si = ORA[curve].gen_scalars(32 + n, n + 7)
            ref = (c.run_scalars(b0, sc), c.run_scalars_batch(b0, [sc[:sb * L] for L in lens]), c.run_scalars_indexed(b0, idx, si))
            assert ref[0] == want
            for b in (b1, b2):
                got = (c.run_scalars(b, sc), c.run_scalars_batch(b, [sc[:sb * L] for L in lens]), c.run_scalars_indexed(b, idx, si))
                assert got == ref, n
            cnt = min(n, 255)
            rb0, raw0 = c.bases_read(b0, 0, cnt)
            rb1, raw1 = c.bases_read(b1, 0, cnt)
            assert rb0 == rb1 == (128 if curve == 0 else 168 if affine else 224)
            assert record_residues(curve, raw1, rb1, cnt) == record_residues(curve, raw0, rb0, cnt), n
            for b in (b0, b1, b2):
                c.release_points(b)


def test_fixed_base_table_from_montgomery_coordinates(pkg):
    n = 1000
    pts = points(0)[:64 * n]
    sc = oracle.gen_scalars(41, n)
    with ctx_for(pkg, 0, scalars_mont=0) as c:
        c.set_option("bind_fixed_base", 16)
        b = c.bind_points(encode_points(0, pts), montgomery=True)
        assert c.run_scalars(b, sc) == oracle.msm(pts, sc, threads=16)
        assert c.get_option("fixed_base_fallbacks") == 0
        c.release_points(b)


def with_point(pts, pb, at, pt):
    a = bytearray(pts)
    a[pb * at:pb * at + pb] = pt
    return bytes(a)


@pytest.mark.parametrize("curve", [0, 1])
def test_checks_decode_montgomery_coordinates(pkg, curve):
    pb = SIZES[curve][0]
    cb, f = COORD[curve], FIELD[curve]
    n = 300
    pts = points(curve)[:pb * n]
    good = encode_points(curve, pts)
    classes = {name: pt for name, pt, _ in (te_bad_classes() if curve == 0 else bls_bad_classes())}
    off = encode_points(curve, classes["y+1"])                                 # an encoded point off the curve
    x_a = int.from_bytes(good[pb * 5:pb * 5 + cb], "little")
    high = (x_a + f).to_bytes(cb, "little") + good[pb * 5 + cb:pb * 6]          # a good point whose stored x is >= p: non-canonical
    if curve == 0:
        p0 = m.xy_from_bytes(pts[:64])
        i4 = next(pt for name, pt, _ in te_bad_classes() if name == "order4")
        coset = m.add(p0, m.xy_from_bytes(i4))                                 # P + T4: on the curve, in an order-4 coset
        assert m.on_curve(coset) and m.scalar_mul(m.L, coset) != m.ZERO
        outside = encode_points(0, coset[0].to_bytes(32, "little") + coset[1].to_bytes(32, "little"))
    else:
        outside = encode_points(1, classes["P+T2"])
    cases = [(with_point(with_point(good, pb, 200, off), pb, 7, off), {1: (7, 2), 2: (7, 2)}),
             (with_point(with_point(good, pb, 5, high), pb, 9, off), {1: (5, 1), 2: (5, 1)}),
             (with_point(good, pb, 299, high), {1: (299, 1), 2: (299, 1)}),
             (with_point(with_point(good, pb, 100, outside), pb, 250, off), {1: (250, 2), 2: (100, 3)}),
             (with_point(good, pb, 0, outside), {1: None, 2: (0, 3)})]
    with ctx_for(pkg, curve, scalars_mont=0) as c:
        c.set_option("points_montgomery", 1)
        dgood = _dev(good)
        for level in (1, 2):
            assert c.check_points(good, level) is None
            assert c.check_points_device(dgood.data_ptr(), n, level) is None
            c.set_option("check_points", level)
            b = c.bind_points(good)
            sc = ORA[curve].gen_scalars(3, n)
            assert c.run_scalars(b, sc) == msm(curve, pts, sc)
            c.release_points(b)
            bound = c.get_option("bases_bound")
            for bad, verdicts in cases:
                v = verdicts[level]
                dbad = _dev(bad)
                assert c.check_points(bad, level) == v
                assert c.check_points_device(dbad.data_ptr(), n, level) == v
                if v is None:
                    c.release_points(c.bind_points(bad))
                    continue
                for bind in (lambda: c.bind_points(bad), lambda: c.bind_points_device(dbad.data_ptr(), n)):
                    with pytest.raises(pkg.MsmError) as e:
                        bind()
                    assert (e.value.code, e.value.index, e.value.reason) == (EPOINT, v[0], v[1])
                assert c.get_option("bases_bound") == bound
        # the canonical reading of the same bytes is another matter: without the option the encoded set is off the curve
        c.set_option("points_montgomery", 0)
        assert c.check_points(good, 1) is not None


@pytest.mark.parametrize("curve", [0, 1])
def test_per_call_points_are_never_decoded(pkg, curve):
    """bind time only: te_msm_run* / te_msm_submit* with "points_montgomery" = 1 read their points as canonical integers (see the top)"""
    pb = SIZES[curve][0]
    n = 1025
    pts = points(curve)[:pb * n]
    sc = ORA[curve].gen_scalars(8, n)
    want = msm(curve, pts, sc)
    dp, ds = _dev(pts), _dev(sc)
    with ctx_for(pkg, curve, scalars_mont=0) as c:
        c.set_option("points_montgomery", 1)
        assert c.run(pts, sc) == want
        assert c.run_device(dp.data_ptr(), ds.data_ptr(), n) == want
        ts = [c.submit(pts, sc), c.submit_async(pts, sc), c.submit_device(dp.data_ptr(), ds.data_ptr(), n)]
        assert [c.collect(t) for t in ts] == [want] * 3
        c.set_option("check_points", 1)                                        # the per-call check reads canonical coordinates too
        assert c.run(pts, sc) == want
        if curve == 0:                                                         # te_msm_bind_points_x keeps its own x-only format
            bx = c.bind_points_x(b"".join(pts[64 * i:64 * i + 32] for i in range(8)))
            assert c.run_scalars(bx, sc[:32 * 8]) == msm(0, pts[:64 * 8], sc[:32 * 8])
            c.release_points(bx)


# ---- Node: setScalarsMontgomery(flag), setBases(buffer, {montgomery: true}) -----------------------------------------------------------------
def test_node_montgomery_switches(pkg, tmp_path):
    """the addon's two switches against the same oracle values: a Montgomery set with canonical and with Montgomery scalars, the set bound
    again after setScalarsMontgomery dropped the context, setBases(null) forgetting the form, and an option that is no boolean"""
    import json
    import os
    import shutil
    import subprocess
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not installed on this box")
    js = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists("/usr/include/node/node_api.h") and not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        pytest.skip("no N-API addon and no node headers to build it")
    subprocess.check_call(["make", "-C", js, "-s"])
    n = 1025
    pts = points(0)[:64 * n]
    smont, scanon = scalars(0, n)
    for name, data in (("p.bin", pts), ("pm.bin", encode_points(0, pts, plus={3: 1, 10: 2})), ("s.bin", scanon), ("sm.bin", smont)):
        (tmp_path / name).write_bytes(data)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
(async () => {
  const [pts, pm, sc, sm] = [2, 3, 4, 5].map((i) => fs.readFileSync(process.argv[i]));
  const xy = (r) => [r.x.toString(), r.y.toString()];
  const out = {};
  m.setBases(pm, { montgomery: true });
  out.montSetCanonScalars = xy(await m.compute_msm(pm, sc));
  m.setScalarsMontgomery(true);                       // drops the context: the set is bound again, still as Montgomery residues
  out.montSetMontScalars = xy(await m.compute_msm(pm, sm));
  out.perCallPoints = xy(await m.compute_msm(pts, sm));   // another buffer: the ordinary path, canonical points, Montgomery scalars
  out.batch = (await m.msmBatch([sm])).map(xy);
  try { m.scalarMul(pts.subarray(0, 64), sc.subarray(0, 32)); out.mul = 'returned'; } catch (e) { out.mul = String(e.message); }
  m.setScalarsMontgomery(false);
  m.setBases(null);
  m.setBases(pts);                                    // the form left with the set it belonged to
  out.canonSetAfterUnbind = xy(await m.compute_msm(pts, sc));
  try { m.setBases(pts, 7); out.badOptions = 'returned'; } catch (e) { out.badOptions = String(e.message); }
  m.setBases(null);
  console.log(JSON.stringify(out));
})();
"""
    files = [str(tmp_path / f) for f in ("p.bin", "pm.bin", "s.bin", "sm.bin")]
    r = subprocess.run([node, "-e", script, js] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    w = want_prefix(0, n)
    want = [str(int.from_bytes(w[:32], "little")), str(int.from_bytes(w[32:], "little"))]
    for key in ("montSetCanonScalars", "montSetMontScalars", "perCallPoints", "canonSetAfterUnbind"):
        assert out[key] == want, key
    assert out["batch"] == [want]
    assert "te_msm error -1" in out["mul"] and "scalars_montgomery" in out["mul"], out["mul"]
    assert "setBases(" in out["badOptions"], out["badOptions"]
