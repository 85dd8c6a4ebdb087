"""MSMs over narrow scalars on the GPU (include/te_msm.h: options "scalar_bits" and "scalar_record_bytes" = 8 / 16, both read when a call
starts).  Every result is compared bit for bit with oracle.msm / oracle377.msm over the ZERO-EXTENDED scalars in the curve's own records,
and with the engine's own result over those records with both options at 0.  The digit rows are compared with a Python-integer
decomposition: stored digit w of s is window w of s + sum_{w<W} 2^(cw + c - 1) (signed digits) or of s itself (unsigned).
One-GPU box: the context of four "devices" names GPU 0 four times."""
import ctypes
import functools

import numpy as np
import pytest

from layout_cases import xs_of_377
from oracle import oracle, oracle377

pytestmark = pytest.mark.gpu

SIZES = {0: (64, 32, 64), 1: (96, 48, 96)}    # point, the curve's own scalar record, result bytes
ORA = {0: oracle, 1: oracle377}
EINVAL, ESCALAR = -1, -3
NS = (1, 2, 299, 300, 1023, 1024, 1025, 2049)
WIDE_BITS = (1, 8, 63, 64, 65, 127, 128, 200)
WINDOW_BITS = (0, 4, 13, 16)
NP = 300                                      # every entry point


def _dev(buf):
    import torch
    t = torch.frombuffer(bytearray(buf) if len(buf) else bytearray(16), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


@functools.lru_cache(maxsize=None)
def points(curve, n=2049):
    return ORA[curve].gen_points(777 + curve, n)


def records(vals, size):
    return b"".join(v.to_bytes(size, "little") for v in vals)


def msm(curve, pts, vals):
    """the oracle over the zero-extended scalars"""
    n = len(vals)
    sc = records(vals, SIZES[curve][1])
    if curve == 1:
        return oracle377.msm(pts[:96 * n], sc, c=16 if n >= 1024 else 8, threads=8)
    return oracle.msm(pts[:64 * n], sc, threads=8)


@functools.lru_cache(maxsize=None)
def vectors(n, b):
    """the scalar classes below 2^b: all 0, all 1, all 2^b - 1 (all equal), and random values with 0, 1 and 2^b - 1 among them -- the
    largest value at the first, a middle and the last position"""
    top = (1 << b) - 1
    rng = np.random.default_rng(100 * n + b)
    raw = rng.bytes(32 * n)
    mixed = [int.from_bytes(raw[32 * i:32 * i + 32], "little") & top for i in range(n)]
    for at, v in ((3, 0), (4, 1), (n // 2, top), (0, top), (n - 1, top)):
        if at < n:
            mixed[at] = v
    return {"zero": (0,) * n, "one": (1,) * n, "top": (top,) * n, "mixed": tuple(mixed)}


@functools.lru_cache(maxsize=None)
def want(curve, n, b, name):
    return msm(curve, points(curve), vectors(n, b)[name])


def ctx_for(pkg, curve, ids=(0,)):
    c = pkg.MsmContext(ids)
    c.set_option("curve", curve)
    c.set_option("prezero", 0)
    return c


def rule(c0, signed, b):
    """the narrow plan: W = ceil((b + g) / c0) windows of the size the plan has anyway"""
    return c0, -(-(b + (2 if signed else 0)) // c0)


def limit(c, W, signed):
    return (1 << (c * W)) - (sum(1 << (c * w + c - 1) for w in range(W)) if signed else 0)


def digit_rows(vals, c, W, signed):
    half = sum(1 << (c * w + c - 1) for w in range(W)) if signed else 0
    zero = (1 << (c - 1)) if signed else 0
    n, nst = len(vals), (len(vals) + 7) & ~7
    rows = np.full((W, nst), zero, dtype=np.uint16)
    # s + half in Python integers; its windows cut out of the bits (c W <= 256 + 16)
    raw = np.frombuffer(b"".join((s + half).to_bytes(40, "little") for s in vals), dtype=np.uint8).reshape(n, 40)
    bits = np.unpackbits(raw, axis=1, bitorder="little")
    weights = (1 << np.arange(c)).astype(np.uint32)
    for w in range(W):
        rows[w, :n] = (bits[:, c * w:c * w + c].astype(np.uint32) @ weights).astype(np.uint16)
    assert all((s + half) >> (c * W) == 0 for s in vals), "a scalar the plan refuses"
    return rows


def x_only(curve, pts):
    """the x-only encoding of the points: 32-byte x on the Twisted-Edwards curve; BLS12-377: 48 bytes with the larger-root flag (layout_cases)"""
    if curve == 1:
        return xs_of_377(pts)
    return b"".join(pts[64 * i:64 * i + 32] for i in range(len(pts) // 64))


def forms(curve, b_wide=WIDE_BITS):
    """(record bytes option, "scalar_bits" option, record size of the buffers, the width b): the two narrow records, then the curve's own with a declared width"""
    own = SIZES[curve][1]
    return [(8, 0, 8, 64), (16, 128, 16, 128)] + [(0, b, own, b) for b in b_wide]         # (16-byte records need their width declared)


def set_form(c, rec_opt, bits_opt):
    """the width first: "scalar_record_bytes" = 16 is accepted only while "scalar_bits" is set"""
    c.set_option("scalar_record_bytes", 0)
    c.set_option("scalar_bits", bits_opt)
    c.set_option("scalar_record_bytes", rec_opt)


def test_options_default_to_zero_and_their_ranges(pkg):
    with pkg.MsmContext((0,)) as c:
        assert c.get_option("scalar_bits") == 0 and c.get_option("scalar_record_bytes") == 0
        for v in (1, 64, 256, 0):
            c.set_option("scalar_bits", v)
            assert c.get_option("scalar_bits") == v
        for v in (8, 32, 0):
            c.set_option("scalar_record_bytes", v)
            assert c.get_option("scalar_record_bytes") == v
        # 16 without a declared width stays the refused value it always was; with one it is a record size
        with pytest.raises(pkg.MsmError) as e:
            c.set_option("scalar_record_bytes", 16)
        assert e.value.code == EINVAL and c.get_option("scalar_record_bytes") == 0
        for bits in (1, 128, 200):
            c.set_option("scalar_bits", bits)
            c.set_option("scalar_record_bytes", 16)
            assert c.get_option("scalar_record_bytes") == 16 and c._sizes[1] == 16
            c.set_option("scalar_record_bytes", 0)
        c.set_option("scalar_bits", 0)
        for key, v in (("scalar_bits", -1), ("scalar_bits", 257), ("scalar_record_bytes", 4), ("scalar_record_bytes", 24)):
            with pytest.raises(pkg.MsmError) as e:
                c.set_option(key, v)
            assert e.value.code == EINVAL


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("curve", [0, 1])
def test_results_digits_and_plan(pkg, curve, n):
    pb, own, _ = SIZES[curve]
    pts = points(curve)[:pb * n]
    with ctx_for(pkg, curve) as c:
        for rec_opt, bits_opt, size, b in forms(curve):
            # the engine's own result over the zero-extended records, both options at 0 (default digits and windows)
            set_form(c, 0, 0)
            c.set_option("signed_digits", 1)
            c.set_option("window_bits", 0)
            c0_auto = c.plan(n)[0]
            for name, vals in vectors(n, b).items():
                w = want(curve, n, b, name)
                assert c.run(pts, records(vals, own)) == w, (size, b, name, "zero-extended, options at 0")
            for signed in (1, 0):
                for wb in WINDOW_BITS:
                    set_form(c, rec_opt, bits_opt)
                    c.set_option("signed_digits", signed)
                    c.set_option("window_bits", wb)
                    cw, W = c.plan(n)
                    assert (cw, W) == rule(wb or c0_auto, signed, b), (size, b, signed, wb)
                    for name, vals in vectors(n, b).items():
                        key = (size, b, signed, wb, name)
                        assert c.run(pts, records(vals, size)) == want(curve, n, b, name), key
                        nst = (n + 7) & ~7
                        raw = c.debug_read("digits", 2 * nst * (W + 2))
                        assert len(raw) == 2 * nst * W, key + ("exactly W digit rows",)
                        got = np.frombuffer(raw, dtype="<u2").reshape(W, nst)
                        assert np.array_equal(got, digit_rows(vals, cw, W, signed)), key


@pytest.mark.parametrize("curve", [0, 1])
def test_the_exact_limit_of_the_plan_that_ran(pkg, curve):
    """wide records: limit - 1 is accepted and exact, limit is TE_MSM_ESCALAR with the output untouched, a scalar between 2^b and the
    limit is exact -- for the (c, W) that te_msm_plan reports"""
    pb, own, rb = SIZES[curve]
    n = NP
    pts = points(curve)[:pb * n]
    base = list(vectors(n, 1)["mixed"])
    with ctx_for(pkg, curve) as c:
        for b in WIDE_BITS:
            for signed in (1, 0):
                for wb in WINDOW_BITS:
                    set_form(c, 0, b)
                    c.set_option("signed_digits", signed)
                    c.set_option("window_bits", wb)
                    cw, W = c.plan(n)
                    lim = limit(cw, W, signed)
                    assert (1 << b) <= lim < (1 << 256)
                    between = {lim - 1, (1 << b), ((1 << b) + lim) // 2} - {lim}
                    for at, v in zip((n - 1, 0, n // 2), sorted(between, reverse=True)):
                        vals = list(base)
                        vals[at] = v
                        assert c.run(pts, records(vals, own)) == msm(curve, pts, vals), (b, signed, wb, at, "accepted and exact")
                    for at in (0, n - 1):
                        vals = list(base)
                        vals[at] = lim
                        out = ctypes.create_string_buffer(b"\xab" * 96, 96)
                        assert c._L.te_msm_run(c._h, pts, records(vals, own), n, out) == ESCALAR, (b, signed, wb, at)
                        assert out.raw == b"\xab" * 96, "output touched"


@pytest.mark.parametrize("curve", [0, 1])
def test_narrow_records_refuse_what_does_not_fit(pkg, curve):
    """8-byte records with a smaller declared width: a scalar at or above the limit of the narrow plan is TE_MSM_ESCALAR"""
    pb = SIZES[curve][0]
    n = NP
    pts = points(curve)[:pb * n]
    with ctx_for(pkg, curve) as c:
        set_form(c, 8, 20)
        cw, W = c.plan(n)
        lim = limit(cw, W, 1)
        vals = list(vectors(n, 20)["mixed"])
        assert c.run(pts, records(vals, 8)) == want(curve, n, 20, "mixed")
        vals[n - 1] = lim - 1
        assert c.run(pts, records(vals, 8)) == msm(curve, pts, vals)
        for v in (lim, 1 << 40, (1 << 64) - 1):
            vals[n - 1] = v
            out = ctypes.create_string_buffer(b"\xab" * 96, 96)
            assert c._L.te_msm_run(c._h, pts, records(vals, 8), n, out) == ESCALAR, hex(v)
            assert out.raw == b"\xab" * 96


@pytest.mark.parametrize("curve", [0, 1])
def test_every_entry_point(pkg, curve):
    import torch
    pb, own, rb = SIZES[curve]
    n = NP
    pts = points(curve)[:pb * n]
    dp = _dev(pts)
    ident = bytes(32) + (1).to_bytes(32, "little") if curve == 0 else bytes(96)
    with ctx_for(pkg, curve) as c:
        b_set = c.bind_points(pts)
        for rec_opt, bits_opt, size, b in forms(curve, b_wide=(64,)):
            set_form(c, rec_opt, bits_opt)
            vals = vectors(n, b)["mixed"]
            sc = records(vals, size)
            w = want(curve, n, b, "mixed")
            ds = _dev(sc)
            key = (size, b)
            assert c.run(pts, sc) == w, key
            assert c.run_device(dp.data_ptr(), ds.data_ptr(), n) == w, key
            ts = [c.submit(pts, sc), c.submit_async(pts, sc), c.submit_device(dp.data_ptr(), ds.data_ptr(), n)]
            assert [c.collect(t) for t in ts] == [w] * 3, key
            for chunks in (1, 3):
                c.set_option("scalar_chunks", chunks)
                assert c.run_scalars(b_set, sc) == w, key
            c.set_option("scalar_chunks", 0)
            assert c.run_scalars_device(b_set, ds.data_ptr()) == w, key
            ts = [c.submit_scalars(b_set, sc), c.submit_scalars_device(b_set, ds.data_ptr())]
            assert [c.collect(t) for t in ts] == [w] * 2, key
            # batch over prefixes: 8-byte slices at odd and even record offsets, a length 0 among them
            lens = (3, 0, 5, 300, 1, 2, 299)
            assert [sum(lens[:m]) % 2 for m in range(len(lens))].count(1) >= 3
            bvals = [vectors(L, b)["mixed"] if L else () for L in lens]
            wants = [ident if not L else want(curve, L, b, "mixed") for L in lens]
            bufs = [records(v, size) for v in bvals]
            packed = _dev(b"".join(bufs))
            for small_max in (1 << 15, 0):
                c.set_option("batch_small_max", small_max)
                assert c.run_scalars_batch(b_set, bufs) == wants, key
                assert c.run_scalars_batch_device(b_set, packed.data_ptr(), lens) == wants, key
            c.set_option("batch_small_max", 1 << 15)
            # indexed subset: repeats, more entries than the set has points
            mi = n + 41
            idx = np.random.default_rng(5 + curve).integers(0, n, size=mi).astype("<u4")
            ivals = vectors(mi, b)["mixed"]
            gathered = np.frombuffer(pts, dtype=np.uint8).reshape(-1, pb)[idx.astype(np.int64)].tobytes()
            want_idx = msm(curve, gathered, ivals)
            si = records(ivals, size)
            di, dsi = _dev(idx.tobytes()), _dev(si)
            assert c.run_scalars_indexed(b_set, idx, si) == want_idx, key
            assert c.run_scalars_indexed_device(b_set, di.data_ptr(), dsi.data_ptr(), mi) == want_idx, key
            ts = [c.submit_scalars_indexed(b_set, idx, si), c.submit_scalars_indexed_device(b_set, di.data_ptr(), dsi.data_ptr(), mi)]
            assert [c.collect(t) for t in ts] == [want_idx] * 2, key
            # x-only points
            assert c.run_x(x_only(curve, pts), sc) == w, key
            # the building block and its host tail, with the narrow c and W
            cw, W = c.plan(n)
            assert (cw, W) == rule(9, 1, b), "n = 300: 9-bit windows, as without a declared width"
            part = torch.zeros(W * c.row_bytes, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c.partial_device(dp.data_ptr(), ds.data_ptr(), n, part.data_ptr())
            c.partial_wait(0)
            assert c.finalize(part.cpu().numpy().tobytes(), cw, W) == w, key
        c.release_points(b_set)


@pytest.mark.parametrize("ids", [(0,), (0, 0, 0, 0)])
def test_a_fixed_base_set_serves_narrow_calls_from_table_0(pkg, ids):
    """... on one device and on four (window shards where the plan has at least four windows, else whole on the holder; host scalars in slices)"""
    n = NP
    pts = points(0)[:64 * n]
    with ctx_for(pkg, 0, ids=ids) as c:
        c.set_option("host_shard_min", 1)
        c.set_option("bind_fixed_base", 16)
        fb = c.bind_points(pts)
        c.set_option("bind_fixed_base", 0)
        for rec_opt, bits_opt, size, b in forms(0, b_wide=(64,)) + [(8, 6, 8, 6)]:
            set_form(c, rec_opt, bits_opt)
            sc = records(vectors(n, b)["mixed"], size)
            w = want(0, n, b, "mixed")
            ds = _dev(sc)
            assert c.run_scalars(fb, sc) == w and c.run_scalars_device(fb, ds.data_ptr()) == w
            ts = [c.submit_scalars(fb, sc), c.submit_scalars_device(fb, ds.data_ptr())]
            assert [c.collect(t) for t in ts] == [w] * 2
            assert c.get_option("fixed_base_fallbacks") == 0
        c.release_points(fb)


@pytest.mark.parametrize("curve", [0, 1])
def test_four_devices_and_one_window(pkg, curve):
    """fewer windows than devices: the lone device-resident call runs whole on the device that holds the inputs"""
    pb, own, _ = SIZES[curve]
    n = NP
    pts = points(curve)[:pb * n]
    dp = _dev(pts)
    with ctx_for(pkg, curve, ids=(0, 0, 0, 0)) as c:
        c.set_option("host_shard_min", 1)
        b_set = c.bind_points(pts)
        for rec_opt, bits_opt, size, b in ((8, 6, 8, 6), (0, 6, own, 6), (8, 0, 8, 64)):
            set_form(c, rec_opt, bits_opt)
            W = c.plan(n)[1]
            assert W == (1 if b == 6 else rule(9, 1, 64)[1])
            sc = records(vectors(n, b)["mixed"], size)
            w = want(curve, n, b, "mixed")
            ds = _dev(sc)
            assert c.run_device(dp.data_ptr(), ds.data_ptr(), n) == w, (size, b)
            assert c.run(pts, sc) == w, (size, b)
            assert c.run_scalars_device(b_set, ds.data_ptr()) == w, (size, b)
            assert c.run_scalars(b_set, sc) == w, (size, b)
        c.release_points(b_set)


@pytest.mark.parametrize("curve", [0, 1])
def test_montgomery_scalars_with_a_declared_width(pkg, curve):
    """"scalars_montgomery" = 1 with "scalar_bits" = 64 over 32-byte records: the width applies to the decoded k"""
    mod = {0: 2111115437357092606062206234695386632838870926408408195193685246394721360383,
           1: 8444461749428370424248824938781546531375899335154063827935233455917409239041}[curve]
    pb, own, _ = SIZES[curve]
    n = NP
    pts = points(curve)[:pb * n]
    vals = vectors(n, 64)["mixed"]
    enc = b"".join(((k << 256) % mod).to_bytes(32, "little") + bytes(own - 32) for k in vals)
    with ctx_for(pkg, curve) as c:
        c.set_option("scalars_montgomery", 1)
        c.set_option("scalar_bits", 64)
        assert c.plan(n) == rule(9, 1, 64)
        assert c.run(pts, enc) == want(curve, n, 64, "mixed")
        # a decoded k of 65 bits does not fit the 64-bit plan of this n when it reaches the limit
        cw, W = c.plan(n)
        big = list(vals)
        big[7] = limit(cw, W, 1)
        bad = b"".join(((k << 256) % mod).to_bytes(32, "little") + bytes(own - 32) for k in big)
        out = ctypes.create_string_buffer(b"\xab" * 96, 96)
        assert c._L.te_msm_run(c._h, pts, bad, n, out) == ESCALAR and out.raw == b"\xab" * 96


@pytest.mark.parametrize("curve", [0, 1])
def test_refusals_leave_the_output_untouched(pkg, curve):
    import torch
    pb, own, _ = SIZES[curve]
    n = NP
    pts = points(curve)[:pb * n]
    vals = vectors(n, 64)["mixed"]
    sc8, sc16, sc_own = records(vals, 8), records(vals, 16), records(vals, own)
    dp = _dev(pts)
    d8 = _dev(bytes(8) + sc8)                           # the records start 8 bytes into the allocation
    d16 = _dev(bytes(8) + sc16)

    def refused(fn, *args, size=96):
        out = ctypes.create_string_buffer(b"\xab" * size, size)
        assert fn(c._h, *args, out) == EINVAL, c._L.te_msm_last_error(c._h)
        assert out.raw == b"\xab" * size, "output touched"

    with ctx_for(pkg, curve) as c:
        b_set = c.bind_points(pts)
        L = c._L
        # narrow records with Montgomery scalars
        c.set_option("scalars_montgomery", 1)
        for size, sc in ((8, sc8), (16, sc16)):
            set_form(c, size, 8 * size)
            refused(L.te_msm_run, pts, sc, n)
            refused(L.te_msm_run_scalars, b_set._h, sc)
            t = ctypes.c_uint64(0)
            assert L.te_msm_submit(c._h, pts, sc, n, ctypes.byref(t)) == EINVAL
            assert L.te_msm_submit_scalars(c._h, b_set._h, sc, ctypes.byref(t)) == EINVAL
        c.set_option("scalars_montgomery", 0)
        # a declared width above the record's
        for size, sc, bits in ((8, sc8, 65), (16, sc16, 129), (8, sc8, 256)):
            set_form(c, size, bits)
            refused(L.te_msm_run, pts, sc, n)
            refused(L.te_msm_run_scalars, b_set._h, sc)
        # 16-byte records whose declared width was reset afterwards
        set_form(c, 16, 128)
        c.set_option("scalar_bits", 0)
        refused(L.te_msm_run, pts, sc16, n)
        refused(L.te_msm_run_scalars, b_set._h, sc16)
        # a device pointer that is not aligned to the record
        set_form(c, 16, 128)
        refused(L.te_msm_run_device, dp.data_ptr(), d16.data_ptr() + 8, n)
        refused(L.te_msm_run_scalars_device, b_set._h, d16.data_ptr() + 8)
        t = ctypes.c_uint64(0)
        assert L.te_msm_submit_device(c._h, dp.data_ptr(), d16.data_ptr() + 8, n, ctypes.byref(t)) == EINVAL
        assert L.te_msm_submit_scalars_device(c._h, b_set._h, d16.data_ptr() + 8, ctypes.byref(t)) == EINVAL
        # ... the batch, indexed and building-block device forms
        lens3 = (ctypes.c_uint64 * 3)(3, 5, 2)
        refused(L.te_msm_run_scalars_batch_device, b_set._h, 3, lens3, d16.data_ptr() + 8, size=3 * 96)
        didx = _dev(np.arange(n, dtype="<u4").tobytes())
        refused(L.te_msm_run_scalars_indexed_device, b_set._h, didx.data_ptr(), d16.data_ptr() + 8, n)
        assert L.te_msm_submit_scalars_indexed_device(c._h, b_set._h, didx.data_ptr(), d16.data_ptr() + 8, n, ctypes.byref(t)) == EINVAL
        part = torch.full((64 * c.row_bytes,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        own_stream = ctypes.c_void_p(-1)
        assert L.te_msm_partial_device(c._h, dp.data_ptr(), d16.data_ptr() + 8, n, part.data_ptr(), own_stream) == EINVAL
        pv = (ctypes.c_void_p * 2)(dp.data_ptr(), dp.data_ptr())
        sv = (ctypes.c_void_p * 2)(d16.data_ptr() + 16, d16.data_ptr() + 8)             # the second of the two is misaligned
        assert L.te_msm_partial_device_batch(c._h, pv, sv, n, 2, part.data_ptr(), own_stream) == EINVAL
        torch.cuda.synchronize()
        assert bool((part == 0xAB).all()), "rows touched"
        assert c.get_option("in_flight") == 0
        set_form(c, 8, 0)
        refused(L.te_msm_run_device, dp.data_ptr(), d8.data_ptr() + 4, n)
        assert c.run_device(dp.data_ptr(), d8.data_ptr() + 8, n) == want(curve, n, 64, "mixed"), "8-byte alignment is enough for 8-byte records"
        # a window shard with step > W
        c.set_option("scalar_bits", 6)
        assert c.plan(n)[1] == 1
        c.set_window_shard(0, 2)
        refused(L.te_msm_run, pts, sc8, n)
        refused(L.te_msm_run_device, dp.data_ptr(), d8.data_ptr() + 8, n)
        c.set_window_shard(0, 1)
        c.set_option("scalar_bits", 0)
        # scalar multiplication reads 32- / 48-byte records only
        base = c.bind_base(pts[:pb])
        dout = torch.full((pb * n,), 0xAB, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        xs = x_only(curve, pts)
        for size, sc, d in ((8, sc8, d8), (16, sc16, d16)):
            set_form(c, size, 8 * size)
            refused(L.te_msm_mul, pts, sc, n, 0, size=pb * n)
            refused(L.te_msm_mul, pts, sc[:size], n, 1, size=pb * n)
            refused(L.te_msm_mul_x, xs, sc, n, 0, size=pb * n)
            refused(L.te_msm_mul_base, base._h, sc, n, size=pb * n)
            assert L.te_msm_mul_device(c._h, dp.data_ptr(), d.data_ptr() + 16, n, 0, dout.data_ptr()) == EINVAL
            assert L.te_msm_mul_base_device(c._h, base._h, d.data_ptr() + 16, n, dout.data_ptr()) == EINVAL
            torch.cuda.synchronize()
            assert bool((dout == 0xAB).all())
        # the context stays usable, and the wide records work as before
        set_form(c, 0, 0)
        assert c.run(pts, sc_own) == want(curve, n, 64, "mixed")
        assert c.mul(pts[:pb], sc_own[:own])[:pb] == ORA[curve].scalar_mul(pts[:pb], vals[0])
        c.release_base(base)
        c.release_points(b_set)


@pytest.mark.parametrize("curve", [0, 1])
def test_tickets_keep_the_form_they_were_submitted_with(pkg, curve):
    pb, own, _ = SIZES[curve]
    n = NP
    pts = points(curve)[:pb * n]
    vals = vectors(n, 64)["mixed"]
    sc8, sc_own = records(vals, 8), records(vals, own)
    w = want(curve, n, 64, "mixed")
    dp, d8 = _dev(pts), _dev(sc8)
    with ctx_for(pkg, curve) as c:
        b_set = c.bind_points(pts)
        submits = [lambda: c.submit(pts, sc8), lambda: c.submit_async(pts, sc8), lambda: c.submit_device(dp.data_ptr(), d8.data_ptr(), n),
                   lambda: c.submit_scalars(b_set, sc8), lambda: c.submit_scalars_device(b_set, d8.data_ptr())]
        for f in submits:
            c.set_option("scalar_bits", 64)
            c.set_option("scalar_record_bytes", 8)
            t = f()
            c.set_option("scalar_bits", 0)
            c.set_option("scalar_record_bytes", 0)
            t_wide = c.submit(pts, sc_own)
            assert c.collect(t) == w and c.collect(t_wide) == w
        c.release_points(b_set)


# ---- Node: setScalarRecordBytes(8 | 16), setScalarBits(b) ----------------------------------------------------------------------------------------
def test_node_narrow_scalar_switches(pkg, tmp_path):
    """the addon's two switches against the same oracle values: u64 and u128 buffers through compute_msm, msmBatch and msmIndexed, a declared
    width over 32-byte records, 16-byte records without a declared width (the call rejects), scalarMul under narrow records, bad arguments"""
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
    n = NP
    pts = points(0)[:64 * n]
    v64, v128 = vectors(n, 64)["mixed"], vectors(n, 128)["mixed"]
    idx = np.random.default_rng(3).integers(0, n, size=n).astype("<u4")
    files = {"p.bin": pts, "s8.bin": records(v64, 8), "s16.bin": records(v128, 16), "s32.bin": records(v64, 32), "i.bin": idx.tobytes()}
    for name, data in files.items():
        (tmp_path / name).write_bytes(data)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
(async () => {
  const [pts, s8, s16, s32, ib] = [2, 3, 4, 5, 6].map((i) => fs.readFileSync(process.argv[i]));
  const idx = new Uint32Array(ib.buffer, ib.byteOffset, ib.length / 4);
  const xy = (r) => [r.x.toString(), r.y.toString()];
  const out = {};
  m.setScalarRecordBytes(8);
  out.u64 = xy(await m.compute_msm(pts, s8, false));
  m.setBases(pts);
  out.u64Bound = xy(await m.compute_msm(pts, s8, false));
  out.u64Batch = (await m.msmBatch([s8, s8.subarray(0, 8 * 5)])).map(xy);
  out.u64Indexed = xy(await m.msmIndexed(idx, s8));
  try { m.scalarMul(pts.subarray(0, 64), s32.subarray(0, 32)); out.mul = 'returned'; } catch (e) { out.mul = String(e.message); }
  m.setBases(null);
  m.setScalarRecordBytes(16);                       // no width declared: the engine refuses 16, the call rejects
  try { await m.compute_msm(pts, s16, false); out.bare16 = 'resolved'; } catch (e) { out.bare16 = String(e.message); }
  m.setScalarBits(128);
  out.u128 = xy(await m.compute_msm(pts, s16, false));
  m.setScalarRecordBytes(0);
  m.setScalarBits(64);
  out.wide64 = xy(await m.compute_msm(pts, s32, false));
  m.setScalarBits(0);
  out.wide = xy(await m.compute_msm(pts, s32, false));
  for (const [k, f] of [['badBytes', () => m.setScalarRecordBytes(24)], ['badBits', () => m.setScalarBits(257)], ['noBits', () => m.setScalarBits()]]) {
    try { f(); out[k] = 'returned'; } catch (e) { out[k] = String(e.message); }
  }
  console.log(JSON.stringify(out));
})();
"""
    r = subprocess.run([node, "-e", script, js] + [str(tmp_path / f) for f in files], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])

    def xy(w):
        return [str(int.from_bytes(w[:32], "little")), str(int.from_bytes(w[32:], "little"))]
    w64, w128 = xy(want(0, n, 64, "mixed")), xy(want(0, n, 128, "mixed"))
    for key in ("u64", "u64Bound", "wide64", "wide"):
        assert out[key] == w64, key
    assert out["u128"] == w128
    assert out["u64Batch"] == [w64, xy(msm(0, pts, v64[:5]))]
    gathered = np.frombuffer(pts, dtype=np.uint8).reshape(-1, 64)[idx.astype(np.int64)].tobytes()
    assert out["u64Indexed"] == xy(msm(0, gathered, v64))
    assert "te_msm error -1" in out["mul"], out["mul"]
    assert "te_msm error -1" in out["bare16"], out["bare16"]
    assert "setScalarRecordBytes(" in out["badBytes"] and "setScalarBits(" in out["badBits"] and "setScalarBits(" in out["noBits"]
