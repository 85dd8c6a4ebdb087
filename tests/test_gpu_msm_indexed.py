"""GPU parity of MSMs over an INDEXED SUBSET of a bound point set (include/te_msm.h: te_msm_run_scalars_indexed[_device],
te_msm_submit_scalars_indexed[_device]): result = sum_j k_j P_{idx[j]}.  Every test calls the new entry points and every result is
compared bit for bit -- with the oracle over the points gathered on the host, with the existing paths (te_msm_run_scalars, the batch
call's prefixes, zero-padded sparse vectors), with the reference's own answers (the WASM goldens under a permutation) and, above 2^23
bound points, with the closed form over chain points.  Bad indices are plain data: the engine must report them, never gather from them.
One-GPU box: contexts of several "devices" name GPU 0 several times (every device holds its own copy of the records)."""
import ctypes
import json
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from oracle import chain_msm as cm
from oracle import oracle, oracle377
from oracle.gen_golden import make_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {0: (64, 32, 64), 1: (96, 48, 96)}          # point, scalar record, result bytes
ORA = {0: oracle, 1: oracle377}
EINVAL, ESCALAR, ESTATE = -1, -3, -4


def _dev(buf):
    import torch
    t = torch.frombuffer(bytearray(buf) if len(buf) else bytearray(16), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    return t


def identity(curve):
    return bytes(32) + (1).to_bytes(32, "little") if curve == 0 else bytes(96)


def rows(buf, width):
    return np.frombuffer(buf, dtype=np.uint8).reshape(-1, width)


def gather(buf, idx, width):
    """records idx[0], idx[1], ... of a buffer of `width`-byte records"""
    return rows(buf, width)[np.asarray(idx, dtype=np.int64)].tobytes()


def expect(curve, pts, idx, sc):
    """the oracle's MSM over the points gathered on the host"""
    if len(idx) == 0:
        return identity(curve)
    return ORA[curve].msm(gather(pts, idx, SIZES[curve][0]), sc, threads=16)


def both_forms(c, b, idx, sc):
    """host form and device form of one indexed MSM; asserts that they agree and returns the bytes"""
    idx = np.ascontiguousarray(idx, dtype="<u4")
    host = c.run_scalars_indexed(b, idx, sc)
    di, ds = _dev(idx.tobytes()), _dev(sc)
    assert c.run_scalars_indexed_device(b, di.data_ptr(), ds.data_ptr(), len(idx)) == host, "device form differs from host form"
    return host


def raw_indexed(c, b, idx, sc, m, out_len=64, device=False, out_ptr=True):
    """the C call itself; returns (rc, out bytes) -- out is pre-filled with 0xAB to show what the call touched.  idx / sc: None, a
    host buffer (bytes / numpy array) or, with device=True, a device address"""
    out = ctypes.create_string_buffer(b"\xab" * out_len, out_len)
    if device:
        fn, ia, sa = c._L.te_msm_run_scalars_indexed_device, idx, sc
    else:
        fn = c._L.te_msm_run_scalars_indexed
        arr = None if idx is None else np.ascontiguousarray(idx, dtype="<u4")      # (alive until the call has returned)
        ia, sa = (None if arr is None else arr.ctypes.data), sc
    rc = fn(c._h, b._h if hasattr(b, "_h") else b, ia, sa, m, out if out_ptr else None)
    return rc, out.raw


untouched = lambda out: out == b"\xab" * len(out)


# ---- 1. against the oracle -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,logn", [(0, 16), (1, 14)])
def test_index_lists_equal_the_oracle_over_the_gathered_points(pkg, curve, logn):
    count = 1 << logn
    sb = SIZES[curve][1]
    pts = ORA[curve].gen_points(91 + curve, count)
    rng = np.random.default_rng(17 + curve)
    lists = {
        "sorted": np.sort(rng.choice(count, size=count // 3, replace=False)),
        "shuffled": rng.permutation(count)[: count // 2],
        "repeats": rng.integers(0, count // 50, size=count // 4),
        "all the same": np.full(5000, count - 1),
    }
    for m in (1, 2, 3, 255, 4097, count, 2 * count + 5):
        lists["m = %d" % m] = rng.integers(0, count, size=m)
    cases = []
    for seed, (name, idx) in enumerate(lists.items()):
        sc = ORA[curve].gen_scalars(300 + seed, len(idx))
        cases.append((name, idx, sc, expect(curve, pts, idx, sc)))
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        b = c.bind_points(pts)
        for signed in (1, 0):
            c.set_option("signed_digits", signed)
            for name, idx, sc, want in cases:
                assert both_forms(c, b, idx, sc) == want, (name, "signed" if signed else "unsigned")
        c.release_points(b)
    assert len(cases[0][2]) == sb * len(cases[0][1])


# ---- 2. against the existing paths -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve,n", [(0, 1 << 16), (1, 1 << 13)])
def test_equal_to_run_scalars_prefixes_and_zero_padded_sparse_vectors(pkg, curve, n):
    pb, sb, _ = SIZES[curve]
    pts = ORA[curve].gen_points(23, n)
    sc = ORA[curve].gen_scalars(24, n)
    rng = np.random.default_rng(25)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        b = c.bind_points(pts)
        whole = c.run_scalars(b, sc)
        assert both_forms(c, b, np.arange(n), sc) == whole, "indices 0 .. n-1 against te_msm_run_scalars"
        lens = [1, 255, 4097, n // 3, n - 1]
        prefixes = c.run_scalars_batch(b, [sc[:sb * L] for L in lens])
        for L, want in zip(lens, prefixes):
            assert both_forms(c, b, np.arange(L), sc[:sb * L]) == want, ("indices 0 .. L-1 against the batch call's prefix", L)
        for density in (2, 8, 64, n):                       # 1/2, 1/8, 1/64 and ONE entry
            k = max(1, n // density)
            where = np.sort(rng.choice(n, size=k, replace=False))
            vals = ORA[curve].gen_scalars(1000 + density, k)
            padded = np.zeros((n, sb), dtype=np.uint8)
            padded[where] = rows(vals, sb)
            assert both_forms(c, b, where, vals) == c.run_scalars(b, padded.tobytes()), ("sparse vector, density 1 /", density)
        c.release_points(b)


# ---- 3. against the reference's own answers --------------------------------------------------------------------------------------------
def test_wasm_goldens_under_a_random_permutation(pkg, wasm_golden, model):
    chosen = [g for g in wasm_golden if g["n"] <= (1 << 16)] + [g for g in wasm_golden if g["n"] == (1 << 20)][:1]
    assert len(chosen) >= 10 and chosen[-1]["n"] == 1 << 20
    with pkg.MsmContext((0,)) as c:
        for k, g in enumerate(chosen):
            n = g["n"]
            pts, sc = make_inputs(g["seed"], n, g["mode"])
            perm = np.random.default_rng(400 + k).permutation(n)
            b = c.bind_points(pts)
            got = both_forms(c, b, perm, gather(sc, perm, 32))
            c.release_points(b)
            assert model.xy_from_bytes(got) == (int(g["x"]), int(g["y"])), g["name"]


# ---- 4. general-form entries and high indices -----------------------------------------------------------------------------------------
def chain_expect(model, pts, idx, sc):
    """[S0] P_0 + [S1] (P_1 - P_0) with S0 = sum k_j, S1 = sum idx_j k_j: the closed form of oracle/chain_msm.py over gathered chain points"""
    ks = [int.from_bytes(sc[32 * j:32 * j + 32], "little") for j in range(len(idx))]
    s0 = sum(ks) % model.L
    s1 = sum(int(i) * k for i, k in zip(idx, ks)) % model.L
    p0, p1 = model.xy_from_bytes(bytes(pts[:64])), model.xy_from_bytes(bytes(pts[64:128]))
    acc = model.add(model.scalar_mul(s0, p0), model.scalar_mul(s1, model.add(p1, model.neg(p0))))
    return model.le32(acc[0]) + model.le32(acc[1])


def test_general_form_entries_and_indices_above_2_23(pkg, model):
    t0 = time.time()
    count = (1 << 23) + 4099                               # the set's count decides the entry form: general (u16 key + u32 index)
    pts, _ = pkg.synth_inputs(0x1D5E7, count, scalars=False)
    cm.check_chain(cm.CURVE_TE, pts, cm.sample_indices(count, 32, seed=3))
    m = 1 << 16
    rng = np.random.default_rng(88)
    idx = rng.integers(0, count, size=m)
    idx[[5, m // 2, m - 1]] = [(1 << 23) - 1, 1 << 23, count - 1]
    sc = oracle.gen_scalars(89, m)
    want = chain_expect(model, pts, idx, sc)
    with pkg.MsmContext((0,)) as c:
        b = c.bind_points(pts)
        assert both_forms(c, b, idx, sc) == want, "2^16 indices over 2^23 + 4099 bound points"
        t = c.submit_scalars_indexed(b, idx, sc)
        assert c.collect(t) == want, "the same as a ticket"
        c.release_points(b)
    small = 1 << 14                                        # the same form forced on a small set (a prefix of the chain)
    idx2 = rng.integers(0, small, size=3 * small + 1)
    sc2 = oracle.gen_scalars(90, len(idx2))
    want2 = chain_expect(model, pts, idx2, sc2)
    with pkg.MsmContext((0,)) as c:
        b = c.bind_points(pts[:64 * small])
        packed = both_forms(c, b, idx2, sc2)
        c.set_option("packed_sort", 0)
        assert both_forms(c, b, idx2, sc2) == want2 == packed, "packed_sort = 0 on a small set"
        c.release_points(b)
    print("\n[indexed, 2^23 + 4099 bound points: %.1f s including input synthesis]" % (time.time() - t0))


# ---- 5. errors ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("curve", [0, 1])
def test_a_bad_index_is_reported_and_never_gathered(pkg, curve):
    count, m = 3000, 5000
    pb, sb, rb = SIZES[curve]
    pts = ORA[curve].gen_points(61, count)
    sc = ORA[curve].gen_scalars(62, m)
    good = np.random.default_rng(63).integers(0, count, size=m)
    want = expect(curve, pts, good, sc)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        b = c.bind_points(pts)
        assert c.get_option("bad_index_position") == -1
        for chunks in (1, 3):
            c.set_option("scalar_chunks", chunks)
            for bad_at, value in (([0], count), ([m // 2], count + 1), ([m - 1], 0xFFFFFFFF), ([4000, 77, 4999, 78], 1 << 31), ([m - 1, m - 2], count)):
                idx = good.copy()
                idx[bad_at] = value
                rc, out = raw_indexed(c, b, idx, sc, m, rb)
                assert rc == EINVAL and untouched(out), (chunks, bad_at)
                assert c.get_option("bad_index_position") == min(bad_at), (chunks, bad_at)
                di, ds = _dev(idx.astype("<u4").tobytes()), _dev(sc)
                rc, out = raw_indexed(c, b, di.data_ptr(), ds.data_ptr(), m, rb, device=True)
                assert rc == EINVAL and untouched(out) and c.get_option("bad_index_position") == min(bad_at), ("device form", bad_at)
                with pytest.raises(pkg.MsmError) as e:
                    c.run_scalars_indexed(b, idx, sc)
                assert e.value.code == EINVAL and e.value.index == min(bad_at)
                assert c.run_scalars_indexed(b, good, sc) == want, "the next call on the same context is correct"
        # a bad index whose scalar is zero is sorted nowhere -- and is reported all the same
        idx = good.copy()
        idx[1234] = count
        zsc = sc[:sb * 1234] + bytes(sb) + sc[sb * 1235:]
        rc, out = raw_indexed(c, b, idx, zsc, m, rb)
        assert rc == EINVAL and untouched(out) and c.get_option("bad_index_position") == 1234
        c.release_points(b)


def test_a_bad_index_on_several_devices_reports_the_lowest_position(pkg):
    count, m = 3000, 40000
    pts = oracle.gen_points(61, count)
    sc = oracle.gen_scalars(64, m)
    good = np.random.default_rng(65).integers(0, count, size=m)
    with pkg.MsmContext((0, 0, 0, 0)) as c:
        b = c.bind_points(pts)
        want = c.run_scalars_indexed(b, good, sc)
        assert want == expect(0, pts, good, sc)
        for bad_at in ([m - 1], [35000, 12000, 25000], [0, m - 1]):
            idx = good.copy()
            idx[bad_at] = count + 7
            rc, out = raw_indexed(c, b, idx, sc, m)
            assert rc == EINVAL and untouched(out) and c.get_option("bad_index_position") == min(bad_at), bad_at
            assert c.run_scalars_indexed(b, good, sc) == want
        c.release_points(b)


def test_a_bad_index_in_a_ticket_comes_at_collect(pkg):
    count, m = 4096, 6000
    pts = oracle.gen_points(66, count)
    rng = np.random.default_rng(67)
    idxs = [rng.integers(0, count, size=m) for _ in range(4)]
    scs = [oracle.gen_scalars(70 + k, m) for k in range(4)]
    want = [expect(0, pts, i, s) for i, s in zip(idxs, scs)]
    bad = idxs[1].copy()
    bad[[4321, 99]] = count
    with pkg.MsmContext((0,)) as c:
        b = c.bind_points(pts)
        dev = [(_dev(i.astype("<u4").tobytes()), _dev(s)) for i, s in zip(idxs, scs)]
        dbad = _dev(bad.astype("<u4").tobytes())
        for host in (True, False):
            t0 = c.submit_scalars_indexed(b, idxs[0], scs[0]) if host else c.submit_scalars_indexed_device(b, dev[0][0].data_ptr(), dev[0][1].data_ptr(), m)
            tb = c.submit_scalars_indexed(b, bad, scs[1]) if host else c.submit_scalars_indexed_device(b, dbad.data_ptr(), dev[1][1].data_ptr(), m)
            t2 = c.submit_scalars_indexed(b, idxs[2], scs[2]) if host else c.submit_scalars_indexed_device(b, dev[2][0].data_ptr(), dev[2][1].data_ptr(), m)
            assert c.get_option("in_flight") == 3
            assert c.collect(t2) == want[2]
            out = ctypes.create_string_buffer(b"\xab" * 64, 64)
            assert c._L.te_msm_collect(c._h, tb, out) == EINVAL and untouched(out.raw), "the error comes at collect"
            assert c.get_option("bad_index_position") == 99
            c._held.pop(tb, None)
            assert c.collect(t0) == want[0], "other tickets are unaffected"
            assert c.get_option("in_flight") == 0
            t = c.submit_scalars_indexed(b, bad, scs[1])
            with pytest.raises(pkg.MsmError) as e:
                c.collect(t)
            assert e.value.code == EINVAL and e.value.index == 99
            assert c.run_scalars_indexed(b, idxs[3], scs[3]) == want[3]
        c.release_points(b)


def test_argument_errors_leave_out_untouched(pkg):
    count, m = 3000, 1000
    pts = oracle.gen_points(2, count)
    sc = oracle.gen_scalars(3, m)
    idx = np.random.default_rng(4).integers(0, count, size=m).astype("<u4")
    di, ds = _dev(idx.tobytes()), _dev(sc)
    with pkg.MsmContext((0,)) as c:
        b = c.bind_points(pts)
        want = expect(0, pts, idx, sc)
        # m = 0: the identity, no pointer needed; no ticket
        for device in (False, True):
            rc, out = raw_indexed(c, b, None, None, 0, device=device)
            assert rc == 0 and out == identity(0)
        assert c.run_scalars_indexed(b, [], b"") == identity(0)
        t = ctypes.c_uint64(0)
        assert c._L.te_msm_submit_scalars_indexed(c._h, b._h, None, None, 0, ctypes.byref(t)) == EINVAL and c.get_option("in_flight") == 0
        # null pointers while m > 0
        for ia, sa in ((None, sc), (idx, None), (None, None)):
            rc, out = raw_indexed(c, b, ia, sa, m)
            assert rc == EINVAL and untouched(out)
        for ia, sa in ((None, ds.data_ptr()), (di.data_ptr(), None)):
            rc, out = raw_indexed(c, b, ia, sa, m, device=True)
            assert rc == EINVAL and untouched(out)
            assert c._L.te_msm_submit_scalars_indexed_device(c._h, b._h, ia, sa, m, ctypes.byref(t)) == EINVAL
        assert c._L.te_msm_submit_scalars_indexed(c._h, b._h, None, sc, m, ctypes.byref(t)) == EINVAL
        assert raw_indexed(c, b, idx, sc, m, out_ptr=False)[0] == EINVAL
        assert c.get_option("in_flight") == 0
        # a window shard set
        assert c._L.te_msm_set_window_shard(c._h, 0, 2) == 0
        rc, out = raw_indexed(c, b, idx, sc, m)
        assert rc == EINVAL and untouched(out)
        rc, out = raw_indexed(c, b, di.data_ptr(), ds.data_ptr(), m, device=True)
        assert rc == EINVAL and untouched(out)
        assert c._L.te_msm_submit_scalars_indexed(c._h, b._h, idx.ctypes.data, sc, m, ctypes.byref(t)) == EINVAL
        assert c._L.te_msm_set_window_shard(c._h, 0, 1) == 0
        # a handle of the other curve
        c.set_option("curve", 1)
        rc, out = raw_indexed(c, b, idx, sc + bytes(16 * m), m, 96)
        assert rc == EINVAL and untouched(out)
        c.set_option("curve", 0)
        # a scalar out of range: TE_MSM_ESCALAR, on both forms and through a ticket
        # (16-bit windows: the reference's own acceptance, 16 x 16 bits; m = 1000 alone plans 26 windows of 10 bits, which hold any 256-bit value)
        c.set_option("window_bits", 16)
        over = sc[:32 * 500] + b"\xff" * 32 + sc[32 * 501:]
        rc, out = raw_indexed(c, b, idx, over, m)
        assert rc == ESCALAR and untouched(out)
        dov = _dev(over)
        rc, out = raw_indexed(c, b, di.data_ptr(), dov.data_ptr(), m, device=True)
        assert rc == ESCALAR and untouched(out)
        tk = c.submit_scalars_indexed(b, idx, over)
        with pytest.raises(pkg.MsmError) as e:
            c.collect(tk)
        assert e.value.code == ESCALAR and e.value.index is None
        c.set_option("signed_digits", 0)                                     # unsigned digits accept any 256-bit scalar
        assert c.run_scalars_indexed(b, np.arange(m), over) == c.run_scalars(b, over + bytes(32 * (count - m)))
        c.set_option("signed_digits", 1)
        c.set_option("window_bits", 0)
        assert c.run_scalars_indexed(b, idx, sc) == want, "the context is still usable"
        # a released handle
        handle = b._h
        c.release_points(b)
        rc, out = raw_indexed(c, handle, idx, sc, m)
        assert rc == EINVAL and untouched(out)
        rc, out = raw_indexed(c, handle, di.data_ptr(), ds.data_ptr(), m, device=True)
        assert rc == EINVAL and untouched(out)
        assert c._L.te_msm_submit_scalars_indexed(c._h, handle, idx.ctypes.data, sc, m, ctypes.byref(t)) == EINVAL
        with pytest.raises(pkg.MsmError):
            c.run_scalars_indexed(b, idx, sc)
    with pkg.MsmContext((0,)) as c2, pkg.MsmContext((0,)) as c3:
        b3 = c3.bind_points(pts)
        rc, out = raw_indexed(c2, b3, idx, sc, m)
        assert rc == EINVAL and untouched(out)                               # a set of another context
        c3.release_points(b3)


# ---- 6. shapes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids", [(0, 0), (0, 0, 0, 0)])
def test_host_form_on_several_devices(pkg, ids):
    count = 1 << 15
    pts = oracle.gen_points(51, count)
    rng = np.random.default_rng(52)
    with pkg.MsmContext((0,)) as one, pkg.MsmContext(ids) as c:
        b1, b = one.bind_points(pts), c.bind_points(pts)
        shard_min = c.get_option("host_shard_min")
        for m in (1, shard_min - 1, shard_min * len(ids) - 1, shard_min * len(ids) + 13, 3 * count + 1):
            idx = rng.integers(0, count, size=m)
            sc = oracle.gen_scalars(500 + m, m)
            got = both_forms(c, b, idx, sc)
            assert got == one.run_scalars_indexed(b1, idx, sc), (ids, m)
            if m <= shard_min * len(ids) + 13:
                assert got == expect(0, pts, idx, sc), (ids, m)
        c.set_option("host_shard_min", 100)
        idx = rng.integers(0, count, size=1001)
        sc = oracle.gen_scalars(77, 1001)
        assert c.run_scalars_indexed(b, idx, sc) == expect(0, pts, idx, sc), "host_shard_min applies to m"
        one.release_points(b1)
        c.release_points(b)


@pytest.mark.parametrize("curve", [0, 1])
def test_scalar_chunks_and_options(pkg, curve):
    count = 1 << 13
    pts = ORA[curve].gen_points(53, count)
    rng = np.random.default_rng(54)
    m = 3 * count + 2
    idx = rng.integers(0, count, size=m)
    sc = ORA[curve].gen_scalars(55, m)
    want = expect(curve, pts, idx, sc)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        b = c.bind_points(pts)
        for chunks in (1, 3, 0):
            c.set_option("scalar_chunks", chunks)
            assert c.run_scalars_indexed(b, idx, sc) == want, ("scalar_chunks", chunks)
            t = c.submit_scalars_indexed(b, idx, sc)
            assert c.collect(t) == want, ("ticket, scalar_chunks", chunks)
        for wb, seg in ((7, 0), (0, 4), (16, 16)):
            c.set_option("window_bits", wb)
            c.set_option("segment_len", seg)
            assert both_forms(c, b, idx, sc) == want, (wb, seg)
        c.release_points(b)


def test_fixed_base_set_is_served_from_its_table_0(pkg):
    count = 1 << 13
    pts = oracle.gen_points(55, count)
    rng = np.random.default_rng(56)
    idx = rng.integers(0, count, size=count + 9)
    sc = oracle.gen_scalars(57, len(idx))
    want = expect(0, pts, idx, sc)
    with pkg.MsmContext((0,)) as c:
        c.set_option("bind_fixed_base", 16)
        bf = c.bind_points(pts)
        c.set_option("bind_fixed_base", 0)
        before = c.get_option("fixed_base_fallbacks")
        assert both_forms(c, bf, idx, sc) == want
        t = c.submit_scalars_indexed(bf, idx, sc)
        di, ds = _dev(idx.astype("<u4").tobytes()), _dev(sc)
        t2 = c.submit_scalars_indexed_device(bf, di.data_ptr(), ds.data_ptr(), len(idx))
        assert c.collect(t2) == want and c.collect(t) == want
        assert c.get_option("fixed_base_fallbacks") == before
        c.release_points(bf)


@pytest.mark.parametrize("ids,pairs", [((0,), 4), ((0, 0), 8)])
def test_indexed_device_tickets_interleaved_with_ordinary_ones(pkg, ids, pairs):
    """`pairs` indexed device tickets and as many te_msm_submit_scalars_device tickets over the same set, all in flight (every work set of
    the context), collected in reverse; on two "devices" every ticket copies its inputs over the peer path (option "stage_device_inputs")"""
    count = 1 << 14
    pts = oracle.gen_points(58, count)
    rng = np.random.default_rng(59)
    full = [oracle.gen_scalars(600 + k, count) for k in range(pairs)]
    idxs = [rng.integers(0, count, size=int(rng.integers(1, 2 * count))) for _ in range(pairs)]
    scs = [oracle.gen_scalars(700 + k, len(i)) for k, i in enumerate(idxs)]
    dev_full = [_dev(s) for s in full]
    dev_idx = [_dev(i.astype("<u4").tobytes()) for i in idxs]
    dev_sc = [_dev(s) for s in scs]
    with pkg.MsmContext(ids) as c:
        if len(ids) > 1:
            c.set_option("stage_device_inputs", 1)
        b = c.bind_points(pts)
        want_full = [c.run_scalars(b, s) for s in full]
        want_idx = [expect(0, pts, i, s) for i, s in zip(idxs, scs)]
        tickets = []
        for k in range(pairs):
            tickets.append(("indexed", k, c.submit_scalars_indexed_device(b, dev_idx[k].data_ptr(), dev_sc[k].data_ptr(), len(idxs[k]))))
            tickets.append(("ordinary", k, c.submit_scalars_device(b, dev_full[k].data_ptr())))
        assert c.get_option("in_flight") == 2 * pairs == pkg.WORKSETS * len(ids)
        with pytest.raises(pkg.MsmError) as e:
            c.release_points(b)
        assert e.value.code == ESTATE
        for kind, k, t in reversed(tickets):
            assert c.collect(t) == (want_idx[k] if kind == "indexed" else want_full[k]), (kind, k)
        assert c.get_option("in_flight") == 0
        c.release_points(b)


@pytest.mark.parametrize("ids", [(0,), (0, 0)])
def test_asynchronous_host_tickets(pkg, ids):
    count = 1 << 14
    pts = oracle.gen_points(68, count)
    rng = np.random.default_rng(69)
    idxs = [rng.integers(0, count, size=int(rng.integers(1, 3 * count))) for _ in range(6)]
    scs = [oracle.gen_scalars(800 + k, len(i)) for k, i in enumerate(idxs)]
    want = [expect(0, pts, i, s) for i, s in zip(idxs, scs)]
    with pkg.MsmContext(ids) as c:
        b = c.bind_points(pts)
        tickets = [c.submit_scalars_indexed(b, i, s) for i, s in zip(idxs, scs)]
        assert c.get_option("in_flight") == 6
        assert c._L.te_msm_release_points(c._h, b._h) == ESTATE, "a set with tickets in flight cannot be released"
        c.ticket_wait(tickets[3])
        for k in (3, 5, 0, 4, 1, 2):                       # any order
            assert c.collect(tickets[k]) == want[k], k
        assert c.get_option("in_flight") == 0
        c.release_points(b)


# ---- 7. Node --------------------------------------------------------------------------------------------------------------------------
def test_node_msm_indexed(pkg, tmp_path):
    node = shutil.which("node")
    if not node:
        pytest.skip("node is not installed on this box")
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists("/usr/include/node/node_api.h") and not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        pytest.skip("no N-API addon and no node headers to build it")
    subprocess.check_call(["make", "-C", js, "-s"])
    count, m = 3000, 4500
    pts = oracle.gen_points(71, count)
    idx = np.random.default_rng(72).integers(0, count, size=m).astype("<u4")
    sc = oracle.gen_scalars(73, m)
    bad = idx.copy()
    bad[[2000, 321]] = count
    for name, data in (("p.bin", pts), ("i.bin", idx.tobytes()), ("b.bin", bad.tobytes()), ("s.bin", sc)):
        (tmp_path / name).write_bytes(data)
    with pkg.MsmContext((0,)) as c:
        b = c.bind_points(pts)
        python_result = c.run_scalars_indexed(b, idx, sc)
        c.release_points(b)
    assert python_result == expect(0, pts, idx, sc)
    script = r"""
const fs = require('fs');
const m = require(process.argv[1] + '/compute_msm.js');
const u32 = (f) => { const b = fs.readFileSync(f); return new Uint32Array(b.buffer, b.byteOffset, b.length / 4); };
(async () => {
  const [pts, idx, bad, sc] = [fs.readFileSync(process.argv[2]), u32(process.argv[3]), u32(process.argv[4]), fs.readFileSync(process.argv[5])];
  const out = {};
  try { await m.msmIndexed(idx, sc); out.unbound = 'resolved'; } catch (e) { out.unbound = String(e.message); }
  m.setBases(pts);
  const r = await m.msmIndexed(idx, sc);
  out.got = [r.x.toString(), r.y.toString()];
  try { await m.msmIndexed(bad, sc); out.bad = 'resolved'; } catch (e) { out.bad = String(e.message); out.badIndex = e.index; }
  const again = await m.msmIndexed(idx, sc);
  out.again = [again.x.toString(), again.y.toString()];
  const empty = await m.msmIndexed(new Uint32Array(0), Buffer.alloc(0));
  out.empty = [empty.x.toString(), empty.y.toString()];
  m.setBases(null);
  console.log(JSON.stringify(out));
})();
"""
    files = [str(tmp_path / f) for f in ("p.bin", "i.bin", "b.bin", "s.bin")]
    r = subprocess.run([node, "-e", script, js] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    want = [str(int.from_bytes(python_result[:32], "little")), str(int.from_bytes(python_result[32:], "little"))]
    assert "te_msm error" in out["unbound"], out["unbound"]
    assert out["got"] == want and out["again"] == want
    assert "te_msm error -1" in out["bad"] and "position 321" in out["bad"] and out["badIndex"] == 321, out
    assert out["empty"] == ["0", "1"]
