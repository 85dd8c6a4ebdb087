"""GPU tests above 2^23 points, where the engine leaves the paths the rest of the suite runs: the general level-1 sort form
(packed entries only while n <= 2^23), record slabs past 4 GiB, sorted / partition arrays past 2^31 bytes, partitions of many
level-2 pieces.  The bit-exact oracle is too slow to call often at these sizes, so results are compared with the closed form
of oracle/chain_msm.py over synth_inputs' chain points P_i = (a + i*b) G; every fixture checks the chain on sampled indices.
One independent-points case pins the closed form to the oracle.  Smaller sizes are prefixes of the two fixtures."""
import warnings

import numpy as np
import pytest

from oracle import chain_msm as cm
from oracle.stage_checks import check_stages

pytestmark = pytest.mark.gpu

NT = (1 << 25) + 4099          # Twisted-Edwards fixture: 128-byte records pass 4 GiB, 16 windows of `sorted` pass 2^31 bytes
NB = 19_200_007                # BLS12-377 fixture: the 224-byte per-call record slab passes 4 GiB
N23 = 1 << 23                  # the last size with packed level-1 entries (index field full)
NM = (1 << 24) + 4099
TE, BLS = 0, 1


def _dev(buf):
    """a device copy of a host buffer (no second host copy of a multi-GB `bytes`)"""
    import torch
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")          # torch warns that `bytes` is read-only; the tensor is only read
        t = torch.frombuffer(buf, dtype=torch.uint8)
    d = t.cuda()
    torch.cuda.synchronize()
    return d


@pytest.fixture(scope="class")
def te(pkg):
    pts, sc = pkg.synth_inputs(0x1A26E0, NT)
    cm.check_chain(TE, pts, cm.sample_indices(NT, 32, seed=1))
    return pts, sc


@pytest.fixture(scope="class")
def te_dev(te):
    return _dev(te[0]), _dev(te[1])


@pytest.fixture(scope="class")
def bls(pkg):
    pts, sc = pkg.synth_inputs(0x377B16, NB, curve=BLS)
    cm.check_chain(BLS, pts, cm.sample_indices(NB, 32, seed=2))
    return pts, sc


def _prefix(fx, curve, n):
    pb, sb = cm.POINT_BYTES[curve], cm.SCALAR_BYTES[curve]
    return fx[0][:pb * n], fx[1][:sb * n]


def _whole_and_pieces(ctx, d_points, pts, d_scalars, sc, n, want):
    """te_msm_run splits host buffers of n >= 3 * 2^18 points into pieces planned at their own size (option host_chunks):
    the whole-n path runs from device inputs and from host buffers with host_chunks = 1, the pieces with the default"""
    assert ctx.run_device(d_points.data_ptr(), d_scalars.data_ptr(), n) == want, "run_device (whole n)"
    ctx.set_option("host_chunks", 1)
    assert ctx.run(pts, sc) == want, "run, host_chunks = 1 (whole n)"
    ctx.set_option("host_chunks", 0)
    assert ctx.run(pts, sc) == want, "run (host buffers in pieces)"


class TestTwistedEdwards:
    """every case over prefixes of the 2^25 + 4099-point chain (freed before the BLS12-377 class builds its own)"""

    # ---- 1. sort stages at the packed boundary --------------------------------------------------------------------------------------------
    @pytest.mark.parametrize("n", [N23, N23 + 1])
    def test_sort_stages_at_the_packed_boundary(self, pkg, te, fpcheck, model, ora, n):
        """2^23: packed level-1 entries with the 23-bit index field full; 2^23 + 1: the first size of the general form by default"""
        pts, sc = _prefix(te, TE, n)
        with pkg.MsmContext((0,)) as ctx:
            ctx.set_option("sort_buckets", 1)
            ctx.set_option("prezero", 0)
            ctx.set_option("host_chunks", 1)             # one whole MSM: the stages read back are those of all n entries
            c, _ = ctx.plan(n)
            res = ctx.run(pts, sc)
            check_stages(ctx, fpcheck, model, ora, pts, sc, n, c)
        assert res == cm.chain_msm(TE, pts, sc)


    # ---- 2. whole-MSM paths --------------------------------------------------------------------------------------------------------------
    @pytest.mark.parametrize("n", [N23 + 1, NM, NT])
    def test_whole_msm_paths(self, pkg, te, te_dev, n):
        pts, sc = _prefix(te, TE, n)
        small = 1 << 20
        want, want_small = cm.chain_msms(TE, pts, sc, [n, small])
        dp, ds = te_dev[0].data_ptr(), te_dev[1].data_ptr()
        with pkg.MsmContext((0,)) as ctx:
            assert ctx.run(pts, sc) == want, "run (host buffers in pieces)"
            assert ctx.run_device(dp, ds, n) == want, "run_device"
            t0 = ctx.submit_device(dp, ds, n)
            t1 = ctx.submit_device(dp, ds, small)       # a prefix of the same buffers between two large tickets
            t2 = ctx.submit_device(dp, ds, n)
            assert [ctx.collect(t0), ctx.collect(t1), ctx.collect(t2)] == [want, want_small, want], "submit_device tickets"
            if n == NM:
                ctx.set_option("signed_digits", 0)
                assert ctx.run_device(dp, ds, n) == want, "unsigned digits"
                ctx.set_option("signed_digits", 1)
                ctx.set_option("window_bits", 13)
                assert ctx.run_device(dp, ds, n) == want, "window_bits 13"
                ctx.set_option("window_bits", 0)
            ctx.trim(0)
            b = ctx.bind_points(pts)
            assert ctx.run_scalars(b, sc) == want, "run_scalars"
            assert ctx.run_scalars_device(b, ds) == want, "run_scalars_device"
            b.release()
        if n == NT:
            with pkg.MsmContext((0, 0)) as two:         # a lone call splits the points across two "devices"
                assert two.run(pts, sc) == want, "two devices"


    # ---- 3. skewed inputs ----------------------------------------------------------------------------------------------------------------
    def test_witness_like_scalars_make_giant_buckets(self, pkg, te, te_dev):
        n = NM
        pts, _ = _prefix(te, TE, n)
        rng = np.random.default_rng(24)
        ks = np.zeros((n, 4), dtype="<u8")
        ks[:, 0] = rng.choice(np.array([0, 1, 2, 3, (1 << 64) - 1], dtype=np.uint64), size=n, p=[0.45, 0.25, 0.1, 0.1, 0.1])
        sc = ks.tobytes()
        del ks
        want = cm.chain_msm(TE, pts, sc)
        with pkg.MsmContext((0,)) as ctx:
            _whole_and_pieces(ctx, te_dev[0], pts, _dev(sc), sc, n, want)


    def test_replicated_point_against_the_closed_form(self, pkg, te, te_dev, model):
        """the harness's one point replicated n times: [sum s_i mod L] H"""
        n = NM
        _, sc = _prefix(te, TE, n)
        fixed, _ = pkg.synth_inputs(0, n, fixed_point=True, scalars=False)
        s0 = cm.scalar_sums(TE, sc, [n])[n][0]
        x, y = model.scalar_mul(s0 % model.L, (model.HX, model.HY))
        want = model.le32(x) + model.le32(y)
        with pkg.MsmContext((0,)) as ctx:
            _whole_and_pieces(ctx, _dev(fixed), fixed, te_dev[1], sc, n, want)


    # ---- 4. batched prefixes of a large bound set ----------------------------------------------------------------------------------------
    def test_batched_prefixes_of_a_large_bound_set(self, pkg, te, te_dev):
        import torch
        pts, sc = te
        lens = [NT, (1 << 24) + 1, N23 + 1, N23, N23 - 1, 32769, 32768, 4097, 1, 0]
        want = cm.chain_msms(TE, pts, sc, lens)
        with pkg.MsmContext((0,)) as ctx:
            b = ctx.bind_points(pts)
            got = ctx.run_scalars_batch(b, [memoryview(sc)[:32 * L] for L in lens])
            for m, L in enumerate(lens):
                assert got[m] == want[m], ("host scalars", L)
            packed = torch.cat([te_dev[1][:32 * L] for L in lens])
            torch.cuda.synchronize()
            got = ctx.run_scalars_batch_device(b, packed.data_ptr(), lens)
            for m, L in enumerate(lens):
                assert got[m] == want[m], ("device scalars", L)
            b.release()


    # ---- 5. fixed-base windows above 2^23 ------------------------------------------------------------------------------------------------
    def test_fixed_base_windows_above_2_23(self, pkg, te):
        """c = 20: 13 tables of 2^23 + 1 records (remapped table indices up to 13 n)"""
        n = N23 + 1
        pts, sc = _prefix(te, TE, n)
        want = cm.chain_msm(TE, pts, sc)
        with pkg.MsmContext((0,)) as ctx:
            ctx.set_option("bind_fixed_base", 20)
            b = ctx.bind_points(pts)
            before = ctx.get_option("fixed_base_fallbacks")
            assert ctx.run_scalars(b, sc) == want
            assert ctx.get_option("fixed_base_fallbacks") == before, "the fixed-base windows did not run"
            b.release()


    # ---- 7. independent points against the oracle ----------------------------------------------------------------------------------------
    def test_random_points_against_the_oracle(self, pkg, te, te_dev, ora):
        """not a chain: pins the large-n path to the bit-exact oracle without the closed form"""
        n = N23 + 1
        _, sc = _prefix(te, TE, n)
        pts, _ = pkg.synth_inputs(0x7A11D, n, fixed_point="random", scalars=False)
        want = ora.msm(pts, sc, threads=16)
        with pkg.MsmContext((0,)) as ctx:
            _whole_and_pieces(ctx, _dev(pts), pts, te_dev[1], sc, n, want)


class TestBls12_377:
    # ---- 6. BLS12-377 --------------------------------------------------------------------------------------------------------------------
    @pytest.mark.parametrize("n", [N23 + 1, NB])
    def test_bls12_377_large(self, pkg, bls, n):
        import torch
        pts, sc = _prefix(bls, BLS, n)
        lens = [NB, N23 + 1, N23, 4097, 0]
        want = cm.chain_msm(BLS, pts, sc)
        with pkg.MsmContext((0,)) as ctx:
            ctx.set_option("curve", pkg.CURVE_BLS12_377_G1)
            assert ctx.run(pts, sc) == want, "run"
            dp, ds = _dev(pts), _dev(sc)
            assert ctx.run_device(dp.data_ptr(), ds.data_ptr(), n) == want, "run_device"
            del dp
            torch.cuda.empty_cache()
            ctx.trim(0)
            b = ctx.bind_points(pts)                     # affine records (option bind_affine, default)
            assert ctx.run_scalars(b, sc) == want, "run_scalars"
            if n == NB:
                exp = cm.chain_msms(BLS, pts, sc, lens)
                got = ctx.run_scalars_batch(b, [memoryview(sc)[:48 * L] for L in lens])
                for m, L in enumerate(lens):
                    assert got[m] == exp[m], ("batch", L)
            b.release()
