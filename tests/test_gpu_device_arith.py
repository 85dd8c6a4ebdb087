"""The gfx950 build of the field and point arithmetic, function by function, on chosen operands (tests/csrc/devcheck.hip, helper
module tests/devcheck.py).  The table operations are compared bit for bit with the host build of the same text, which the host tests
pin to bigints; the device-only code -- the DPP team addition, the block-wide sum, the three fold kernels, the reduction tail -- is
launched directly and compared with the bigint models as group elements.  No tolerance anywhere: the arithmetic is integer."""
import ctypes
import random

import numpy as np
import pytest

import devcheck as dc
from devcheck import dc_dec, dc_dev, dc_host, dc_pools  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def _u32(vals):
    return (ctypes.c_uint32 * len(vals))(*vals)


def _sample(pool, rnd, n, repeats=True):
    """n pool indices: mostly generic points; some O in both representations; some entries repeat their predecessor"""
    every = list(range(len(pool.pts)))
    out = []
    for _ in range(n):
        r = rnd.random()
        if repeats and out and r < 0.12:
            out.append(out[-1])
        elif repeats and r < 0.22:
            out.append(rnd.choice((pool.ident, pool.zero_p)))
        else:
            out.append(rnd.choice(every))
    return out


@pytest.mark.parametrize("N", (9, 14))
def test_table_operations_equal_the_host_build(N, dc_dev, dc_host, dc_pools):
    """every operation of the table with N limbs (N = 9 also: mask_select and the two scalar decoders): the device compilation
    gives the host compilation's words, limb by limb"""
    assert dc_dev.dc_table() == dc_host.dc_table()
    failures = []
    for name in dc.OPS_OF[N]:
        inp = dc.table_inputs(name, dc_pools)
        got, want = dc.run_device(name, inp), dc.run_host(name, inp)
        try:
            dc.compare_bits(name, got, want, inp)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("N", (9, 14))
def test_team_addition(N, dc_dev, dc_dec, dc_pools):
    """ete_add_team<N>, one quad per operand pair (more pairs than one block holds, the last block part-filled): the model's sum
    as a group element, the same element as the device's ete_add<N> on the same operands, and an output that keeps the contract
    of a product output (class N, below 1.1 p -- inside Decoders.point)"""
    pool = dc_pools[N]
    cases = pool.pair_cases()
    a, b = pool.acc[[c[1] for c in cases]], pool.acc[[c[2] for c in cases]]
    d_a, d_b, d_out = dc.to_device(a), dc.to_device(b), dc.device_zeros(len(cases), 4 * N)
    dc.launch("ete_add_team<%d>" % N, getattr(dc_dev, "dc_add_team_%d" % N), d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), len(cases))
    team = dc.from_device(d_out)
    full = dc.run_device("add_%d" % N, np.hstack([a, b]))
    for i, (name, ia, ib) in enumerate(cases):
        want = dc.msum(N, [pool.pts[ia], pool.pts[ib]])
        dc_dec.check("ete_add_team<%d>" % N, N, team[i], want, name)
        dc_dec.check("ete_add<%d>" % N, N, full[i], want, name)
        assert dc_dec.point("ete_add_team<%d>" % N, N, team[i]) == dc_dec.point("ete_add<%d>" % N, N, full[i]), name


@pytest.mark.parametrize("N", (9, 14))
def test_team_addition_at_the_limb_extremes(N, dc_dev):
    """ete_add_team<N> on synthetic accumulators whose limbs sit at the edges of the contract (devcheck.extreme_pairs): first-point
    differences and sums at the largest limbs their classes allow, where a missing normalisation overflows a 64-bit column.  The
    operands are no curve points, so there is no group element to compare: the team addition forms the same nine products as
    ete_add<N> -- A, B, T1 T2, Z1 Z2, 2d T1 T2, then E F, H G, E H, F G -- so each output coordinate is congruent mod p to that of
    the host build's ete_add<N> (which the table test compares with the device's bit for bit), and keeps the contract."""
    F = dc.FIELDS[N]
    pairs = dc.extreme_pairs(N)
    want = dc.run_host("add_%d" % N, pairs)
    d_a, d_b = dc.to_device(pairs[:, :4 * N]), dc.to_device(pairs[:, 4 * N:])
    d_out = dc.device_zeros(len(pairs), 4 * N)
    op = "ete_add_team<%d>" % N
    dc.launch(op, getattr(dc_dev, "dc_add_team_%d" % N), d_a.data_ptr(), d_b.data_ptr(), d_out.data_ptr(), len(pairs))
    team = dc.from_device(d_out)
    for e in range(len(pairs)):
        dc.check_contract(op, N, team[e])
        for c, name in enumerate("xyzt"):
            g, h = F.val(team[e, N * c:N * (c + 1)]) % F.P, F.val(want[e, N * c:N * (c + 1)]) % F.P
            assert g == h, "%s: pair %d, coordinate %s: residue %x, ete_add<%d> of the host build gives %x" % (op, e, name, g, N, h)


BLOCK_SUM_COUNTS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256)
GIANT_RUN = 256                                     # TE_GIANT_RUN of kernels.hip.hpp: the stride of the second-level sum
BLOCK_SUM_STRIDED = (2, 3, 5)


@pytest.mark.parametrize("N", (9, 14))
def test_block_sum_points(N, dc_dev, dc_dec, dc_pools):
    """block_sum_points<N, COHERENT>: the model's sum of src[0], src[stride], ... for every count around the quad count (64) and
    the tree levels at stride 1, for 2, 3 and 5 points at stride TE_GIANT_RUN, in both COHERENT forms; over generic points, over one
    point repeated (every tree level doubles) and over P, -P alternating with O in between (partial sums pass through O).
    cnt = 0 is not run: no call site can pass it.  k_seg_combine_all calls with cnt = min(TE_GIANT_RUN, ns - part), where part < ns
    is a chunk entry k_l2_place_order wrote for an existing part, and with cnt = nchunks only behind `nchunks == 1 -> continue`,
    i.e. nchunks >= 2."""
    pool, rnd = dc_pools[N], random.Random(41 + N)
    n_src = (max(BLOCK_SUM_STRIDED) - 1) * GIANT_RUN + len(BLOCK_SUM_COUNTS) + 1
    n_src = max(n_src, len(BLOCK_SUM_COUNTS) + max(BLOCK_SUM_COUNTS))
    g = pool.gen
    neg = next((i, j) for i in g for j in g if pool.pts[j] == dc.mneg(N, pool.pts[i]))
    lists = {"generic points": _sample(pool, rnd, n_src, repeats=False),
             "one point repeated": [g[3]] * n_src,
             "P, O, -P, O' in turn": [(neg[0], pool.ident, neg[1], pool.zero_p)[j % 4] for j in range(n_src)]}
    # job j starts at src[j]: the runs of a giant bucket do not start at the head of the buffer either
    jobs = [(j, 1, c) for j, c in enumerate(BLOCK_SUM_COUNTS)] + [(j, GIANT_RUN, c) for j, c in enumerate(BLOCK_SUM_STRIDED)]
    first, stride, cnt = (_u32([jb[k] for jb in jobs]) for k in range(3))
    for what, idx in lists.items():
        d_src = dc.to_device(pool.acc[idx])
        want = [dc.msum(N, [pool.pts[idx[f + t * s]] for t in range(c)]) for f, s, c in jobs]
        for coherent in (0, 1):
            op = "block_sum_points<%d, %s>" % (N, "true" if coherent else "false")
            d_out = dc.device_zeros(len(jobs), 4 * N)
            dc.launch(op, getattr(dc_dev, "dc_block_sum_%d" % N), coherent, d_src.data_ptr(), n_src, first, stride, cnt, len(jobs), d_out.data_ptr())
            out = dc.from_device(d_out)
            for j, (f, s, c) in enumerate(jobs):
                dc_dec.check(op, N, out[j], want[j], "%s, cnt = %d at stride %d" % (what, c, s))


FOLD_FORMS = ("k_sum_groups<%d, false>", "k_sum_groups<%d, true>", "k_sum_groups_team<%d>")


@pytest.mark.parametrize("N", (9, 14))
def test_fold_kernels_agree(N, dc_dev, dc_dec, dc_pools):
    """k_sum_groups<N, false>, k_sum_groups<N, true> and k_sum_groups_team<N> on the same job, launched with reduce_t's grids:
    out[o] = sum_{t < K} in[((o / inner) K + t) inner + o % inner] per window, equal to the model and to each other as group
    elements.  K = 2, 4, 8; inner = 1, 5; 1, 5 and 67 outputs (odd: pairs and quads meet the end of the range); 1 and 3 windows;
    some inputs are O, some repeat their neighbour."""
    pool, rnd = dc_pools[N], random.Random(51 + N)
    for K in (2, 4, 8):
        for inner in (1, 5):
            for n_out in (1, 5, 67):
                for nw in (1, 3):
                    ipw = -(-n_out // inner) * inner * K
                    idx = _sample(pool, rnd, ipw * nw)
                    d_in = dc.to_device(pool.acc[idx])
                    want = [dc.msum(N, [pool.pts[idx[k * ipw + ((o // inner) * K + t) * inner + o % inner]] for t in range(K)])
                            for k in range(nw) for o in range(n_out)]
                    got = []
                    for form in range(3):
                        op = FOLD_FORMS[form] % N
                        d_out = dc.device_zeros(n_out * nw, 4 * N)
                        dc.launch(op, getattr(dc_dev, "dc_sum_groups_%d" % N), form, d_in.data_ptr(), ipw * nw, d_out.data_ptr(), n_out * nw,
                                  n_out, K, inner, ipw, n_out, nw)
                        out = dc.from_device(d_out)
                        what = "K = %d, inner = %d, n_out = %d, nw = %d" % (K, inner, n_out, nw)
                        pts = [dc_dec.point(op, N, out[i], "%s, output %d" % (what, i)) for i in range(n_out * nw)]
                        for i, p in enumerate(pts):
                            assert p == want[i], "%s: %s, window %d output %d: %s, the model gives %s" % (op, what, i // n_out, i % n_out, p, want[i])
                        got.append(pts)
                    assert got[0] == got[1] == got[2]


@pytest.mark.parametrize("N", (9, 14))
def test_reduce_tail_rows(N, dc_dev, dc_dec, dc_pools):
    """k_reduce_tail<N> with reduce_t's launch shape: rows [T | W0 | W1 | W2 | W3] against the definition -- X2[hi] = sum_g xin[hi rx + g],
    Y2[lo] = sum_h yin[h L + lo], the digit marginals M_k of X2 (digits 2, 3) and Y2 (digits 0, 1), W_k = sum_v v M_k[v], T = sum Y2 --
    computed from the bigint points.  Digit widths w[k] = (logB + 3 - k) // 4 for logB = 3 (a digit of 0 bits), 5, 12 and 16 (16 values
    in step C, LDS above 48 KB for N = 14); 1, 2-3 and 4 partial sums per value; 1 and 2 windows; generic inputs and one point
    throughout (every tree level doubles).  xin and yin are independent inputs here, so T can only come from yin."""
    pool, rnd = dc_pools[N], random.Random(61 + N)
    fn = getattr(dc_dev, "dc_reduce_tail_%d" % N)
    op = "k_reduce_tail<%d>" % N
    for logB in (3, 5, 12, 16):
        w = [(logB + 3 - k) // 4 for k in range(4)]
        L, H = 1 << (w[0] + w[1]), 1 << (w[2] + w[3])
        for rx, ry in ((1, 1), (2, 3), (4, 4)):
            for nw in (1, 2):
                for equal in (False, True):
                    xpw, ypw = H * rx, L * ry
                    xi = [pool.gen[5]] * (xpw * nw) if equal else _sample(pool, rnd, xpw * nw)
                    yi = [pool.gen[5]] * (ypw * nw) if equal else _sample(pool, rnd, ypw * nw)
                    d_x, d_y, d_rows = dc.to_device(pool.acc[xi]), dc.to_device(pool.acc[yi]), dc.device_zeros(5 * nw, 4 * N)
                    dc.launch(op, fn, d_x.data_ptr(), xpw * nw, d_y.data_ptr(), ypw * nw, rx, ry, xpw, ypw, _u32(w), d_rows.data_ptr(), 5 * nw, nw)
                    rows = dc.from_device(d_rows)
                    what = "logB = %d, rx = %d, ry = %d, nw = %d, %s" % (logB, rx, ry, nw, "one point throughout" if equal else "generic inputs")
                    for k in range(nw):
                        X2 = [dc.msum(N, [pool.pts[xi[k * xpw + hi * rx + g]] for g in range(rx)]) for hi in range(H)]
                        Y2 = [dc.msum(N, [pool.pts[yi[k * ypw + h * L + lo]] for h in range(ry)]) for lo in range(L)]
                        want = [dc.msum(N, Y2)]
                        for dgt in range(4):
                            src, lo_w = (Y2, w[0]) if dgt < 2 else (X2, w[2])
                            M = {}
                            for j, p in enumerate(src):
                                v = (j & ((1 << lo_w) - 1)) if dgt in (0, 2) else (j >> lo_w)
                                M.setdefault(v, []).append(p)
                            assert len(M) == 1 << w[dgt]
                            want.append(dc.msum(N, [dc.mmul(N, v, dc.msum(N, ps)) for v, ps in M.items() if v]))
                        for slot in range(5):
                            dc_dec.check(op, N, rows[5 * k + slot], want[slot], "%s, window %d, %s" % (what, k, "T" if slot == 0 else "W%d" % (slot - 1)))


# ---- the second table: check.hip.hpp, from_x.hip.hpp, scalar_mul.hip.hpp ------------------------------------------------------------
BLOCK_EDGE_COUNTS = (1, 255, 256, 257)


@pytest.mark.parametrize("name", list(dc.OPS2))
def test_second_table_operations_equal_the_host_build(name, dc_host):
    """every operation of the second table (tests/csrc/devcheck_ops2.hpp): the gfx950 compilation gives the host compilation's words bit
    for bit -- on the operation's whole operand set (a few hundred elements, pinned to bigints by tests/test_device_arith_host.py) and on
    1, 255, 256 and 257 elements of it, rotated so that its first operand, an edge of the contract, sits in the last lane of a full block,
    alone in a block, and in a part-filled block"""
    assert dc.device_lib2().dc_table() == dc.host_lib2().dc_table()
    inp = dc.table2_inputs(name)
    sets = [("all %d elements" % len(inp), inp)]
    for n in BLOCK_EDGE_COUNTS:
        reps = -(-n // len(inp)) + 1
        rows = np.roll(np.tile(inp, (reps, 1)), n - 1, axis=0)[:n]
        assert (rows[n - 1] == inp[0]).all()
        sets.append(("%d elements" % n, rows))
    failures = []
    for what, rows in sets:
        got, want = dc.run_device(name, rows), dc.run_host(name, rows)
        try:
            dc.compare_bits("%s, %s" % (name, what), got, want, rows)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)
