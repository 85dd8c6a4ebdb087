"""BLS12-377 G1 (option "curve" = 1) stage by stage and at its edges: digits, the sort, bucket sums and reduction rows against
the bigint model (oracle/model377.py); exceptional multisets of G1 points, non-canonical coordinates and edge scalars through
every entry point; a seeded differential over the options.  The reference holds no vector for this curve, so the model and the
group law are the only pins -- which is why every stage is checked, not just the final point."""
import random

import numpy as np
import pytest

from oracle import model377 as m
from oracle import oracle377 as o
from bls377_decode import ACC, Decoder as _Decoder, psum as _psum

pytestmark = pytest.mark.gpu

Q, R_ORDER = m.Q, m.R_ORDER


def _ctx(pkg, **opts):
    c = pkg.MsmContext((0,))
    c.set_option("curve", pkg.CURVE_BLS12_377_G1)
    for k, v in opts.items():
        c.set_option(k, v)
    return c


def _dev(b):
    import torch
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()


def _pmul(k, pt):
    return m.scalar_mul(k, pt)


def _model_digits(ks, c, W, signed):
    """digit rows [W][n] as the engine stores them: signed digits + 2^(c-1) (model377.decompose_scalar_signed), or the plain
    c-bit windows"""
    if signed:
        return np.array([m.decompose_scalar_signed(k, W, c) for k in ks], dtype=np.int64).T
    return np.array([[(k >> (c * w)) & ((1 << c) - 1) for w in range(W)] for k in ks], dtype=np.int64).T


def _signed_carry(k, c, W):
    """the engine refuses a scalar (TE_MSM_ESCALAR) exactly when W signed windows of c bits cannot hold it: the model's
    "final carry", or bits above the c * W the windows cover"""
    try:
        m.decompose_scalar_signed(k, W, c)
    except ValueError as e:
        assert "final carry" in str(e)
        return True
    return (k >> (c * W)) != 0


# ---------------------------------------------------------------- B1: stage verifiers against the model
@pytest.mark.parametrize("n,c,signed,packed", [(1000, 8, 1, 1), (5003, 13, 1, 1), (20011, 16, 1, 0), (2000, 8, 0, 1)])
def test_stages_against_the_model(pkg, fq377check, n, c, signed, packed):
    pts, sc = o.gen_points(900 + n, n), o.gen_scalars(900 + n, n)
    ks = [int.from_bytes(sc[48 * i:48 * i + 48], "little") for i in range(n)]
    plist = [m.xy_from_bytes(pts[96 * i:96 * i + 96]) for i in range(n)]
    with _ctx(pkg, window_bits=c, signed_digits=signed, sort_buckets=1, packed_sort=packed, prezero=0) as ctx:
        res = ctx.run(pts, sc)
        cb, W = ctx.plan(n)
        assert cb == c
        B = 1 << (c - 1 if signed else c)
        half = B if signed else 0
        nst = (n + 7) & ~7
        dig = np.frombuffer(ctx.debug_read("digits", W * nst * 2), dtype=np.uint16).reshape(W, nst)
        cnt = np.frombuffer(ctx.debug_read("bucket_count", W * B * 4), dtype=np.uint32).reshape(W, B)
        start = np.frombuffer(ctx.debug_read("bucket_start", W * B * 4), dtype=np.uint32).reshape(W, B)
        srt = np.frombuffer(ctx.debug_read("sorted", W * n * 4), dtype=np.uint32).reshape(W, n)
        bk = ctx.debug_read("buckets", W * B * ACC)
        rows = ctx.debug_read("partials", W * 1120)
    # digits
    assert np.all(dig[:, n:] == half), "padding entries must hold the zero digit"
    exp = _model_digits(ks, c, W, signed)
    assert np.array_equal(dig[:, :n].astype(np.int64), exp), "digits differ from the model"
    d_all = exp - half                                   # signed digit values (unsigned: the window itself)
    # counts, starts and the sorted permutation
    for w in range(W):
        d = d_all[w]
        bucket, nz = np.abs(d) - 1, d != 0
        e_cnt = np.bincount(bucket[nz], minlength=B)
        assert np.array_equal(cnt[w], e_cnt), f"window {w} counts"
        assert np.array_equal(start[w], np.concatenate([[0], np.cumsum(e_cnt)[:-1]])), f"window {w} starts"
        used = int(e_cnt.sum())
        ent = srt[w][:used]
        idx, neg = (ent & 0x7FFFFFFF).astype(np.int64), ent >> 31
        assert np.array_equal(np.sort(idx), np.nonzero(nz)[0]), f"window {w}: sorted is not a permutation of the non-zero digits"
        assert np.array_equal(bucket[idx], np.repeat(np.arange(B), e_cnt)), f"window {w}: entry in the wrong bucket"
        assert np.array_equal(neg.astype(bool), d[idx] < 0), f"window {w}: sign bit"
    # bucket sums: (0, 0), (W-1, B-1), an empty bucket and random ones
    dec = _Decoder(fq377check)
    empty = [(int(w), int(b)) for w, b in zip(*np.nonzero(cnt == 0))]
    assert empty, "the plan leaves no bucket empty: pick other parameters"
    rng = np.random.default_rng(n)
    sample = [(0, 0), (W - 1, B - 1), empty[len(empty) // 2]] + [(int(rng.integers(W)), int(rng.integers(B))) for _ in range(7)]
    for w, b in sample:
        got = dec.point(bk[(w * B + b) * ACC:(w * B + b + 1) * ACC])
        d = d_all[w]
        sel = np.nonzero(np.abs(d) - 1 == b)[0]
        e = _psum(plist[i] if d[i] > 0 else m.neg(plist[i]) for i in sel)
        assert got == e, f"bucket ({w},{b}) of {len(sel)} points"
        if cnt[w, b] == 0:
            assert got is None, f"empty bucket ({w},{b}) is not the neutral element"
    # reduction rows [T | W0 | W1 | W2 | W3]
    logB = c - 1 if signed else c
    dw = [(logB + 3 - k) // 4 for k in range(4)]
    for w in (0, W // 2, W - 2):
        got = [dec.point(rows[1120 * w + ACC * k:1120 * w + ACC * (k + 1)]) for k in range(5)]
        d = d_all[w]
        members = {}
        for i in np.nonzero(d)[0]:
            members.setdefault(abs(int(d[i])) - 1, []).append(plist[i] if d[i] > 0 else m.neg(plist[i]))
        S = {b: _psum(v) for b, v in members.items()}
        T = _psum(S.values())
        Wk, sh = [], 0
        for k in range(4):
            M = {}
            for b, s in S.items():
                v = (b >> sh) & ((1 << dw[k]) - 1)
                if v:
                    M.setdefault(v, []).append(s)
            Wk.append(_psum(_pmul(v, _psum(ss)) for v, ss in M.items()))
            sh += dw[k]
        assert got[0] == T, f"window {w}: T"
        for k in range(4):
            assert got[1 + k] == Wk[k], f"window {w}: W{k}"
        V, sh = T, 0
        for k in range(4):
            V = m.add(V, _pmul(1 << sh, Wk[k]))
            sh += dw[k]
        wsc = m.scalars_to_bytes([int(x) % R_ORDER for x in d])
        assert m.result_to_bytes(V) == o.msm(pts, wsc, threads=8), f"window {w}: folded row"
    assert res == o.msm(pts, sc, threads=8)                 # last: a wrong stage above names itself first


# ---------------------------------------------------------------- B2: exceptional multisets of G1 points
def _g1_multiset(seed, n):
    """seeded multiset of G1 points that puts repeats, inverses and sums through the neutral element into buckets"""
    rnd = random.Random(seed)
    base = m.gen_points(seed, 6)
    G = m.G
    mult = [G]
    for _ in range(15):
        mult.append(m.add(mult[-1], G))                                    # [1..16] G
    pts, ks = [], []
    while len(pts) < n:
        kind = rnd.randrange(5)
        P = base[rnd.randrange(len(base))]
        if kind == 0:                                                      # one point many times, equal or small scalars
            k = rnd.randrange(R_ORDER) if rnd.random() < 0.5 else None
            for _ in range(rnd.randrange(20, 300)):
                pts.append(P)
                ks.append(k if k is not None else rnd.randrange(1, 6))
        elif kind == 1:                                                    # P and -P interleaved
            k = rnd.choice([1, 2, 3, rnd.randrange(R_ORDER)])
            for j in range(rnd.randrange(2, 40)):
                pts.append(P if j % 2 == 0 else m.neg(P))
                ks.append(k if rnd.random() < 0.7 else rnd.randrange(1, 5))
        elif kind == 2:                                                    # (P, k) and (P, r - k)
            for _ in range(rnd.randrange(1, 20)):
                k = rnd.randrange(1, R_ORDER)
                pts += [P, P]
                ks += [k, R_ORDER - k]
        else:                                                              # small multiples of G, their inverses, repeats
            for _ in range(rnd.randrange(4, 40)):
                j = rnd.randrange(16)
                pts.append(mult[j] if rnd.random() < 0.6 else m.neg(mult[j]))
                ks.append(rnd.randrange(1, 4))
    return pts[:n], ks[:n]


def _total_infinity(seed, n):
    """sum_i k_i P_i + sum_i (r - k_i) P_i = O, the halves shuffled together"""
    rnd = random.Random(seed)
    P = m.gen_points(seed, n // 2)
    ks = [rnd.randrange(1, R_ORDER) for _ in P]
    pairs = [(p, k) for p, k in zip(P, ks)] + [(p, R_ORDER - k) for p, k in zip(P, ks)]
    rnd.shuffle(pairs)
    return [p for p, _ in pairs], [k for _, k in pairs]


def _every_path(pkg, pb, sb, n, exp, label):
    import torch
    with _ctx(pkg) as ctx:
        for c in (0, 4, 9, 13, 16):
            ctx.set_option("window_bits", c)
            for signed in (1, 0):
                ctx.set_option("signed_digits", signed)
                assert ctx.run(pb, sb) == exp, (label, "run", c, signed)
        ctx.set_option("window_bits", 0)
        ctx.set_option("signed_digits", 1)
        dp, ds = _dev(pb), _dev(sb)
        torch.cuda.synchronize()
        assert ctx.run_device(dp.data_ptr(), ds.data_ptr(), n) == exp, (label, "run_device")
        t = ctx.submit_device(dp.data_ptr(), ds.data_ptr(), n)
        assert ctx.collect(t) == exp, (label, "submit_device")
        for aff in (1, 0):
            ctx.set_option("bind_affine", aff)
            bases = ctx.bind_points(pb)
            try:
                assert ctx.run_scalars(bases, sb) == exp, (label, "bound set", aff)
                ctx.set_option("signed_digits", 0)
                assert ctx.run_scalars(bases, sb) == exp, (label, "bound set, unsigned", aff)
                ctx.set_option("signed_digits", 1)
            finally:
                ctx.release_points(bases)
        ctx.set_option("check_points", 2)
        assert ctx.run(pb, sb) == exp, (label, "check_points 2")


@pytest.mark.parametrize("seed,n", [(1, 40), (2, 200), (3, 3000)])
def test_exceptional_g1_multisets(pkg, seed, n):
    pts, ks = _g1_multiset(seed, n)
    assert all(m.on_curve(p) for p in pts)
    pb, sb = m.points_to_bytes(pts), m.scalars_to_bytes(ks)
    exp = o.msm(pb, sb, threads=8)
    if n <= 200:
        assert exp == m.result_to_bytes(m.msm_naive(pts, ks))
    _every_path(pkg, pb, sb, n, exp, (seed, n))


@pytest.mark.parametrize("n", [2, 64, 2000])
def test_total_is_infinity(pkg, n):
    pts, ks = _total_infinity(40 + n, n)
    pb, sb = m.points_to_bytes(pts), m.scalars_to_bytes(ks)
    exp = o.msm(pb, sb, threads=8)
    assert exp == bytes(96)
    if n <= 200:
        assert m.msm_naive(pts, ks) is m.INF
    _every_path(pkg, pb, sb, n, exp, ("infinity", n))


# ---------------------------------------------------------------- B3: non-canonical coordinates (check_points = 0)
def test_non_canonical_coordinates(pkg):
    """x + k q and y + k q, for every k that keeps the value below 2^384, are other names of the same point"""
    import torch
    n = 400
    pts, sc = o.gen_points(61, n), o.gen_scalars(61, n)
    exp = o.msm(pts, sc, threads=8)
    rnd = random.Random(61)
    top = 1 << 384
    out = []
    for i in range(n):
        x, y = m.xy_from_bytes(pts[96 * i:96 * i + 96])
        kx, ky = (top - 1 - x) // Q, (top - 1 - y) // Q
        mode = i % 4                                                   # 0: canonical, 1: x, 2: y, 3: both
        pick = lambda kmax: [1, 75, kmax, rnd.randint(1, kmax)][(i // 4) % 4] if kmax >= 75 else rnd.randint(1, kmax)
        if mode in (1, 3):
            x += pick(kx) * Q
        if mode in (2, 3):
            y += pick(ky) * Q
        assert x < top and y < top
        out.append(m.le48(x) + m.le48(y))
    shifted = b"".join(out)
    assert max(int.from_bytes(shifted[48 * j:48 * j + 48], "little") for j in range(2 * n)) + Q >= top   # the largest k occurs
    with _ctx(pkg, check_points=0) as ctx:
        for c in (0, 8, 16):
            ctx.set_option("window_bits", c)
            assert ctx.run(shifted, sc) == exp, ("run", c)
        ctx.set_option("window_bits", 0)
        dp, ds = _dev(shifted), _dev(sc)
        torch.cuda.synchronize()
        assert ctx.run_device(dp.data_ptr(), ds.data_ptr(), n) == exp, "run_device"
        for aff in (1, 0):
            ctx.set_option("bind_affine", aff)
            bases = ctx.bind_points(shifted)
            try:
                assert ctx.run_scalars(bases, sc) == exp, ("bound set", aff)
            finally:
                ctx.release_points(bases)


# ---------------------------------------------------------------- B4: edge scalars
def _edge_scalars(c):
    top = (1 << 256) - 1
    every_half = sum((1 << (c - 1)) << (c * w) for w in range(256 // c + 1)) & top
    every_below = sum(((1 << (c - 1)) - 1) << (c * w) for w in range(256 // c + 1)) & top
    return [0, 1, R_ORDER - 1, R_ORDER, R_ORDER + 1, (1 << 253) - 1, 1 << 255, top, every_half, every_below]


@pytest.mark.parametrize("c", [4, 8, 11, 13, 15, 16])
def test_edge_scalars_against_the_model(pkg, c):
    ks_all = _edge_scalars(c)
    n0 = 24
    pts = o.gen_points(70 + c, n0 + len(ks_all))
    rest = [int.from_bytes(b, "little") for b in (o.gen_scalars(70 + c, n0)[48 * i:48 * i + 48] for i in range(n0))]
    plist = [m.xy_from_bytes(pts[96 * i:96 * i + 96]) for i in range(n0 + len(ks_all))]
    with _ctx(pkg, window_bits=c) as ctx:
        for signed in (1, 0):
            ctx.set_option("signed_digits", signed)
            W = ctx.plan(1)[1]
            carry = [signed and _signed_carry(k, c, W) for k in ks_all]
            ok = [k for k, bad in zip(ks_all, carry) if not bad]
            ks = rest + ok
            n = len(ks)
            exp = m.result_to_bytes(m.msm_naive(plist[:n], [k % R_ORDER for k in ks]))
            assert ctx.run(pts[:96 * n], m.scalars_to_bytes(ks)) == exp, (c, signed, "edge scalars")
            for k, bad in zip(ks_all, carry):
                if not bad:
                    e1 = m.result_to_bytes(m.scalar_mul(k % R_ORDER, plist[0]))
                    assert ctx.run(pts[:96], m.scalars_to_bytes([k])) == e1, (c, signed, hex(k))
                    continue
                with pytest.raises(pkg.MsmError) as e:
                    ctx.run(pts[:96 * 4], m.scalars_to_bytes(rest[:3] + [k]))
                assert e.value.code == -3, (c, hex(k))
            if signed and c * W <= 256:
                assert carry[ks_all.index((1 << 256) - 1)], "2^256 - 1 must leave a final carry"


@pytest.mark.parametrize("n", [3000, 70000])
def test_witness_like_scalars(pkg, n):
    """zeros, ones and values below 2^20 among uniform scalars: one bucket of window 0 holds a large share of the points"""
    rnd = random.Random(33)
    sc = bytearray(o.gen_scalars(80 + n, n))
    for i in range(n):
        q = rnd.random()
        if q < 0.5:
            v = 0 if q < 0.2 else 1 if q < 0.4 else rnd.randrange(1 << 20)
            sc[48 * i:48 * i + 48] = m.le48(v)
    sc = bytes(sc)
    pts = o.gen_points(80 + n, n)
    exp = o.msm(pts, sc, threads=8)
    with _ctx(pkg) as ctx:
        for c in (0, 16):
            ctx.set_option("window_bits", c)
            assert ctx.run(pts, sc) == exp, (n, c)
        ctx.set_option("window_bits", 0)
        ctx.set_option("signed_digits", 0)
        assert ctx.run(pts, sc) == exp, (n, "unsigned")


# ---------------------------------------------------------------- B5: random configurations
def test_random_configurations(pkg):
    rnd = random.Random(20261015)
    with _ctx(pkg) as ctx:
        for it in range(30):
            n = rnd.choice([1, 2, 7, 64, 65, 300, 1023, 4096, 5000, 20011, 66000])
            cfg = {"window_bits": rnd.choice([0, 4, 6, 9, 12, 14, 15, 16]), "signed_digits": rnd.choice([0, 1]),
                   "segment_len": rnd.choice([1, 2, 5, 64, 300]), "sort_buckets": rnd.choice([0, 1]), "host_chunks": rnd.choice([0, 1, 2, 5]),
                   "packed_sort": rnd.choice([1, 1, 0]), "fold_pairs": rnd.choice([1, 1, 0]), "prezero": rnd.choice([1, 0])}
            for k, v in cfg.items():
                ctx.set_option(k, v)
            mode = rnd.choice(["uniform", "equal", "small", "witness"])
            pts, sc = o.gen_points(3000 + it, n), o.gen_scalars(3000 + it, n)
            if mode == "equal":
                sc = sc[:48] * n
            elif mode == "small":
                sc = b"".join(sc[48 * i:48 * i + 3] + bytes(45) for i in range(n))
            elif mode == "witness":
                sc = b"".join(sc[48 * i:48 * i + 48] if i % 3 == 0 else m.le48([0, 1, i & 0xFFFFF][i % 3]) for i in range(n))
            assert ctx.run(pts, sc) == o.msm(pts, sc, threads=8), (it, n, cfg, mode)


# ---------------------------------------------------------------- B6: bucket-shape extremes at 14 limbs
def test_many_parts_per_bucket(pkg):
    """segment length 1 with 64 buckets a window: thousands of parts per bucket for the giant-bucket combine"""
    n = 150001
    pts, sc = o.gen_points(95, n), o.gen_scalars(95, n)
    with _ctx(pkg, window_bits=7, segment_len=1) as ctx:
        assert ctx.run(pts, sc) == o.msm(pts, sc, threads=8)


def test_schedule_slices_beyond_the_register_form(pkg):
    """n = 2^19 in segments of one or two entries: more than 64 x 8192 segment ids per window, the two-pass schedule"""
    n = 1 << 19
    pts, sc = o.gen_points(96, n), o.gen_scalars(96, n)
    exp = o.msm(pts, sc, threads=8)
    with _ctx(pkg, window_bits=16) as ctx:
        for seg in (1, 2):
            ctx.set_option("segment_len", seg)
            assert ctx.run(pts, sc) == exp, seg
