"""GPU parity of k_accumulate's sign state (csrc/kernels.hip.hpp: an entry's sign is carried in the lane's accumulator -- negated where
the sign changes, inside a branch -- and the record is added as loaded; the segment's last addition closes into the true sign) and of
the placement that goes with it (k_l2_local puts a bucket's positive entries in front of its negative ones).

One thread, one bucket, as tests/test_gpu_bucket_start.py builds it: 4-bit windows and scalars of one magnitude put all n entries in
ONE bucket per window, and segment_len 64 (checked through `segment_len_used`) gives that bucket to ONE thread, so n is the segment's
length and the number of positive scalars is the position of its one sign change -- the pair start (entries 0, 1), every pass of the
loop, the strip refills (entries 16, 32) and the tail of one or two.  Orders the sort does not produce (negative before positive,
alternating) reach the kernel through the pieces of an over-long partition, which keep arrival order (test_pieces_* below), and every
pattern of up to six entries is checked on the host build of the same code (tests/test_sign_state_host.py).
Every result bit for bit against the oracle."""
import numpy as np
import pytest

from oracle import model377 as m377
from oracle import oracle377 as o377

pytestmark = pytest.mark.gpu

POS, NEG = 3, 13             # 4-bit signed windows: 3 -> digit +3; 13 -> digit -3 and a carry (digit +1 in window 1)
ONE_THREAD = 64              # segment_len: every bucket of the one-thread tests (at most 33 entries) is one segment
SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.MsmContext((0,))
    c.set_option("window_bits", 4)
    c.set_option("segment_len", ONE_THREAD)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pts99(ora):
    return ora.gen_points(0x51C4, 99)


def _check(c, o, pts, sc, seg, what):
    got = c.run(pts, sc)
    assert c.get_option("segment_len_used") == seg, what
    assert got == o.msm(pts, sc, threads=2), what


def _scalars(model, pattern, n):
    return model.scalars_to_bytes([pattern[i % len(pattern)] for i in range(n)])


@pytest.mark.parametrize("pattern", [(POS,), (NEG,), (POS, NEG), (NEG, POS)], ids=["plus", "minus", "plus-minus", "minus-plus"])
def test_one_bucket_all_of_one_sign_and_alternating(ctx, model, ora, pts99, pattern):
    """never flipped, flipped from the first entry to the store, and half of each (the change in the middle of the segment)"""
    for n in SIZES:
        _check(ctx, ora, pts99[:64 * n], _scalars(model, pattern, n), ONE_THREAD, n)


@pytest.mark.parametrize("n", [6, 17, 33])
def test_one_sign_change_at_every_position(ctx, model, ora, pts99, n):
    """k positive entries, then n - k negative ones, for every k: the change falls on the pair (k = 1), on the first and the second
    addition of a pass, on the strip refills (k = 16, 32 with n = 33; k = 16 with n = 17) and on either addition of the tail"""
    for k in range(n + 1):
        sc = model.scalars_to_bytes([POS] * k + [NEG] * (n - k))
        _check(ctx, ora, pts99[:64 * n], sc, ONE_THREAD, (n, k))


def test_sorted_entries_have_the_positive_ones_first(ctx, model, pts99):
    """what the cases above rely on: the one bucket of window 0 lists its k positive entries, then the negative ones"""
    n, k = 33, 16
    sc = model.scalars_to_bytes([NEG if i % 2 else POS for i in range(2 * k)] + [NEG] * (n - 2 * k))
    ctx.set_option("prezero", 0)
    try:
        ctx.run(pts99[:64 * n], sc)
        ent = np.frombuffer(ctx.debug_read("sorted", n * 4), dtype=np.uint32)         # window 0: one bucket (digit 3), n entries
    finally:
        ctx.set_option("prezero", 1)
    assert sorted(int(e) & 0x7FFFFFFF for e in ent) == list(range(n))
    assert [int(e) >> 31 for e in ent] == [0] * k + [1] * (n - k)


@pytest.mark.parametrize("chunks", [2, 3])
def test_later_pieces_continue_the_bucket_unflipped(ctx, model, ora, pts99, chunks):
    """a host buffer in equal pieces over one bucket: part 0 of every later piece continues the bucket's sum (`onto`) -- it starts
    unflipped whatever sign the piece before ended in, flips at its first entry if that one is negative, and stores the true sum.
    Pieces of 1, 2, 3, 17 and 33 entries; all negative, and positive entries first"""
    ctx.set_option("host_chunks", chunks)
    try:
        for piece in (1, 2, 3, 17, 33):
            n = chunks * piece
            for pattern in ((NEG,), (POS, NEG), (POS, POS, NEG)):
                _check(ctx, ora, pts99[:64 * n], _scalars(model, pattern, n), ONE_THREAD, (n, pattern))
    finally:
        ctx.set_option("host_chunks", 0)


def test_bls12_377_both_record_kinds(pkg):
    """the projective record of a per-call MSM and the affine record of bound bases: all negative, and a sign change at every
    position of a segment of 6 and at the strip refill of one of 18 and of 33"""
    pts = o377.gen_points(0x51C4, 33)
    cases = [(1, 0), (2, 0), (3, 0)] + [(6, k) for k in range(1, 6)] + [(18, 16), (33, 32), (33, 0)]
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        c.set_option("window_bits", 4)
        c.set_option("segment_len", ONE_THREAD)
        for n, k in cases:
            sc = m377.scalars_to_bytes([POS] * k + [NEG] * (n - k))
            want = o377.msm(pts[:96 * n], sc, threads=2)
            assert c.run(pts[:96 * n], sc) == want, (n, k)
            assert c.get_option("segment_len_used") == ONE_THREAD, (n, k)
            b = c.bind_points(pts[:96 * n])
            try:
                assert c.run_scalars(b, sc) == want, (n, k)
            finally:
                c.release_points(b)


# ------------------------------------------------------------------ the sort: positive entries first
def _positive_first(ctx, n, c):
    """in every bucket of a partition that was not cut into pieces no negative entry stands before a positive one"""
    W, B = (256 + c - 1) // c, 1 << (c - 1)
    cnt = np.frombuffer(ctx.debug_read("bucket_count", W * B * 4), dtype=np.uint32).reshape(W, B).astype(np.int64)
    start = np.frombuffer(ctx.debug_read("bucket_start", W * B * 4), dtype=np.uint32).reshape(W, B).astype(np.int64)
    srt = np.frombuffer(ctx.debug_read("sorted", W * n * 4), dtype=np.uint32).reshape(W, n)
    S = min(B, 256)
    whole = cnt.reshape(W, B // S, S).sum(axis=2) <= 9208                  # TE_L2_CAP: a larger partition is sorted in pieces
    checked = 0
    for w in range(W):
        used = int(cnt[w].sum())
        neg = (srt[w][:used] >> 31).astype(np.int8)
        # a negative entry followed by a positive one may only happen across a bucket boundary
        bad = np.nonzero((neg[:-1] == 1) & (neg[1:] == 0))[0] + 1
        firsts = set(int(s) for s in start[w])
        for pos in bad:
            if int(pos) in firsts:
                continue
            b = int(np.searchsorted(start[w], pos, side="right")) - 1
            assert not whole[w][b // S], f"window {w} bucket {b}: a negative entry in front of a positive one at {pos}"
        checked += int(whole[w].sum())
    assert checked > 0


@pytest.mark.parametrize("n,c", [(5003, 13), (70001, 16)])
def test_sorted_buckets_list_positive_entries_first(pkg, ora, n, c):
    pts, sc = ora.gen_points(500 + n, n), ora.gen_scalars(500 + n, n)
    with pkg.MsmContext((0,)) as x:
        x.set_option("window_bits", c)
        x.set_option("prezero", 0)
        assert x.run(pts, sc) == ora.msm(pts, sc, threads=8)
        _positive_first(x, n, c)


@pytest.fixture(scope="module")
def pts12k(ora):
    return ora.gen_points(0x51C5, 12000)


def test_pieces_of_one_giant_bucket_keep_any_order(pkg, model, ora, pts12k):
    """8-bit windows, digits +3 and -3 alternating: one bucket of window 0 holds all 12 000 entries, its partition is sorted in two
    pieces placed in arrival order by k_l2_place_order -- the segments meet sign changes in any order and number; then all-equal
    scalars (one giant bucket in every window)"""
    n = 12000
    with pkg.MsmContext((0,)) as x:
        x.set_option("window_bits", 8)
        x.set_option("prezero", 0)
        for ks in ([3, 256 - 3], [0x0123456789ABCDEF0123456789ABCDEF]):
            sc = model.scalars_to_bytes([ks[i % len(ks)] for i in range(n)])
            assert x.run(pts12k, sc) == ora.msm(pts12k, sc, threads=8)
            if len(ks) == 2:
                # the case is what it claims to be: window 0's entries are not all positive-first
                neg = np.frombuffer(x.debug_read("sorted", n * 4), dtype=np.uint32) >> 31
                assert int(neg.sum()) == n // 2 and np.any((neg[:-1] == 1) & (neg[1:] == 0))


def test_witness_mix(pkg, model, ora, pts12k):
    """zeros, ones and small values among uniform scalars: bucket 0 of window 0 is giant (pieces), the rest ordinary"""
    n = 12000
    rnd = np.random.RandomState(31)
    ks = model.gen_scalars(n, n)
    for i in range(n):
        q = rnd.random_sample()
        if q < 0.5:
            ks[i] = 0 if q < 0.1 else 1 if q < 0.4 else int(rnd.randint(1 << 20))
    sc = model.scalars_to_bytes(ks)
    with pkg.MsmContext((0,)) as x:
        assert x.run(pts12k, sc) == ora.msm(pts12k, sc, threads=8)


@pytest.mark.parametrize("opts", [{"signed_digits": 0}, {"sort_buckets": 0}], ids=["unsigned", "unscheduled"])
def test_unsigned_digits_and_natural_order(pkg, ora, pts12k, opts):
    """unsigned digits never flip; sort_buckets = 0 runs the segments in natural order -- n = 3000"""
    n = 3000
    pts, sc = pts12k[:64 * n], ora.gen_scalars(0x51C6, n)
    with pkg.MsmContext((0,)) as x:
        for k, v in opts.items():
            x.set_option(k, v)
        assert x.run(pts, sc) == ora.msm(pts, sc, threads=8)
