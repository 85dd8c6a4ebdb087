"""GPU parity of k_accumulate's segment start (csrc/kernels.hip.hpp): the first two entries of a segment are added as records
(ete_from_pair), a single entry is converted, a segment that continues a bucket takes neither; the loop behind it consumes two
entries per pass from entry 0 or 2 on, refills its index strip every 16 entries, and ends in a tail of one or two.  Shapes are the
smallest at which that can go wrong: 4-bit windows and equal scalars put all n entries in ONE bucket per window, and segment_len 64
(checked through `segment_len_used`) gives that bucket to ONE thread, so n is the segment's length.  (Left to itself the plan cuts
these buckets into parts of 16: no in-loop refill ever runs; that geometry is run once as well.)  Every result against the oracle,
as tests/test_gpu_parity.py does."""
import pytest

from oracle import model377 as m377
from oracle import oracle377 as o377

pytestmark = pytest.mark.gpu

# cnt = 1 (conversion), 2 (the pair alone), 3 (pair + a tail of one), 4 (a tail of two), 5 (one pass), and every alignment of
# the in-loop strip refill with the loop entered at entry 2: the refill falls due in the pass of entries 14 / 30 (pn = 16 / 32),
# which runs from cnt = 17 / 33 on -- with one or two entries (17, 18) or a whole strip (31, 32) behind the first, one (33) behind the
# second; 14, 15 and 16 end just in front of it
SIZES = [1, 2, 3, 4, 5, 14, 15, 16, 17, 18, 31, 32, 33]
POS, NEG = 3, 13             # 4-bit signed windows: 3 -> digit +3; 13 -> digit -3 and a carry (digit +1 in window 1)
ONE_THREAD = 64              # segment_len: every bucket of this file (at most 33 entries) is one segment


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.MsmContext((0,))
    c.set_option("window_bits", 4)
    c.set_option("segment_len", ONE_THREAD)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pts99(ora):
    return ora.gen_points(0xB0C, 99)


@pytest.fixture(scope="module")
def pts33(pts99):
    return pts99[:64 * 33]


def _check(c, o, pts, sc, seg, what):
    got = c.run(pts, sc)
    assert c.get_option("segment_len_used") == seg, what
    assert got == o.msm(pts, sc, threads=2), what


def _scalars(model, pattern, n):
    return model.scalars_to_bytes([pattern[i % len(pattern)] for i in range(n)])


@pytest.mark.parametrize("pattern", [(POS,), (NEG,), (POS, NEG), (NEG, POS)], ids=["plus", "minus", "plus-minus", "minus-plus"])
def test_one_bucket_of_every_length_and_sign_pattern(ctx, model, ora, pts33, pattern):
    """all digits equal, all negative, and alternating signs starting with either (first or second entry of the pair negated)"""
    for n in SIZES:
        _check(ctx, ora, pts33[:64 * n], _scalars(model, pattern, n), ONE_THREAD, n)


def test_one_bucket_in_the_plan_s_own_parts(ctx, model, ora, pts33):
    """segment_len from n (16 here): parts of 16 + 1, 16 + 2, 16 + 15, 16 + 16 + 1 -- each part starts with its own pair or
    conversion, k_seg_combine_all sums them"""
    ctx.set_option("segment_len", 0)
    try:
        for n in SIZES:
            _check(ctx, ora, pts33[:64 * n], _scalars(model, (POS, NEG), n), 16, n)
    finally:
        ctx.set_option("segment_len", ONE_THREAD)


def test_doubling_and_inverse_in_the_pair(ctx, model, ora, pts33):
    """the complete formula's cases at the start of a bucket: two equal points, and P followed by -P, alone (n = 2: whichever order
    the sort leaves them in) and in front of further entries"""
    p0 = model.xy_from_bytes(pts33[:64])
    same, inverse = model.points_to_bytes([p0, p0]), model.points_to_bytes([p0, model.neg(p0)])
    for head in (same, inverse):
        for n in (2, 3, 4, 17):
            pts = head + pts33[64 * 2:64 * n]
            for pattern in ((POS,), (NEG,), (POS, NEG)):
                sc = _scalars(model, pattern, n)
                _check(ctx, ora, pts, sc, ONE_THREAD, (n, pattern))
    # P with digit +3 and P with digit -3 are P and -P in the bucket as well
    pts, sc = same, model.scalars_to_bytes([POS, NEG])
    _check(ctx, ora, pts, sc, ONE_THREAD, "P, -P by digit")


@pytest.mark.parametrize("n", [9, 10])
def test_split_bucket_with_a_short_last_part(ctx, model, ora, pts33, n):
    """segment_len 4: parts of 4, 4 and 1 (a conversion) or 2 (the pair alone), summed by k_seg_combine_all"""
    ctx.set_option("segment_len", 4)
    try:
        for pattern in ((POS,), (POS, NEG)):
            pts, sc = pts33[:64 * n], _scalars(model, pattern, n)
            _check(ctx, ora, pts, sc, 4, pattern)
    finally:
        ctx.set_option("segment_len", ONE_THREAD)


@pytest.mark.parametrize("chunks", [2, 3])
def test_later_pieces_continue_the_bucket(ctx, model, ora, pts99, chunks):
    """a host buffer in equal pieces over one bucket: part 0 of every later piece continues the bucket's sum (`onto`) and must add
    ALL its entries to it, from entry 0 on -- later pieces of 1, 2 and 3 entries, and of 17, 18 and 33: the continuation across the
    in-loop strip refill (pn = 16, 32) with one or two entries behind it"""
    ctx.set_option("host_chunks", chunks)
    try:
        for piece in (1, 2, 3, 17, 18, 33):
            n = chunks * piece
            for pattern in ((POS,), (NEG, POS)):
                _check(ctx, ora, pts99[:64 * n], _scalars(model, pattern, n), ONE_THREAD, (n, pattern))
        n = 35                                               # unequal pieces: 17 + 18, or 11 + 12 + 12
        _check(ctx, ora, pts99[:64 * n], _scalars(model, (POS, NEG), n), ONE_THREAD, n)
    finally:
        ctx.set_option("host_chunks", 0)


def test_bls12_377_both_record_kinds(pkg):
    """the projective record of a per-call MSM (its start is a conversion and an addition, as before) and the affine record of bound
    bases (pair start), one bucket of every length class"""
    sizes = [1, 2, 3, 4, 17, 18, 33]
    pts = o377.gen_points(0xB0C, 33)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        c.set_option("window_bits", 4)
        c.set_option("segment_len", ONE_THREAD)
        for n in sizes:
            sc = m377.scalars_to_bytes([(POS, NEG)[i % 2] for i in range(n)])
            want = o377.msm(pts[:96 * n], sc, threads=2)
            assert c.run(pts[:96 * n], sc) == want, n
            assert c.get_option("segment_len_used") == ONE_THREAD, n
            b = c.bind_points(pts[:96 * n])
            try:
                assert c.run_scalars(b, sc) == want, n
                assert c.get_option("segment_len_used") == ONE_THREAD, n
            finally:
                c.release_points(b)
