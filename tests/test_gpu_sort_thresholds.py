"""The bucket sort and the segment plan at their exact thresholds (csrc/kernels.hip.hpp: k_part_scatter, k_l2_local, l2_piece_of_block,
seg_plan_block, k_l2_place_order with order_scatter_block, l2_place_piece, k_seg_combine_all), on histograms written by hand
(tests/sort_cases.py): scalars d1 * 2^c + d0 choose every bucket count of window 0, window 1 is seeded, the windows above are empty.

  (a) a level-1 partition of 9207 / 9208 / 9209 / 18416 / 18417 / 27625 entries (TE_L2_CAP = 9208: 1, 1, 2, 2, 3 and 4 pieces) at the
      first, a middle and the last position of the window, starting at 0, 1 and 7 mod 8 (a piece's 16-byte loads start at a & ~7),
      beside an empty partition (the first, the last, the one in front, the one behind)
  (b) buckets of 1, 1, 1, 2, 16, 17, 256, 257, 512 and 513 parts (TE_COMBINE_SMALL = 16, TE_GIANT_RUN = 256) in one partition of
      128 buckets, spread over 13-bit partitions with two giants and the 16-part bucket sharing one, and with plain windows
  (c) segments of 1023, 1024 and 1500 entries: lengths above 1023 share one slot of the schedule's histogram
Every case reads the stages back through oracle/stage_checks.py: check_sort_plan, decodes the named buckets against the bigint model
and compares the result with the oracle bit for bit, on both curves; one case of (a) and of (b) per curve also goes through a bound
point set, plain and indexed.  The functions without the gpu mark check the cases and the checker themselves and need no device."""
import numpy as np
import pytest

import sort_cases as sc
from oracle import model
from oracle.stage_checks import check_sort_plan, decode_te_bucket

gpu = pytest.mark.gpu
CURVES = [sc.TE, sc.G1]
ACC_BYTES = {sc.TE: 144, sc.G1: 224}


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


# ================================================================ no device: the cases are what they claim
def test_partition_cases_cross_every_threshold_position_and_alignment():
    cases = [sc.partition_case(*k) for k in sc.A_CASES]
    assert [x.T for x in cases] == [9207, 9208, 9209, 18416, 18417, 27625]
    assert {x.pos for x in cases} == {0, 5, 7, 15} and {x.align for x in cases} == {0, 1, 7}
    assert {(x.T, x.align) for x in cases} >= {(9209, 7), (18417, 7)}
    assert {x.empty for x in cases} >= {0, 15} and any(x.empty == x.pos - 1 for x in cases) and any(x.empty == x.pos + 1 for x in cases)
    assert [x.pieces for x in cases] == [1, 1, 2, 2, 3, 4]
    assert all(x.d0.min() == -4096 for x in cases if x.pos == 15), "the last partition's last bucket is reached by -2^(c-1) alone"
    assert all(k in sc.A_CASES for k in sc.A_CASES_G1)
    for x in cases:                                         # the default segment length makes the heaviest bucket a giant one
        assert x.counts.max() > sc.COMBINE_SMALL * sc.default_segment_len(x.n, x.B)


@pytest.mark.parametrize("form", list(sc.B_FORMS))
def test_parts_cases_hold_the_named_buckets(form):
    case = sc.parts_case(form)
    S = sc.geometry(case.c, case.signed)[1]
    assert [int(case.counts[b]) for _, b in case.named.values()] == sc.B_COUNTS
    assert S == (128 if form == "c8" else 256)


def test_clamp_case_holds_one_long_bucket():
    case = sc.clamp_case()
    assert int(case.counts[40]) == 3000 and int(case.counts[41]) == 0 and np.sort(case.counts)[-2] <= 3


ALL_CASES = [("partition", k) for k in sc.A_CASES] + [("parts", f) for f in sc.B_FORMS] + [("clamp", "clamp")]
G1_CASES = [("partition", k) for k in sc.A_CASES_G1] + [("parts", f) for f in sc.B_FORMS] + [("clamp", "clamp")]


@pytest.mark.parametrize("curve,kind,key", [(sc.TE,) + x for x in ALL_CASES] + [(sc.G1,) + x for x in G1_CASES], ids=_id)
def test_scalars_decompose_into_the_requested_digits(ora, curve, kind, key):
    """the oracle's (Twisted-Edwards) and the model's (BLS12-377) own decomposition give (d0, d1, 0, 0, ...) back"""
    case, scal, rows = sc.inputs(curve, kind, key)
    assert rows.shape == (sc.windows(case.c, case.signed), case.n) and len(scal) == (32, 48)[curve] * case.n
    assert np.array_equal(rows[0], case.d0) and not rows[2:].any()
    nz = case.d0[case.d0 != 0]
    assert np.array_equal(np.bincount(np.abs(nz) - 1, minlength=case.B), case.counts)


# ================================================================ no device: the checker accepts the documented layout, refuses mistakes
def _model_of(kind, key, seg_len):
    case, _, rows = sc.inputs(sc.TE, kind, key)
    return case, rows, sc.PlanModel(rows, case.n, case.c, case.signed, seg_len)


def _refused(ctx, rows, case, what):
    with pytest.raises(AssertionError):
        check_sort_plan(ctx, rows, case.n, case.c, case.signed, len(rows))
        pytest.fail("the checker accepted: " + what, pytrace=False)


def test_checker_on_a_partition_of_9209():
    case, rows, ctx = _model_of("partition", (9209, 5, 7, 4), 16)
    info = check_sort_plan(ctx, rows, case.n, case.c, case.signed, len(rows))
    assert info.part_count[0][5] == 9209 and info.part_start[0][5] % 8 == 7 and info.part_count[0][4] == 0
    # an expected count off by one: one entry of p* expected in the partition behind it
    wrong = rows.copy()
    i = int(np.nonzero(np.abs(wrong[0]) - 1 == 5 * 256 + 100)[0][0])
    wrong[0][i] = 6 * 256 + 1
    _refused(ctx, wrong, case, "9208 entries expected where the partition holds 9209")
    # a multi-piece partition may list a bucket's entries in any order of sign; a partition sorted whole may not
    srt = ctx.arrays["sorted"]
    lo = int(info.bucket_start[0][5 * 256 + 100])
    hi = lo + int(info.bucket_count[0][5 * 256 + 100]) - 1
    assert srt[0, lo] >> 31 == 0 and srt[0, hi] >> 31 == 1
    srt[0, lo], srt[0, hi] = srt[0, hi], srt[0, lo]
    check_sort_plan(ctx, rows, case.n, case.c, case.signed, len(rows))
    w1 = ctx.arrays["sorted"][1]                          # window 1: every partition whole, every digit positive -- flip one sign
    w1[0] |= 0x80000000
    _refused(ctx, rows, case, "a wrong sign bit")
    w1[0] &= 0x7FFFFFFF
    # an id between a partition's last segment and the next partition's base left valid
    gap = int(np.nonzero(ctx.arrays["seg_len"][:info.cap_w] == 0xFFFFFFFF)[0][0])
    ctx.arrays["seg_len"][gap] = ctx.arrays["seg_bucket"][gap] = 0
    _refused(ctx, rows, case, "a stale id between two partitions")


def test_checker_on_positive_first():
    case, rows, ctx = _model_of("parts", "c8", sc.B_SEG)
    info = check_sort_plan(ctx, rows, case.n, case.c, case.signed, len(rows))
    lo = int(info.bucket_start[0][64])                      # 65 entries: 33 positive ones, then 32 negative ones
    srt = ctx.arrays["sorted"]
    srt[0, lo + 32], srt[0, lo + 33] = srt[0, lo + 33], srt[0, lo + 32]
    _refused(ctx, rows, case, "a negative entry in front of a positive one in a partition sorted whole")


def test_checker_on_a_bucket_of_17_parts():
    case, rows, ctx = _model_of("parts", "c8", sc.B_SEG)
    info = check_sort_plan(ctx, rows, case.n, case.c, case.signed, len(rows))
    assert [int(info.parts[0][b]) for _, b in case.named.values()] == sc.B_PARTS
    # the 17-part bucket planned as 16 parts: its last segment record missing
    a = ctx.arrays
    last = int(np.nonzero(a["seg_bucket"] == 64)[0][-1])
    assert a["seg_len"][last] == 1
    a["seg_len"][last] = a["seg_bucket"][last] = 0xFFFFFFFF
    a["order"] = a["order"][a["order"] != last]
    a["num_segments"][0] -= 1
    _refused(ctx, rows, case, "16 segments for a bucket of 65 entries in segments of 4")


def test_checker_on_lengths_above_1023():
    case, rows, ctx = _model_of("clamp", "clamp", 1500)
    check_sort_plan(ctx, rows, case.n, case.c, case.signed, len(rows))
    # segments of 1800 and 1200 entries share the histogram's last slot: either order is the kernel's, an unclamped comparison is wrong
    ctx = sc.PlanModel(rows, case.n, case.c, case.signed, 1800)
    order = ctx.arrays["order"]
    lens = [int(ctx.arrays["seg_len"][i]) for i in order[:3]]
    assert lens[:2] == [1800, 1200] and lens[2] < 100
    order[0], order[1] = order[1], order[0]
    check_sort_plan(ctx, rows, case.n, case.c, case.signed, len(rows))
    order[1], order[2] = order[2], order[1]
    _refused(ctx, rows, case, "a short segment scheduled before one of 1800 entries")


# ================================================================ on the device
@pytest.fixture(scope="module")
def contexts(pkg):
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = pkg.MsmContext((0,))
            made[curve].set_option("curve", curve)
        return made[curve]
    yield get
    for c in made.values():
        c.close()


@pytest.fixture(scope="module")
def decode(model, fq377check):
    from bls377_decode import Decoder
    g1 = Decoder(fq377check)

    def point(curve, raw):
        """affine point of an accumulator, in the form sort_cases.bucket_sum returns it"""
        return decode_te_bucket(model, raw) if curve == sc.TE else g1.point(raw)
    return point


def _run(ctx, curve, kind, key, decode, seg_len=None, packed=1):
    """runs the case whole with the stages kept, checks digits, sort, plan, the named buckets' sums and the result; returns what
    check_sort_plan read"""
    case = sc.inputs(curve, kind, key)[0]
    seg_len = case.seg_len if seg_len is None else seg_len
    for k, v in (("window_bits", case.c), ("signed_digits", int(case.signed)), ("segment_len", seg_len), ("packed_sort", packed),
                 ("prezero", 0), ("sort_buckets", 1), ("host_chunks", 1)):
        ctx.set_option(k, v)
    n = case.n
    cb, W = ctx.plan(n)
    assert cb == case.c
    case, scal, rows = sc.inputs(curve, kind, key, W)
    res = ctx.run(sc.points_of(curve, n), scal)
    assert ctx.get_option("segment_len_used") == (seg_len or sc.default_segment_len(n, case.B))
    half, nst = (case.B if case.signed else 0), (n + 7) & ~7
    dig = np.frombuffer(ctx.debug_read("digits", W * nst * 2), dtype=np.uint16).reshape(W, nst)
    assert np.all(dig[:, n:] == half) and np.array_equal(dig[:, :n].astype(np.int64) - half, rows), "digits"
    info = check_sort_plan(ctx, rows, n, case.c, case.signed, W)
    assert not info.bucket_count[2:].any(), "the windows above the second are empty"
    acc = ACC_BYTES[curve]
    bk = ctx.debug_read("buckets", case.B * acc)              # window 0
    for name, (w, b) in case.named.items():
        e, members = sc.bucket_sum(curve, kind, key, w, b)
        assert members == case.counts[b] == info.bucket_count[w][b]
        assert decode(curve, bk[b * acc:(b + 1) * acc]) == e, f"sum of bucket {b} ({name}: {members} entries, {int(info.parts[w][b])} parts)"
        if members == 0:
            assert e == (model.ZERO if curve == sc.TE else None)
    assert res == sc.want(curve, kind, key), "result"
    print(f"\ncurve {curve} {kind} {key} seg_len {info.seg_len} packed {packed}: n = {n}, W = {W}, num_segments = {info.num_segments}, named parts = "
          f"{[int(info.parts[w][b]) for w, b in case.named.values()]}")
    return case, info


@gpu
@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("key", sc.A_CASES, ids=_id)
def test_partition_totals(contexts, decode, key, packed):
    _partition(contexts(sc.TE), sc.TE, key, decode, packed)


@gpu
@pytest.mark.parametrize("packed", [1, 0])
@pytest.mark.parametrize("key", sc.A_CASES_G1, ids=_id)
def test_partition_totals_bls377(contexts, decode, key, packed):
    _partition(contexts(sc.G1), sc.G1, key, decode, packed)


def _partition(ctx, curve, key, decode, packed):
    case, info = _run(ctx, curve, "partition", key, decode, packed=packed)
    T, pos, align, empty = key
    assert info.part_count[0][pos] == T and -(-int(info.part_count[0][pos]) // sc.L2_CAP) == case.pieces == sc.A_PIECES[T]
    assert info.part_start[0][pos] % 8 == align and info.part_count[0][empty] == 0
    assert info.seg_len == 16 and info.parts[0][case.named["heaviest"][1]] > sc.COMBINE_SMALL
    print(f"  part_count[0][{pos}] = {info.part_count[0][pos]}, pieces = {case.pieces}, part_start % 8 = {info.part_start[0][pos] % 8}, "
          f"runs of the heaviest bucket = {-(-int(info.parts[0][case.named['heaviest'][1]]) // sc.GIANT_RUN)}")


@gpu
@pytest.mark.parametrize("form", list(sc.B_FORMS))
@pytest.mark.parametrize("curve", CURVES)
def test_parts_per_bucket(contexts, decode, curve, form):
    case, info = _run(contexts(curve), curve, "parts", form, decode)
    assert info.seg_len == sc.B_SEG and info.S == (128 if form == "c8" else 256)
    assert [int(info.parts[w][b]) for w, b in case.named.values()] == sc.B_PARTS
    for (w, b), parts in zip(case.named.values(), sc.B_PARTS):
        ids = np.nonzero(info.seg_bucket == w * case.B + b)[0]
        assert ids.size == parts and np.array_equal(ids, np.arange(ids[0], ids[0] + parts)), "a bucket's segments have consecutive ids"


@gpu
@pytest.mark.parametrize("seg_len", sc.C_SEG)
@pytest.mark.parametrize("curve", CURVES)
def test_segment_lengths_around_the_clamp(contexts, decode, curve, seg_len):
    case, info = _run(contexts(curve), curve, "clamp", "clamp", decode, seg_len=seg_len)
    ids = np.nonzero(info.seg_bucket == 40)[0]
    assert [int(x) for x in info.seg_lens[ids]] == {1023: [1023, 1023, 954], 1024: [1024, 1024, 952], 1500: [1500, 1500]}[seg_len]
    top = sorted(int(x) for x in info.order[:2])
    assert top == [int(ids[0]), int(ids[1])], "the two longest segments lead the schedule"


@gpu
@pytest.mark.parametrize("kind,key", [("partition", None), ("parts", "c8")], ids=["partition", "parts"])
@pytest.mark.parametrize("curve", CURVES)
def test_bound_set_plain_and_indexed(contexts, curve, kind, key):
    """the same histograms through the record kind of a bound set (BLS12-377: affine records) and through k_part_scatter_indexed: a
    permutation of 0..n-1 over scalars permuted to match is the same sum"""
    key = key or {sc.TE: (18417, 15, 7, 14), sc.G1: (9209, 5, 7, 4)}[curve]
    ctx = contexts(curve)
    case, scal, _ = sc.inputs(curve, kind, key)
    for k, v in (("window_bits", case.c), ("signed_digits", int(case.signed)), ("segment_len", case.seg_len), ("packed_sort", 1), ("bind_affine", 1)):
        ctx.set_option(k, v)
    want, sb = sc.want(curve, kind, key), len(scal) // case.n
    perm = np.random.default_rng(case.n).permutation(case.n).astype(np.uint32)
    permuted = b"".join(scal[sb * int(i):sb * int(i) + sb] for i in perm)
    bases = ctx.bind_points(sc.points_of(curve, case.n))
    try:
        assert ctx.run_scalars(bases, scal) == want, "bound set"
        assert ctx.run_scalars_indexed(bases, perm, permuted) == want, "indexed"
    finally:
        ctx.release_points(bases)
