"""Engineered histograms for the bucket sort and the segment plan (tests/test_gpu_sort_thresholds.py).  A plain module.

A scalar s = d1 * 2^c + d0 with d0 in [-2^(c-1), 2^(c-1) - 1] and d1 >= 1 has the signed digits (d0, d1, 0, 0, ...); with plain windows
d0 and d1 are the two low windows themselves.  So a case WRITES window 0's histogram -- every bucket count, hence every partition total
and start -- chooses window 1 as well and leaves every higher window empty.  A digit value d != 0 is an entry of bucket |d| - 1.

digit_row        a list of bucket counts -> one window's digit values in seeded shuffled order, signs alternating inside a bucket
scalars_of       two digit rows -> scalars, checked through the oracle's / the model's own decomposition (decompose)
partition_case   (a) one level-1 partition of exactly T entries at a chosen position and start alignment
parts_case       (b) buckets of 1, 1, 1, 2, 16, 17, 256, 257, 512 and 513 parts
clamp_case       (c) one bucket of 3000 entries for segment lengths around 1023
PlanModel        the documented layout of the sort and plan arrays computed from the digits: what the checker of oracle/stage_checks.py
                 must accept, and the base of the mutations it must refuse (the checker's own test, no GPU)
"""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import model, model377, oracle, oracle377

L2_CAP = 9208              # TE_L2_CAP
COMBINE_SMALL = 16         # TE_COMBINE_SMALL
GIANT_RUN = 256            # TE_GIANT_RUN
TE, G1 = 0, 1              # option "curve"
MODEL = {TE: model, G1: model377}
ORACLE = {TE: oracle, G1: oracle377}
POINT_BYTES = {TE: 64, G1: 96}


def geometry(c, signed):
    """(B buckets a window, S buckets a level-1 partition, P partitions)"""
    B = 1 << (c - 1 if signed else c)
    S = min(B, 256)
    return B, S, B // S


def windows(c, signed):
    """the plan's window count for full-width scalars (csrc/plan_arith.hpp: windows_for)"""
    return -(-(255 if signed else 256) // c)


def default_segment_len(n, B):
    """csrc/plan_arith.hpp: default_seg_len"""
    a, s = (2 * n + B - 1) // B, 16
    while s < a and s < 64:
        s <<= 1
    return s


# ---------------------------------------------------------------- digit rows and scalars
def digit_row(counts, c, signed, seed, zeros=0):
    """counts[b] entries for every bucket b of one window, and `zeros` points with digit 0, in seeded shuffled order (level-1 tiles and
    chunks see the buckets interleaved).  Signs alternate inside every bucket, starting positive; bucket B - 1 of a signed window is
    reached by the digit -2^(c-1) alone and stays all negative.  Plain windows have no signs, and their bucket B - 1 no digit."""
    B = geometry(c, signed)[0]
    counts = np.asarray(counts, dtype=np.int64)
    assert counts.shape == (B,) and counts.min() >= 0
    out = []
    for b in np.nonzero(counts)[0]:
        k, v = int(counts[b]), int(b) + 1
        if not signed:
            assert b < B - 1, "no plain window reaches bucket B - 1"
            out += [v] * k
        elif b == B - 1:
            out += [-v] * k
        else:
            out += [v if j % 2 == 0 else -v for j in range(k)]
    row = np.array(out + [0] * zeros, dtype=np.int64)
    np.random.default_rng(seed).shuffle(row)
    nz = row[row != 0]
    assert np.array_equal(np.bincount(np.abs(nz) - 1, minlength=B), counts), "the row does not have the requested histogram"
    if signed:
        neg = np.bincount(np.abs(nz[nz < 0]) - 1, minlength=B)
        assert np.array_equal(neg[:B - 1], counts[:B - 1] // 2) and neg[B - 1] == counts[B - 1]
    return row


def decompose(curve, ks, c, signed, W):
    """digit values [W][n] by the oracle's (Twisted-Edwards) or the model's (BLS12-377) own signed decomposition, plain windows by
    model.to_words_le; the windows above W must be empty"""
    half = 1 << (c - 1)
    if not signed:
        rows = np.array([model.to_words_le(k, W + 1, c) for k in ks], dtype=np.int64).T
    elif curve == TE:
        rows = oracle.decompose_scalars_signed(model.scalars_to_bytes(ks), c).astype(np.int64) - half
    else:
        rows = np.array([model377.decompose_scalar_signed(k, W + 1, c) for k in ks], dtype=np.int64).T - half
    assert rows.shape[0] >= W and not rows[W:].any(), "a digit above the plan's windows"
    return rows[:W]


def scalars_of(curve, d0, d1, c, signed, W=None):
    """(scalars as integers, scalars as bytes, digit values [W][n]); asserts that the decomposition gives (d0, d1, 0, 0, ...) back"""
    half, full = 1 << (c - 1), 1 << c
    d0, d1 = np.asarray(d0, dtype=np.int64), np.asarray(d1, dtype=np.int64)
    assert d0.shape == d1.shape
    if signed:
        assert d0.min() >= -half and d0.max() <= half - 1 and d1.min() >= 1 and d1.max() <= half - 1
    else:
        assert d0.min() >= 0 and d0.max() <= full - 1 and d1.min() >= 0 and d1.max() <= full - 1
    ks = [(int(b) << c) + int(a) for a, b in zip(d0, d1)]
    assert min(ks) >= 0
    W = windows(c, signed) if W is None else W
    rows = decompose(curve, ks, c, signed, W)
    assert np.array_equal(rows[0], d0) and np.array_equal(rows[1], d1) and not rows[2:].any(), "the digits are not what was asked for"
    return ks, MODEL[curve].scalars_to_bytes(ks), rows


@functools.lru_cache(maxsize=None)
def points(curve, n=30000):
    return ORACLE[curve].gen_points(0x50B7 + curve, n)


def points_of(curve, n):
    return points(curve)[:POINT_BYTES[curve] * n]


def msm(curve, n, sc):
    return ORACLE[curve].msm(points_of(curve, n), sc, threads=8)


def _case(kind, key, c, signed, counts, seed, zeros, named, seg_len=0, **more):
    """one window-0 histogram with a seeded window 1 (signed: digits 1 .. 2^(c-1) - 1, plain: 0 .. 2^c - 1)"""
    B = geometry(c, signed)[0]
    d0 = digit_row(counts, c, signed, seed, zeros)
    rng = np.random.default_rng(seed + 1)
    d1 = rng.integers(1, 1 << (c - 1), d0.size) if signed else rng.integers(0, 1 << c, d0.size)
    return SimpleNamespace(kind=kind, key=key, c=c, signed=signed, counts=np.asarray(counts, dtype=np.int64), d0=d0, d1=d1, n=int(d0.size),
                           seg_len=seg_len, named=named, B=B, **more)


# ---------------------------------------------------------------- (a) partition totals
A_C = 13
# (T, position of p*, part_start[p*] % 8, the empty partition): every T, the positions 0, middle and P - 1, the alignments 0, 1 and 7;
# T = 9209 and T = 18417 with a start at 7 mod 8; the empty partition in front, behind, first and last of the window
A_CASES = [(9207, 0, 0, 15), (9208, 5, 1, 6), (9209, 5, 7, 4), (18416, 15, 0, 0), (18417, 15, 7, 14), (27625, 7, 1, 6)]
A_CASES_G1 = [(9209, 5, 7, 4), (18417, 15, 7, 14)]
A_PIECES = {9207: 1, 9208: 1, 9209: 2, 18416: 2, 18417: 3, 27625: 4}


@functools.lru_cache(maxsize=None)
def partition_case(T, pos, align, empty):
    """c = 13 signed (B = 4096, S = 256, P = 16): partition `pos` of window 0 holds exactly T entries, spread unevenly over its 256 buckets
    -- some empty, one with more than a third of T, the first and the last occupied --, partition `empty` none, the others a few; the
    totals in front of `pos` make its start = align mod 8"""
    B, S, P = geometry(A_C, True)
    rng = np.random.default_rng(100 * T + pos)
    counts = np.zeros(B, dtype=np.int64)
    lo = pos * S
    heavy = lo + 100
    counts[heavy], counts[lo], counts[lo + S - 1] = T // 3 + 40, 3, 5
    free = np.array([lo + j for j in range(1, S - 1) if j != 100 and j % 7 != 3])
    rem = T - int(counts[lo:lo + S].sum())
    w = rng.integers(1, 20, free.size)
    share = rem * w // int(w.sum())
    share[0] += rem - int(share.sum())
    counts[free] = share
    assert empty != pos
    for q in range(P):
        if q not in (pos, empty):
            np.add.at(counts, q * S + rng.integers(0, S, 3 + q % 5), 1)
    if pos:
        q0 = min(q for q in range(pos) if q != empty)
        counts[q0 * S + 17] += (align - int(counts[:lo].sum())) % 8
    case = _case("partition", (T, pos, align, empty), A_C, True, counts, 7 * T + pos, 11,
                 {"heaviest": (0, heavy), "first": (0, lo), "last": (0, lo + S - 1)}, T=T, pos=pos, align=align, empty=empty, pieces=A_PIECES[T])
    part = case.counts.reshape(P, S).sum(axis=1)
    own = case.counts[lo:lo + S]
    assert part[pos] == T and part[empty] == 0 and -(-T // L2_CAP) == case.pieces
    assert all(0 < part[q] < 20 for q in range(P) if q not in (pos, empty)), "the other partitions hold a few entries"
    assert int(part[:pos].sum()) % 8 == align, "part_start[p*] % 8"
    assert (own == 0).sum() >= 30 and own[100] > T / 3 and own[0] > 0 and own[S - 1] > 0 and own.max() == own[100]
    assert case.n < 30000
    return case


# ---------------------------------------------------------------- (b) parts per bucket
B_SEG = 4
B_COUNTS = [0, 1, 4, 5, 64, 65, 1024, 1025, 2048, 2049]
B_PARTS = [1, 1, 1, 2, 16, 17, 256, 257, 512, 513]     # the split list at its maximum, a giant of one run, a full run, a second run of one part
B_FORMS = {
    # c, signed, the buckets of B_COUNTS in order
    "c8": (8, True, [5, 0, 17, 30, 31, 64, 77, 100, 126, 127]),               # one partition of S = 128 < 256 buckets; bucket B - 1 all negative
    # two giants (1024, 2049 entries) and the 16-part bucket share partition 3; 2048 entries in bucket B - 1
    "c13": (13, True, [7, 0, 5 * 256 + 3, 9 * 256 + 200, 3 * 256, 8 * 256 + 128, 3 * 256 + 10, 12 * 256 + 255, 4095, 3 * 256 + 255]),
    "u8": (8, False, [5, 0, 17, 30, 31, 64, 77, 100, 200, 254]),
}


@functools.lru_cache(maxsize=None)
def parts_case(form):
    c, signed, at = B_FORMS[form]
    B = geometry(c, signed)[0]
    rng = np.random.default_rng(len(form) + c)
    counts = np.zeros(B, dtype=np.int64)
    others = [b for b in rng.choice(B - 1, 40, replace=False) if b not in at]
    counts[others] = rng.integers(1, 4, len(others))
    counts[at] = B_COUNTS
    case = _case("parts", form, c, signed, counts, 31 + c, 9, {"count %d" % k: (0, b) for k, b in zip(B_COUNTS, at)}, seg_len=B_SEG)
    assert [max(1, -(-int(case.counts[b]) // B_SEG)) for b in at] == B_PARTS
    assert [p > COMBINE_SMALL for p in B_PARTS] == [False] * 5 + [True] * 5 and [-(-p // GIANT_RUN) for p in B_PARTS[5:]] == [1, 1, 2, 2, 3]
    assert case.n < 6500
    if form == "c13":
        share = [b // 256 for k, b in zip(B_COUNTS, at) if k in (64, 1024, 2049)]
        assert share == [3, 3, 3] and len(set(b // 256 for b in at)) == 7
    return case


# ---------------------------------------------------------------- (c) the length clamp
C_SEG = [1023, 1024, 1500]


@functools.lru_cache(maxsize=None)
def clamp_case():
    """c = 8 signed: bucket 40 holds 3000 entries -- segments of 1023, 1023 and 954, of 1024, 1024 and 952, of 1500 and 1500"""
    B = geometry(8, True)[0]
    rng = np.random.default_rng(77)
    counts = np.zeros(B, dtype=np.int64)
    others = [b for b in rng.choice(B, 60, replace=False) if b not in (40, 41)]
    counts[others] = rng.integers(1, 4, len(others))
    counts[40] = 3000
    case = _case("clamp", "clamp", 8, True, counts, 78, 5, {"count 3000": (0, 40), "empty": (0, 41), "small": (0, int(others[0]))})
    assert case.n < 3200 and case.counts.sum() - 3000 < 200
    return case


@functools.lru_cache(maxsize=None)
def inputs(curve, kind, key, W=None):
    """(case, scalars as bytes, digit values [W][n]) of a case on a curve: the digits are checked through the decomposition"""
    case = {"partition": lambda: partition_case(*key), "parts": lambda: parts_case(key), "clamp": clamp_case}[kind]()
    _, sc, rows = scalars_of(curve, case.d0, case.d1, case.c, case.signed, W)
    return case, sc, rows


@functools.lru_cache(maxsize=None)
def want(curve, kind, key):
    case, sc, _ = inputs(curve, kind, key)
    return msm(curve, case.n, sc)


@functools.lru_cache(maxsize=None)
def bucket_sum(curve, kind, key, window, bucket):
    """the bigint model's sum of the members of a bucket, negated where the digit is negative (affine; None / (0, 1) = neutral)"""
    case, _, rows = inputs(curve, kind, key)
    d = rows[window]
    m, pb = MODEL[curve], POINT_BYTES[curve]
    pts = points_of(curve, case.n)
    members = []
    for i in np.nonzero(np.abs(d) - 1 == bucket)[0]:
        p = m.xy_from_bytes(pts[pb * int(i):pb * int(i) + pb])
        members.append(m.neg(p) if d[i] < 0 else p)
    if curve == G1:
        from bls377_decode import psum
        return psum(members), len(members)
    e = m.ZERO
    for p in members:
        e = m.add(e, p)
    return e, len(members)


# ---------------------------------------------------------------- the documented layout, computed from the digits
class PlanModel:
    """Stands in for a context that ran the MSM: debug_read() serves the sort and plan arrays as csrc/kernels.hip.hpp documents them
    (k_part_scatter, k_l2_local, seg_plan_block, order_scatter_block), computed from the digit values.  `arrays` may be edited."""

    def __init__(self, digits, n, c, signed, seg_len):
        B, S, P = geometry(c, signed)
        W, nst = len(digits), (n + 7) & ~7
        logS = S.bit_length() - 1
        cap_w = B + n // seg_len
        a = {k: np.zeros((W, P), dtype=np.uint32) for k in ("part_start", "part_count")}
        a.update({k: np.zeros((W, B), dtype=np.uint32) for k in ("bucket_start", "bucket_count")})
        a["part_keys"], a["part_idx"] = np.zeros((W, nst), dtype=np.uint16), np.zeros((W, nst), dtype=np.uint32)
        a["sorted"] = np.zeros((W, n), dtype=np.uint32)
        a["seg_bucket"], a["seg_len"] = np.full(W * cap_w, 0xFFFFFFFF, dtype=np.uint32), np.full(W * cap_w, 0xFFFFFFFF, dtype=np.uint32)
        for w in range(W):
            d = np.asarray(digits[w]).astype(np.int64)
            idx = np.nonzero(d)[0]
            bucket, neg = np.abs(d[idx]) - 1, (d[idx] < 0).astype(np.int64)
            cnt = np.bincount(bucket, minlength=B)
            pcnt = cnt.reshape(P, S).sum(axis=1)
            a["part_count"][w], a["part_start"][w] = pcnt, np.cumsum(pcnt) - pcnt
            a["bucket_count"][w], a["bucket_start"][w] = cnt, np.cumsum(cnt) - cnt
            by_part = np.argsort(bucket >> logS, kind="stable")                       # arrival order inside a partition
            a["part_idx"][w, :idx.size] = idx[by_part]
            a["part_keys"][w, :idx.size] = (bucket[by_part] & (S - 1)) | (neg[by_part] << 15)
            by_bucket = np.lexsort((neg, bucket))                                      # bucket order, positive entries first
            a["sorted"][w, :idx.size] = idx[by_bucket] | (neg[by_bucket] << 31)
            extra = 0
            for p in range(P):
                at = w * cap_w + p * S + extra
                for b in range(p * S, (p + 1) * S):
                    k = int(cnt[b])
                    parts = max(1, -(-k // seg_len))
                    a["seg_bucket"][at:at + parts] = w * B + b
                    a["seg_len"][at:at + parts] = [min(seg_len, k - j * seg_len) if k else 0 for j in range(parts)]
                    at += parts
                extra += int(pcnt[p]) // seg_len
        valid = np.nonzero(a["seg_len"] != 0xFFFFFFFF)[0]
        a["order"] = valid[np.argsort(-np.minimum(a["seg_len"][valid].astype(np.int64), 1023), kind="stable")].astype(np.uint32)
        a["num_segments"] = np.array([valid.size], dtype=np.uint32)
        self.arrays, self.seg_len = a, seg_len

    def get_option(self, key):
        assert key == "segment_len_used"
        return self.seg_len

    def debug_read(self, stage, nbytes):
        return self.arrays[stage].tobytes()[:nbytes]
