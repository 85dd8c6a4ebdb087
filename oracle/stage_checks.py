"""Stage checks of one MSM (the reference's per-stage `debug` checks, submission.ts:892-1363).

TEST INFRASTRUCTURE ONLY: shared by tests/test_gpu_parity.py::test_stages_against_oracle, tests/test_gpu_large_n.py and
tests/test_gpu_sort_thresholds.py.  The context must have run the MSM last, whole (not in host-buffer pieces), with options
"sort_buckets" = 1 and "prezero" = 0 set.

check_stages      one Twisted-Edwards MSM over (pts, sc): records, digits, the sort and plan, a sample of bucket sums
check_sort_plan   the sort and the segment plan alone, from the expected digit values: none of these arrays depends on the curve
"""
from __future__ import annotations

import ctypes
from types import SimpleNamespace

import numpy as np

L2_CAP = 9208          # TE_L2_CAP: a level-1 partition of more entries is sorted in pieces, which keep arrival order inside a bucket
LEN_SLOTS = 1023       # segment lengths above share the last slot of the length histogram: the schedule orders by min(len, 1023)
INVALID = 0xFFFFFFFF


def _u32(ctx, stage, count):
    raw = ctx.debug_read(stage, count * 4)
    assert len(raw) == count * 4, f"{stage}: {len(raw)} bytes read, {count * 4} expected"
    return np.frombuffer(raw, dtype=np.uint32)


def check_sort_plan(ctx, digits, n: int, c: int, signed: bool, W: int):
    """Level-1 partitions, level-2 buckets and the sorted permutation, the segment records and the schedule order of the MSM `ctx` ran
    last, against the expected digit VALUES digits[W][n] (any integer type): signed digits, or the plain c-bit windows where signed is
    false.  A value d != 0 is an entry of bucket |d| - 1 (B = 2^(c-1) buckets a window for signed digits, 2^c for plain windows, whose
    last bucket stays empty), negative where d < 0; d == 0 is no entry.  Returns what it read, for checks of the caller's own."""
    B = 1 << (c - 1 if signed else c)
    nst = (n + 7) & ~7                                  # digit rows are padded to a multiple of 8 entries (digit 0)
    assert len(digits) == W
    # K2 level 1: partitions of S = min(B, 256) buckets (order inside a partition is free)
    S = min(B, 256)
    P, logS = B // S, S.bit_length() - 1
    pstart = _u32(ctx, "part_start", W * P).reshape(W, P)
    pcount = _u32(ctx, "part_count", W * P).reshape(W, P)
    pkeys = np.frombuffer(ctx.debug_read("part_keys", W * nst * 2), dtype=np.uint16).reshape(W, nst)
    pidx = _u32(ctx, "part_idx", W * nst).reshape(W, nst)
    for w in range(W):
        d = np.asarray(digits[w]).astype(np.int64)
        assert d.shape == (n,)
        bucket = np.abs(d) - 1
        nz = d != 0
        assert signed or not np.any(d < 0), "plain windows are not negative"
        assert int(bucket.max(initial=0)) < B, "digit value outside the window's buckets"
        e_cnt = np.bincount(bucket[nz] >> logS, minlength=P)
        assert np.array_equal(pcount[w], e_cnt), f"window {w} partition counts"
        assert np.array_equal(pstart[w], np.concatenate([[0], np.cumsum(e_cnt)[:-1]])), f"window {w} partition starts"
        used = int(e_cnt.sum())
        idx, key = pidx[w][:used].astype(np.int64), pkeys[w][:used].astype(np.int64)
        assert np.array_equal(np.sort(idx), np.nonzero(nz)[0]), "entries are not a permutation of the non-zero digits"
        assert np.array_equal(bucket[idx] >> logS, np.repeat(np.arange(P), e_cnt)), "entry in the wrong partition"
        assert np.array_equal(key & 0x7FFF, bucket[idx] & (S - 1)), "key low bits"
        assert np.array_equal((key >> 15).astype(bool), d[idx] < 0), "sign bit"
    del pkeys, pidx
    # K2 level 2: bucket_count/bucket_start == cpu_transpose's column pointers folded by sign (transpose.ts:14-62)
    cnt = _u32(ctx, "bucket_count", W * B).reshape(W, B)
    start = _u32(ctx, "bucket_start", W * B).reshape(W, B)
    srt = _u32(ctx, "sorted", W * n).reshape(W, n)
    for w in range(W):
        d = np.asarray(digits[w]).astype(np.int64)
        bucket = np.abs(d) - 1
        nz = d != 0
        e_cnt = np.bincount(bucket[nz], minlength=B)
        assert np.array_equal(cnt[w], e_cnt), f"window {w} counts"
        assert np.array_equal(start[w], np.concatenate([[0], np.cumsum(e_cnt)[:-1]])), f"window {w} starts"
        used = int(e_cnt.sum())
        ent = srt[w][:used]
        idx, neg = ent & 0x7FFFFFFF, ent >> 31
        assert np.array_equal(np.sort(idx), np.sort(np.nonzero(nz)[0])), "sorted is not a permutation of the non-zero digits"
        where = np.repeat(np.arange(B), e_cnt)          # the bucket every position of the sorted run belongs to
        assert np.array_equal(bucket[idx], where), "entry in the wrong bucket"
        assert np.array_equal(neg.astype(bool), d[idx] < 0), "sign bit"
        # a partition that one block sorts whole (at most TE_L2_CAP entries) lists a bucket's positive entries in front of its negative
        # ones: a negative entry followed by a positive one only happens across a bucket boundary
        whole = e_cnt.reshape(P, S).sum(axis=1) <= L2_CAP
        if used > 1 and whole.any():
            bad = (neg[:-1] == 1) & (neg[1:] == 0) & (where[:-1] == where[1:]) & whole[where[1:] >> logS]
            assert not bad.any(), f"window {w} bucket {int(where[1:][bad][0]) if bad.any() else -1}: a negative entry in front of a positive one"
    del srt
    # work segments: every bucket is cut into pieces of at most segment_len entries -- full ones, then the remainder; an empty bucket
    # has one segment of length 0; the schedule is a permutation of the segments in descending length
    seg_len = ctx.get_option("segment_len_used")
    nseg = int(_u32(ctx, "num_segments", 1)[0])
    cnt64 = cnt.reshape(-1).astype(np.int64)
    per_bucket = np.maximum(1, -(-cnt64 // seg_len))
    assert nseg == int(per_bucket.sum())
    # segment ids: window k owns [k * capW, (k+1) * capW), capW = B + n // seg_len; inside, partition p starts at
    # p * S + sum_{p' < p} floor(count_p' / seg_len); ids are dense inside a level-1 partition, in bucket order, and the ids a partition
    # does not use -- up to the next partition's base, and behind the last partition up to the end of the window's range -- are
    # marked invalid (0xffffffff) in both arrays
    cap_w = B + n // seg_len
    ids = W * cap_w
    seg_bucket_all = _u32(ctx, "seg_bucket", ids)
    seg_lens_all = _u32(ctx, "seg_len", ids)
    valid = seg_bucket_all != INVALID
    assert np.array_equal(valid, seg_lens_all != INVALID) and int(valid.sum()) == nseg
    part_segs = per_bucket.reshape(W, P, S).sum(axis=2)
    exp_valid = np.zeros(ids, dtype=bool)
    for w in range(W):
        extra = np.concatenate([[0], np.cumsum(pcount[w].astype(np.int64) // seg_len)[:-1]])
        for p in range(P):
            base = w * cap_w + p * S + int(extra[p])
            end = w * cap_w + (p + 1) * S + int(extra[p + 1]) if p + 1 < P else (w + 1) * cap_w
            assert base + int(part_segs[w, p]) <= end, "the plan's id ranges overlap: the checker's own arithmetic is wrong"
            exp_valid[base:base + int(part_segs[w, p])] = True
    miss = np.nonzero(valid != exp_valid)[0]
    assert miss.size == 0, f"segment id {int(miss[0])} (window {int(miss[0]) // cap_w}): valid = {bool(valid[miss[0]])}, expected the opposite"
    seg_bucket, seg_lens = seg_bucket_all[valid], seg_lens_all[valid]
    assert np.array_equal(seg_bucket, np.repeat(np.arange(W * B), per_bucket)), "segments are not in bucket order"
    assert np.all(seg_bucket // B == np.nonzero(valid)[0] // cap_w), "segment id outside its window's range"
    assert np.array_equal(np.bincount(seg_bucket, weights=seg_lens, minlength=W * B).astype(np.int64), cnt64)
    assert seg_lens.max() <= seg_len
    first_seg = np.concatenate([[0], np.cumsum(per_bucket)[:-1]])
    part_no = np.arange(nseg) - np.repeat(first_seg, per_bucket)             # which part of its bucket a segment is
    exp_lens = np.clip(np.repeat(cnt64, per_bucket) - part_no * seg_len, 0, seg_len)
    assert np.array_equal(seg_lens.astype(np.int64), exp_lens), "a bucket's segments are not full ones followed by the remainder"
    for w in np.nonzero(cnt.sum(axis=1) == 0)[0]:                            # an empty window: one segment of length 0 per bucket
        own = slice(int(w) * cap_w, (int(w) + 1) * cap_w)
        assert valid[own][:B].all() and not valid[own][B:].any() and not seg_lens_all[own][:B].any(), f"empty window {w}"
        assert np.array_equal(seg_bucket_all[own][:B], np.arange(int(w) * B, (int(w) + 1) * B)), f"empty window {w}"
    order = _u32(ctx, "order", nseg)
    assert np.array_equal(np.sort(order), np.nonzero(valid)[0]), "order is not a permutation of the valid segments"
    sizes = np.minimum(seg_lens_all[order], LEN_SLOTS)                      # what order_scatter_block sorts by
    assert np.all(sizes[:-1] >= sizes[1:]), "order is not descending"
    return SimpleNamespace(B=B, S=S, P=P, part_start=pstart, part_count=pcount, bucket_count=cnt, bucket_start=start, seg_len=seg_len,
                           num_segments=nseg, cap_w=cap_w, seg_bucket=seg_bucket_all, seg_lens=seg_lens_all, order=order,
                           parts=per_bucket.reshape(W, B))


def decode_te_bucket(model, raw):
    """144 bytes of one Twisted-Edwards accumulator (x | y | z | t, 9 limbs of 29 bits, Montgomery form, R = 2^261) -> affine (x, y)"""
    P = model.P
    rinv = pow(1 << 261, -1, P)
    words = np.frombuffer(raw, dtype=np.uint32).reshape(4, 9)
    assert np.all(words[:, :8] < (1 << 29)), "limb class N violated"
    x, y, z, t = [sum(int(v) << (29 * i) for i, v in enumerate(words[k])) for k in range(4)]
    assert max(x, y, z, t) < 2 * P, "lazy bound < 2p violated"
    zi = pow(z * rinv % P, -1, P)
    return (x * rinv * zi % P, y * rinv * zi % P)


def check_stages(ctx, fpcheck, model, ora, pts, sc, n: int, c: int) -> None:
    """records, digits, level-1 partitions, buckets, sorted entries, segments, schedule order and a sample of bucket sums"""
    W, B = (256 + c - 1) // c, 1 << (c - 1)
    # K1a: records == the same limb code compiled for the host
    recs = ctx.debug_read("records", n * 128)
    for i in list(range(0, n, max(1, n // 97))) + [n - 1]:
        r = ctypes.create_string_buffer(128)
        fpcheck.fpc_prep_point(bytes(pts[64 * i:64 * i + 64]), r)
        assert recs[128 * i:128 * i + 128] == r.raw, f"record {i}"
    del recs
    # K1b: digits == decompose_scalars_signed (miscellaneous/utils.ts:52-95)
    nst = (n + 7) & ~7                                  # digit rows are padded to a multiple of 8 entries (digit 0)
    dig = np.frombuffer(ctx.debug_read("digits", W * nst * 2), dtype=np.uint16).reshape(W, nst)
    assert np.all(dig[:, n:] == B)
    dig = dig[:, :n]
    exp = ora.decompose_scalars_signed(sc, c)
    assert np.array_equal(dig.astype(np.uint32), exp)
    del dig
    vals = exp.view(np.int32)                           # the signed digit values, in place (2^23 entries a window)
    vals -= B
    del exp
    # K2 and the work schedule
    check_sort_plan(ctx, vals, n, c, True, W)
    # K3: a sample of bucket sums == affine sums of the model
    bk = ctx.debug_read("buckets", W * B * 144)
    rng = np.random.default_rng(1)
    for w, b in [(0, 0), (W - 1, B - 1)] + [(int(rng.integers(W)), int(rng.integers(B))) for _ in range(6)]:
        got = decode_te_bucket(model, bk[(w * B + b) * 144:(w * B + b + 1) * 144])
        d = vals[w].astype(np.int64)
        e = model.ZERO
        for i in np.nonzero(np.abs(d) - 1 == b)[0]:
            p_i = model.xy_from_bytes(bytes(pts[64 * int(i):64 * int(i) + 64]))
            e = model.add(e, model.neg(p_i) if d[i] < 0 else p_i)
        assert got == e, f"bucket ({w},{b})"
