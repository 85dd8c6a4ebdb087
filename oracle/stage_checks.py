"""Stage checks of one Twisted-Edwards MSM (the reference's per-stage `debug` checks, submission.ts:892-1363).

TEST INFRASTRUCTURE ONLY: shared by tests/test_gpu_parity.py::test_stages_against_oracle and tests/test_gpu_large_n.py.  The context
must have run the MSM over (pts, sc) last, whole (not in host-buffer pieces), with options "sort_buckets" = 1 and "prezero" = 0 set.
"""
from __future__ import annotations

import ctypes

import numpy as np


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
    # K2 level 1: partitions of S = min(B, 256) buckets (order inside a partition is free)
    S = min(B, 256)
    P, logS = B // S, S.bit_length() - 1
    pstart = np.frombuffer(ctx.debug_read("part_start", W * P * 4), dtype=np.uint32).reshape(W, P)
    pcount = np.frombuffer(ctx.debug_read("part_count", W * P * 4), dtype=np.uint32).reshape(W, P)
    pkeys = np.frombuffer(ctx.debug_read("part_keys", W * nst * 2), dtype=np.uint16).reshape(W, nst)
    pidx = np.frombuffer(ctx.debug_read("part_idx", W * nst * 4), dtype=np.uint32).reshape(W, nst)
    for w in range(W):
        d = exp[w].astype(np.int64) - B
        bucket = np.abs(d) - 1
        nz = d != 0
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
    cnt = np.frombuffer(ctx.debug_read("bucket_count", W * B * 4), dtype=np.uint32).reshape(W, B)
    start = np.frombuffer(ctx.debug_read("bucket_start", W * B * 4), dtype=np.uint32).reshape(W, B)
    srt = np.frombuffer(ctx.debug_read("sorted", W * n * 4), dtype=np.uint32).reshape(W, n)
    for w in range(W):
        d = exp[w].astype(np.int64) - B
        bucket = np.abs(d) - 1
        nz = d != 0
        e_cnt = np.bincount(bucket[nz], minlength=B)
        assert np.array_equal(cnt[w], e_cnt), f"window {w} counts"
        assert np.array_equal(start[w], np.concatenate([[0], np.cumsum(e_cnt)[:-1]])), f"window {w} starts"
        used = int(e_cnt.sum())
        ent = srt[w][:used]
        idx, neg = ent & 0x7FFFFFFF, ent >> 31
        assert np.array_equal(np.sort(idx), np.sort(np.nonzero(nz)[0])), "sorted is not a permutation of the non-zero digits"
        assert np.array_equal(bucket[idx], np.repeat(np.arange(B), e_cnt)), "entry in the wrong bucket"
        assert np.array_equal(neg.astype(bool), d[idx] < 0), "sign bit"
    del srt
    # work segments: every bucket is cut into pieces of at most segment_len entries; the schedule is a permutation of
    # the segments in descending length
    seg_len = ctx.get_option("segment_len_used")
    nseg = int(np.frombuffer(ctx.debug_read("num_segments", 4), dtype=np.uint32)[0])
    per_bucket = np.maximum(1, -(-cnt.reshape(-1).astype(np.int64) // seg_len))
    assert nseg == int(per_bucket.sum())
    # segment ids: window k owns [k * capW, (k+1) * capW), capW = B + n // seg_len; ids are dense inside a level-1 partition,
    # in bucket order, and the ids a partition does not use are marked invalid (0xffffffff)
    cap_w = B + n // seg_len
    ids = W * cap_w
    seg_bucket_all = np.frombuffer(ctx.debug_read("seg_bucket", ids * 4), dtype=np.uint32)
    seg_lens_all = np.frombuffer(ctx.debug_read("seg_len", ids * 4), dtype=np.uint32)
    valid = seg_bucket_all != 0xFFFFFFFF
    assert np.array_equal(valid, seg_lens_all != 0xFFFFFFFF) and int(valid.sum()) == nseg
    seg_bucket, seg_lens = seg_bucket_all[valid], seg_lens_all[valid]
    assert np.array_equal(seg_bucket, np.repeat(np.arange(W * B), per_bucket)), "segments are not in bucket order"
    assert np.all(seg_bucket // B == np.nonzero(valid)[0] // cap_w), "segment id outside its window's range"
    assert np.array_equal(np.bincount(seg_bucket, weights=seg_lens, minlength=W * B).astype(np.int64), cnt.reshape(-1).astype(np.int64))
    assert seg_lens.max() <= seg_len
    order = np.frombuffer(ctx.debug_read("order", nseg * 4), dtype=np.uint32)
    assert np.array_equal(np.sort(order), np.nonzero(valid)[0]), "order is not a permutation of the valid segments"
    sizes = seg_lens_all[order]
    assert np.all(sizes[:-1] >= sizes[1:]), "order is not descending"
    # K3: a sample of bucket sums == affine sums of the model
    bk = ctx.debug_read("buckets", W * B * 144)
    P = model.P
    rinv = pow(1 << 261, -1, P)
    rng = np.random.default_rng(1)
    for w, b in [(0, 0), (W - 1, B - 1)] + [(int(rng.integers(W)), int(rng.integers(B))) for _ in range(6)]:
        raw = bk[(w * B + b) * 144:(w * B + b + 1) * 144]
        words = np.frombuffer(raw, dtype=np.uint32).reshape(4, 9)
        assert np.all(words[:, :8] < (1 << 29)), "limb class N violated"
        x, y, z, t = [sum(int(v) << (29 * i) for i, v in enumerate(words[k])) for k in range(4)]
        assert max(x, y, z, t) < 2 * P, "lazy bound < 2p violated"
        zi = pow(z * rinv % P, -1, P)
        got = (x * rinv * zi % P, y * rinv * zi % P)
        d = exp[w].astype(np.int64) - B
        e = model.ZERO
        for i in np.nonzero(np.abs(d) - 1 == b)[0]:
            p_i = model.xy_from_bytes(bytes(pts[64 * int(i):64 * int(i) + 64]))
            e = model.add(e, model.neg(p_i) if d[i] < 0 else p_i)
        assert got == e, f"bucket ({w},{b})"
