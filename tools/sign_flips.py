#!/usr/bin/env python3
"""How often does a wave of k_accumulate run the sign-change block?  (the static instruction count of the loop
includes the block in front of either addition, a wave executes it only where one of its lanes changes sign.)

Runs ONE MSM of the headline shape on the GPU (n = 2^20 synthetic inputs, 16-bit signed windows), reads `sorted`, `order` and the
segment tables back with debug_read and replays the kernel's control flow on the host, wave by wave (64 consecutive entries of
`order`): per addition of the per-point loop and of the tail, does any active lane find its entry's sign different from its flag?

usage: python tools/sign_flips.py [--log-n 20] [--window-bits 16] [--json out.json]
Prints wave-level additions, executions of the block and their ratio, for the loop and for the tail, and what the same entries
would cost in arrival order (the placement of k_l2_local undone by a shuffle of every segment's entries)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def replay(signs_of, order, seg_start, seg_cnt):
    """signs_of(start, cnt) -> sign bits of a segment's entries; returns counters of the wave-level replay"""
    out = {"waves": 0, "loop_additions": 0, "loop_blocks": 0, "tail_additions": 0, "tail_blocks": 0, "lane_additions": 0, "lane_flips": 0}
    for w0 in range(0, len(order), 64):
        seg = order[w0:w0 + 64]
        cnt, start = seg_cnt[seg].astype(np.int64), seg_start[seg]
        L = int(cnt.max())
        out["waves"] += 1
        if L <= 2:
            continue                                              # pair start or conversion only: no sign block runs
        j = np.arange(L)[None, :]
        live = j < cnt[:, None]
        s = np.zeros((len(seg), L), dtype=np.int8)
        for lane in range(len(seg)):
            s[lane, :cnt[lane]] = signs_of(int(start[lane]), int(cnt[lane]))
        prev = np.empty_like(s)
        prev[:, 1:] = s[:, :-1]
        prev[:, :3] = s[:, :1]                                    # the flag at entry 2 is the first entry's sign (entry 1 went under pnt_cneg)
        flip = (s != prev) & live & (j >= 2)
        in_loop = live & (j >= 2) & ((j - (j & 1)) + 2 < cnt[:, None])
        in_tail = live & (j >= 2) & ~in_loop
        passes = int(np.any(in_loop, axis=0).sum() + 1) // 2      # a pass issues both additions for the wave
        out["loop_additions"] += 2 * passes
        out["loop_blocks"] += int(np.any(flip & in_loop, axis=0).sum())
        first_tail = in_tail & ((j & 1) == 0)                     # the tail's first addition holds an even entry, its second an odd one
        second_tail = in_tail & ((j & 1) == 1)
        for t in (first_tail, second_tail):
            if t.any():
                out["tail_additions"] += 1
                out["tail_blocks"] += int((flip & t).any())
        out["lane_additions"] += int((live & (j >= 2)).sum())
        out["lane_flips"] += int(flip.sum())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--window-bits", type=int, default=16)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    n, c = 1 << a.log_n, a.window_bits
    W, B = (256 + c - 1) // c, 1 << (c - 1)
    pts, sc = pkg.synth_inputs(0x5EED0000 + a.log_n, n)
    with pkg.MsmContext((0,)) as ctx:
        ctx.set_option("window_bits", c)
        ctx.set_option("prezero", 0)
        ctx.set_option("host_chunks", 1)              # the whole buffer as ONE piece: the tables read back are those of all n points
        ctx.run(pts, sc)
        seg_len = ctx.get_option("segment_len_used")
        u32 = lambda name, words: np.frombuffer(ctx.debug_read(name, words * 4), dtype=np.uint32).copy()
        nseg = int(u32("num_segments", 1)[0])
        srt, order = u32("sorted", W * n), u32("order", nseg)
        bstart = u32("bucket_start", W * B)
        sbucket, slen = u32("seg_bucket", W * (B + n)), u32("seg_len", W * (B + n))      # the library returns the id space it has
        ids = len(sbucket)
        assert len(slen) == ids
    if ids != W * (B + n // seg_len):
        # the option names another length than the tables were sized for: a split bucket's full parts tell the one in use
        print("# segment_len_used = %d does not give %d segment ids; taking the longest segment's length" % (seg_len, ids), file=sys.stderr)
        seg_len = int(slen[sbucket != 0xFFFFFFFF].max())
    valid = sbucket != 0xFFFFFFFF
    g = np.where(valid, sbucket, 0).astype(np.int64)
    # a bucket's parts have consecutive ids (segments are dense inside a partition, in bucket order): part = id - the bucket's first id
    vid = np.nonzero(valid)[0]
    first = np.zeros(W * B, dtype=np.int64)
    ug, ui = np.unique(g[vid], return_index=True)
    first[ug] = vid[ui]
    part = np.where(valid, np.arange(ids, dtype=np.int64) - first[g], 0)
    seg_start = (g // B) * n + bstart[g] + part * seg_len
    seg_cnt = np.where(valid, slen, 0)
    neg = (srt >> 31).astype(np.int8)
    res = {"n": n, "window_bits": c, "segment_len": int(seg_len), "segments": nseg,
           "as_sorted": replay(lambda st, ct: neg[st:st + ct], order, seg_start, seg_cnt)}
    rng = np.random.RandomState(1)
    res["arrival_order"] = replay(lambda st, ct: rng.permutation(neg[st:st + ct]), order, seg_start, seg_cnt)
    for k in ("as_sorted", "arrival_order"):
        r = res[k]
        r["blocks_per_loop_addition"] = round(r["loop_blocks"] / max(1, r["loop_additions"]), 4)
        r["blocks_per_tail_addition"] = round(r["tail_blocks"] / max(1, r["tail_additions"]), 4)
        r["flips_per_lane_addition"] = round(r["lane_flips"] / max(1, r["lane_additions"]), 4)
    print(json.dumps(res, indent=1))
    if a.json:
        json.dump(res, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
