"""Fixed-base windows (option "bind_fixed_base" = c in 16..21) as a model in Python integers.

TEST INFRASTRUCTURE ONLY, written from DESIGN.md's description of the feature, not from csrc/fb_plan.hpp: the host tests compare that
header with this module (tests/test_fixed_base_host.py) and the GPU tests compare what the engine wrote with it
(tests/test_gpu_fixed_base_stages.py).

With the points resident, table w holds 2^(c w) P_i.  A scalar k is walked in W = ceil(255 / c) signed windows, k = sum_w d_w 2^(c w) with
d_w in [-2^(c-1), 2^(c-1)); a non-zero digit is an ENTRY (table index w n + i, sign) of bucket b = |d_w| - 1 of ONE bucket set of 2^(c-1)
buckets.  b is cut into (hb | lo: 15 bits); the entries of equal hb form a row of 2^15 buckets; the top window's entries with hb = 0 go
to an extra row (index rb = 2^(c-16)) so that the rows stay balanced.  Row weights: hb 2^15 + lo + 1.
"""
from __future__ import annotations

LO_BITS = 15
LO_MASK = (1 << LO_BITS) - 1
C_RANGE = range(16, 22)
THREADS = 256                 # scalars per block of the digit kernel
SCATTER_BLOCKS = 1024         # level-1 blocks the sort aims at
MIN_CHUNK = 4096              # one tile
ROW_FILL_WORDS = 64


def windows(c: int) -> int:
    return -(-255 // c)


def regular_rows(c: int) -> int:
    return 1 << (c - 1 - LO_BITS)


# ------------------------------------------------------------------ the walk
def walk(k: int, c: int):
    """(digits d_0 .. d_{W-1}, final carry): k = sum_w d_w 2^(c w) + carry 2^(c W)"""
    W, full, half = windows(c), 1 << c, 1 << (c - 1)
    ds = []
    for _ in range(W):
        d = k & (full - 1)
        k >>= c
        if d >= half:
            d -= full
            k += 1
        ds.append(d)
    return ds, k


def entry_of(d: int, w: int, c: int):
    """digit d != 0 of window w -> (row, lo, sign); sign = 1 for a negative digit"""
    b = abs(d) - 1
    hb, lo = b >> LO_BITS, b & LO_MASK
    row = regular_rows(c) if (w == windows(c) - 1 and hb == 0) else hb
    return row, lo, 1 if d < 0 else 0


def entries(k: int, c: int):
    """([(w, row, lo, sign)] of the non-zero digits in window order, carry)"""
    ds, carry = walk(k, c)
    return [(w,) + entry_of(d, w, c) for w, d in enumerate(ds) if d], carry


def weight(row: int, lo: int, c: int) -> int:
    """|digit| of an entry: the extra row weighs like row 0"""
    hb = 0 if row == regular_rows(c) else row
    return (hb << LO_BITS) + lo + 1


def largest_accepted(c: int) -> int:
    """the largest 256-bit scalar whose walk leaves no carry: every digit at its maximum 2^(c-1) - 1"""
    W = windows(c)
    top = sum(((1 << (c - 1)) - 1) << (c * w) for w in range(W))
    return min(top, (1 << 256) - 1)


def smallest_refused(c: int):
    """the smallest scalar with a final carry, or None where every 256-bit scalar is accepted"""
    k = largest_accepted(c) + 1
    return k if k < (1 << 256) else None


# ------------------------------------------------------------------ the plan
def geometry(n: int, c: int) -> dict:
    W, rb = windows(c), regular_rows(c)
    rows = rb + 1
    reg = -(-(W - 1) * n // rb)
    big = max(reg, n)
    cap = (big + big // 16 + 4096 + 7) // 8 * 8
    ch = max(1, min(256, SCATTER_BLOCKS // rows))
    ch = max(1, min(ch, -(-cap // MIN_CHUNK)))
    chunk_len = -(-(-(-cap // ch)) // 4096) * 4096
    CH = -(-cap // chunk_len)
    mean2 = -(-2 * W * n // (rb << LO_BITS))
    seg_len = 16
    while seg_len < mean2 and seg_len < 64:
        seg_len *= 2
    half = sum(1 << (c * w + c - 1) for w in range(W))
    P = (1 << LO_BITS) // 256
    return dict(W=W, rb=rb, rows=rows, reg=reg, cap=cap, chunks=ch, chunk_len=chunk_len, CH=CH, S=256, P=P, logS=8, seg_len=seg_len,
                half=[(half >> (32 * j)) & 0xFFFFFFFF for j in range(10)], lds_bytes=4 * (2 * rows + rows * 2 * P))


def bind_refused(c: int, n_table: int) -> bool:
    return windows(c) * n_table >= 1 << 31


def msm_refused(n: int, c: int, n_table: int) -> bool:
    g = geometry(n, c)
    return g["rows"] * g["cap"] >= 1 << 31 or g["W"] * n_table >= 1 << 31


# ------------------------------------------------------------------ the rows of an MSM
def _ext(model, p):
    return (p[0], p[1], p[0] * p[1] % model.P, 1)


def _aff(model, e):
    zi = model.inv(e[3])
    return (e[0] * zi % model.P, e[1] * zi % model.P)


def _ext_mul(model, k: int, e):
    acc = (0, 1, 0, 1)
    while k:
        if k & 1:
            acc = model._ext_add(acc, e)
        e = model._ext_add(e, e)
        k >>= 1
    return acc


def tables(model, pts, c: int):
    """tables[w][i] = 2^(c w) P_i (affine), table w from table w - 1 by c doublings (the model's extended addition of a point with itself)"""
    out = [list(pts)]
    for _ in range(1, windows(c)):
        nxt = []
        for p in out[-1]:
            e = _ext(model, p)
            for _ in range(c):
                e = model._ext_add(e, e)
            nxt.append(_aff(model, e))
        out.append(nxt)
    return out


def bucket_members(ks, c: int):
    """{row: {lo: set((table index, sign))}} of an MSM over a table of len(ks) points; any carry raises"""
    n = len(ks)
    out = {}
    for i, k in enumerate(ks):
        es, carry = entries(k, c)
        assert carry == 0, "scalar %d is out of the walk's range" % i
        for w, row, lo, sg in es:
            out.setdefault(row, {}).setdefault(lo, set()).add((w * n + i, sg))
    return out


DW = [(LO_BITS + 3 - k) // 4 for k in range(4)]           # 4, 4, 4, 3


def msm_rows(model, tabs, ks, c: int):
    """{row: [T, W0, W1, W2, W3]} (affine model points) for the rows that hold an entry: T = the sum of the row's buckets,
    W_k = sum_v v M_k[v] with M_k[v] the sum of the buckets whose index lo has digit k (DW[k] bits) equal to v"""
    n = len(ks)
    zero = (0, 1, 0, 1)
    rows = {}
    for row, buckets in bucket_members(ks, c).items():
        T, M = zero, [dict() for _ in range(4)]
        for lo, members in buckets.items():
            s = zero
            for idx, sg in members:
                p = tabs[idx // n][idx % n]
                s = model._ext_add(s, _ext(model, model.neg(p) if sg else p))
            T = model._ext_add(T, s)
            sh = 0
            for k in range(4):
                v = (lo >> sh) & ((1 << DW[k]) - 1)
                sh += DW[k]
                if v:
                    M[k][v] = model._ext_add(M[k].get(v, zero), s)
        Wk = []
        for k in range(4):
            acc = zero
            for v, s in M[k].items():
                acc = model._ext_add(acc, _ext_mul(model, v, s))
            Wk.append(_aff(model, acc))
        rows[row] = [_aff(model, T)] + Wk
    return rows


def tail(model, rows: dict, c: int):
    """sum_r (T_r + sum_k 2^(dw_0 + .. + dw_{k-1}) W_{k,r}) + 2^15 sum_{r < rb} r T_r"""
    rb = regular_rows(c)
    acc = model.ZERO
    for r, (T, *Wk) in rows.items():
        acc = model.add(acc, T)
        sh = 0
        for k in range(4):
            acc = model.add(acc, model.scalar_mul(1 << sh, Wk[k]))
            sh += DW[k]
        if r < rb and r:
            acc = model.add(acc, model.scalar_mul(r << LO_BITS, T))
    return acc


# ------------------------------------------------------------------ bounds replay of the digit kernel and the level-1 scatter's reads
def buffer_sizes(g: dict) -> dict:
    """element counts of the buffers the fixed-base code indexes, as te_msm.hip's ensure_buffers sizes them for this plan:
         nd = nw * nst + 64                      ("const size_t nd = (size_t)p.nw * p.nst + 64")   d_digits (u16), d_fb_remap (u32)
         c1 = nw * CH * P                        ("const size_t c1 = (size_t)p.nw * p.CH * p.P")   d_counts1, words of the zeroed block
         row fill: the 64 words at the block's end ("+ 64: the row fill counters of fixed-base windows")"""
    nd = g["rows"] * g["cap"] + 64
    return dict(digits=nd, remap=nd, row_fill=ROW_FILL_WORDS, counts1=g["rows"] * g["CH"] * g["P"], lds_words=g["lds_bytes"] // 4)


def replay(ks, c: int, n_table: int | None = None, idx_base: int = 0) -> dict:
    """k_fb_digits over the scalars ks, block by block in launch order and thread by thread inside a block (one legal order of its
    atomics), then the read range of the sort's first level.  Every index the fixed-base code forms is checked against buffer_sizes();
    violations are collected, not raised.  Returns fill (entries reserved per row), fallback (a row overflowed), carry (a scalar is out
    of range), violations, written ({row: {pos: (code, remap word)}}) and counts1 ({(row, chunk, partition): count})."""
    n = len(ks)
    n_table = n if n_table is None else n_table
    g = geometry(n, c)
    sz = buffer_sizes(g)
    rows, rb, cap, W, P, CH, chunk_len = g["rows"], g["rb"], g["cap"], g["W"], g["P"], g["CH"], g["chunk_len"]
    bad = []

    def chk(what, idx, size):
        if not 0 <= idx < size:
            bad.append("%s[%d] outside %d" % (what, idx, size))

    if rows > sz["row_fill"]:
        bad.append("rows %d exceed the %d row fill words" % (rows, sz["row_fill"]))
    if g["lds_bytes"] > 64 * 1024:
        bad.append("LDS %d bytes" % g["lds_bytes"])
    row_fill = [0] * rows
    written = {r: {} for r in range(rows)}
    counts1 = {}
    carry = False
    for b0 in range(0, n, THREADS):
        # phase A: ranks among the block's entries of a row
        cnt = [0] * rows
        ents = []
        for i in range(b0, min(n, b0 + THREADS)):
            es, cy = entries(ks[i], c)
            carry |= cy != 0
            for w, row, lo, sg in es:
                chk("cnt", row, rows)
                ents.append((i, w, row, lo, sg, cnt[row]))
                cnt[row] += 1
        # one reservation per block and row
        base = [0] * rows
        for r in range(rows):
            if cnt[r]:
                chk("row_fill", r, sz["row_fill"])
                base[r] = row_fill[r]
                row_fill[r] += cnt[r]
        # phase B
        hist = {}
        for i, w, row, lo, sg, rank in ents:
            pos = base[row] + rank
            if pos >= cap:
                continue                                   # the guard: err word 1, the engine falls back
            at = row * cap + pos
            chk("digits", at, sz["digits"])
            chk("remap", at, sz["remap"])
            word = w * n_table + idx_base + i
            if not word < W * n_table:
                bad.append("remap word %d (window %d, scalar %d) is outside the table of %d records" % (word, w, i, W * n_table))
            if idx_base + i >= n_table:
                bad.append("scalar %d at table position %d of %d: its entries alias the next table" % (i, idx_base + i, n_table))
            if word >= 1 << 31:
                bad.append("remap word %d collides with the sign bit" % word)
            assert pos not in written[row]
            written[row][pos] = (lo + 1, word | (sg << 31))
            ch = pos // chunk_len
            slot = ch - base[row] // chunk_len
            part = lo >> g["logS"]
            if slot < 2:
                at = (row * 2 + slot) * P + part
                chk("hist", 2 * rows + at, sz["lds_words"])
                hist[at] = hist.get(at, 0) + 1
            else:
                at = (row * CH + ch) * P + part
                chk("counts1", at, sz["counts1"])
                counts1[(row, ch, part)] = counts1.get((row, ch, part), 0) + 1
        for at, v in hist.items():
            row, rem = divmod(at, 2 * P)
            slot, part = divmod(rem, P)
            ch = base[row] // chunk_len + slot
            if ch < CH:
                chk("counts1", (row * CH + ch) * P + part, sz["counts1"])
                counts1[(row, ch, part)] = counts1.get((row, ch, part), 0) + v
            else:
                bad.append("histogram slot of row %d counts chunk %d of %d" % (row, ch, CH))
    # the first level of the sort: block (chunk, row) reads codes and remap words of [chunk start, hi), hi = min(fill, cap, chunk end);
    # codes come in groups of eight clamped to the row's last group
    for r in range(rows):
        hi_row = min(row_fill[r], cap)
        if sorted(written[r]) != list(range(hi_row)):
            bad.append("row %d: positions below %d are read but not all were written" % (r, hi_row))
        for ch in range(CH):
            lo_, hi = ch * chunk_len, min(hi_row, (ch + 1) * chunk_len)
            if lo_ < hi:
                chk("scatter remap", r * cap + hi - 1, sz["remap"])
            last8 = cap // 8 - 1
            chk("scatter digits", (r * cap // 8 + min((lo_ >> 3) + 511, last8)) * 8 + 7, sz["digits"])
    # the histogram the scatter will read is the histogram of what was written
    direct = {}
    for r in range(rows):
        for pos, (code, _) in written[r].items():
            key = (r, pos // chunk_len, (code - 1) >> g["logS"])
            direct[key] = direct.get(key, 0) + 1
    if direct != counts1:
        bad.append("counts1 differs from the histogram of the written entries")
    return dict(geometry=g, fill=row_fill, fallback=any(f > cap for f in row_fill), carry=carry, violations=bad, written=written, counts1=counts1)
