"""Scalar classes for the fixed-base windows (option "bind_fixed_base" = c), shared by tests/test_fixed_base_host.py and
tests/test_gpu_fixed_base_stages.py.  A plain module: every builder returns Python integers below 2^256."""
import random

from oracle import fixed_base as fbm
from oracle import model

L = model.L
TOP = 1 << 256


def _from_digits(ds, c):
    k = sum(d << (c * w) for w, d in enumerate(ds))
    assert 0 <= k < TOP, "digit pattern outside 256 bits"
    return k


def _fit(ds, c):
    """the digit pattern with its top digits replaced by 0 (then 1, to stay positive) until it is a 256-bit integer"""
    ds = list(ds)
    for top in range(len(ds) - 1, -1, -1):
        k = sum(d << (c * w) for w, d in enumerate(ds))
        if 0 <= k < TOP:
            return k
        ds[top] = 1 if k < 0 and ds[top] <= 0 else 0
    raise AssertionError("no 256-bit form")


def classes(c):
    """{class name: [scalars]} of ACCEPTED scalars (no final carry) for window bits c"""
    W, rb, half = fbm.windows(c), fbm.regular_rows(c), 1 << (c - 1)
    out = {
        "zero": [0],
        "one": [1],
        "L-1": [L - 1],
        "2^253-1": [(1 << 253) - 1],
        "window boundaries": [v for w in range(1, W) for v in ((1 << (c * w)) - 1, 1 << (c * w), (1 << (c * w)) + 1)],
        # bucket hb = rb - 1, lo = 2^15 - 1: every digit at +2^(c-1) - 1, and at -2^(c-1) below a top digit 1
        "digits +max": [_fit([half - 1] * W, c)],
        "digits -2^(c-1)": [_fit([-half] * (W - 1) + [1], c)],
        "digits +1": [_from_digits([1] * W, c)],
        "digits -1": [_from_digits([-1] * (W - 1) + [1], c), _from_digits([1, -1] * ((W - 1) // 2) + [1] * (1 + (W - 1) % 2), c)],
        "largest accepted": [fbm.largest_accepted(c)],
    }
    if c >= 17:                                            # the hb 0 / 1 border
        for name, d in (("|d| = 2^15", 1 << 15), ("|d| = 2^15 + 1", (1 << 15) + 1)):
            out[name] = [_fit([d] * W, c), _fit([-d] * (W - 1) + [1], c), _fit([d, -d] * (W // 2) + [1] * (W % 2), c)]
    # a top window with hb != 0: only a non-canonical scalar reaches it, and only where the top window holds 17 bits below 2^256
    tops = [d << (c * (W - 1)) for d in ((1 << 15) + 1, (1 << 15) + 77, half - 1) if d < half and (d - 1) >> fbm.LO_BITS and (d << (c * (W - 1))) < TOP]
    tops = [k for k in tops if fbm.walk(k, c)[1] == 0]
    if tops:
        out["top window hb != 0"] = tops + [tops[0] + 12345]
    # all entries in the extra row: only the top window is non-zero, hb = 0
    out["extra row only"] = [d << (c * (W - 1)) for d in (1, 2, 7)]      # (c = 18, 21: the top window starts at bit 252, above L)
    # all entries in row rb - 1: digits of the windows below the top with hb = rb - 1
    hi = (rb - 1) << fbm.LO_BITS
    out["row rb-1 only"] = [_from_digits([hi + 1, -(hi + 0x8000), hi + 0x7FFF] + [0] * (W - 3), c), _from_digits([0, hi + 300] + [0] * (W - 2), c),
                            _from_digits([-(hi + 5), hi + 5] + [0] * (W - 2), c)]
    for name, ks in out.items():
        for k in ks:
            assert 0 <= k < TOP and fbm.walk(k, c)[1] == 0, (name, c)
    return out


def refused(c):
    """scalars with a final carry (error -3): the smallest one and 2^256 - 1, where the walk of c bits refuses any"""
    k = fbm.smallest_refused(c)
    return [] if k is None else [k, TOP - 1]


def randoms(c, count, seed):
    """seeded scalars over the canonical range, a quarter of them over the whole accepted range"""
    rng = random.Random((seed << 8) | c)
    top = fbm.largest_accepted(c)
    return [rng.randrange(L) if j % 4 else rng.randrange(top + 1) for j in range(count)]


def mixed(c, n, seed, canonical_only=False):
    """n scalars: every accepted class scalar (all of them where n allows), spread among seeded random ones.  Returns (scalars, canonical):
    canonical is False when a scalar is L or above"""
    rng = random.Random((seed << 8) | c | 0x5000)
    cl = [[k for k in ks if not canonical_only or k < L] for ks in classes(c).values()]
    edge = [ks[0] for ks in cl if ks] + [k for ks in cl for k in ks[1:]]       # one of every class first: a small n keeps every class
    ks = [rng.randrange(L) for _ in range(n)]
    slots = rng.sample(range(n), min(max(1, 3 * n // 4), len(edge)))
    for s, k in zip(slots, edge):
        ks[s] = k
    return ks, all(k < L for k in ks)


def one_among_zeros(n, at, k=None):
    ks = [0] * n
    ks[at] = L - 2 if k is None else k
    return ks


def only_row(c, n, row, seed):
    """n scalars whose entries all land in `row`: the extra row (row == rb: top window alone, hb = 0) or a regular row (windows below
    the top, hb = row)"""
    W, rb = fbm.windows(c), fbm.regular_rows(c)
    rng = random.Random((seed << 8) | c | 0x7000)
    out = []
    for _ in range(n):
        if row == rb:
            d = rng.randrange(1, min(1 << 12, TOP >> (c * (W - 1))))       # (c = 18, 21: four bits are left below 2^256)
            out.append(d << (c * (W - 1)))
        else:
            ds = [rng.choice((-1, 1)) * ((row << fbm.LO_BITS) + rng.randrange(fbm.LO_MASK) + 1) if rng.random() < 0.5 else 0 for _ in range(W - 1)]
            k = sum(d << (c * w) for w, d in enumerate(ds))
            if k <= 0:
                k = (row << fbm.LO_BITS) + 1
            out.append(k)
    return out


def fill_case(c, n, row, fill, seed=1):
    """n scalars that put exactly `fill` entries into regular row `row` and none elsewhere: three non-zero windows (windows 0..2) for
    n_A = fill // 3 points, one window for n_B = fill % 3 points, zero for the rest; the buckets are spread over the row"""
    rng = random.Random((seed << 8) | c | 0x9000)
    n_a, n_b = divmod(fill, 3)
    assert n_a + n_b <= n and row < fbm.regular_rows(c)
    d = lambda: (row << fbm.LO_BITS) + rng.randrange(fbm.LO_MASK) + 1          # (positive digits: below 2^(c-1) in row rb - 1 too)
    ks = [d() + (d() << c) + (d() << (2 * c)) for _ in range(n_a)] + [d() for _ in range(n_b)]
    return ks + [0] * (n - len(ks))
