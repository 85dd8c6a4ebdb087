"""Closed-form MSM over CHAIN points, for sizes where the bit-exact oracle is too slow to call many times.

TEST INFRASTRUCTURE ONLY.  te_msm_synth_inputs' default points form an arithmetic progression on both curves,
P_i = (a + i*b) * G (webgpu-msm-twisted-edwards_amd/csrc/synth.hpp), so for any scalars s_i

    sum_{i<L} [s_i] P_i = [S0] P_0 + [S1] (P_1 - P_0),    S0 = sum s_i mod ord,  S1 = sum i * s_i mod ord

(ord = L on the Twisted-Edwards curve, r on BLS12-377).  a and b are not needed, only two scalar multiplications in the
bigint models and two O(n) sums.  The weights a + i*b are distinct mod ord, so a dropped, doubled or misplaced entry changes
the result.  check_chain() asserts the chain structure of a given point buffer, so a change of the generator fails loudly
instead of making the comparison meaningless.
"""
from __future__ import annotations

import numpy as np

from . import model, model377

CURVE_TE, CURVE_BLS12_377 = 0, 1
POINT_BYTES = {CURVE_TE: 64, CURVE_BLS12_377: 96}
SCALAR_BYTES = {CURVE_TE: 32, CURVE_BLS12_377: 48}
ORDER = {CURVE_TE: model.L, CURVE_BLS12_377: model377.R_ORDER}

# Entries summed in uint64 before the totals move to Python ints.  A 16-bit limb is below 2^16 and the index inside a block
# below BLOCK = 2^20, so per block: sum of limbs < 2^20 * 2^16 = 2^36, sum of j * limb < 2^20 * 2^20 * 2^16 = 2^56 < 2^64.
BLOCK = 1 << 20


def scalar_sums(curve: int, sc, lens) -> dict:
    """{L: (S0, S1)} for every L in lens: sum s_i and sum i * s_i over the first L scalar records, as exact Python ints (not reduced).
    One pass over the buffer: the segments between block boundaries and the requested lengths are summed in uint64 (BLOCK bounds them)."""
    sb = SCALAR_BYTES[curve]
    limbs = np.frombuffer(sc, dtype="<u2")
    n = limbs.size // (sb // 2)
    limbs = limbs[: n * (sb // 2)].reshape(n, sb // 2)
    want = sorted({int(x) for x in lens})
    if want and (want[0] < 0 or want[-1] > n):
        raise ValueError(f"prefix lengths must lie in [0, {n}]")
    weights = [1 << (16 * k) for k in range(sb // 2)]
    out, s0, s1, pos = {}, 0, 0, 0
    for L in want:
        while pos < L:
            end = min(L, pos + BLOCK)
            seg = limbs[pos:end].astype(np.uint64)
            j = np.arange(end - pos, dtype=np.uint64)
            tot = seg.sum(axis=0, dtype=np.uint64)
            wtot = (seg * j[:, None]).sum(axis=0, dtype=np.uint64)
            t0 = sum(int(v) * w for v, w in zip(tot, weights))
            s0 += t0
            s1 += pos * t0 + sum(int(v) * w for v, w in zip(wtot, weights))
            pos = end
        out[L] = (s0, s1)
    return out


def _point(curve: int, pts, i: int):
    pb = POINT_BYTES[curve]
    m = model if curve == CURVE_TE else model377
    return m.xy_from_bytes(bytes(pts[pb * i:pb * (i + 1)]))


def _to_bytes(curve: int, pt) -> bytes:
    if curve == CURVE_TE:
        return model.le32(pt[0]) + model.le32(pt[1])
    return model377.result_to_bytes(pt)


def _combine(curve: int, pts, s0: int, s1: int, L: int) -> bytes:
    m = model if curve == CURVE_TE else model377
    ordv = ORDER[curve]
    if L == 0:
        return _to_bytes(curve, model.ZERO if curve == CURVE_TE else model377.INF)
    p0 = _point(curve, pts, 0)
    acc = m.scalar_mul(s0 % ordv, p0)
    if L > 1:
        step = m.add(_point(curve, pts, 1), m.neg(p0))
        acc = m.add(acc, m.scalar_mul(s1 % ordv, step))
    return _to_bytes(curve, acc)


def chain_msms(curve: int, pts, sc, lens) -> list:
    """expected result bytes of the MSM over the first L entries, for every L in lens (in order): one pass over the scalars"""
    sums = scalar_sums(curve, sc, lens)
    return [_combine(curve, pts, *sums[int(L)], int(L)) for L in lens]


def chain_msm(curve: int, pts, sc, L: int | None = None) -> bytes:
    """expected result bytes (64 B Twisted-Edwards x || y, 96 B BLS12-377 x || y with infinity as zeros) of the first L entries
    (default: all of sc) of a chain point buffer"""
    if L is None:
        L = len(sc) // SCALAR_BYTES[curve]
    return chain_msms(curve, pts, sc, [L])[0]


def check_chain(curve: int, pts, idx) -> None:
    """asserts P_i = P_0 + [i] (P_1 - P_0) for every i in idx (the structure chain_msm rests on)"""
    m = model if curve == CURVE_TE else model377
    p0 = _point(curve, pts, 0)
    step = m.add(_point(curve, pts, 1), m.neg(p0))
    for i in idx:
        i = int(i)
        assert _point(curve, pts, i) == m.add(p0, m.scalar_mul(i, step)), f"point {i} is not on the chain"


def sample_indices(n: int, k: int = 32, seed: int = 0) -> list:
    """k indices of [0, n) for check_chain: 0, 1, 2, n - 1 and seeded-random ones"""
    rng = np.random.default_rng(seed)
    fixed = [i for i in (0, 1, 2, n - 1) if 0 <= i < n]
    return sorted(set(fixed) | {int(v) for v in rng.integers(0, n, size=max(0, k - len(fixed)))})
