"""Decoding of BLS12-377 bucket accumulators and projective sums of the bigint model (oracle/model377.py), shared by
tests/test_gpu_bls377_stages.py and tests/test_gpu_sort_thresholds.py.  A plain module."""
import numpy as np

from oracle import model377 as m
from test_oracle_bls377 import _edwards_consts, edwards_to_weierstrass

Q = m.Q
RINV = pow(1 << 406, -1, Q)
ACC = 224                                   # one ete_t<14> accumulator: x | y | z | t, 14 limbs of 29 bits in u32 words

# ---------------------------------------------------------------- model side: projective sums (complete law), decoding
_PINF = (0, 1, 0)


def _proj(pt):
    return _PINF if pt is m.INF else (pt[0], pt[1], 1)


def psum(pts):
    acc = _PINF
    for p in pts:
        acc = m._padd(acc, _proj(p))
    return m._to_affine(acc)


class Decoder:
    def __init__(self, fq377check):
        self.s, self.f, self.d = _edwards_consts(fq377check)

    def point(self, raw):
        """224 bytes of an ete_t<14> (Montgomery form, R = 2^406) -> affine point of y^2 = x^3 + 1 (None = infinity)"""
        words = np.frombuffer(raw, dtype=np.uint32).reshape(4, 14)
        assert np.all(words[:, :13] < (1 << 29)), "limb class N violated"
        X, Y, Z, T = [sum(int(v) << (29 * i) for i, v in enumerate(words[k])) for k in range(4)]
        assert max(X, Y, Z, T) < 1.1 * Q, "product outputs are below 1.1 q (curve.hpp)"
        X, Y, Z, T = (v * RINV % Q for v in (X, Y, Z, T))
        zi = pow(Z, -1, Q)
        xa, ya = X * zi % Q, Y * zi % Q
        assert (-xa * xa + ya * ya - 1 - self.d * xa * xa * ya * ya) % Q == 0, "not on the Edwards curve"
        assert xa * ya % Q == T * zi % Q, "T != XY/Z"
        return edwards_to_weierstrass(xa, ya, self.s, self.f)
