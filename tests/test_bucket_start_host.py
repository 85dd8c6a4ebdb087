"""The two-record bucket start of k_accumulate (csrc/curve.hpp ete_from_pair: 1 + 7 products for the first two entries of a segment
instead of a conversion and an addition, 3 + 7), compiled for the host by tests/csrc/pairstart.cpp -- the same limb code the GPU runs --
for both curves and every record kind the kernel gathers:
  * ete_from_pair(a, b) and ete_madd(ete_from_pnt(a), b) are the same projective point, and that point is the bigint model's a + b,
    for subgroup points, b = a, b = -a, the neutral element on either side, and the four sign combinations through pnt_cneg;
  * every output coordinate is in the class the comment states (class N, value below 1.02 p);
  * replayed on BOUNDS (as tests/test_limb_bounds_te.py / test_limb_bounds_bls377.py do for the additions) no 64-bit column wraps and
    every offset subtraction has a subtrahend it covers; the 14-limb host build checks every column of the runs above as well."""
import ctypes
import os
import subprocess

import pytest

from oracle import model377 as m377

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB = 29
LM = (1 << LB) - 1
U32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def ps(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("pairstart") / "libpairstart.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "csrc", "pairstart.cpp")])
    L = ctypes.CDLL(so)
    L.ps_record.argtypes = [ctypes.c_char_p, ctypes.POINTER(U32)]
    L.ps377_record.argtypes = [ctypes.c_char_p, ctypes.POINTER(U32)]
    return L


def val(ls):
    return sum(int(x) << (LB * i) for i, x in enumerate(ls))


def limbs(v, nl):
    """class N: nl - 1 limbs of 29 bits, the rest in the top limb"""
    return [(v >> (LB * i)) & LM for i in range(nl - 1)] + [v >> (LB * (nl - 1))]


def class_n(ls, modulus, nl):
    """limbs below 2^29 except the top one, value below 1.02 x the modulus"""
    return all(int(x) <= LM for x in ls[:nl - 1]) and val(ls) < modulus + modulus // 50


def check_pair(call_pair, call_ref, ra, rb, nl, modulus, want, name=lambda x, y: (x, y)):
    """both forms for the four sign combinations: classes, the extended-coordinate invariant, equality as projective points and with
    the model's sum want(neg_a, neg_b); name(x, y) turns the affine Edwards point into the model's name of it"""
    for na in (0, 1):
        for nb in (0, 1):
            out = []
            for f in (call_pair, call_ref):
                o = (U32 * (4 * nl))()
                f((U32 * len(ra))(*ra), na, (U32 * len(rb))(*rb), nb, o)
                c = [list(o[nl * k:nl * k + nl]) for k in range(4)]                  # x | y | z | t
                assert all(class_n(ls, modulus, nl) for ls in c), (na, nb)
                out.append([val(ls) % modulus for ls in c])
            (X, Y, Z, T), (X2, Y2, Z2, T2) = out
            assert Z != 0 and Z2 != 0
            assert (X * Z2 - X2 * Z) % modulus == 0 and (Y * Z2 - Y2 * Z) % modulus == 0 and (T * Z2 - T2 * Z) % modulus == 0, (na, nb)
            assert (T * Z - X * Y) % modulus == 0, (na, nb)                          # T = X Y / Z (both sides carry R^2)
            zi = pow(Z, -1, modulus)
            assert name(X * zi % modulus, Y * zi % modulus) == want(na, nb), (na, nb)


# ------------------------------------------------------------------ Twisted-Edwards BLS12, 9 limbs
def test_pair_start_is_the_sum_on_the_twisted_edwards_curve(ps, model):
    P = model.P
    rec = {}

    def record(pt):
        if pt not in rec:
            out = (U32 * 27)()
            ps.ps_record(model.points_to_bytes([pt]), out)
            rec[pt] = list(out)
        return rec[pt]

    pts = model.gen_points(0xB0C, 24) + model.gen_points_random(0xB0C, 6)
    pairs = list(zip(pts[:-1], pts[1:]))
    a = pts[3]
    pairs += [(a, a), (a, model.neg(a)), (model.ZERO, a), (a, model.ZERO), (model.ZERO, model.ZERO), (model.neg(a), model.neg(a))]
    sign = lambda pt, n: model.neg(pt) if n else pt
    for pa, pb in pairs:
        assert model.on_curve(pa) and model.on_curve(pb)
        check_pair(ps.ps_pair, ps.ps_convert_add, record(pa), record(pb), 9, P,
                   lambda na, nb: model.add(sign(pa, na), sign(pb, nb)))


# ------------------------------------------------------------------ BLS12-377 G1 in its twisted-Edwards form, 14 limbs
def _edwards_map(ps):
    """Edwards (x, y) -> short Weierstrass (None = infinity), with the constants s and f as the device header holds them"""
    Q, R = m377.Q, 1 << (14 * LB)
    c = (U32 * 56)()
    ps.ps377_constants(c)
    v = [val(c[14 * k:14 * k + 14]) for k in range(4)]
    rinv = pow(R, -1, Q)
    assert v[0] % Q == R % Q
    s, f = v[2] * rinv * rinv % Q, v[3] * rinv % Q

    def to_sw(x, y):
        if x == 0:
            return None if y == 1 else (Q - 1, 0)
        u = (1 + y) * pow(1 - y, -1, Q) % Q
        w = f * u * pow(x, -1, Q) % Q
        return ((u * pow(s, -1, Q) - 1) % Q, w * pow(s, -1, Q) % Q)
    return to_sw


def test_pair_start_is_the_sum_on_bls12_377_for_both_record_kinds(ps):
    Q, R = m377.Q, 1 << (14 * LB)
    to_sw = _edwards_map(ps)
    half_R = pow(2, -1, Q) * R % Q
    proj, aff = {}, {}

    def record(pt):
        """(projective record, affine record) of a short-Weierstrass point; the neutral element is (1, 1, 0, 2) times anything,
        and (1/2, 1/2, 0) affine"""
        if pt not in proj:
            if pt is None:
                proj[pt] = limbs(R % Q, 14) * 2 + [0] * 14 + limbs(2 * R % Q, 14)
                aff[pt] = limbs(half_R, 14) * 2 + [0] * 14
            else:
                out = (U32 * 56)()
                ps.ps377_record(m377.points_to_bytes([pt]), out)
                proj[pt] = list(out)
                hm, hp, dt, z = (val(out[14 * k:14 * k + 14]) for k in range(4))
                zi = pow(z, -1, Q) * R % Q                                           # (hm' R) / (z' R) * R: Montgomery form of hm' / z'
                aff[pt] = sum((limbs(c * zi % Q, 14) for c in (hm, hp, dt)), [])
        return proj[pt], aff[pt]

    pts = m377.gen_points(0xB0C, 16)
    pairs = list(zip(pts[:-1], pts[1:]))
    a = pts[5]
    pairs += [(a, a), (a, m377.neg(a)), (None, a), (a, None), (None, None), (m377.neg(a), m377.neg(a))]
    sign = lambda pt, n: m377.neg(pt) if n else pt
    ps.ps377_overflow_and_reset()
    for pa, pb in pairs:
        for kind, (pair, ref) in enumerate(((ps.ps377_pair, ps.ps377_convert_add), (ps.ps377_pair_aff, ps.ps377_convert_add_aff))):
            check_pair(pair, ref, record(pa)[kind], record(pb)[kind], 14, Q,
                       lambda na, nb: m377.add(sign(pa, na), sign(pb, nb)), to_sw)
    assert ps.ps377_overflow_and_reset() == 0                   # no column of any product above wrapped


# ------------------------------------------------------------------ the limb rule, on bounds
class B:
    def __init__(self, lim, top, val):
        self.lim, self.top, self.val = lim, top, val


class Bounds:
    """interval arithmetic over (largest ordinary limb, largest top limb, largest value in units of the modulus) for a field of nl
    limbs: every product's worst column must stay below 2^64, every offset subtraction must cover its subtrahend"""

    def __init__(self, nl, modulus):
        self.nl, self.m, self.worst = nl, modulus, 0.0

    def N(self, v):
        return B(LM, int(v * self.m) >> (LB * (self.nl - 1)), v)

    def add(self, a, b):
        return B(a.lim + b.lim, a.top + b.top, a.val + b.val)

    def offset(self, K):
        v = K * self.m
        l = limbs(v, self.nl)
        for i in range(self.nl - 1):
            l[i] += 1 << LB
            l[i + 1] -= 1
        return max(l[:-1]), l[-1]

    def sub(self, a, b, K):
        ol, ot = self.offset(K)
        assert b.lim <= LM and b.top <= ot and b.val < K, "subtrahend must be normalised and below the offset"
        return B(a.lim + ol, a.top + ot, a.val + K)

    def neg(self, b, K):
        ol, ot = self.offset(K)
        assert b.lim <= LM and b.top <= ot
        return B(ol, ot, K)

    def norm(self, a):
        assert a.lim < 1 << 32 and a.top + (a.lim >> LB) + 1 < 1 << 32
        return self.N(a.val)

    def mul(self, a, b):
        ma, mb = max(a.lim, a.top), max(b.lim, b.top)
        col = self.nl * ma * mb + (self.nl - 1) * LM * LM + LM
        self.worst = max(self.worst, col / 2.0 ** 64)
        assert col < 1 << 64, f"column overflow: limbs up to 2^{ma.bit_length()} x 2^{mb.bit_length()}"
        return self.N(a.val * b.val * self.m / 2.0 ** (LB * self.nl) + 1.0)


def _pair_on_bounds(F, rec_a, rec_b, wide_ok):
    """ete_from_pair replayed on bounds; wide_ok: the 9-limb rule (difference x sum is exact), else one operand of every product is
    normalised (E before it meets H, E3 and G in ete_close).

    This is a RE-STATEMENT of csrc/curve.hpp, line for line: the compiled 14-limb code also checks its own columns
    (TE377_CHECK_COLUMNS in pairstart.cpp), the 9-limb code has no such switch and is bounded only here.  Whoever edits
    ete_from_pair(const pnt&, const pnt&), its pnt_aff377 twin or ete_close edits the marked line below with it."""
    nrm = (lambda x: x) if wide_ok else F.norm
    hm1, hp1, _ = rec_a
    hm2, hp2, dt2 = rec_b
    # T1 = mont_mul(fp_add(a.hp, a.hm), fp_sub<2>(a.hp, a.hm))          [14 limbs: fe_norm around the difference]
    T1 = F.mul(F.add(hp1, hm1), nrm(F.sub(hp1, hm1, 2)))
    # in1 = {fp_add(a.hm, a.hm), fp_add(a.hp, a.hp), T1}, in2 = {b.hm, b.hp, b.dt}; mont_mul_x<3>(in1, in2, abc)
    A, Bp, Cn = F.mul(F.add(hm1, hm1), hm2), F.mul(F.add(hp1, hp1), hp2), F.mul(T1, dt2)
    # one = fp_R1(); ete_close(fp_sub<2>(B, A), fp_add(B, A), fp_add(one, Cn), fp_sub<2>(one, Cn))
    one = F.N(1.0)
    E, H, Fs, G = nrm(F.sub(Bp, A, 2)), F.add(Bp, A), F.add(one, Cn), nrm(F.sub(one, Cn, 2))
    # ete_close: x = E F, y = H G, z = F G, t = E H                       [14 limbs: E and G normalised first]
    return F.mul(E, Fs), F.mul(H, G), F.mul(G, Fs), F.mul(E, H)


@pytest.mark.parametrize("nl,wide_ok", [(9, True), (14, False)])
def test_limb_rule_holds_for_every_product_of_the_pair_start(model, nl, wide_ok):
    F = Bounds(nl, model.P if nl == 9 else m377.Q)
    rec = (F.N(1.1), F.N(1.1), F.N(1.1))                        # record fields: class N, below 1.1 p
    rec_neg = (rec[1], rec[0], F.neg(F.N(1.1), 4))              # pnt_cneg: hm <-> hp, 4p - dt
    for ra in (rec, rec_neg):
        for rb in (rec, rec_neg):
            out = _pair_on_bounds(F, ra, rb, wide_ok)
            assert all(c.lim == LM and c.val < 1.02 for c in out)          # class N, below 1.02 p: what ete_madd takes next
    assert 0.5 < F.worst < 1.0                                  # the rule is tight, not vacuous
