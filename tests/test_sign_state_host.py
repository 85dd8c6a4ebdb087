"""The sign state of k_accumulate (csrc/curve.hpp ete_open / ete_uv_neg / ete_madd_raw and the SGN closings: an entry's sign lives in the
accumulator, Q - P = -((-Q) + P), and every record is added as loaded), compiled for the host by tests/csrc/signstate.cpp -- the same limb
code the GPU runs, the kernel's statements for one segment -- for both curves and every record kind the kernel gathers:
  * a segment of 1 ... 6 entries with EVERY sign pattern is the bigint model's signed sum, and the same projective point as the earlier
    form (every record negated by pnt_cneg, added with ete_madd); a sorted pattern pays at most one sign change;
  * continued accumulators (`onto`) at the neutral element, (0, -1), the points of order 4, and P with -P and with P (inverse, doubling);
  * negating the opened form twice gives it back limb for limb, once gives (V, U, Z, -T) mod p with limbs below 2^30.6 / 2^30;
  * what a lane stores, flipped or not, is class N and below 2p, as oracle/stage_checks.py asks of the buckets -- in fact four product
    outputs below 1.02 p: the segment's last addition closes into the true sign, nothing is negated behind it;
  * replayed on BOUNDS and iterated to a fixed point (as tests/test_limb_bounds_te.py does for the additions) no 64-bit column wraps
    and every offset subtraction has a subtrahend it covers, negated or not, for 9 and 14 limbs; the 14-limb host build checks every
    column of the runs above as well."""
import ctypes
import itertools
import os
import subprocess

import pytest

from oracle import model377 as m377

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LB = 29
LM = (1 << LB) - 1
U32 = ctypes.c_uint32
I32 = ctypes.c_int


@pytest.fixture(scope="module")
def ss(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("signstate") / "libsignstate.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", so, os.path.join(ROOT, "tests", "csrc", "signstate.cpp")])
    L = ctypes.CDLL(so)
    L.ss_record.argtypes = [ctypes.c_char_p, ctypes.POINTER(U32)]
    L.ss377_record.argtypes = [ctypes.c_char_p, ctypes.POINTER(U32)]
    return L


def val(ls):
    return sum(int(x) << (LB * i) for i, x in enumerate(ls))


def limbs(v, nl):
    """class N: nl - 1 limbs of 29 bits, the rest in the top limb"""
    return [(v >> (LB * i)) & LM for i in range(nl - 1)] + [v >> (LB * (nl - 1))]


def stored_form(coords, modulus, nl):
    """what the buckets and seg_out hold: limbs below 2^29 except the top one, value below 2 x the modulus -- and, being product
    outputs (or the 1 of an affine start), below 1.02 x the modulus, which the offset of the next subtraction needs with 14 limbs"""
    return all(all(int(x) <= LM for x in ls[:nl - 1]) and val(ls) < 2 * modulus and val(ls) < modulus + modulus // 50 for ls in coords)


def run(f, recs, signs, nl, onto=None, trace=True):
    flat = [w for r in recs for w in r]
    out, tr = (U32 * (4 * nl))(), (U32 * 3)()
    args = [(U32 * max(1, len(flat)))(*flat), (I32 * max(1, len(signs)))(*signs), len(signs), (U32 * (4 * nl))(*onto) if onto else None, out]
    f(*(args + [tr] if trace else args))
    return [list(out[nl * k:nl * k + nl]) for k in range(4)], list(tr)


def affine(coords, modulus):
    """(x, y) of an accumulator x | y | z | t, after checking T = X Y / Z"""
    X, Y, Z, T = (val(ls) % modulus for ls in coords)
    assert Z != 0 and (T * Z - X * Y) % modulus == 0
    zi = pow(Z, -1, modulus)
    return X * zi % modulus, Y * zi % modulus


def same_point(c1, c2, modulus):
    (X, Y, Z, T), (X2, Y2, Z2, T2) = ([val(ls) % modulus for ls in c] for c in (c1, c2))
    return (X * Z2 - X2 * Z) % modulus == 0 and (Y * Z2 - Y2 * Z) % modulus == 0 and (T * Z2 - T2 * Z) % modulus == 0


def patterns(upto):
    for n in range(1, upto + 1):
        yield from itertools.product((0, 1), repeat=n)


def changes(signs, first):
    """sign changes a lane pays for: from its flag at the start (`first`) along the entries"""
    return sum(1 for a, b in zip((first,) + tuple(signs), signs) if a != b)


# ------------------------------------------------------------------ Twisted-Edwards BLS12, 9 limbs
def _records(ss, model, pts):
    out = []
    for pt in pts:
        o = (U32 * 27)()
        ss.ss_record(model.points_to_bytes([pt]), o)
        out.append(list(o))
    return out


def _ete(model, pt):
    """the accumulator (x R, y R, R, x y R) of an affine point, class N"""
    R = 1 << (9 * LB)
    x, y = pt
    return sum((limbs(c % model.P, 9) for c in (x * R, y * R, R, x * y * R)), [])


def _signed_sum(model, start, pts, signs):
    acc = start
    for pt, s in zip(pts, signs):
        acc = model.add(acc, model.neg(pt) if s else pt)
    return acc


def test_every_sign_pattern_is_the_signed_sum_on_the_twisted_edwards_curve(ss, model):
    pts = model.gen_points(0x51C4, 5) + model.gen_points_random(0x51C4, 1)
    recs = _records(ss, model, pts)
    for signs in patterns(6):
        n = len(signs)
        got, tr = run(ss.ss_segment, recs[:n], signs, 9)
        ref, _ = run(ss.ss_segment_cneg, recs[:n], signs, 9, trace=False)
        assert stored_form(got, model.P, 9), signs
        assert same_point(got, ref, model.P), signs
        assert affine(got, model.P) == _signed_sum(model, model.ZERO, pts, signs), signs
        # the pair start takes the first sign as the flag and the second entry under pnt_cneg: changes are paid from entry 2 on
        assert tr[2] == (changes(signs[2:], signs[0]) if n > 2 else 0), signs
        assert tr[0] < 2 ** 30.6 and tr[1] < 1 << 30, signs
        if list(signs) == sorted(signs):
            assert tr[2] <= 1                                # positive entries first: one change per segment at most


def test_continued_accumulators_at_the_special_points(ss, model):
    """`onto`: the segment continues a stored sum and starts unflipped -- at the neutral element, the point of order 2, both points of
    order 4, and P itself, so that the first entry makes P + (-P) and P + P; then two more entries of either sign"""
    P = model.P
    i = model.sqrt_mod_p(P - 1)
    assert i is not None and i * i % P == P - 1
    pts = model.gen_points(0x51C4, 3)
    p0 = pts[0]
    specials = [model.ZERO, (0, P - 1), (i, 0), (P - i, 0), p0, model.neg(p0)]
    assert all(model.on_curve(q) for q in specials)
    recs = _records(ss, model, pts)
    for q in specials:
        for signs in patterns(3):
            n = len(signs)
            got, tr = run(ss.ss_segment, recs[:n], signs, 9, onto=_ete(model, q))
            assert stored_form(got, P, 9), (q, signs)
            assert affine(got, P) == _signed_sum(model, q, pts, signs), (q, signs)
            assert tr[2] == changes(signs, 0), (q, signs)
        got, _ = run(ss.ss_segment, [], [], 9, onto=_ete(model, q))          # an empty continuation stores what it loaded
        assert got == [_ete(model, q)[9 * k:9 * k + 9] for k in range(4)]
    # the same cases at a segment's start, through the pair: P, P and P, -P by either route (record sign or entry sign)
    for signs in patterns(4):
        n = len(signs)
        got, _ = run(ss.ss_segment, [recs[0]] * n, signs, 9)
        assert affine(got, P) == _signed_sum(model, model.ZERO, [p0] * n, signs), signs


def _check_open_neg(open_neg, acc, nl, modulus):
    flat = sum(acc, [])
    o = [(U32 * (4 * nl))() for _ in range(3)]
    for times in range(3):
        open_neg((U32 * (4 * nl))(*flat), times, o[times])
    u0, v0, z0, t0 = ([list(o[0][nl * k:nl * k + nl]) for k in range(4)])
    u1, v1, z1, t1 = ([list(o[1][nl * k:nl * k + nl]) for k in range(4)])
    assert list(o[2]) == list(o[0])                          # twice: the identity, limb for limb
    assert u1 == v0 and v1 == u0 and z1 == z0
    assert (val(t1) + val(t0)) % modulus == 0
    assert max(t1[:nl - 1]) < 1 << 30 and max(u0[:nl - 1] + v0[:nl - 1]) < 2 ** 30.6
    X, Y = val(acc[0]), val(acc[1])
    assert (val(u0) - (Y - X)) % modulus == 0 and (val(v0) - (Y + X)) % modulus == 0


def test_negation_of_the_opened_form(ss, model):
    recs = _records(ss, model, model.gen_points(0x51C4, 4))
    for n in (1, 2, 3, 4):
        acc, _ = run(ss.ss_segment, recs[:n], [0] * n, 9)
        _check_open_neg(ss.ss_open_neg, acc, 9, model.P)
    pts = m377.gen_points(0x51C4, 3)
    for n in (1, 3):
        rr = []
        for k in range(n):
            o = (U32 * 56)()
            ss.ss377_record(m377.points_to_bytes([pts[k]]), o)
            rr.append(list(o))
        acc, _ = run(ss.ss377_segment, rr, [0] * n, 14)
        _check_open_neg(ss.ss377_open_neg, acc, 14, m377.Q)


# ------------------------------------------------------------------ BLS12-377 G1 in its twisted-Edwards form, 14 limbs
def _edwards_map(ss):
    """Edwards (x, y) -> short Weierstrass (None = infinity), with the constants s and f as the device header holds them"""
    Q, R = m377.Q, 1 << (14 * LB)
    c = (U32 * 56)()
    ss.ss377_constants(c)
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


def test_every_sign_pattern_is_the_signed_sum_on_bls12_377_for_both_record_kinds(ss):
    Q, R = m377.Q, 1 << (14 * LB)
    to_sw = _edwards_map(ss)
    pts = list(m377.gen_points(0x51C4, 6))
    pts[3] = pts[1]                                          # a doubling and an inverse inside the patterns
    proj, aff = [], []
    for pt in pts:
        o = (U32 * 56)()
        ss.ss377_record(m377.points_to_bytes([pt]), o)
        proj.append(list(o))
        hm, hp, dt, z = (val(o[14 * k:14 * k + 14]) for k in range(4))
        zi = pow(z, -1, Q) * R % Q                           # (hm' R) / (z' R) * R: Montgomery form of hm' / z'
        aff.append(sum((limbs(c * zi % Q, 14) for c in (hm, hp, dt)), []))
    ss.ss377_overflow_and_reset()
    for signs in patterns(6):
        n = len(signs)
        want = None
        for pt, s in zip(pts, signs):
            want = m377.add(want, m377.neg(pt) if s else pt)
        for kind, (f, recs) in enumerate(((ss.ss377_segment, proj), (ss.ss377_segment_aff, aff))):
            got, tr = run(f, recs[:n], signs, 14)
            assert stored_form(got, Q, 14), (kind, signs)
            assert to_sw(*affine(got, Q)) == want, (kind, signs)
            assert tr[2] == (changes(signs[2:], signs[0]) if n > 2 else 0), (kind, signs)
            assert tr[0] < 2 ** 30.6 and tr[1] < 1 << 30, (kind, signs)
        # continued from a stored sum (the projective result of the first entries), unflipped at its start
        if n >= 3:
            head, _ = run(ss.ss377_segment_aff, aff[:2], signs[:2], 14)
            got, tr = run(ss.ss377_segment_aff, aff[2:n], signs[2:], 14, onto=sum(head, []))
            assert stored_form(got, Q, 14) and to_sw(*affine(got, Q)) == want, signs
            assert tr[2] == changes(signs[2:], 0), signs
    assert ss.ss377_overflow_and_reset() == 0                # no column of any product above wrapped


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
        l = limbs(K * self.m, self.nl)
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
        assert b.lim <= LM and b.top <= ot and b.val < K
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


def _addition_on_bounds(F, acc, rec, negate, wide_ok, neg_out=False):
    """ete_open, ete_uv_neg (if negate) and ete_madd_raw replayed on bounds: a RE-STATEMENT of csrc/curve.hpp, line for line -- whoever
    edits those functions or ete_close edits the marked lines with them.  rec: (hm, hp, dt) or (hm, hp, dt, z)."""
    nrm = (lambda x: x) if wide_ok else F.norm
    X, Y, Z, T = acc
    # ete_open: r.u = fe_sub<2>(a.y, a.x); r.v = fe_add(a.y, a.x)
    u, v, t = F.sub(Y, X, 2), F.add(Y, X), T
    if negate:
        # ete_uv_neg: swap(u, v); a.t = fe_neg<2>(a.t)
        u, v, t = v, u, F.neg(T, 2)
        assert t.lim < 1 << 30
    # ete_madd_raw: in1 = {a.u, a.v, a.t [, a.z]}, in2 = {b.hm, b.hp, b.dt [, b.z]}
    A, Bp, Cn = F.mul(u, rec[0]), F.mul(v, rec[1]), F.mul(t, rec[2])
    D = F.mul(Z, rec[3]) if len(rec) == 4 else Z
    # ete_close(fe_sub<2>(B, A), fe_add(B, A), fe_add(D, Cn), fe_sub<2>(D, Cn))         [14 limbs: E and G normalised]
    # fe_diff<SGN>: E = B - A, or A - B where the segment's last addition closes into a negated sum
    E = nrm(F.sub(A, Bp, 2)) if neg_out else nrm(F.sub(Bp, A, 2))
    H, Fs, G = F.add(Bp, A), F.add(D, Cn), nrm(F.sub(D, Cn, 2))
    # x = E F, y = H G, z = G F, t = E H
    return F.mul(E, Fs), F.mul(H, G), F.mul(G, Fs), F.mul(E, H)


@pytest.mark.parametrize("nl,wide_ok,fields", [(9, True, 3), (14, False, 3), (14, False, 4)], ids=["9-affine", "14-affine", "14-projective"])
def test_limb_rule_holds_at_the_fixed_point_negated_or_not(model, nl, wide_ok, fields):
    F = Bounds(nl, model.P if nl == 9 else m377.Q)
    rec = tuple(F.N(1.1) for _ in range(fields))             # record fields as loaded: class N, below 1.1 p -- never negated
    state = (F.N(1.1),) * 4                                  # what a continued bucket holds: product outputs, class N, below 1.1p
    for _ in range(16):
        outs = [_addition_on_bounds(F, state, rec, negate, wide_ok) for negate in (False, True)]
        nxt = tuple(F.N(max(o[k].val for o in outs)) for k in range(4))
        assert all(c.lim == LM and c.val < 1.02 for c in nxt)                # class N, below 1.02 p: the loop's invariant
        if all(a.val == b.val and a.top == b.top for a, b in zip(nxt, state)):
            break
        state = nxt
    else:
        raise AssertionError("the bounds did not reach a fixed point")
    # the last addition of a flipped lane: the same closing with A - B for E
    for negate in (False, True):
        assert all(c.lim == LM and c.val < 1.02 for c in _addition_on_bounds(F, state, rec, negate, wide_ok, neg_out=True))
    assert 0.4 < F.worst < 1.0                               # the rule is tight, not vacuous
