"""Shared by tests/test_field_ops_host.py and tests/test_gpu_field_ops.py: the host shim of csrc/field_ops.hip.hpp
(tests/csrc/fieldopscheck.cpp), the bigint model of te_msm_field_op on wire bytes, and the case lists."""
import ctypes
import functools
import os
import random
import subprocess

from oracle import model as m
from oracle import model377 as b

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELD_P, FIELD_Q377 = 0, 1                                         # TE_MSM_FIELD_*
ADD, SUB, MUL, DOUBLE, NEG, SQUARE, INV, POW, SQRT = range(9)
OPS = {"add": ADD, "sub": SUB, "mul": MUL, "double": DOUBLE, "neg": NEG, "square": SQUARE, "inv": INV, "pow": POW, "sqrt": SQRT}
BINARY = (ADD, SUB, MUL, POW)
SHARED_B, MONTGOMERY, ZERO_OK = 1, 2, 4
ZERO, NOT_SQUARE = 1, 2                                            # reasons
EFIELD = -6
GROUPS = (8, 16, 32, 64)                                           # elements of an inversion chain: every value the measurement tries
M_WALK, M_ZERO, M_LARGER, M_REDUCE = 1, 2, 4, 8                    # the shim's deliberate mistakes
FIELDS = (FIELD_P, FIELD_Q377)


def modulus(field):
    return b.Q if field == FIELD_Q377 else m.P


def nbytes(field):
    return 48 if field == FIELD_Q377 else 32


def b_bytes(field, op):
    return 32 if op == POW else nbytes(field)                      # an exponent is 32 bytes on both fields


def pack(vals, size):
    return b"".join(int(v).to_bytes(size, "little") for v in vals)


def unpack(raw, size):
    return [int.from_bytes(raw[i:i + size], "little") for i in range(0, len(raw), size)]


def shim():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libfieldopscheck.so"), os.path.join(d, "fieldopscheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("field_ops.hip.hpp", "scalar_mul.hip.hpp", "from_x.hip.hpp", "check.hip.hpp", "fp.hpp", "fq377.hpp",
                                                         "field.hpp", "curve.hpp", "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    ci, vp, u64, u32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.fo_field_op.argtypes = [ci, ci, vp, vp, u64, ci, u32, ci, vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ci)]
    L.fo_field_op.restype = ci
    return L


def shim_op(L, field, op, a, bb=None, flags=0, group=16, mistake=0, in_place=False, fill=0xA5):
    """(rc, out bytes, lowest failing index, reason); the output starts as `fill` bytes, or -- in_place -- as a itself"""
    eb = nbytes(field)
    n = len(a) // eb
    buf_a = ctypes.create_string_buffer(bytes(a), max(1, len(a)))
    out = buf_a if in_place else ctypes.create_string_buffer(bytes([fill]) * max(1, eb * n), max(1, eb * n))
    buf_b = ctypes.create_string_buffer(bytes(bb), len(bb)) if bb else None
    bad, why = ctypes.c_int64(), ctypes.c_int()
    rc = L.fo_field_op(field, op, ctypes.addressof(buf_a), ctypes.addressof(buf_b) if buf_b else None, n, flags, group, mistake,
                       ctypes.addressof(out), ctypes.byref(bad), ctypes.byref(why))
    return rc, out.raw[:eb * n], bad.value, why.value


# ---- the model: Python integers ---------------------------------------------------------------------------------------------------
def tonelli(a, p):
    """a square root of a mod p, or None (any odd prime; p - 1 = 2^s t)"""
    a %= p
    if a == 0:
        return 0
    if pow(a, (p - 1) // 2, p) != 1:
        return None
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (p - 1) // 2, p) == 1:
        z += 1
    c, r, u, k = pow(z, t, p), pow(a, (t + 1) // 2, p), pow(a, t, p), s
    while u != 1:
        i, w = 0, u
        while w != 1:
            w, i = w * w % p, i + 1
        f = pow(c, 1 << (k - i - 1), p)
        r, c, k = r * f % p, f * f % p, i
        u = u * c % p
    return r


def model_op(field, op, a, bb=None, flags=0):
    """te_msm_field_op on wire bytes: (0, out bytes, -1, 0), or (EFIELD, None, lowest failing index, reason)"""
    p, eb = modulus(field), nbytes(field)
    A = 1 << (8 * eb)
    mont = bool(flags & MONTGOMERY)
    dec = (lambda x: x * pow(A, -1, p) % p) if mont else (lambda x: x % p)
    enc = (lambda v: v * A % p) if mont else (lambda v: v % p)
    av = [dec(x) for x in unpack(a, eb)]
    n = len(av)
    bv = None
    if op in BINARY:
        raw = unpack(bb, b_bytes(field, op))
        raw = raw * n if flags & SHARED_B else raw
        bv = raw if op == POW else [dec(x) for x in raw]            # an exponent is the integer itself
    out = []
    for i, v in enumerate(av):
        if op == ADD:
            r = v + bv[i]
        elif op == SUB:
            r = v - bv[i]
        elif op == MUL:
            r = v * bv[i]
        elif op == DOUBLE:
            r = 2 * v
        elif op == NEG:
            r = -v
        elif op == SQUARE:
            r = v * v
        elif op == INV:
            if v == 0 and not flags & ZERO_OK:
                return EFIELD, None, i, ZERO
            r = pow(v, -1, p) if v else 0
        elif op == POW:
            r = pow(v, bv[i], p)
        else:
            r = tonelli(v, p)
            if r is None:
                return EFIELD, None, i, NOT_SQUARE
            r = min(r, p - r) if r else 0
        out.append(enc(r % p))
    return 0, pack(out, eb), -1, 0


# ---- case lists -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def extremes(field):
    """limb-class extremes as raw integers: 0, 1, m - 1, m, m + 1, all ones (every 29-bit limb full), a single bit at every limb
    boundary and the value just below it, and a few random residues and random full-width values"""
    p, bits = modulus(field), 8 * nbytes(field)
    rnd = random.Random(0xE17 + field)
    v = [0, 1, p - 1, p, p + 1, (1 << bits) - 1, (1 << bits) - p]
    for k in range(1, (bits + 28) // 29):
        v += [1 << (29 * k), (1 << (29 * k)) - 1]
    v += [rnd.randrange(p) for _ in range(6)] + [rnd.randrange(1 << bits) for _ in range(6)]
    return tuple(v)


@functools.lru_cache(maxsize=None)
def binary_operands(field):
    """(a bytes, b bytes): every extreme against every one of the first seven, and against itself rotated"""
    ex, eb = extremes(field), nbytes(field)
    pairs = [(x, y) for x in ex for y in ex[:7]] + list(zip(ex, ex[3:] + ex[:3]))
    return pack([x for x, _ in pairs], eb), pack([y for _, y in pairs], eb)


@functools.lru_cache(maxsize=None)
def unary_operands(field):
    return pack(extremes(field), nbytes(field))


@functools.lru_cache(maxsize=None)
def nonzero_operands(field):
    """the extremes whose residue is not 0 -- in either form: x A^-1 is 0 exactly when x is"""
    p = modulus(field)
    return pack([x for x in extremes(field) if x % p], nbytes(field))


def root_of_unity(field):
    """an element of order 2^S (S = 47 / 46) and the smallest non-square it is a power of (11 mod p, 5 mod q)"""
    p = modulus(field)
    s, t = 0, p - 1
    while t % 2 == 0:
        s, t = s + 1, t // 2
    z = 2
    while pow(z, (p - 1) // 2, p) == 1:
        z += 1
    return pow(z, t, p), z, s


@functools.lru_cache(maxsize=None)
def sqrt_inputs(field):
    """(squares, non-squares) as raw integers: (g^(2^k))^2 for every k < S -- Tonelli-Shanks corrects a different number of times for
    each -- and 0, 1, 4; the same values times the non-square"""
    p = modulus(field)
    g, z, s = root_of_unity(field)
    sq = [pow(pow(g, 1 << k, p), 2, p) for k in range(s)] + [4, 9 * pow(g, 3, p) ** 2 % p]
    return tuple([0] + sq), tuple(x * z % p for x in sq)


@functools.lru_cache(maxsize=None)
def pow_exponents(field):
    """every 2-bit window value at the top, a middle and the bottom window, all ones, and 0, 1, 17, m - 2, m - 1, m, m + 5"""
    p = modulus(field)
    e = [d << sh for sh in (254, 126, 0) for d in range(4)] + [(3 << 254) | (2 << 126) | 1, (1 << 256) - 1, 0, 1, 17]
    return tuple(e + [x for x in (p - 2, p - 1, p, p + 5) if x < 1 << 256])


@functools.lru_cache(maxsize=None)
def pow_operands(field):
    """(a bytes, exponent bytes): a few bases, 0 among them (0^0 = 1), against every exponent"""
    p = modulus(field)
    rnd = random.Random(0x90 + field)
    bases = [0, 1, p - 1, 3, (1 << (8 * nbytes(field))) - 1, rnd.randrange(p)]
    pairs = [(x, e) for x in bases for e in pow_exponents(field)]
    return pack([x for x, _ in pairs], nbytes(field)), pack([e for _, e in pairs], 32)


# ---- the piece loops of points.hip (tests/test_gpu_piece_loops.py, pinned on the host by tests/test_piece_cases_host.py) ---------------
def piece_constant(name):
    """a `constexpr uint64_t <name> = 1ull << N;` of points.hip as an integer; a line that is gone is an error, never a default"""
    import re
    src = open(os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc", "points.hip")).read()
    found = re.findall(r"^constexpr uint64_t %s = 1ull << (\d+);" % re.escape(name), src, re.M)
    assert len(found) == 1, "points.hip: %d lines define %s" % (len(found), name)
    return 1 << int(found[0])


TILE = 4099                                                        # prime: a pattern of this period lines up with no tile, chain or piece


@functools.lru_cache(maxsize=None)
def tile_set(field, zeros=True):
    """TILE raw values: the extremes, 2 m, and random full-width integers; without `zeros`, 1 stands where a residue would be 0"""
    p, bits = modulus(field), 8 * nbytes(field)
    rnd = random.Random(0x4099 + field)
    v = list(extremes(field)) + [2 * p]
    v += [rnd.randrange(1 << bits) for _ in range(TILE - len(v))]
    rnd.shuffle(v)
    assert sum(1 for x in v if x % p == 0) >= 3
    return tuple(v if zeros else [x if x % p else 1 for x in v])


@functools.lru_cache(maxsize=None)
def tile_inverses(field, flags, zeros=True):
    """what te_msm_field_op(INV) makes of tile_set: TILE integers, 0 for a zero residue.  MONTGOMERY: x = a A -> (1 / a) A = A^2 / x"""
    p, A = modulus(field), 1 << (8 * nbytes(field))
    k = A * A % p if flags & MONTGOMERY else 1
    return tuple(pow(x, -1, p) * k % p if x % p else 0 for x in tile_set(field, zeros))


def tiled(table, n):
    """v[i] = table[i % TILE], as bytes: the host's form of the index_select the GPU tests do on the device"""
    return b"".join(table[i % TILE] for i in range(n))


def inv_sizes(group):
    t = 256 * group
    return (1, 255, 256, 257, t - 1, t, t + 1, 2 * t + 300)


@functools.lru_cache(maxsize=None)
def inv_values(field, n, group, zeros=True):
    """n raw values: random full-width integers; with `zeros`, planted in the chains of the first tile (lane l of a block owns elements
    l, l + 256, ..): a zero at the first / a middle / the last position of the chains of lanes 3 / 4 / 5, a whole chain of zeros
    (lane 6), the only non-zero of a chain (lane 7), and the multiples m and 2 m as zeros"""
    p, bits = modulus(field), 8 * nbytes(field)
    rnd = random.Random(n * 131 + group * 7 + field)
    v = [rnd.randrange(1, 1 << bits) for _ in range(n)]
    v = [x if x % p else 1 for x in v]
    if zeros:
        def put(lane, j, x):
            if j * 256 + lane < n:
                v[j * 256 + lane] = x
        put(3, 0, 0)
        put(4, group // 2, p)
        put(5, group - 1, 2 * p)
        for j in range(group):
            put(6, j, 0)
            if j != 1:
                put(7, j, 0)
        if n > 9:
            v[n - 1] = 0
    return tuple(v)
