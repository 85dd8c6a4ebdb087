"""Cases of the fixed-base batch scalar multiplication (te_msm_mul_base*, csrc/mul_base.hip.hpp), shared by the host test
(tests/test_mul_base_host.py: the lane code compiled for the CPU) and the GPU test (tests/test_gpu_mul_base.py).

The recoding is restated here in Python: K = k + C, C = sum_{i < M} 2^(W-1) 2^(W i), M = ceil(257 / W); digit i is window i of K minus
2^(W-1).  Scalars with a PRESCRIBED digit vector are built from their digits, and the builder checks with that restatement that the
prescription is met, that k < 2^256 and that sum d_i 2^(W i) = k."""
import ctypes
import functools
import os
import random
import subprocess

from oracle import model as m
from oracle import model377 as b
from oracle import oracle377
from test_scalar_mul_host import EDGE_377, EDGE_TE, TOP, te_points, te_torsion_points

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = (4, 5, 8, 11, 12)          # 5 and 11: windows that straddle 32-bit words
DEFAULT_W = 12                       # option "mul_base_window" as a context starts with it
SLOT = 128                           # bytes of a table entry
R256 = 1 << 256


# ---- the recoding, restated --------------------------------------------------------------------------------------------------------
def geometry(W):
    """(M windows, H = 2^(W-1), entries = M (H + 1))"""
    M = -(-257 // W)
    H = 1 << (W - 1)
    return M, H, M * (H + 1)


def offset(W):
    M, H, _ = geometry(W)
    return sum(H << (W * i) for i in range(M))


def recode(k, W):
    """the M signed digits of k, lowest window first"""
    M, H, _ = geometry(W)
    K = k + offset(W)
    assert K < 1 << (W * M)
    return [((K >> (W * i)) & ((1 << W) - 1)) - H for i in range(M)]


def value_of(digits, W):
    return sum(d << (W * i) for i, d in enumerate(digits))


def first_straddling_window(W):
    """the first window whose bits lie in two 32-bit words; where W divides 32 none does: the first window of the second word"""
    M = geometry(W)[0]
    for i in range(M):
        if (W * i) % 32 + W > 32:
            return i
    return 32 // W


def prescribed(W):
    """[(what, k)]: scalars below 2^256 whose digit vector at window bits W is the one named.  The top window takes what k < 2^256 leaves
    it: a small non-negative digit (none at all from a single non-zero digit where W divides 256)."""
    M, H, _ = geometry(W)
    lo, hi = -H, H - 1
    top_shift = W * (M - 1)

    def with_top(lower, want_top):
        """lower digits + the top digit nearest want_top that keeps 0 <= k < 2^256"""
        base = value_of(lower, W)
        t_min = 0 if base >= 0 else -(base >> top_shift)                 # smallest top digit with k >= 0
        t_max = (R256 - 1 - base) >> top_shift                           # largest with k < 2^256
        assert 0 <= t_min <= t_max
        return lower + [min(max(want_top, t_min), t_max, hi)]

    sw = first_straddling_window(W)
    plans = [("every lower window at -2^(W-1)", with_top([lo] * (M - 1), 0)),
             ("every window at 2^(W-1) - 1", with_top([hi] * (M - 1), hi)),
             ("alternating -2^(W-1), 2^(W-1) - 1", with_top([(lo, hi)[i & 1] for i in range(M - 1)], 0)),
             ("alternating 2^(W-1) - 1, -2^(W-1)", with_top([(hi, lo)[i & 1] for i in range(M - 1)], 0)),
             ("all digits 0", [0] * M),
             ("a single digit in window 0", [hi] + [0] * (M - 1)),
             ("a single digit in window %d" % sw, [hi if i == sw else 0 for i in range(M)])]
    if top_shift < 256:
        plans.append(("a single digit in the top window", with_top([0] * (M - 1), hi)))
    else:                                                                # the top window starts at bit 256: it only ever takes a borrow
        plans.append(("top digit 1 over -2^(W-1) below it", [0] * (M - 2) + [lo, 1]))
    out = []
    for what, digits in plans:
        k = value_of(digits, W)
        assert 0 <= k < R256, (W, what)
        assert recode(k, W) == digits and value_of(recode(k, W), W) == k, (W, what)
        out.append(("W = %d: %s" % (W, what), k))
    assert recode(TOP, W)[-1] >= 0 and value_of(recode(TOP, W), W) == TOP
    out.append(("W = %d: 2^256 - 1" % W, TOP))
    # what the plans are for: both extreme digits, a non-zero top digit, a digit across a word boundary
    seen = [recode(k, W) for _, k in out]
    assert any(lo in d for d in seen) and any(hi in d for d in seen) and any(d[-1] > 0 for d in seen)
    return out


@functools.lru_cache(maxsize=None)
def case_scalars(curve):
    """[(what, k)] for a curve (0 / 1): its edge scalars and the prescribed digit vectors of every window in WINDOWS"""
    edge = EDGE_377 if curve else EDGE_TE
    out = [("edge scalar %d" % i, k) for i, k in enumerate(edge)]
    have = {k for _, k in out}
    for W in WINDOWS:
        for what, k in prescribed(W):
            if k not in have:
                have.add(k)
                out.append((what, k))
    return out


def padded_scalars(curve, n, seed):
    """the case scalars followed by random ones, n in all"""
    rnd = random.Random(seed)
    ks = [k for _, k in case_scalars(curve)]
    assert len(ks) <= n
    return ks + [rnd.getrandbits(256) for _ in range(n - len(ks))]


# ---- base points ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def te_base_points():
    """[(name, (x, y))]: four subgroup points, O and the torsion points T2, +-T4, G + T2, G + T4"""
    return [("subgroup point %d" % i, p) for i, p in enumerate(te_points(0xBA5E, 4))] + [("O", (0, 1))] + te_torsion_points()


@functools.lru_cache(maxsize=None)
def bls_base_points():
    """[(name, wire bytes, (x, y))]: two G1 points"""
    raw = oracle377.gen_points(0xBA5E, 2)
    return [("G1 point %d" % i, raw[96 * i:96 * i + 96], b.xy_from_bytes(raw[96 * i:96 * i + 96])) for i in range(2)]


def te_point(name):
    return dict(te_base_points())[name]


# ---- the model's answers (memoised per point: the host and the GPU test ask for the same products) ---------------------------------
@functools.lru_cache(maxsize=None)
def _te_mul(k, p):
    return m.points_to_bytes([m.scalar_mul(k, p)])


@functools.lru_cache(maxsize=None)
def _bls_mul(k, p):
    return b.result_to_bytes(b.scalar_mul(k, p))


def te_expected(p, ks):
    return b"".join(_te_mul(k, p) for k in ks)


def bls_expected(p, ks):
    return b"".join(_bls_mul(k, p) for k in ks)


def scalar_bytes(curve, ks):
    return b"".join(k.to_bytes(48 if curve else 32, "little") for k in ks)


def scalar_modulus(curve):
    return b.R_ORDER if curve else m.L


def montgomery_decode(curve, a):
    """what a record a stands for under option "scalars_montgomery": a 2^-256 mod (L or r)"""
    mod = scalar_modulus(curve)
    return a * pow(R256, -1, mod) % mod


def bls_infinity_plans(n):
    """[(what, scalars)] for n results: 0, r and 2 r at the first, a middle and the last slot, and over a whole affine group of 8"""
    r = b.R_ORDER
    zero = (0, r, 2 * r)
    plans = [("infinity first", [zero[n % 3] if i == 0 else 1000 + i for i in range(n)]),
             ("infinity in the middle", [zero[(n + 1) % 3] if i == n // 2 else 1000 + i for i in range(n)]),
             ("infinity last", [zero[(n + 2) % 3] if i == n - 1 else 1000 + i for i in range(n)]),
             ("a whole group at infinity", [zero[i % 3] if i < 8 else 1000 + i for i in range(n)])]
    return plans


# ---- table entries -------------------------------------------------------------------------------------------------------------------
def _limbs(raw, count):
    return sum(int.from_bytes(raw[4 * j:4 * j + 4], "little") << (29 * j) for j in range(count))


def entry_point(curve, slot):
    """the affine point a 128-byte entry stands for: Twisted-Edwards hm | hp | dt (9 limbs of 29 bits, Montgomery form with R = 2^261;
    dt = -d x y is checked), BLS12-377 x | y (14 limbs, R = 2^406; entry 0 holds x = y = 0 mod q, which is no point of the curve: the
    point at infinity the affine pass wrote as zeros)"""
    assert len(slot) == SLOT
    if curve:
        assert slot[112:] == bytes(16)
        rinv = pow(1 << 406, -1, b.Q)
        xy = (_limbs(slot[:56], 14) * rinv % b.Q, _limbs(slot[56:112], 14) * rinv % b.Q)
        return b.INF if xy == (0, 0) else xy
    assert slot[108:] == bytes(20)
    rinv = pow(1 << 261, -1, m.P)
    hm, hp, dt = (_limbs(slot[36 * k:36 * k + 36], 9) * rinv % m.P for k in range(3))
    x, y = (hp - hm) % m.P, (hp + hm) % m.P
    assert dt == -m.D * x * y % m.P
    return (x, y)


def model_table(curve, W, p):
    """[[j 2^(W i)] p for i < M for j <= H], by repeated addition in the bigint model"""
    M, H, _ = geometry(W)
    add, zero = (b.add, b.INF) if curve else (m.add, m.ZERO)
    out, base = [], p
    for _ in range(M):
        cur = zero
        for _ in range(H + 1):
            out.append(cur)
            cur = add(cur, base)
        for _ in range(W):
            base = add(base, base)
    return out


# ---- the host shim -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shim():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libmulbasecheck.so"), os.path.join(d, "mulbasecheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("mul_base.hip.hpp", "scalar_mul.hip.hpp", "scalar_form.hpp", "from_x.hip.hpp", "check.hip.hpp",
                                                         "fp.hpp", "fq377.hpp", "field.hpp", "curve.hpp", "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    u32p, cp, ci = ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_int
    L.mbc_set_variant.argtypes = [ci]
    L.mbc_out_of_table.restype = ctypes.c_uint64
    L.mbc_geometry.argtypes = [ci, ctypes.POINTER(ci), u32p, u32p, u32p]
    L.mbc_digits.argtypes = [ci, cp, ctypes.POINTER(ctypes.c_int32)]
    L.mbc_table_scalars.argtypes = [ci, ci, cp]
    L.mbc_table_from_scalars.argtypes = [ci, cp, cp, ctypes.c_uint32, cp]
    L.mbc_table_by_addition.argtypes = [ci, ci, cp, cp]
    L.mbc_mul.argtypes = [ci, ci, ci, cp, u32p, cp, ctypes.c_uint64, cp]
    return L


@functools.lru_cache(maxsize=None)
def shim_table(curve, W, point_bytes):
    """the table of window bits W over a point (wire bytes), by the shim's repeated additions"""
    out = ctypes.create_string_buffer(geometry(W)[2] * SLOT)
    shim().mbc_table_by_addition(curve, W, point_bytes, out)
    return out.raw


def shim_mul(curve, W, table, ks, form=0, C=None):
    """the lane code over scalars ks (ints) -> result bytes; the accessor must not have been asked for an entry outside the table"""
    L = shim()
    n = len(ks)
    pb = 96 if curve else 64
    out = ctypes.create_string_buffer(max(1, pb * n))
    before = L.mbc_out_of_table()
    cw = (ctypes.c_uint32 * 9)(*[(C >> (32 * j)) & 0xffffffff for j in range(9)]) if C is not None else None
    L.mbc_mul(curve, form, W, table, cw, scalar_bytes(curve, ks), n, out)
    assert L.mbc_out_of_table() == before, "a lane asked for an entry outside the table"
    return out.raw[:pb * n]
