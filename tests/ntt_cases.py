"""Shared by tests/test_ntt_host.py and tests/test_gpu_ntt.py: the host shim of csrc/ntt.hip.hpp (tests/csrc/nttcheck.cpp), the model
of te_msm_ntt in Python integers, and the case lists."""
import ctypes
import functools
import os
import random
import subprocess

import field_cases as fc
from oracle import model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = m.P
INVERSE, MONTGOMERY = 1, 2                                          # TE_MSM_NTT_*
MAX_LOG_N = 24
TWO_ADICITY = 47
W = pow(22, (P - 1) >> TWO_ADICITY, P)
A = 1 << 256
EINVAL = -1
M_ROOT, M_SCALE, M_BITREV, M_SHIFT_AFTER, M_TWIDDLE, M_SPLIT = range(1, 7)      # the shim's deliberate mistakes
BOUNDS = -100
FLAGS = (0, INVERSE, MONTGOMERY, INVERSE | MONTGOMERY)
pack, unpack = fc.pack, fc.unpack


def shim():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "libnttcheck.so"), os.path.join(d, "nttcheck.cpp")
    hdr_dir = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
    deps = [src] + [os.path.join(hdr_dir, f) for f in ("ntt.hip.hpp", "ntt_plan.hpp", "plan_arith.hpp", "field_ops.hip.hpp", "scalar_mul.hip.hpp", "from_x.hip.hpp",
                                                         "check.hip.hpp", "fp.hpp", "fq377.hpp", "field.hpp", "curve.hpp", "fp_constants.inc", "fq377_constants.inc")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    ci, vp, u64, u32 = ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    L.ntt_ref.argtypes = [vp, u32, u64, ci, vp, vp]
    L.ntt_ref.restype = ci
    L.ntt_emulate.argtypes = [vp, u32, u64, ci, vp, ci, u64, vp, ctypes.POINTER(ci)]
    L.ntt_emulate.restype = ci
    L.ntt_replay.argtypes = [u32, u64, ctypes.POINTER(u64)]
    L.ntt_replay.restype = ci
    L.ntt_plan_info.argtypes = [u32, u64, ctypes.POINTER(u64)]
    L.ntt_root.argtypes = [vp, ctypes.POINTER(u32)]
    L.ntt_tile_record.argtypes = [u32, u32, u64, u32, ctypes.POINTER(u64)]
    L.ntt_tile_record.restype = u64
    return L


def tile_corners(L, log_n):
    """where the first and the last record of the first, second and last tile of every pass are written"""
    out = set()
    for p in range(plan_info(L, log_n)["passes"]):
        tiles = ctypes.c_uint64()
        L.ntt_tile_record(log_n, p, 0, 0, ctypes.byref(tiles))
        for t in {0, min(1, tiles.value - 1), tiles.value - 1}:
            out |= {L.ntt_tile_record(log_n, p, t, x, ctypes.byref(tiles)) for x in (0, 1023)}
    return sorted(v for v in out if v < 1 << log_n)


def _shift_buf(shift):
    return None if shift is None else ctypes.create_string_buffer(int(shift).to_bytes(32, "little"), 32)


def ref(L, a, log_n, count=1, flags=0, shift=None):
    """ntt_ref on bytes -> bytes (shift: a raw integer below 2^256, or None)"""
    size = max(1, len(a))
    src, out, sb = ctypes.create_string_buffer(bytes(a), size), ctypes.create_string_buffer(size), _shift_buf(shift)
    rc = L.ntt_ref(ctypes.addressof(src), log_n, count, flags, ctypes.addressof(sb) if sb else None, ctypes.addressof(out))
    assert rc == 0, rc
    return out.raw[:len(a)]


def emulate(L, a, log_n, count=1, flags=0, shift=None, mistake=0, in_place=False, piece=0, fill=0xA5, null=None):
    """(rc, out bytes, reason): ntt_emulate; the output starts as `fill` bytes, or -- in_place -- as a itself.  null: "a" / "out" passes NULL"""
    size = max(1, len(a))
    src, sb = ctypes.create_string_buffer(bytes(a), size), _shift_buf(shift)
    out = src if in_place else ctypes.create_string_buffer(bytes([fill]) * size, size)
    why = ctypes.c_int()
    rc = L.ntt_emulate(None if null == "a" else ctypes.addressof(src), log_n, count, flags, ctypes.addressof(sb) if sb else None, mistake, piece,
                       None if null == "out" else ctypes.addressof(out), ctypes.byref(why))
    return rc, out.raw[:len(a)], why.value


def plan_info(L, log_n, count=1):
    out = (ctypes.c_uint64 * 9)()
    L.ntt_plan_info(log_n, count, out)
    return dict(passes=out[0], r=[int(x) for x in out[1:4] if x], per_tile=int(out[4]), piece=int(out[5]), tmp_records=int(out[6]), lds_bytes=int(out[7]),
                table_bytes=int(out[8]))


def top_log_n(L):
    """the first size at which the plan uses its largest number of passes"""
    most = max(plan_info(L, k)["passes"] for k in range(MAX_LOG_N + 1))
    return min(k for k in range(MAX_LOG_N + 1) if plan_info(L, k)["passes"] == most)


# ---- the model: Python integers ---------------------------------------------------------------------------------------------------
def omega(log_n):
    return pow(W, 1 << (TWO_ADICITY - log_n), P)


def decode(vals, flags):
    ia = pow(A, -1, P)
    return [v * ia % P for v in vals] if flags & MONTGOMERY else [v % P for v in vals]


def encode(vals, flags):
    return [v * A % P for v in vals] if flags & MONTGOMERY else [v % P for v in vals]


def naive(v, log_n, inverse=False, s=1):
    """the definition, O(n^2)"""
    n, w = 1 << log_n, omega(log_n)
    if not inverse:
        x = [a * pow(s, i, P) % P for i, a in enumerate(v)]
        return [sum(x[i] * pow(w, i * j % n, P) for i in range(n)) % P for j in range(n)]
    wi, ni, si = pow(w, -1, P), pow(n, -1, P), pow(s, -1, P)
    return [pow(si, i, P) * ni * sum(v[j] * pow(wi, i * j % n, P) for j in range(n)) % P for i in range(n)]


def _fft(x, w):
    n = len(x)
    if n == 1:
        return x
    w2 = w * w % P
    ev, od = _fft(x[0::2], w2), _fft(x[1::2], w2)
    out, t = [0] * n, 1
    for k in range(n // 2):
        q = t * od[k] % P
        out[k], out[k + n // 2] = (ev[k] + q) % P, (ev[k] - q) % P
        t = t * w % P
    return out


def fast(v, log_n, inverse=False, s=1):
    """the same by recursion (decimation in time)"""
    n, w = 1 << log_n, omega(log_n)
    if not inverse:
        x, t = [], 1
        for a in v:
            x.append(a * t % P)
            t = t * s % P
        return _fft(x, w)
    y, t, si, out = _fft(list(v), pow(w, -1, P)), pow(n, -1, P), pow(s, -1, P), []
    for a in y:
        out.append(a * t % P)
        t = t * si % P
    return out


def model(a, log_n, count=1, flags=0, shift=None, transform=fast):
    """te_msm_ntt on wire bytes"""
    n = 1 << log_n
    s = 1 if shift is None else decode([shift], flags)[0]
    vals, out = decode(unpack(a, 32), flags), []
    for t in range(count):
        out += transform(vals[t * n:(t + 1) * n], log_n, bool(flags & INVERSE), s)
    return pack(encode(out, flags), 32)


# ---- case lists -------------------------------------------------------------------------------------------------------------------
SHIFTS = (None, 22, (1 << 256) - 5)                                  # none, arkworks' coset generator of this field, a raw value >= p


@functools.lru_cache(maxsize=None)
def values(n, seed=0):
    """n raw 256-bit values: the limb-class extremes of field_cases first (0, 1, p - 1, p, p + 1, 2^256 - 1, limb boundaries, ..), then
    random residues and random full-width integers"""
    rnd = random.Random(0x277 + 1000003 * seed + n)
    ex = list(fc.extremes(fc.FIELD_P))
    rnd.shuffle(ex)
    v = ex[:n]
    while len(v) < n:
        v.append(rnd.randrange(P) if len(v) & 1 else rnd.randrange(1 << 256))
    return pack(v, 32)


# ---- closed forms for the sizes and batches no textbook transform reaches in a test's time (tests/test_gpu_piece_loops.py; each is pinned
# to model() at small sizes by tests/test_piece_cases_host.py).  Inputs and outputs are wire integers: encode()d under MONTGOMERY ------------
def shift_value(flags, shift):
    """the s a call multiplies by: 1 without a shift, else the shift record decoded as the elements are"""
    return 1 if shift is None else decode([shift], flags)[0]


def const_forward(log_n, c):
    """forward of the all-c input, canonical form, no shift: n c delta_0 -- small enough to need no reduction"""
    n = 1 << log_n
    assert 0 < c and n * c < 1 << 40
    return [n * c] + [0] * (n - 1)


def delta0_inverse(log_n, c):
    """inverse of c delta_0, canonical form, no shift: c / n at every place -- this one integer"""
    return c * pow(1 << log_n, -1, P) % P


def delta_place(log_n, t):
    """where transform t of a batch of deltas has its one: odd multiples of a large odd constant, so every digit of the plan moves"""
    return 2654435761 * (t + 1) % (1 << log_n)


def terms_input(log_n, terms, flags=0):
    """the sum of c delta_k over terms = [(k, c), ..] as n wire integers"""
    a = [0] * (1 << log_n)
    for k, c in terms:
        a[k] = encode([c], flags)[0]
    return a


def terms_forward(log_n, terms, j, flags=0, shift=None):
    """output j of the forward transform of terms_input: sum of c s^k w^(j k)"""
    n, w, s = 1 << log_n, omega(log_n), shift_value(flags, shift)
    return encode([sum(c * pow(s, k, P) * pow(w, j * k % n, P) for k, c in terms) % P], flags)[0]


def geometric_input(log_n, g):
    """a_i = g^i, canonical"""
    a, t = [], 1
    for _ in range(1 << log_n):
        a.append(t)
        t = t * g % P
    return a


def geometric_forward(log_n, g, j):
    """output j of the forward transform of geometric_input: (g^n - 1) / (g w^j - 1); g^n != 1 keeps every denominator away from 0"""
    n = 1 << log_n
    top = (pow(g, n, P) - 1) % P
    assert top
    return top * pow(g * pow(omega(log_n), j, P) - 1, -1, P) % P


def plan_digits(r, k):
    """the digits of an input index as the plan cuts it: the first pass's on top (csrc/ntt_plan.hpp)"""
    out, low = [], sum(r)
    for width in r:
        low -= width
        out.append((k >> low) & ((1 << width) - 1))
    return out


def distinct_digit_places(log_n, r):
    """three input indices whose plan digits are all non-zero and pairwise different; the first is odd and near n"""
    n = 1 << log_n

    def ok(k):
        d = plan_digits(r, k)
        return all(d) and len(set(d)) == len(d)
    out = []
    for start, step in ((n - 12345, -2), (n // 3, 1), (0x9E3779B1 % (n // 2), 1)):
        k = start
        while not ok(k) or k in out:
            k += step
        assert 0 < k < n
        out.append(k)
    assert out[0] & 1 and out[0] > n - (n >> 4)
    return out


def sample_places(L, log_n, seed, want=4096):
    """about `want` output indices: the tile corners of every pass, 0, 1, n / 2, n - 1 and random ones (all of a small transform)"""
    n = 1 << log_n
    if n <= want:
        return list(range(n))
    rnd = random.Random(seed)
    js = set(tile_corners(L, log_n)) | {0, 1 % n, n // 2, n - 1} | {rnd.randrange(n) for _ in range(want)}
    return sorted(js)


def batch_counts(per_tile):
    """transforms of a one-pass launch that leave the last block partly filled, fill it, and pass it"""
    return sorted({1, 2, 3, max(1, per_tile - 1), per_tile, per_tile + 1, 1000})
