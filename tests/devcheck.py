"""Helper module of the device-arithmetic tests (tests/test_device_arith_host.py, tests/test_gpu_device_arith.py): builds and loads
the two compilations of the operation table (tests/csrc/devcheck_ops.hpp: g++ -> libdevcheck_host.so, hipcc gfx950 -> libdevcheck.so,
which also holds the direct launches of the device-only code), the limb codecs, the operand generators the host tests share with the
device tests, and the comparators.  Not a conftest: test modules import what they need, fixtures included."""
import ctypes
import functools
import importlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

from oracle import model as te_model
from oracle import model377 as m377

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tests", "csrc")
PRODUCT_CSRC = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
HOST_SO, DEV_SO = os.path.join(CSRC, "libdevcheck_host.so"), os.path.join(CSRC, "libdevcheck.so")
HOST2_SO, DEV2_SO = os.path.join(CSRC, "libdevcheck2_host.so"), os.path.join(CSRC, "libdevcheck2.so")     # the second table (devcheck_ops2.hpp)
LB = 29
LM = (1 << LB) - 1
RA = 1 << 256                                     # radix of the callers' Montgomery form of a scalar (scalar_form.hpp)
SCALAR_MODULI = {"scalar_te": te_model.L, "scalar_377": m377.R_ORDER}

# name -> (words in, words out): the Python side's copy of DC_OPS, checked against dc_table() of both libraries
OPS = {
    "mul_9": (18, 9), "mul_14": (28, 14), "mul_x2_9": (36, 18), "mul_x2_14": (56, 28), "mul_x3_9": (54, 27), "mul_x3_14": (84, 42),
    "mul_x4_9": (72, 36), "mul_x4_14": (112, 56), "mul_k2d_9": (9, 9), "mul_d_9": (9, 9), "mul3_14": (14, 14), "norm_9": (9, 9),
    "norm_14": (14, 14), "sub2_9": (18, 9), "sub2_14": (28, 14), "sub4_9": (18, 9), "sub4_14": (28, 14), "sub16_9": (18, 9),
    "sub16_14": (28, 14), "neg2_9": (9, 9), "neg2_14": (14, 14), "neg4_9": (9, 9), "neg4_14": (14, 14), "from_words_9": (8, 9),
    "from_words_14": (12, 14), "select": (3, 1), "rec_te": (18, 27), "rec_te_mont": (18, 27), "rec_sw": (28, 56), "rec_sw_mont": (28, 56),
    "cneg_9": (28, 27), "cneg_14": (57, 56), "cneg_aff": (43, 42), "from_pnt_9": (27, 36), "from_pnt_14": (56, 56),
    "from_pnt_aff": (42, 56), "from_pair_9": (54, 36), "from_pair_14": (112, 56), "from_pair_aff": (84, 56), "madd_9": (63, 36),
    "madd_14": (112, 56), "madd_aff": (98, 56), "add_9": (72, 36), "add_14": (112, 56), "scalar_te": (8, 8), "scalar_377": (8, 8),
}
# the operations of each limb count (the operations without one -- select, the scalar decoders -- ride with N = 9)
OPS_OF = {9: [k for k in OPS if k.endswith("_9") or k in ("rec_te", "rec_te_mont", "select", "scalar_te", "scalar_377")],
          14: [k for k in OPS if k.endswith("_14") or k.endswith("_aff") or k in ("rec_sw", "rec_sw_mont")]}
# the second table (DC_OPS2 of devcheck_ops2.hpp): check.hip.hpp, from_x.hip.hpp, scalar_mul.hip.hpp
OPS2 = {
    "is_zero_9": (9, 1), "is_zero_14": (14, 1), "to_canon_9": (9, 8), "to_canon_14": (14, 12), "from_canon_9": (8, 9), "from_canon_14": (12, 14),
    "inv_9": (9, 9), "inv_14": (14, 14), "sqrt_ratio_9": (18, 10), "sqrt_14": (14, 15), "words_lt_8": (8, 1), "words_lt_12": (12, 1),
    "words_neg_8": (8, 8), "words_neg_12": (12, 12), "sw_add": (84, 42), "sw_dbl": (42, 42), "sw_cneg": (43, 42), "add_cneg": (73, 36),
    "mul_order_te": (35, 36), "sm_digits": (8, 138), "naf_digit": (18, 1), "exp_bit": (14, 1), "aff_group_te": (225, 128),
    "aff_group_377": (353, 192), "check_form_te": (16, 1), "check_form_te_mont": (16, 1), "check_form_377": (24, 1),
    "check_form_377_mont": (24, 1), "in_subgroup_te": (16, 1), "in_subgroup_377": (24, 1),
}
DEVICE_ONLY = ["add_team", "block_sum", "sum_groups", "reduce_tail"]


class Field:
    """one base field of the engine: N limbs of 29 bits, Montgomery radix 2^(29 N)"""

    def __init__(self, N, P):
        self.N, self.P, self.R = N, P, 1 << (LB * N)
        self.rinv = pow(self.R, -1, P)
        self.acc_words = 4 * N

    def limbs(self, v):
        """integer -> N limbs, class N (the top limb takes what is left)"""
        return [(v >> (LB * i)) & LM for i in range(self.N - 1)] + [v >> (LB * (self.N - 1))]

    @staticmethod
    def val(ls):
        return sum(int(l) << (LB * i) for i, l in enumerate(ls))

    def offset(self, K):
        """K p in offset form (fp_kp_offset / fq_kq_offset): limbs 0..N-2 raised by 2^29, the next limb lowered by 1"""
        ls = self.limbs(K * self.P)
        out = [ls[0] + (1 << LB)] + [l + (1 << LB) - 1 for l in ls[1:-1]] + [ls[-1] - 1]
        assert self.val(out) == K * self.P
        return out


FIELDS = {9: Field(9, te_model.P), 14: Field(14, m377.Q)}


# ---------------------------------------------------------------------------------------------- building and loading
def _stale(so, srcs):
    return not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs)


def _sources(second=False):
    hdrs = [os.path.join(PRODUCT_CSRC, f) for f in sorted(os.listdir(PRODUCT_CSRC)) if f.endswith((".hpp", ".inc"))]
    return hdrs + [os.path.join(CSRC, "devcheck_ops.hpp")] + ([os.path.join(CSRC, "devcheck_ops2.hpp")] if second else [])


def makefile_flags():
    """HIPCC, ARCH and CXXFLAGS as csrc/Makefile sets them (`?=`: the environment wins, as it does for make)"""
    text = open(os.path.join(PRODUCT_CSRC, "Makefile")).read()
    out = {}
    for name in ("HIPCC", "ARCH", "CXXFLAGS"):
        mt = re.search(r"^%s \?= (.*)$" % name, text, re.M)
        assert mt, "csrc/Makefile no longer sets " + name
        out[name] = os.environ.get(name, mt.group(1).strip())
    return out


def device_build_command(second=False):
    f = makefile_flags()
    so, src = (DEV2_SO, "devcheck2.hip") if second else (DEV_SO, "devcheck.hip")
    return [f["HIPCC"], "--offload-arch=" + f["ARCH"]] + f["CXXFLAGS"].split() + ["-shared", "-o", so, os.path.join(CSRC, src)]


def build(force=False):
    """compiles whichever of the four libraries is older than its sources (the device ones cross-compile without a GPU)"""
    for second, host_so, dev_so, host_src, dev_src in ((False, HOST_SO, DEV_SO, "devcheck_host.cpp", "devcheck.hip"),
                                                       (True, HOST2_SO, DEV2_SO, "devcheck2_host.cpp", "devcheck2.hip")):
        src = os.path.join(CSRC, host_src)
        if force or _stale(host_so, _sources(second) + [src]):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", host_so, src])
        if force or _stale(dev_so, _sources(second) + [os.path.join(CSRC, dev_src)]):
            subprocess.check_call(device_build_command(second))


def _declare(L, device, ops=None):
    u32p, vp, u32, u64, ci = ctypes.POINTER(ctypes.c_uint32), ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int
    for name in (OPS if ops is None else ops):
        fn = getattr(L, "dc_" + name)
        fn.argtypes, fn.restype = [vp, vp, u32], ci
    L.dc_table.restype = ctypes.c_char_p
    if device and ops is None:
        for n in (9, 14):
            getattr(L, "dc_add_team_%d" % n).argtypes = [vp, vp, vp, u32]
            getattr(L, "dc_block_sum_%d" % n).argtypes = [ci, vp, u64, u32p, u32p, u32p, u32, vp]
            getattr(L, "dc_sum_groups_%d" % n).argtypes = [ci, vp, u64, vp, u64, u32, u32, u32, u32, u32, u32]
            getattr(L, "dc_reduce_tail_%d" % n).argtypes = [vp, u64, vp, u64, u32, u32, u32, u32, u32p, vp, u64, u32]
            for k in DEVICE_ONLY:
                getattr(L, "dc_%s_%d" % (k, n)).restype = ci
    return L


@functools.lru_cache(maxsize=None)
def host_lib():
    build()
    return _declare(ctypes.CDLL(HOST_SO), False)


@functools.lru_cache(maxsize=None)
def device_lib():
    """libdevcheck.so -- or the file TE_DEVCHECK_LIB names, used as it is (a build of devcheck.hip against other headers)"""
    other = os.environ.get("TE_DEVCHECK_LIB")
    if other:
        importlib.import_module("webgpu-msm-twisted-edwards_amd.binding")._share_hip_runtime_with_torch()
        return _declare(ctypes.CDLL(other), True)
    build()
    importlib.import_module("webgpu-msm-twisted-edwards_amd.binding")._share_hip_runtime_with_torch()   # one HIP runtime per process
    return _declare(ctypes.CDLL(DEV_SO), True)


@functools.lru_cache(maxsize=None)
def host_lib2():
    build()
    return _declare(ctypes.CDLL(HOST2_SO), False, OPS2)


@functools.lru_cache(maxsize=None)
def device_lib2():
    """libdevcheck2.so -- or the file TE_DEVCHECK2_LIB names, used as it is"""
    other = os.environ.get("TE_DEVCHECK2_LIB")
    if not other:
        build()
    importlib.import_module("webgpu-msm-twisted-edwards_amd.binding")._share_hip_runtime_with_torch()   # one HIP runtime per process
    return _declare(ctypes.CDLL(other or DEV2_SO), True, OPS2)


def _op(name):
    return OPS[name] if name in OPS else OPS2[name]


@pytest.fixture(scope="session")
def dc_host():
    """host build of the operation table"""
    return host_lib()


@pytest.fixture(scope="session")
def dc_dev():
    """gfx950 build of the operation table and the device-only launches"""
    return device_lib()


class HipError(RuntimeError):
    pass


_FAULT = []


def launch(what, fn, *args):
    """one call of a device entry point; after a HIP error nothing more is launched in this process"""
    if _FAULT:
        raise HipError("not launched: %s failed earlier in this process" % _FAULT[0])
    rc = fn(*args)
    if rc == -1:
        raise ValueError("%s: the harness refused the arguments (they reach outside the buffers)" % what)
    if rc != 0:
        _FAULT.append(what)
        raise HipError("%s: HIP error %d" % (what, rc))


def run_host(name, inp):
    """inp: uint32 array [n, words in] -> uint32 array [n, words out], through the host build"""
    iw, ow = _op(name)
    inp = np.ascontiguousarray(inp, dtype=np.uint32).reshape(-1, iw)
    out = np.zeros((inp.shape[0], ow), dtype=np.uint32)
    rc = getattr(host_lib() if name in OPS else host_lib2(), "dc_" + name)(inp.ctypes.data, out.ctypes.data, inp.shape[0])
    assert rc == 0, name
    return out


def to_device(arr):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.uint32).view(np.int32)).cuda()


def from_device(t):
    return t.cpu().numpy().view(np.uint32)


def device_zeros(*shape):
    import torch
    return torch.zeros(shape, dtype=torch.int32, device="cuda")


def run_device(name, inp):
    iw, ow = _op(name)
    inp = np.ascontiguousarray(inp, dtype=np.uint32).reshape(-1, iw)
    d_in, d_out = to_device(inp), device_zeros(inp.shape[0], ow)
    launch(name, getattr(device_lib() if name in OPS else device_lib2(), "dc_" + name), d_in.data_ptr(), d_out.data_ptr(), inp.shape[0])
    return from_device(d_out)


# ---------------------------------------------------------------------------------------------- comparators
def compare_bits(op, got, want, inputs=None):
    """bit-for-bit, limb by limb; names the operation, the element and the limb"""
    got, want = np.asarray(got, dtype=np.uint32), np.asarray(want, dtype=np.uint32)
    assert got.shape == want.shape, "%s: shape %s against %s" % (op, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        e, l = (int(v) for v in bad[0])
        ins = "" if inputs is None else " operand words " + " ".join("%08x" % int(v) for v in np.asarray(inputs).reshape(got.shape[0], -1)[e])
        raise AssertionError("%s: element %d word %d: %08x, the host build gives %08x (%d words differ in %d elements).%s"
                             % (op, e, l, int(got[e, l]), int(want[e, l]), len(bad), len(set(int(b[0]) for b in bad)), ins))


def check_contract(op, N, acc):
    """an accumulator is four product outputs: limbs 0..N-2 below 2^29, value below 1.1 p"""
    F = FIELDS[N]
    w = np.asarray(acc, dtype=np.uint32).reshape(4, N)
    for c, name in enumerate("xyzt"):
        if not all(int(v) <= LM for v in w[c, :N - 1]):
            raise AssertionError("%s: coordinate %s is not of limb class N: %s" % (op, name, [hex(int(v)) for v in w[c]]))
        if not F.val(w[c]) < 1.1 * F.P:
            raise AssertionError("%s: coordinate %s is not below 1.1 p: %x" % (op, name, F.val(w[c])))


class Decoders:
    """accumulator words -> the model's affine point, through the decoders the suite already has (their T Z = X Y and on-curve
    assertions included): _ete_affine of test_host_logic (N = 9), _Decoder of test_gpu_bls377_stages (N = 14)"""

    def __init__(self, fq377check):
        from test_gpu_bls377_stages import _Decoder
        self.d377 = _Decoder(fq377check)

    def point(self, op, N, acc, what=""):
        from test_host_logic import _ete_affine
        raw = np.ascontiguousarray(acc, dtype=np.uint32).tobytes()
        check_contract(op, N, acc)
        try:
            if N == 9:
                pt = _ete_affine(te_model, raw)
                assert te_model.on_curve(pt), "not on the curve"
                return pt
            return self.d377.point(raw)
        except (AssertionError, ValueError, ZeroDivisionError) as e:
            raise AssertionError("%s: %s: %s" % (op, what, str(e) or "T Z != X Y")) from e

    def check(self, op, N, acc, want, what=""):
        got = self.point(op, N, acc, what)
        if got != want:
            raise AssertionError("%s: %s decodes to %s, the model gives %s" % (op, what, got, want))


@pytest.fixture(scope="session")
def dc_dec(fq377check):
    return Decoders(fq377check)


# ---------------------------------------------------------------------------------------------- model sums
def msum(N, pts):
    """sum of model points (N = 9: twisted Edwards affine, ZERO = (0, 1); N = 14: short Weierstrass affine, INF = None)"""
    if N == 9:
        P, acc = te_model.P, (0, 1, 0, 1)
        for x, y in pts:
            acc = te_model._ext_add(acc, (x, y, x * y % P, 1))
        zi = te_model.inv(acc[3])
        return (acc[0] * zi % P, acc[1] * zi % P)
    acc = (0, 1, 0)
    for p in pts:
        acc = m377._padd(acc, (0, 1, 0) if p is None else (p[0], p[1], 1))
    return m377._to_affine(acc)


def mmul(N, k, pt):
    return te_model.scalar_mul(k, pt) if N == 9 else m377.scalar_mul(k, pt)


def mneg(N, pt):
    return te_model.neg(pt) if N == 9 else m377.neg(pt)


def mzero(N):
    return te_model.ZERO if N == 9 else m377.INF


# ---------------------------------------------------------------------------------------------- field operands
def mont_mul_pairs(N, n_random=200, n_wide=100, n_col0=100):
    """(a limbs, b limbs) for one Montgomery product: the sets of test_mont_mul_values_and_limb_classes (N = 9) and of
    test_device_field_377_on_the_host (N = 14), which draw them from here.
      random values below 8p / 16p; the widest limb classes the formulas use at their maximum (N = 9: D x S, S x S; N = 14: one
      operand normalised, the other with limbs up to 2^30.8); zero, one, p, p +- 1, R mod p, R^2 mod p, [LM] * (N-1) and sparse
      operands (the carry-folded quotient's special columns, 0 * b = p); column 0 = 0 (mod 2^29), where q_0 = 2^29."""
    F, rnd = FIELDS[N], random.Random(11 + N)
    P, R, lim = F.P, F.R, F.limbs
    top = 1 << 22 if N == 9 else 7
    out = [(lim(rnd.randrange(8 * P)), lim(rnd.randrange((16 if N == 9 else 8) * P))) for _ in range(n_random)]
    if N == 9:
        d_max, s_max = LM + max(F.offset(2)[:8]), 2 * LM
        out += [([d_max] * 8 + [top], [s_max] * 8 + [top]), ([s_max] * 8 + [top], [s_max] * 8 + [top]), ([LM] * 8 + [top], [(1 << 31) - 1] * 8 + [top])]
        out += [([rnd.randrange(d_max + 1) for _ in range(8)] + [rnd.randrange(top)], [rnd.randrange(s_max + 1) for _ in range(8)] + [rnd.randrange(top)])
                for _ in range(n_wide)]
    else:
        wide = int(2 ** 30.8)
        out += [([LM] * 13 + [top], [wide] * 13 + [top]), ([wide] * 13 + [top], [LM] * 13 + [top])]
        out += [([rnd.randrange(LM + 1) for _ in range(13)] + [rnd.randrange(top)], [rnd.randrange(wide + 1) for _ in range(13)] + [rnd.randrange(top)])
                for _ in range(n_wide)]
    zero, one = [0] * N, [1] + [0] * (N - 1)
    las = [zero, one, [0, 1] + [0] * (N - 2), [1 << 28] + [0] * (N - 1), [LM] * (N - 1) + [top if N == 14 else LM], [0] * (N - 1) + [top],
           lim(P), lim(P - 1), lim(R % P), lim(R * R % P)]
    if N == 14:
        las += [lim(LM), lim(1 << 377)]
    lbs = [zero, one, [2] + [0] * (N - 1), [LM] * (N - 1) + [top], lim(P), lim(P + 1), lim(R % P), lim(R * R % P),
           ([1 << 30] * (N - 1) + [0]) if N == 9 else lim((1 << 58) - (1 << 29))]
    out += [(la, lb) for la in las for lb in lbs]
    for _ in range(n_col0):                               # a_0 * b_0 = 0 (mod 2^29): column 0 takes q_0 = 2^29
        la, lb = lim(rnd.randrange(4 * P)), lim(rnd.randrange(4 * P))
        la[0] &= ~((1 << rnd.randrange(1, 29)) - 1)
        lb[0] = (lb[0] << 20) & LM
        out.append((la, lb))
    return out


def small_product_values(K, n_random=100, n_product=100):
    """class-N operands below 2^254 for fp_mul_k2d (K = 6042) / fp_mul_d (K = 3021): the edges of test_small_constant_product, the
    values where K a crosses a multiple of p (where the quotient estimate is tightest), random values, random product outputs"""
    P, rnd = te_model.P, random.Random(21)
    edge = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, (1 << 254) - 1, 1 << 253, (1 << 232) - 1, 1 << 232, (1 << 222) - 1, 1 << 222]
    for q in range(1, K + 58, 97):
        for d in (-1, 0, 1):
            edge.append(max(0, (q * P + K - 1) // K + d))
    vals = [v for v in edge if v < 1 << 254]
    vals += [rnd.randrange(1 << 254) for _ in range(n_random)]
    vals += [rnd.randrange(P + P // 8) for _ in range(n_product)]          # the range product outputs live in
    return vals


def helper_operands(N, n=200):
    """per draw: (limbs below 2^32 under a small top limb, x < 2p, y < 2p, a 256- / 384-bit value) -- the operands of test_field_helpers
    for fe_norm, fe_sub<2> and the word loads"""
    F, rnd = FIELDS[N], random.Random(12)
    bits = 256 if N == 9 else 384
    return [([rnd.randrange(1 << 32) for _ in range(N - 1)] + [rnd.randrange(1 << 20)], rnd.randrange(2 * F.P), rnd.randrange(2 * F.P),
             rnd.randrange(1 << bits)) for _ in range(n)]


def words32(v, n):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(n)]


def sub_operands(N, K, n=150):
    """(a, b) for fe_sub<K> / fe_neg<K>: a with limbs below 2^30 (a sum of two class-N values), b of class N as the callers pass it -- a
    product output, below 1.1 p -- and at the edges of what the offset form of K p admits: 0, p, p +- 1 and every lower limb at its
    maximum under a top limb one below K p's"""
    F, rnd = FIELDS[N], random.Random(13 * N + K)
    edge_b = [F.limbs(b) for b in (0, 1, F.P - 1, F.P, F.P + 1)] + [[LM] * (N - 1) + [0], [LM] * (N - 1) + [F.limbs(K * F.P)[-1] - 1]]
    out = [(F.limbs(rnd.randrange(2 * F.P)), b) for b in edge_b]
    out += [([2 * LM] * (N - 1) + [3], [LM] * (N - 1) + [0]), ([0] * N, [LM] * (N - 1) + [0])]
    for _ in range(n):
        a = [x + y for x, y in zip(F.limbs(rnd.randrange(2 * F.P)), F.limbs(rnd.randrange(2 * F.P)))]
        out.append((a, F.limbs(rnd.randrange(F.P + F.P // 10))))
    return out


def scalar_edge_values(mod):
    """edge_values(mod) of tests/test_gpu_montgomery_inputs.py"""
    single = [0xffffffff << (32 * j) for j in range(8)]
    all_but_one = [(RA - 1) ^ (0xffffffff << (32 * j)) for j in range(8)]
    return [RA - 1, mod, RA % mod, mod + 1, mod - 1, 1, 0] + single + all_but_one


# ---------------------------------------------------------------------------------------------- points, records, accumulators
class Pool:
    """Operands of one curve as the HOST build produces them (the host twins of fpc_prep_point / f377_prep_point and chains of fpc_madd /
    f377_madd in the table): records and accumulators whose coordinates are real product outputs, each with the model's point.
      acc   uint32 [n, 4 N]   accumulators          pts   the model's point of each
      named indices: ident (ete_identity), zero_p (an O that came out of P + (-P): its zero coordinates are the representative p),
      gen (generic points: conversions and partial sums), TE only: t2, t4, t4n (order 2 and 4), p_t2 (P + T2)
      rec   uint32 [m, record words] records (projective for N = 14), rec_pts their points; rec_aff (N = 14): affine records"""

    def __init__(self, N, consts377=None):
        self.N, self.F = N, FIELDS[N]
        self.d = te_model.D if N == 9 else consts377[2]                           # the curve constant of the twisted-Edwards form
        F = self.F
        if N == 9:
            base = te_model.gen_points(21, 20)
            base += [te_model.neg(base[0]), te_model.neg(base[1])]
            i4 = te_model.sqrt_mod_p(F.P - 1)
            t2, t4 = (0, F.P - 1), (i4, 0)
            assert te_model.add(t4, t4) == t2 and te_model.on_curve(t4)
            special = [t2, t4, te_model.neg(t4), te_model.add(base[0], t2)]
            base = base + special
            xy = np.array([F.limbs(x) + F.limbs(y) for x, y in base], dtype=np.uint32)
            self.rec = run_host("rec_te", xy)
            conv, mad = "from_pnt_9", "madd_9"
        else:
            from test_gpu_bls377_stages import _g1_multiset
            base = m377.gen_points(21, 12)
            base += [m377.neg(base[0]), m377.neg(base[1])] + _g1_multiset(5, 700)[0][::29]       # then repeats, inverses, small multiples of G
            special = []
            xy = np.array([F.limbs(x) + F.limbs(y) for x, y in base], dtype=np.uint32)
            self.rec = run_host("rec_sw", xy)
            conv, mad = "from_pnt_14", "madd_14"
            s_, f_, d_ = consts377
            self.rec_aff = np.array([self._aff377(pt, s_, f_, d_) for pt in base], dtype=np.uint32)
        self.rec_pts = base
        nb = len(base)
        one = F.limbs(F.R % F.P)
        ident = np.array([[0] * N + one + one + [0] * N], dtype=np.uint32)
        conv_acc = run_host(conv, self.rec)                                       # P_i
        neg0 = run_host("cneg_%d" % N, np.hstack([self.rec[:1], np.ones((1, 1), dtype=np.uint32)]))
        zero_p = run_host(mad, np.hstack([conv_acc[:1], neg0]))                   # P_0 + (-P_0)
        chain, chain_pts, cur, cur_pt = [], [], conv_acc[0:1], base[0]
        for j in range(1, nb - len(special)):                                      # partial sums P_0 + ... + P_j
            cur = run_host(mad, np.hstack([cur, self.rec[j:j + 1]]))
            cur_pt = msum(N, [cur_pt, base[j]])
            chain.append(cur[0])
            chain_pts.append(cur_pt)
        self.acc = np.vstack([ident, zero_p, conv_acc, np.array(chain, dtype=np.uint32)])
        self.pts = [mzero(N), mzero(N)] + list(base) + chain_pts
        self.ident, self.zero_p = 0, 1
        ns = len(special)
        self.gen = [i for i in range(2, len(self.pts)) if not (2 + nb - ns <= i < 2 + nb)]
        if N == 9:
            self.t2, self.t4, self.t4n, self.p_t2 = (2 + nb - ns + k for k in range(4))
        assert len(self.pts) == len(self.acc)

    def _aff377(self, pt, s_, f_, d_):
        """the affine record of a bound BLS12-377 point: ((Y - X)/2, (Y + X)/2, -d X Y) of its Edwards form, times R, canonical"""
        Q, F = m377.Q, self.F
        u, v = s_ * (pt[0] + 1) % Q, s_ * pt[1] % Q
        X, Y = f_ * u * pow(v, -1, Q) % Q, (u - 1) * pow(u + 1, -1, Q) % Q
        h = pow(2, -1, Q)
        return sum((F.limbs(c * F.R % Q) for c in ((Y - X) * h, (Y + X) * h, -d_ * X * Y)), [])

    def pair_cases(self, n_random=120):
        """(name, index a, index b) for a full addition: O + O, O + P, P + O, P + P, P + (-P), P + Q, each O in both representations;
        the Twisted-Edwards curve also with the points of order 2 and 4"""
        g, N = self.gen, self.N
        neg = {i: j for i in g for j in g if self.pts[j] == mneg(N, self.pts[i])}
        cases = [("O+O", 0, 0), ("O+P", 0, g[0]), ("P+O", g[1], 0), ("O'+O'", 1, 1), ("O'+P", 1, g[2]), ("P+O'", g[3], 1), ("O+O'", 0, 1), ("O'+O", 1, 0),
                 ("P+P", g[0], g[0]), ("P+P of a sum", g[-1], g[-1]), ("P+Q", g[0], g[1]), ("P+Q of sums", g[-1], g[-2])]
        if N == 9:
            cases += [("P+T2", g[0], self.t2), ("T2+P", self.t2, g[4]), ("T4+T4", self.t4, self.t4), ("T4+(-T4)", self.t4, self.t4n), ("T2+T2", self.t2, self.t2),
                      ("T4+T2", self.t4, self.t2), ("P+T4", g[5], self.t4), ("(P+T2)+T2", self.p_t2, self.t2), ("O+T2", 0, self.t2), ("O'+T4", 1, self.t4)]
        assert neg, "the pool holds a point and its inverse"
        cases += [("P+(-P)", i, j) for i, j in list(neg.items())[:6]]
        rnd = random.Random(31 + N)
        every = list(range(len(self.pts)))
        cases += [("pool %d + pool %d" % (a, b), a, b) for a, b in ((rnd.choice(every), rnd.choice(every)) for _ in range(n_random))]
        return cases


@functools.lru_cache(maxsize=None)
def _pool(N, consts377):
    return Pool(N, consts377)


@pytest.fixture(scope="session")
def dc_pools(fq377check):
    from test_oracle_bls377 import _edwards_consts
    return {9: _pool(9, None), 14: _pool(14, tuple(_edwards_consts(fq377check)))}


def extreme_pairs(N, n_random=40):
    """uint32 [n, 8 N]: pairs of SYNTHETIC accumulators at the edges of an accumulator's contract (class N, below 1.1 p) -- every limb
    below p's leading one at 2^29 - 1, or at 0, or alternating, or random, so that Y - X + 2p and Y + X reach the largest limbs the D
    and S classes allow.  Points of the curve reach such limbs with probability 2^-29 per limb; these are not points of the curve: a
    full addition is nine products of sums and differences of its operands whatever they are, and is compared as such."""
    F, rnd = FIELDS[N], random.Random(71 + N)
    pl = F.limbs(F.P)
    h = max(i for i in range(N) if pl[i])                # p's leading limb: one below it keeps the value below p

    def coord(kind):
        low = {"max": [LM] * h, "zero": [0] * h, "alt": [LM * (i & 1) for i in range(h)], "alt2": [LM * (~i & 1) for i in range(h)],
               "rnd": [rnd.randrange(LM + 1) for _ in range(h)]}[kind]
        lead = pl[h] - 1 if kind in ("max", "alt") else 0 if kind == "zero" else rnd.randrange(pl[h])
        c = low + [lead] + [0] * (N - 1 - h)
        assert F.val(c) < F.P and all(x <= LM for x in c)
        return c
    shapes = [("zero", "max", "max", "max"), ("max", "zero", "zero", "max"), ("max", "max", "max", "max"), ("zero", "zero", "zero", "zero"),
              ("alt", "alt2", "rnd", "max"), ("alt2", "alt", "max", "rnd")]
    accs = [sum((coord(k) for k in sh), []) for sh in shapes]
    pairs = [a + b for a in accs for b in accs]
    kinds = ("max", "zero", "alt", "alt2", "rnd")
    pairs += [sum((coord(rnd.choice(kinds)) for _ in range(8)), []) for _ in range(n_random)]
    return np.array(pairs, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------- inputs of the table operations
def table_inputs(name, pools):
    """uint32 [n, words in] for one operation of the table: seeded, a few hundred elements, the edges of its operand classes"""
    iw, _ = OPS[name]
    N = 14 if (name.endswith("_14") or name.endswith("_aff") or name.startswith("rec_sw")) else 9
    F, pool = FIELDS[N], pools[N]
    rnd = random.Random(name)
    kind = name.rsplit("_", 1)[0] if name.endswith(("_9", "_14")) else name
    pairs = mont_mul_pairs(N)
    if kind == "mul":
        rows = [a + b for a, b in pairs]
    elif kind.startswith("mul_x"):
        M = int(kind[-1])                                  # chain m of element e takes pair e M + m: different operands in every chain
        rows = [sum((pairs[(e * M + m) % len(pairs)][0] + pairs[(e * M + m) % len(pairs)][1] for m in range(M)), []) for e in range(len(pairs))]
    elif kind in ("mul_k2d", "mul_d"):
        rows = [[(v >> (LB * i)) & LM for i in range(8)] + [v >> 232] for v in small_product_values(6042 if kind == "mul_k2d" else 3021)]
    elif kind == "mul3":
        rows = [[LM] * 13 + [LM], [0] * 14] + [F.limbs(rnd.randrange(2 * F.P)) for _ in range(200)]
    elif kind == "norm":
        rows = [ls for ls, _, _, _ in helper_operands(N)] + [[0xFFFFFFF8] * (N - 1) + [5], [LM] * N, [0] * N, [LM + 1] + [LM] * (N - 2) + [0]]
    elif kind.startswith("sub"):
        rows = [a + b for a, b in sub_operands(N, int(kind[3:]))]
    elif kind.startswith("neg"):
        rows = [b for _, b in sub_operands(N, int(kind[3:]))]
    elif kind == "from_words":
        nw = iw
        vals = [w for _, _, _, w in helper_operands(N)] + [0, 1, (1 << (32 * nw)) - 1, F.P, F.P - 1] + [0xFFFFFFFF << (32 * j) for j in range(nw)]
        rows = [words32(v, nw) for v in vals]
    elif kind == "select":
        rows = [[mk, rnd.getrandbits(32), rnd.getrandbits(32)] for mk in [0, 0xFFFFFFFF, 1, 0x80000000, 0xAAAAAAAA] + [rnd.getrandbits(32) for _ in range(200)]]
    elif kind in ("rec_te", "rec_te_mont", "rec_sw", "rec_sw_mont"):
        bits = 256 if N == 9 else 384
        top = (1 << bits) - 1
        mont = kind.endswith("mont")
        vals = [((x << bits) % F.P, (y << bits) % F.P) if mont else (x, y) for x, y in pool.rec_pts]
        vals += [(x + F.P, y) for x, y in vals[:3] if x + F.P <= top] + [(x, y + F.P) for x, y in vals[:3] if y + F.P <= top]     # non-canonical
        vals += [(0, 1), (1, 0), (0, 0), (top, top), (top, 0), (F.P, F.P), (F.P - 1, 1)]
        vals += [(rnd.getrandbits(bits), rnd.getrandbits(bits)) for _ in range(150)]                # any value is accepted
        lim = lambda v: [(v >> (LB * i)) & LM for i in range(N)]                                     # what fp_ / fq_from_words32 make of it
        rows = [lim(x) + lim(y) for x, y in vals]
    elif kind in ("cneg", "cneg_aff"):
        recs = pool.rec_aff if name == "cneg_aff" else pool.rec
        rows = [list(r) + [s] for r in recs for s in (0, 1, 0xFFFFFFFF, 2)]
    elif kind in ("from_pnt", "from_pnt_aff", "from_pair", "from_pair_aff", "madd", "madd_aff"):
        aff = kind.endswith("_aff")
        recs = pool.rec_aff if aff else pool.rec
        cn = "cneg_aff" if aff else "cneg_%d" % N
        both = np.vstack([recs, run_host(cn, np.hstack([recs, np.ones((len(recs), 1), dtype=np.uint32)]))])        # P_i, then -P_i as k_accumulate forms it
        nr = len(recs)
        if kind.startswith("from_pnt"):
            rows = both
        elif kind.startswith("from_pair"):                 # P + P, P + (-P), (-P) + P, (-P) + (-P), P + Q with every sign
            idx = [(i, i) for i in range(nr)] + [(i, i + nr) for i in range(nr)] + [(i + nr, i) for i in range(nr)] + [(i + nr, i + nr) for i in range(nr)]
            idx += [(rnd.randrange(2 * nr), rnd.randrange(2 * nr)) for _ in range(150)]
            rows = np.array([np.concatenate([both[a], both[b]]) for a, b in idx], dtype=np.uint32)
        else:                                              # O + P, O' + P, P + P, P + (-P), sums + every record
            idx = [(0, r) for r in range(2 * nr)] + [(1, r) for r in range(2 * nr)] + [(2 + r, r) for r in range(nr)] + [(2 + r, r + nr) for r in range(nr)]
            idx += [(rnd.randrange(len(pool.acc)), rnd.randrange(2 * nr)) for _ in range(150)]
            rows = np.array([np.concatenate([pool.acc[a], both[b]]) for a, b in idx], dtype=np.uint32)
    elif kind == "add":
        rows = np.vstack([np.array([np.concatenate([pool.acc[a], pool.acc[b]]) for _, a, b in pool.pair_cases()], dtype=np.uint32), extreme_pairs(N)])
    elif kind in ("scalar_te", "scalar_377"):
        rows = [words32(v, 8) for v in scalar_edge_values(SCALAR_MODULI[kind]) + [rnd.getrandbits(256) for _ in range(300)]]
    else:
        raise KeyError(name)
    arr = np.array(rows, dtype=np.uint64)
    assert arr.ndim == 2 and arr.shape[1] == iw and arr.max() < (1 << 32), (name, arr.shape)
    return arr.astype(np.uint32)


# ---------------------------------------------------------------------------------------------- the second table: inputs and bigint pins
def mont(N, v):
    """v in Montgomery form, canonical: class N, below the modulus"""
    F = FIELDS[N]
    return F.limbs(v % F.P * F.R % F.P)


def unmont(N, ls):
    F = FIELDS[N]
    return F.val(ls) * F.rinv % F.P


def naf_words(k):
    """the 17 words of a naf_t (check.hip.hpp) for k >= 1: pos[8] | neg[8] | top, built here as sm_shared_naf builds it on the host"""
    assert 0 < k < 1 << 255
    pos = neg = 0
    i = 0
    while k:
        if k & 1:
            if k & 3 == 3:
                neg |= 1 << i
                k += 1
            else:
                pos |= 1 << i
                k -= 1
            top = i
        k >>= 1
        i += 1
    return words32(pos, 8) + words32(neg, 8) + [top]


def naf_value(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w[:8])) - sum(int(x) << (32 * i) for i, x in enumerate(w[8:16]))


def root_exponents():
    """name -> (value, exp_t words[12] | top): (t - 1) / 2 of both fields (kRootExp*) and modulus - 2 (kInvExp*)"""
    out = {}
    for name, N in (("Te", 9), ("377", 14)):
        P = FIELDS[N].P
        t = P - 1
        while t % 2 == 0:
            t //= 2
        for kind, e in (("kRootExp", (t - 1) // 2), ("kInvExp", P - 2)):
            out[kind + name] = (e, words32(e, 12) + [e.bit_length() - 1])
    return out


class SwPool:
    """projective short-Weierstrass operands of sw377_add / sw377_dbl (Montgomery form, class N below 1.1 q) with the model's affine point:
    G1 points with Z = 1, outputs of earlier host additions and doublings (Z != 1), O as (0 : 1 : 0) and as it comes out of P + (-P), the
    points of order 3 (0, +-1), and T2 = (-1, 0) of order 2 with P + T2"""

    def __init__(self):
        Q = m377.Q
        base = m377.gen_points(33, 8) + [m377.G]
        base += [m377.neg(base[0]), m377.neg(base[1])]
        self.t3, self.t2 = [(0, 1), (0, Q - 1)], (Q - 1, 0)
        aff = base + self.t3 + [self.t2, m377.add(base[2], self.t2)]
        rows = [mont(14, x) + mont(14, y) + mont(14, 1) for x, y in aff]
        pts = list(aff)
        rows.append(mont(14, 0) + mont(14, 1) + mont(14, 0))
        pts.append(m377.INF)
        self.n_affine, self.ident = len(aff), len(rows) - 1
        arr = np.array(rows, dtype=np.uint32)
        nb = len(base)
        # Z != 1: sums and doubles of the G1 points, and O out of P + (-P)
        pairs = [(i, (i + 1) % nb) for i in range(nb - 2)] + [(0, nb - 2)]
        sums = run_host("sw_add", np.array([np.concatenate([arr[a], arr[c]]) for a, c in pairs], dtype=np.uint32))
        dbls = run_host("sw_dbl", arr[:4])
        self.zero_p = len(arr) + len(pairs) - 1
        self.acc = np.vstack([arr, sums, dbls])
        self.pts = pts + [m377.add(aff[a], aff[c]) for a, c in pairs] + [m377.add(p, p) for p in aff[:4]]
        assert self.pts[self.zero_p] is m377.INF
        self.g1 = list(range(nb)) + list(range(len(arr), len(arr) + len(pairs) - 1)) + list(range(len(arr) + len(pairs), len(self.acc)))
        self.i_t3, self.i_t2, self.i_p_t2 = [nb, nb + 1], nb + 2, nb + 3

    def decode(self, op, w, what=""):
        """(X : Y : Z) words -> the affine point; the coordinates keep the contract of a normalised value below 20 q"""
        Q = m377.Q
        c = [np.asarray(w[14 * k:14 * k + 14]) for k in range(3)]
        for k in range(3):
            assert all(int(v) <= LM for v in c[k][:13]) and FIELDS[14].val(c[k]) < 20 * Q, "%s: %s: coordinate %d leaves its class" % (op, what, k)
        X, Y, Z = (unmont(14, ck) for ck in c)
        if Z == 0:
            assert Y != 0, "%s: %s: (X : 0 : 0) is no point" % (op, what)
            assert X == 0, "%s: %s: Z = 0 with X != 0" % (op, what)
            return m377.INF
        zi = pow(Z, -1, Q)
        pt = (X * zi % Q, Y * zi % Q)
        assert m377.on_curve(pt), "%s: %s: not on the curve" % (op, what)
        return pt

    def pair_cases(self):
        """(name, a, b, exceptional): exceptional pairs differ by the point of order 2 -- the header states they give (0 : 0 : 0)"""
        g, I, Zp = self.g1, self.ident, self.zero_p
        neg = {i: j for i in range(self.n_affine) for j in range(self.n_affine) if self.pts[i] is not None and self.pts[j] == m377.neg(self.pts[i]) and i != j}
        cases = [("P+Q", g[0], g[1], False), ("P+Q of sums", g[-1], g[-3], False), ("P+P", g[0], g[0], False), ("P+P of a sum", g[-2], g[-2], False),
                 ("O+P", I, g[2], False), ("P+O", g[3], I, False), ("O+O", I, I, False), ("O'+P", Zp, g[4], False), ("P+O'", g[-1], Zp, False), ("O+O'", I, Zp, False),
                 ("T3+T3", self.i_t3[0], self.i_t3[0], False), ("T3+(-T3)", self.i_t3[0], self.i_t3[1], False), ("P+T3", g[0], self.i_t3[1], False),
                 ("T3+O", self.i_t3[0], I, False), ("T2+T2", self.i_t2, self.i_t2, False), ("(P+T2)+(P+T2)", self.i_p_t2, self.i_p_t2, False),
                 ("T2+T3", self.i_t2, self.i_t3[0], False),
                 ("T2+O", self.i_t2, I, True), ("O+T2", I, self.i_t2, True), ("O'+T2", Zp, self.i_t2, True), ("P+(P+T2)", 2, self.i_p_t2, True),
                 ("(P+T2)+P", self.i_p_t2, 2, True)]
        cases += [("P+(-P)", i, j, False) for i, j in list(neg.items())[:4]]
        rnd = random.Random(77)
        cases += [("pool %d + pool %d" % (a, c), a, c, False) for a, c in ((rnd.choice(g + [I, Zp]), rnd.choice(g + [I, Zp])) for _ in range(150))]
        return cases


@functools.lru_cache(maxsize=None)
def sw_pool():
    return SwPool()


def sqrt_cases(N):
    """(k, u, v, representative shifts): u / v of exact 2-adic order k for every k = 0 .. S (test_points_from_x_host.two_adic_radicands),
    u = 0, and u, v at the top of their bound (normalised, below 3.3 modulus: the canonical Montgomery value + 2 modulus)"""
    from test_points_from_x_host import two_adic_radicands
    P, rnd = FIELDS[N].P, random.Random(90 + N)
    out = []
    for k, r in two_adic_radicands(P):
        v = rnd.randrange(1, P) if N == 9 else 1
        out.append((k, r * v % P, v, (0, 0)))
    out += [(k, u, v, (2, 2)) for k, u, v, _ in out[::7]] + [(k, u, v, (2, 0)) for k, u, v, _ in out[3::11]]
    out += [(None, 0, rnd.randrange(1, P) if N == 9 else 1, sh) for sh in ((0, 0), (1, 0), (2, 2))]
    return out


def aff_cases(curve):
    """(slots: 8 pool indices, cnt): cnt = 1 .. 8 over projective results with Z != 1; BLS12-377 also infinity (both representations of
    Z = 0) at the first, a middle and the last slot, in runs and in every slot"""
    rnd = random.Random(5 + curve)
    if curve == 0:
        n = len(_pool(9, None).pts)
        return [([rnd.randrange(n) for _ in range(8)], cnt) for cnt in range(1, 9) for _ in range(4)]
    sp = sw_pool()
    fin = [i for i in sp.g1 if i >= sp.n_affine + 1]                          # Z != 1
    inf = [sp.ident, sp.zero_p]
    out = []
    for cnt in range(1, 9):
        pats = [set(), {0}, {cnt - 1}, {cnt // 2}, set(range(cnt)), set(range(0, cnt, 2)), set(range(cnt // 2, cnt)), set(range(0, max(1, cnt - 1)))]
        for pat in pats:
            out.append(([rnd.choice(inf) if j in pat else rnd.choice(fin) for j in range(8)], cnt))
    return out


def wire_points(curve, mont_form):
    """(name, wire words, reason at level 2): te_bad_classes / bls_bad_classes of test_point_checks_host and valid points; mont_form: every
    coordinate c stored as c 2^256 / c 2^384 mod the modulus, + the modulus where c was not canonical"""
    from test_point_checks_host import bls_bad_classes, te_bad_classes
    cb, P = (32, te_model.P) if curve == 0 else (48, m377.Q)
    if curve == 0:
        good = te_model.gen_points(3, 12) + [(te_model.GX, te_model.GY), (0, 1)]
        cases = te_bad_classes() + [("valid %d" % i, te_model.points_to_bytes([p]), 0) for i, p in enumerate(good)]
    else:
        good = m377.gen_points(3, 12) + [m377.G]
        cases = bls_bad_classes() + [("valid %d" % i, m377.points_to_bytes([p]), 0) for i, p in enumerate(good)]
    out = []
    for name, raw, reason in cases:
        cs = [int.from_bytes(raw[cb * k:cb * k + cb], "little") for k in range(2)]
        if mont_form:
            cs = [(c % P << (8 * cb)) % P + (P if c >= P else 0) for c in cs]
        out.append((name, sum((words32(c, cb // 4) for c in cs), []), reason))
    return out


def table2_inputs(name):
    """uint32 [n, words in] for one operation of the second table, inside the contract its header states, at the contract's edges"""
    iw, _ = OPS2[name]
    N = 14 if (name.endswith(("_14", "_12", "_377", "_377_mont")) or name.startswith("sw_") or name == "sqrt_14") else 9
    F = FIELDS[N]
    P, lim = F.P, F.limbs
    rnd = random.Random(name)
    kind = name.rsplit("_", 1)[0] if name.endswith(("_9", "_14", "_8", "_12")) else name
    nw = 8 if N == 9 else 12
    if kind == "is_zero":
        rows = [lim(v) for v in (0, P, 1, P - 1, P + 1, 2 * P - 1, 2 * P, 2 * P + 1)] + [lim(k * P) for k in range(3, 20)] + [lim(k * P + 1) for k in range(3, 20, 3)]
        for K in (2, 4):                                   # a - b + K p for equal residues in different representatives
            vs = [0, 1] + [rnd.randrange(P // 10) for _ in range(20)]
            pairs = [(lim(v), lim(v + P)) for v in vs] + [(lim(v + P), lim(v)) for v in vs] + [(lim(v), lim(v)) for v in vs] + [(lim(v + 1), lim(v + P)) for v in vs[:6]]
            rows += [list(r) for r in run_host("sub%d_%d" % (K, N), np.array([a + c for a, c in pairs], dtype=np.uint32))]
        rows += [lim(rnd.randrange(1, P)) for _ in range(100)]
    elif kind == "to_canon":
        vs = [0, 1, P - 1, F.R % P, (P - 1) * F.R % P] + [rnd.randrange(P // 10) for _ in range(40)] + [P // 10 - 1]
        rows = [lim(v) for v in vs] + [lim(v + P) for v in vs if v + P < 1.1 * P]
        rows += [lim(rnd.randrange(P)) for _ in range(60)]
        prod = run_host("mul_%d" % N, np.array([lim(rnd.randrange(P)) + lim(rnd.randrange(P)) for _ in range(100)], dtype=np.uint32))
        rows += [list(r) for r in prod]
    elif kind == "from_canon":
        vals = [0, 1, P - 1, P, P + 1, (1 << (32 * nw)) - 1] + [rnd.getrandbits(32 * nw) for _ in range(150)] + [rnd.randrange(P) for _ in range(100)]
        rows = [words32(v, nw) for v in vals]
    elif kind == "inv":
        rows = [mont(N, v) for v in (1, P - 1, 2)] + [lim(0), lim(P)] + [mont(N, rnd.randrange(1, P)) for _ in range(120)]
        rows += [lim(F.val(r) + P) for r in rows[5:] if F.val(r) + P < 1.1 * P][:10]
    elif name in ("sqrt_ratio_9", "sqrt_14"):
        rows = []
        for _, u, v, (su, sv) in sqrt_cases(N):
            ur = lim(u * F.R % P + su * P)
            rows.append(ur + lim(v * F.R % P + sv * P) if N == 9 else ur)
    elif kind in ("words_lt", "words_neg"):
        top = 1 << (32 * (nw - 1))
        vals = [P, P - 1, P + 1, P - top, P + top, 0, 1, (1 << (32 * nw)) - 1, P ^ 1, P - 2] + [rnd.randrange(P) for _ in range(150)]
        vals += [rnd.getrandbits(32 * nw) for _ in range(100)] + [(P >> (32 * j) << (32 * j)) + rnd.getrandbits(32 * j) for j in range(1, nw)]
        rows = [words32(v, nw) for v in vals]
    elif name in ("sw_add", "sw_dbl", "sw_cneg"):
        sp = sw_pool()
        if name == "sw_add":
            rows = np.array([np.concatenate([sp.acc[a], sp.acc[c]]) for _, a, c, _ in sp.pair_cases()], dtype=np.uint32)
        elif name == "sw_dbl":
            rows = sp.acc
        else:
            rows = np.array([list(r) + [s] for r in sp.acc for s in (0, 1, 0xFFFFFFFF, 2)], dtype=np.uint32)
    elif name == "add_cneg":
        pool = _pool(9, None)
        rows = np.array([np.concatenate([pool.acc[a], pool.acc[c], [s]]) for _, a, c in pool.pair_cases() for s in (0, 1)], dtype=np.uint32)
    elif name == "mul_order_te":
        rows = [mont(9, x) + mont(9, y) + naf_words(k) for _, (x, y), k in order_cases()]
    elif name == "sm_digits":
        rows = [words32(k, 8) for k in digit_scalars()]
    elif name == "naf_digit":
        nafs = [naf_words(k) for k in (te_model.L, m377.R_ORDER, 4 * te_model.L - 1, 1, (1 << 254) + 1)] + [naf_words(rnd.getrandbits(253) | 1) for _ in range(2)]
        rows = [w + [i] for w in nafs for i in range(256)]
    elif name == "exp_bit":
        rows = [w + [i] for _, (_, w) in sorted(root_exponents().items()) for i in range(384)]
    elif name in ("aff_group_te", "aff_group_377"):
        curve = 0 if name.endswith("te") else 1
        acc = _pool(9, None).acc if curve == 0 else sw_pool().acc
        n3, jw = (27, 28) if curve == 0 else (42, 44)
        rows = []
        for slots, cnt in aff_cases(curve):
            row = []
            for j, i in enumerate(slots):                  # the slot's padding words, and the slots past cnt, hold what must never be read
                row += ([int(v) for v in acc[i][:n3]] if j < cnt else [0xFFFFFFFF] * n3) + [0xDEADBEEF] * (jw - n3)
            rows.append(row + [cnt])
    elif name.startswith(("check_form_", "in_subgroup_")):
        rows = [w for _, w, _ in wire_points(0 if "_te" in name else 1, name.endswith("_mont"))]
    else:
        raise KeyError(name)
    arr = np.array(rows, dtype=np.uint64)
    assert arr.ndim == 2 and arr.shape[1] == iw and arr.max() < (1 << 32), (name, arr.shape)
    return arr.astype(np.uint32)


def digit_scalars():
    from test_scalar_mul_host import EDGE_377, EDGE_TE, digit_pattern_scalars
    rnd = random.Random(44)
    return EDGE_TE + EDGE_377 + digit_pattern_scalars() + [rnd.getrandbits(256) for _ in range(150)]


@functools.lru_cache(maxsize=None)
def order_cases():
    """(name, point, k) for mul_order_te: the NAF of L and of edge k below 4 L over subgroup points, the points of order 2 and 4, P + T2, P + T4"""
    from test_scalar_mul_host import te_torsion_points
    L = te_model.L
    rnd = random.Random(45)
    pts = [("subgroup point %d" % i, p) for i, p in enumerate(te_model.gen_points(23, 3))] + [("O", (0, 1))] + te_torsion_points()
    ks = [L, 1, 2, 3, L - 1, L + 1, 2 * L, 2 * L + 1, 4 * L - 1, (1 << 253) - 1, 1 << 252] + [rnd.randrange(1, 4 * L) for _ in range(8)]
    return [("[%d] %s" % (k, pn), p, k) for pn, p in pts for k in ks]


def check_table2(name, inp, out, dec=None):
    """the bigint pin of one operation of the second table: raises AssertionError naming the operation and the element"""
    N = 14 if (name.endswith(("_14", "_12", "_377", "_377_mont")) or name.startswith("sw_") or name == "sqrt_14") else 9
    F = FIELDS[N]
    P, val = F.P, F.val
    nw = 8 if N == 9 else 12
    kind = name.rsplit("_", 1)[0] if name.endswith(("_9", "_14", "_8", "_12")) else name
    wv = lambda ws: sum(int(x) << (32 * i) for i, x in enumerate(ws))
    class_n = lambda ls: all(int(x) <= LM for x in ls[:N - 1]) and val(ls) < 1.1 * P
    n = len(inp)
    assert len(out) == n, name

    def fail(e, msg):
        raise AssertionError("%s: element %d: %s" % (name, e, msg))
    if kind == "is_zero":
        for e in range(n):
            if int(out[e, 0]) != (1 if val(inp[e]) % P == 0 else 0):
                fail(e, "verdict %d for the value %x" % (int(out[e, 0]), val(inp[e])))
        assert 30 < int(out.sum()) < n - 30
    elif kind == "to_canon":
        for e in range(n):
            want = val(inp[e]) * F.rinv % P
            if wv(out[e]) != want:
                fail(e, "%x is not the canonical value %x%s" % (wv(out[e]), want, " (it is that + the modulus)" if wv(out[e]) == want + P else ""))
    elif kind == "from_canon":
        for e in range(n):
            if not (class_n(out[e]) and val(out[e]) % P == wv(inp[e]) * F.R % P):
                fail(e, "not w R in class N below 1.1 modulus")
    elif kind == "inv":
        for e in range(n):
            a = unmont(N, inp[e])
            if not (class_n(out[e]) and unmont(N, out[e]) == (pow(a, -1, P) if a else 0)):
                fail(e, "not the inverse")
    elif name in ("sqrt_ratio_9", "sqrt_14"):
        Z = 11 if N == 9 else 5
        cases = sqrt_cases(N)
        assert n == len(cases)
        S = 47 if N == 9 else 46
        assert {k for k, _, _, _ in cases} >= set(range(S + 1))
        for e, (k, u, v, _) in enumerate(cases):
            flag, y = int(out[e, 0]), unmont(N, out[e, 1:])
            r = u * pow(v, -1, P) % P
            want = r != 0 and pow(r, (P - 1) // 2, P) == 1
            assert k is None or (k < S) == want
            if flag != int(want):
                fail(e, "flag %d for a radicand of 2-adic order %s" % (flag, k))
            if not class_n(out[e, 1:]) or y * y % P != (r if want else Z * r % P):
                fail(e, "y is no root of %s (2-adic order %s)" % ("u / v" if want else "Z u / v", k))
    elif kind == "words_lt":
        for e in range(n):
            if int(out[e, 0]) != int(wv(inp[e]) < P):
                fail(e, "verdict %d" % int(out[e, 0]))
    elif kind == "words_neg":
        for e in range(n):
            a = wv(inp[e])
            if wv(out[e]) != (0 if a == 0 else (P - a) % (1 << (32 * nw))):
                fail(e, "not modulus - a")
    elif name in ("sw_add", "sw_dbl", "sw_cneg"):
        sp = sw_pool()
        if name == "sw_add":
            for e, (what, a, c, exceptional) in enumerate(sp.pair_cases()):
                if exceptional:                            # check.hip.hpp: "turns into (0 : 0 : 0)"
                    if any(unmont(14, out[e, 14 * k:14 * k + 14]) for k in range(3)):
                        fail(e, "%s: an exceptional pair must give (0 : 0 : 0)" % what)
                elif sp.decode(name, out[e], what) != m377.add(sp.pts[a], sp.pts[c]):
                    fail(e, "%s: not the model's sum" % what)
        elif name == "sw_dbl":
            for e in range(n):
                if sp.decode(name, out[e], "entry %d" % e) != m377.add(sp.pts[e], sp.pts[e]):
                    fail(e, "not the model's double")
        else:
            for e in range(n):
                pt, sign = sp.pts[e // 4], int(inp[e, 42])
                if sign == 0 and list(out[e]) != list(inp[e, :42]):
                    fail(e, "sign 0 changed the point")
                if list(out[e, :14]) != list(inp[e, :14]) or list(out[e, 28:]) != list(inp[e, 28:42]):
                    fail(e, "X or Z changed")
                if sp.decode(name, out[e], "entry %d" % e) != (m377.neg(pt) if sign else pt):
                    fail(e, "not %sP" % ("-" if sign else ""))
                if sign and pt is not None and pt[1] and unmont(14, out[e, 14:28]) == unmont(14, inp[e, 14:28]):
                    fail(e, "Y kept under a set sign")
    elif name == "add_cneg":
        pool = _pool(9, None)
        cases = [(what, a, c, s) for what, a, c in pool.pair_cases() for s in (0, 1)]
        negb = []
        for what, a, c, s in cases:                        # (a, -b) for ete_add<9>: -b = (-x, y, z, -t), canonical
            b4 = pool.acc[c].reshape(4, 9)
            nb = [F.limbs((P - val(b4[0]) % P) % P), list(b4[1]), list(b4[2]), F.limbs((P - val(b4[3]) % P) % P)] if s else [list(r) for r in b4]
            negb.append(np.concatenate([pool.acc[a], np.array(sum(nb, []), dtype=np.uint32)]))
        ref = run_host("add_9", np.array(negb, dtype=np.uint32))
        for e, (what, a, c, s) in enumerate(cases):
            want = msum(9, [pool.pts[a], mneg(9, pool.pts[c]) if s else pool.pts[c]])
            try:
                got = dec.point("ete_add_cneg", 9, out[e], what)
                same = dec.point("ete_add<9>", 9, ref[e], what)
            except AssertionError as err:
                fail(e, str(err))
            if got != want or got != same:
                fail(e, "%s, sign %d: %s, the model gives %s, ete_add<9> on (a, %sb) %s" % (what, s, got, want, "-" if s else "", same))
    elif name == "mul_order_te":
        for e, (what, pt, k) in enumerate(order_cases()):
            assert naf_value(inp[e, 18:]) == k
            try:
                dec.check("mul_order_te", 9, out[e], te_model.scalar_mul(k, pt), what)
            except AssertionError as err:
                fail(e, str(err))
    elif name == "sm_digits":
        C = sum(2 << (2 * i) for i in range(129))
        for e, k in enumerate(digit_scalars()):
            ds = [int(np.int32(x)) for x in out[e, 9:].view(np.int32)]
            if wv(out[e, :9]) != k + C or not all(-2 <= d <= 1 for d in ds) or sum(d << (2 * i) for i, d in enumerate(ds)) != k:
                fail(e, "the digits of %x do not sum to it" % k)
    elif name == "naf_digit":
        for e in range(n):
            i = int(inp[e, 17])
            want = ((int(inp[e, i >> 5]) >> (i & 31)) & 1) - ((int(inp[e, 8 + (i >> 5)]) >> (i & 31)) & 1)
            if int(out[e:e + 1, 0].view(np.int32)[0]) != want:
                fail(e, "digit %d" % i)
        assert naf_value(inp[0, :17]) == te_model.L and naf_value(inp[256, :17]) == m377.R_ORDER
    elif name == "exp_bit":
        exps = [v for _, (v, _) in sorted(root_exponents().items())]
        for e in range(n):
            if int(out[e, 0]) != (exps[e // 384] >> (e % 384)) & 1:
                fail(e, "bit %d" % (e % 384))
    elif name in ("aff_group_te", "aff_group_377"):
        curve = 0 if name.endswith("te") else 1
        pts = _pool(9, None).pts if curve == 0 else sw_pool().pts
        pw = 16 if curve == 0 else 24
        for e, (slots, cnt) in enumerate(aff_cases(curve)):
            for j in range(8):
                got = [int(x) for x in out[e, pw * j:pw * (j + 1)]]
                pt = pts[slots[j]]
                want = [0xA5A5A5A5] * pw if j >= cnt else [0] * pw if pt is None else words32(pt[0], pw // 2) + words32(pt[1], pw // 2)
                if got != want:
                    fail(e, "cnt = %d, slot %d (%s)" % (cnt, j, "past cnt" if j >= cnt else "infinity" if pt is None else "finite"))
    elif name.startswith("check_form_"):
        for e, (what, _, reason) in enumerate(wire_points(0 if "_te" in name else 1, name.endswith("_mont"))):
            if int(out[e, 0]) != (reason if reason < 3 else 0):
                fail(e, "%s: verdict %d" % (what, int(out[e, 0])))
    elif name.startswith("in_subgroup_"):
        for e, (what, _, reason) in enumerate(wire_points(0 if "_te" in name else 1, False)):
            if reason in (0, 3) and int(out[e, 0]) != int(reason == 0):
                fail(e, "%s: verdict %d" % (what, int(out[e, 0])))
    else:
        raise KeyError(name)
