"""Native-layout inputs without a GPU (include/te_msm.h: options "scalar_record_bytes", "point_stride", "point_infinity_flag").

  * the case builders of tests/layout_cases.py against the bigint reading of the records;
  * a bounds replay of every kernel load that depends on the scalar record size: the address arithmetic of digits_block, k_digits_ragged
    (csrc/kernels.hip.hpp) and of k_scalar_mul / k_mul_base (csrc/scalar_mul.hip.hpp, csrc/mul_base.hip.hpp) is restated here and
    walked for every shape tests/test_gpu_native_layout.py runs -- no read may start before the buffer or end past byte n * record;
  * the binding: `_sizes` follows the option and the length checks refuse buffers of the other size;
  * points at a stride: a bounds replay of the strided loader (csrc/strided.hip.hpp) over every shape of the GPU tests; the strided
    conversion compiled for the host (tests/csrc/layoutcheck.cpp) against bigints, flagged records included; the deliberate mistakes."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import layout_cases as lc
from oracle import model377 as m377
from oracle import oracle, oracle377

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "csrc")
PKG = "webgpu-msm-twisted-edwards_amd"


# ---- the case builders -----------------------------------------------------------------------------------------------------------------------
def test_repack_keeps_the_values(pkg):
    n = 300
    pts, sc48, sc32 = lc.synth377(PKG, 3, n)
    assert len(pts) == 96 * n and len(sc48) == 48 * n and len(sc32) == 32 * n
    for i in (0, 1, 7, 299):
        v = int.from_bytes(sc48[48 * i:48 * i + 48], "little")
        assert v < lc.R_377 and v == int.from_bytes(sc32[32 * i:32 * i + 32], "little")
    assert lc.widen48(sc32) == sc48
    with pytest.raises(AssertionError):
        lc.repack32(sc48[:40] + b"\x01" + sc48[41:])                              # a value of 2^320: no 32-byte record holds it


def test_montgomery_records_decode_to_the_values():
    rng = np.random.default_rng(1)
    ks = [int.from_bytes(rng.bytes(32), "little") % lc.R_377 for _ in range(9)] + [0, 1, lc.R_377 - 1]
    sc32 = b"".join(k.to_bytes(32, "little") for k in ks)
    m32, m48 = lc.to_montgomery(sc32, 32), lc.to_montgomery(lc.widen48(sc32), 48)
    assert lc.widen48(m32) == m48
    rinv = pow(lc.RA, -1, lc.R_377)
    assert [int.from_bytes(m32[32 * i:32 * i + 32], "little") * rinv % lc.R_377 for i in range(len(ks))] == ks


# ---- bounds replay -----------------------------------------------------------------------------------------------------------------------------
DIG_BLOCK, DIG_THREADS = 1024, 512          # TE_DIG_BLOCK, TE_DIG_THREADS


def test_the_replay_restates_the_kernels_as_they_are():
    """the lines whose arithmetic the replay below repeats are still in the sources, and the launch geometry is the one assumed"""
    k = open(os.path.join(CSRC, "kernels.hip.hpp")).read()
    assert "#define TE_DIG_BLOCK 1024u" in k and "#define TE_DIG_THREADS 512u" in k
    def has(text, *exprs):                   # the arithmetic expressions only, whatever the spacing around them
        flat = re.sub(r"\s+", "", text)
        return all(re.sub(r"\s+", "", e) in flat for e in exprs)
    assert has(k, "min(i0, n - 1u)", "min(i0 + 1u, n - 1u)", "scalars[st * ia + 1]", "scalars[st * ib + 1]", "scalars[st * ia + 2]", "scalars[st * ib + 2]",
               "scalars + tab.off[m] * prm.sc_stride")
    t = open(os.path.join(CSRC, "te_msm.hip")).read()
    assert has(t, "prm.sc_stride = (uint32_t)p.sc_bytes / 16u", "(prm.nst + TE_DIG_BLOCK - 1u) / TE_DIG_BLOCK")
    for name in ("scalar_mul.hip.hpp", "mul_base.hip.hpp"):
        assert has(open(os.path.join(CSRC, name)).read(), "sc[(size_t)i * SQ + j]", "int SQ = (CURVE == 1 ? 3 : 2)")
    # (a 32-byte record reaches the kernels with SQ = 2 on both curves, BLS12-377's own 48-byte record with SQ = 3: with_scalar_quads)
    assert has(open(os.path.join(CSRC, "points.hip")).read(), "te::k_scalar_mul<C, false, decltype(q)::value>", "te::k_mul_base<C, FORM, decltype(q)::value>",
               "if (sb != 32) { f(std::integral_constant<int, 3>{}); return; }", "f(std::integral_constant<int, 2>{});", "(m + 255u) / 256u")


def digit_reads(n, nst, stride, first=0):
    """every 16-byte load of the digit kernel over n records that start `first` records into the buffer: (byte offset, bytes)"""
    out = []
    blocks = (nst + DIG_BLOCK - 1) // DIG_BLOCK
    steps = DIG_BLOCK // (2 * DIG_THREADS)
    for blk in range(blocks):
        for step in range(steps):
            for t in range(DIG_THREADS):
                i0 = 2 * ((blk * steps + step) * DIG_THREADS + t)
                ia, ib = min(i0, n - 1), min(i0 + 1, n - 1)
                words = [stride * ia, stride * ia + 1, stride * ib, stride * ib + 1]
                if stride == 3:
                    words += [stride * ia + 2, stride * ib + 2]
                out += [(16 * (first * stride + w), 16) for w in words]
    return out


def lane_reads(m, sq):
    """k_scalar_mul / k_mul_base over a piece of m records: lane i < m (grid of 256-lane blocks) loads words i SQ, i SQ + 1"""
    out = []
    for i in range(((m + 255) // 256) * 256):
        if i >= m:
            continue
        out += [(16 * (i * sq + j), 16) for j in range(2)]
    return out


def inside(reads, nbytes):
    return all(0 <= at and at + size <= nbytes for at, size in reads)


def row_stride(n):
    return (n + 7) // 8 * 8                 # at most: the digit rows' stride is n rounded up to a multiple of 8 (plan_arith.hpp)


@pytest.mark.parametrize("rec", [32, 48])
def test_no_scalar_load_leaves_the_buffer(rec):
    stride = rec // 16
    shapes = set(lc.SCALAR_SHAPES) | {n + 5 for n in lc.SCALAR_SHAPES} | {50, 1024, 1025}
    for n in sorted(shapes):
        for nst in (row_stride(n), row_stride(n) + 8, 4096):                    # whatever stride a plan gives the rows
            assert inside(digit_reads(n, nst, stride), n * rec), (n, nst)
        assert inside(lane_reads(n, stride), n * rec), n
    # the packed batch: MSM m's len[m] >= 1 records start off[m] records in (an empty MSM runs no digit kernel)
    total = sum(lc.BATCH_LENS)
    nst = row_stride(max(lc.BATCH_LENS))
    off = 0
    for L in lc.BATCH_LENS:
        if L:
            reads = digit_reads(L, nst, stride, first=off)
            assert inside(reads, total * rec), L
            assert min(at for at, _ in reads) == off * rec and max(at + s for at, s in reads) == (off + L) * rec, L
        off += L


def test_deliberate_mistakes_are_caught():
    # 32-byte records read with the 48-byte stride leave the buffer; the third load of a 48-byte record does too at stride 2's size
    assert not inside(digit_reads(300, 304, 3), 300 * 32)
    assert not inside(lane_reads(300, 3), 300 * 32)
    # an offset in bytes of the OTHER record size lands elsewhere than the MSM's first record
    assert digit_reads(3, 8, 2, first=5)[0][0] == 5 * 32 != 5 * 48
    # unclamped indices (i0 + 1 for an odd n) would read one record past the end
    n = 257
    assert max(at + s for at, s in digit_reads(n, row_stride(n), 2)) == n * 32
    assert 16 * (2 * n + 1) + 16 > n * 32


# ---- the binding ---------------------------------------------------------------------------------------------------------------------------------
class _NoLibrary:
    """stands in for libtemsm.so: options are accepted, any other call means a length check let a wrong buffer through"""

    def te_msm_set_option(self, h, key, value):
        return 0

    def __getattr__(self, name):
        def called(*args):
            raise AssertionError("the binding called %s" % name)
        return called


def _context(pkg):
    c = object.__new__(pkg.MsmContext)
    c._h, c._L, c._held = None, _NoLibrary(), {}
    c._sizes, c.curve, c._scalar_record_bytes, c._point_stride = (64, 32, 64), pkg.CURVE_TE_BLS12, 0, 0
    return c


def test_binding_sizes_follow_the_option(pkg):
    c = _context(pkg)
    assert c._sizes == (64, 32, 64)
    c.set_option("scalar_record_bytes", 32)
    assert c._sizes == (64, 32, 64)
    c.set_option("curve", pkg.CURVE_BLS12_377_G1)
    assert c._sizes == (96, 32, 96)
    c.set_option("scalar_record_bytes", 0)
    assert c._sizes == (96, 48, 96)
    c.set_option("scalar_record_bytes", 48)
    assert c._sizes == (96, 48, 96)
    c.set_option("scalar_record_bytes", 32)
    assert c._sizes == (96, 32, 96)
    c.set_option("window_bits", 13)                                              # another option leaves them alone
    assert c._sizes == (96, 32, 96)
    c.set_option("curve", pkg.CURVE_TE_BLS12)
    assert c._sizes == (64, 32, 64)


def test_binding_length_checks_refuse_the_other_size(pkg):
    n = 6
    pts, s48, s32 = bytes(96 * n), bytes(48 * n), bytes(32 * n)
    c = _context(pkg)
    c.set_option("curve", pkg.CURVE_BLS12_377_G1)
    bases = pkg.binding.Bases(c, object(), n, pkg.CURVE_BLS12_377_G1)
    for rec, wrong in ((32, s48), (48, s32), (0, s32)):
        c.set_option("scalar_record_bytes", rec)
        calls = [lambda: c.run(pts, wrong), lambda: c.submit(pts, wrong), lambda: c.submit_async(pts, wrong), lambda: c.run_x(bytes(48 * n), wrong),
                 lambda: c.mul(pts, wrong), lambda: c.mul_x(bytes(48 * n), wrong), lambda: c.run_scalars(bases, wrong),
                 lambda: c.submit_scalars(bases, wrong), lambda: c.run_scalars_indexed(bases, list(range(n)), wrong)]
        for call in calls:
            with pytest.raises(pkg.MsmError) as e:
                call()
            assert e.value.code == -1 and "bytes" in str(e.value), rec
    # whole records only: 5 records of 48 bytes are no whole number of 32-byte ones
    c.set_option("scalar_record_bytes", 32)
    for call in (lambda: c.run_scalars_batch(bases, [bytes(48 * 5)]), lambda: c.mul_base(object(), bytes(48 * 5))):
        with pytest.raises(pkg.MsmError):
            call()


# ---- points at a stride: bounds replay of the strided loader (csrc/strided.hip.hpp) ------------------------------------------------------------
TILE, STRIDE_MAX = 256, 128                 # TE_STRIDE_TILE, TE_STRIDE_MAX


def strided_reads(n, stride, pw, flag, s8=None, flag_word=None):
    """strided_stage + strided_pick restated: (global 8-byte loads as byte ranges, LDS word indices written, LDS word indices read), for a
    launch of (n + 255) / 256 blocks of 256 threads.  s8 / flag_word: the deliberate mistakes below override them"""
    s8 = stride // 8 if s8 is None else s8
    flag_word = pw // 2 if flag_word is None else flag_word
    glob, lds_w, lds_r = [], [], []
    for blk in range((n + TILE - 1) // TILE):
        base = blk * TILE
        cnt = min(TILE, n - base)
        words, first = cnt * s8, blk * TILE * s8
        picks = []
        for t in range(TILE):
            for g in range(t, words, TILE):
                glob.append((8 * (first + g), 8))
                lds_w.append(g)
            if base + t < n:
                picks += [t * s8 + j for j in range(pw // 2)] + ([t * s8 + flag_word] if flag else [])
        assert all(r < words for r in picks), "a lane picks a word its block did not stage"
        lds_r += picks
    return glob, lds_w, lds_r


def test_the_strided_replay_restates_the_loader():
    s = open(os.path.join(CSRC, "strided.hip.hpp")).read()
    assert "#define TE_STRIDE_MAX 128u" in s and "#define TE_STRIDE_TILE 256u" in s
    flat = re.sub(r"\s+", "", s)
    for e in ("(uint64_t)blk * TE_STRIDE_TILE * (stride / 8u)", "g = threadIdx.x; g < words; g += TE_STRIDE_TILE", "tile[g] = from[g]",
              "tile + (size_t)t * (stride / 8u)", "r[PW / 2] & 0xffu"):
        assert re.sub(r"\s+", "", e) in flat, e


@pytest.mark.parametrize("curve", [0, 1])
def test_no_strided_load_leaves_the_buffer(curve):
    pw = 24 if curve else 16
    strides = set(lc.STRIDES[curve]) | {4 * pw, STRIDE_MAX}                     # the packed size as a stride, and the cap
    shapes = set(lc.STRIDE_SHAPES) | {299, 300, 1, 2}                           # n = 1; partial last tiles; 104 x 256 is no multiple of 16: a tile boundary inside a 16-byte word
    for stride in sorted(strides):
        for flag in ((False, True) if curve and stride >= 104 else (False,)):
            for n in sorted(shapes):
                glob, lds_w, lds_r = strided_reads(n, stride, pw, flag)
                assert inside(glob, n * stride), (n, stride)
                assert min(at for at, _ in glob) == 0 and max(at + s for at, s in glob) == n * stride      # the whole buffer, nothing else
                assert len(set(glob)) == len(glob), "a word is loaded twice"
                assert max(lds_w) < TILE * STRIDE_MAX // 8 and max(lds_r) < TILE * STRIDE_MAX // 8


def test_strided_loader_mistakes_are_caught():
    # the stride applied in 16-byte units: the loads leave an n x 104-byte buffer (or, where they fit, miss the records)
    glob, _, _ = strided_reads(300, 104, 24, False, s8=2 * (104 // 16))
    assert max(at + s for at, s in glob) != 300 * 104
    glob, _, _ = strided_reads(300, 128, 24, False, s8=2 * 128 // 8)
    assert not inside(glob, 300 * 128)
    # the flag read one 8-byte word late (offset 104 = the next record's x) leaves the staged tile for the block's last record
    with pytest.raises(AssertionError):
        strided_reads(256, 104, 24, True, flag_word=13)


# ---- the strided conversion, compiled for the host, against bigints (tests/csrc/layoutcheck.cpp) -----------------------------------------------
Q = lc.Q_377
R406, R261 = 1 << 406, 1 << 261                  # the engine's Montgomery radices: 14 and 9 limbs of 29 bits


@pytest.fixture(scope="module")
def layoutcheck():
    d = os.path.join(ROOT, "tests", "csrc")
    so, src = os.path.join(d, "liblayoutcheck.so"), os.path.join(d, "layoutcheck.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("strided.hip.hpp", "curve.hpp", "fp.hpp", "fq377.hpp", "field.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    L = ctypes.CDLL(so)
    L.lc_convert377.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.lc_convert377.restype = ctypes.c_int64
    L.lc_convert_te.argtypes = [ctypes.c_char_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.c_void_p]
    L.lc_convert_te.restype = ctypes.c_int64
    return L


def convert377(L, img, n, stride, mont, flag):
    """(records as [hm, hp, dt, z] residues with the Montgomery factor taken off, end of the highest byte the loader read)"""
    out = (ctypes.c_uint32 * (56 * n))()
    end = L.lc_convert377(img, n, stride, int(mont), int(flag), out)
    rinv = pow(R406, -1, Q)
    return [[sum(int(out[56 * i + 14 * k + j]) << (29 * j) for j in range(14)) * rinv % Q for k in range(4)] for i in range(n)], end


def weierstrass_of(rec, consts):
    """the short-Weierstrass point a projective record (times 2: hm = Y - X, hp = Y + X, dt = -2 d T, z = 2 Z) stands for; None = infinity"""
    from test_oracle_bls377 import edwards_to_weierstrass
    s, f, d = consts
    hm, hp, dt, z = rec
    i2 = pow(2, -1, Q)
    X, Y, Z = (hp - hm) * i2 % Q, (hp + hm) * i2 % Q, z * i2 % Q
    assert Z != 0 and dt * Z % Q == -2 * d * X * Y % Q, "dt is not -2 d T with T = X Y / Z"
    zi = pow(Z, -1, Q)
    return edwards_to_weierstrass(X * zi % Q, Y * zi % Q, s, f)


IDENTITY = [1, 1, 0, 2]                          # the neutral element (0 : 1 : 1 : 0) in that form; its affine record is (1/2, 1/2, 0)


def test_strided_conversion_against_bigints_377(layoutcheck, fq377check):
    from test_oracle_bls377 import _edwards_consts
    consts = _edwards_consts(fq377check)
    n = 300
    pts = oracle377.gen_points(21, n)
    xy = [m377.xy_from_bytes(pts[96 * i:96 * i + 96]) for i in range(n)]
    rng = np.random.default_rng(4)
    for stride in (96, 104, 112, 128):
        for mont in (False, True):
            src = lc.to_montgomery_points(pts, 1) if mont else pts
            img = lc.at_stride(src, 96, stride)
            recs, end = convert377(layoutcheck, img, n, stride, mont, False)
            assert end == n * stride
            assert [weierstrass_of(r, consts) for r in recs] == xy, (stride, mont)
            if stride < 104:
                continue
            # flagged records: zero, random and all-0xff coordinate bytes give the identity, their neighbours their own points
            for junk in (bytes(96), rng.bytes(96), b"\xff" * 96):
                a = bytearray(img)
                flagged = (0, 8, 255, 256, 299)
                for i in range(n):
                    a[stride * i + 96] = 0
                for i in flagged:
                    a[stride * i:stride * i + 96] = junk
                    a[stride * i + 96] = 1
                recs, end = convert377(layoutcheck, bytes(a), n, stride, mont, True)
                assert end == n * stride
                for i in range(n):
                    if i in flagged:
                        assert recs[i] == IDENTITY and weierstrass_of(recs[i], consts) is None, (stride, mont, i)
                        zi = pow(recs[i][3], -1, Q)                              # the affine record k_affine377 makes of it: (hm, hp, dt) / z
                        assert [v * zi % Q for v in recs[i][:3]] == [pow(2, -1, Q), pow(2, -1, Q), 0]
                    else:
                        assert weierstrass_of(recs[i], consts) == xy[i], (stride, mont, i)


def test_strided_conversion_against_bigints_te(layoutcheck):
    n = 300
    P = lc.P_TE
    D = 3021
    pts = oracle.gen_points(22, n)
    rinv, i2 = pow(R261, -1, P), pow(2, -1, P)
    for stride in (64, 72, 80, 128):
        for mont in (False, True):
            img = lc.at_stride(lc.to_montgomery_points(pts, 0) if mont else pts, 64, stride)
            out = (ctypes.c_uint32 * (27 * n))()
            assert layoutcheck.lc_convert_te(img, n, stride, int(mont), out) == n * stride
            for i in (0, 1, 7, 255, 256, 257, 299):
                x, y = (int.from_bytes(pts[64 * i + 32 * k:64 * i + 32 * k + 32], "little") for k in (0, 1))
                got = [sum(int(out[27 * i + 9 * k + j]) << (29 * j) for j in range(9)) * rinv % P for k in range(3)]
                assert got == [(y - x) * i2 % P, (y + x) * i2 % P, -D * x * y % P], (stride, mont, i)


def test_conversion_mistakes_are_caught(layoutcheck, fq377check):
    """each deliberate mistake gives another answer than the loader's, so the tests above (and the GPU tests) would see it"""
    from test_oracle_bls377 import _edwards_consts
    consts = _edwards_consts(fq377check)
    n = 9
    pts = oracle377.gen_points(23, n)
    xy = [m377.xy_from_bytes(pts[96 * i:96 * i + 96]) for i in range(n)]
    img = bytearray(lc.arkworks_image(pts, (4,), b"\x00"))
    good, _ = convert377(layoutcheck, bytes(img), n, 104, True, True)
    assert good[4] == IDENTITY and weierstrass_of(good[3], consts) == xy[3]
    # the flag read at offset 97: the padding byte there is the fill, so EVERY record would read as flagged
    moved = bytearray(img)
    for i in range(n):
        moved[104 * i + 96], moved[104 * i + 97] = moved[104 * i + 97], moved[104 * i + 96]
    at97, _ = convert377(layoutcheck, bytes(moved), n, 104, True, True)
    assert at97 != good and all(r == IDENTITY for r in at97)
    # the stride applied in 16-byte units (104 -> 96): record 1 onwards is read from the wrong bytes
    wrong, _ = convert377(layoutcheck, bytes(img)[:96 * n], n, 96, True, False)
    assert wrong[0] == good[0] and wrong[1] != good[1]
    # x, y mapped instead of ignored under the flag: zeros map to a record with z = 0, not to the identity
    mapped, _ = convert377(layoutcheck, bytes(img), n, 104, True, False)
    assert mapped[4] != IDENTITY and mapped[4][3] == 0
    # the identity's affine record written as zeros: (0, 0, 0) is not (1/2, 1/2, 0).  (No host code writes the affine record -- k_affine377 is
    # device code -- so this line only pins the expected value; the guard that runs the code is the GPU test's identity_residues(168).)
    zi = pow(good[4][3], -1, Q)
    assert [v * zi % Q for v in good[4][:3]] != [0, 0, 0]
