"""Shared case builders for the native-layout tests (include/te_msm.h: options "scalar_record_bytes", "point_stride",
"point_infinity_flag").  Scalars: BLS12-377 scalars as a native prover holds them -- 32-byte records -- beside the 48-byte records of the
wire format, over the same values.  Points: packed points laid out at a stride with filled padding, Montgomery coordinates, and the image
of arkworks' &[G1Affine] (stride 104, a flag byte).  Host code only; the expected results come from oracle/oracle377.py, oracle/oracle.py
and the engine's own packed / 48-byte calls."""
import functools

import numpy as np

R_377 = 8444461749428370424248824938781546531375899335154063827935233455917409239041
Q_377 = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
RA = 1 << 256
CURVE_BLS = 1
# every n of the scalar tests: one scalar, a pair (the digit kernel decomposes two per thread), an odd tail, one below and two above a
# 256-lane block of the multiplication kernels, and an n that is none of these
SCALAR_SHAPES = (1, 2, 3, 255, 257, 300)
# one packed batch: an empty MSM, MSMs that start at odd and even record offsets (the digit kernel reads records in pairs from off[m])
BATCH_LENS = (0, 1, 2, 3, 255, 257)


def repack32(sc48: bytes) -> bytes:
    """48-byte scalar records (value in bytes 0..31, zeros above) -> 32-byte records: just the values"""
    a = np.frombuffer(sc48, dtype=np.uint8).reshape(-1, 48)
    assert not a[:, 32:].any(), "a 48-byte record holds a value of 256 bits or more"
    return a[:, :32].tobytes()


def widen48(sc32: bytes) -> bytes:
    """the inverse: 32-byte values -> 48-byte records"""
    a = np.frombuffer(sc32, dtype=np.uint8).reshape(-1, 32)
    return np.concatenate([a, np.zeros((len(a), 16), dtype=np.uint8)], axis=1).tobytes()


@functools.lru_cache(maxsize=None)
def synth377(pkg_name: str, seed: int, n: int):
    """(points 96 n bytes, scalar records 48 n bytes, the same scalars in 32-byte records) of te_msm_synth_inputs_bls12_377"""
    import importlib
    pkg = importlib.import_module(pkg_name)
    pts, sc48 = pkg.synth_inputs(seed, n, curve=CURVE_BLS)
    return pts, sc48, repack32(sc48)


def to_montgomery(sc: bytes, rec: int) -> bytes:
    """every record's value k -> a = k 2^256 mod r, in records of the same size (option "scalars_montgomery")"""
    out = bytearray()
    for i in range(len(sc) // rec):
        k = int.from_bytes(sc[rec * i:rec * i + 32], "little")
        out += (k * RA % R_377).to_bytes(32, "little") + bytes(rec - 32)
    return bytes(out)


def xs_of_377(pts: bytes) -> bytes:
    """the x-only form of BLS12-377 points x || y (te_msm_points_from_x's): the 48-byte x with bit 7 of byte 47 set for the larger root"""
    a = np.frombuffer(pts, dtype=np.uint8).reshape(-1, 96)
    xs = a[:, :48].copy()
    half = (Q_377 - 1) // 2
    for i in range(len(a)):
        if int.from_bytes(a[i, 48:].tobytes(), "little") > half:
            xs[i, 47] |= 0x80
    return xs.tobytes()


# ---- points at a stride, and arkworks' G1Affine image (options "point_stride", "point_infinity_flag", "points_montgomery") -----------------
FILL = 0xA5                                  # padding bytes: never zeros, so that a kernel that interprets them is found out
P_TE = 8444461749428370424248824938781546531375899335154063827935233455917409239041      # base field of the Twisted-Edwards curve
# the n of the strided binds: the affine group of 8, the 256-record tile and block, two and three tiles, and an n that is none of these
STRIDE_SHAPES = (1, 7, 8, 9, 255, 256, 257, 511, 512, 513, 300)
STRIDES = {0: (72, 80, 128), 1: (104, 112, 128)}       # curve -> strides (the packed sizes 64 / 96 are the host test's)


def at_stride(pts: bytes, pb: int, stride: int, fill: int = FILL) -> bytes:
    """packed points of pb bytes -> records of `stride` bytes: x || y first, `fill` behind"""
    a = np.frombuffer(pts, dtype=np.uint8).reshape(-1, pb)
    out = np.full((len(a), stride), fill, dtype=np.uint8)
    out[:, :pb] = a
    return out.tobytes()


def to_montgomery_points(pts: bytes, curve: int) -> bytes:
    """every coordinate x -> x 2^256 mod p (32 bytes) / x 2^384 mod q (48 bytes): option "points_montgomery" """
    cb, f = (48, Q_377) if curve == CURVE_BLS else (32, P_TE)
    ra = 1 << (8 * cb)
    return b"".join((int.from_bytes(pts[cb * i:cb * i + cb], "little") * ra % f).to_bytes(cb, "little") for i in range(len(pts) // cb))


def arkworks_image(pts96: bytes, flagged=(), garbage: bytes = b"", flag_value: int = 1, fill: int = FILL) -> bytes:
    """&[G1Affine] of arkworks 0.4 on a 64-bit little-endian host, as pinned in include/te_msm.h: per point x[48] | y[48] as Montgomery
    residues | infinity: one byte | 7 bytes of padding = 104 bytes.  flagged: indices whose flag byte is flag_value and whose 96 coordinate
    bytes are `garbage` repeated (arkworks stores zeros there; the engine must not care)"""
    out = np.frombuffer(at_stride(to_montgomery_points(pts96, CURVE_BLS), 96, 104, fill), dtype=np.uint8).reshape(-1, 104).copy()
    out[:, 96] = 0
    junk = np.frombuffer((garbage * 96)[:96] if garbage else bytes(96), dtype=np.uint8)
    for i in flagged:
        out[i, :96] = junk
        out[i, 96] = flag_value
    return out.tobytes()


def without(buf: bytes, rec: int, drop) -> bytes:
    """the records of buf whose index is not in drop"""
    a = np.frombuffer(buf, dtype=np.uint8).reshape(-1, rec)
    keep = np.ones(len(a), dtype=bool)
    keep[list(drop)] = False
    return a[keep].tobytes()
