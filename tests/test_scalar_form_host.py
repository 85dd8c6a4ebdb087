"""Montgomery-form inputs (options "scalars_montgomery" / "points_montgomery"), without a GPU: csrc/scalar_form.hpp -- the reduction the
digit kernels run on every scalar -- and the Montgomery-input instantiations of the bind path's record conversions, compiled for the host
by tests/csrc/scalarform.cpp and checked against Python integers; the generated constants; a stand-alone sanitizer build of the same
program; and the new names in the header, the cross-compiled library, the package and the addon."""
import ctypes
import inspect
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "csrc", "scalarform.cpp")
L_TE = 2111115437357092606062206234695386632838870926408408195193685246394721360383
R_377 = 8444461749428370424248824938781546531375899335154063827935233455917409239041
P = R_377                                   # the Twisted-Edwards base field is BLS12-377's scalar field
Q = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
MODULI = {1: L_TE, 2: R_377}                # te::SCALAR_FORM_TE / SCALAR_FORM_377
RA, RA377 = 1 << 256, 1 << 384              # the caller's Montgomery radices
RE, RE377 = 1 << 261, 1 << 406              # the engine's
D_TE = 3021


@pytest.fixture(scope="module")
def sf(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("scalarform") / "libscalarform.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    L = ctypes.CDLL(so)
    L.sf_decode.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p]
    L.sf_decode.restype = None
    return L


def decode_all(sf, form, values):
    buf = b"".join(v.to_bytes(32, "little") for v in values)
    out = ctypes.create_string_buffer(len(buf))
    sf.sf_decode(form, buf, len(values), out)
    return [int.from_bytes(out.raw[32 * i:32 * i + 32], "little") for i in range(len(values))]


def edge_values(m):
    """the edge values of the issue: 0, 1, m - 1, m, m + 1, 2^256 mod m (decodes to 1), 2^256 - 1"""
    return [0, 1, m - 1, m, m + 1, RA % m, RA - 1]


def limb_patterns():
    single = [0xffffffff << (32 * j) for j in range(8)]
    all_but_one = [(RA - 1) ^ (0xffffffff << (32 * j)) for j in range(8)]
    return single + all_but_one


@pytest.mark.parametrize("form", (1, 2))
def test_decode_equals_a_times_inverse_radix(sf, form):
    m = MODULI[form]
    rinv = pow(RA, -1, m)
    rng = random.Random(0x5ca1a + form)
    values = edge_values(m) + limb_patterns() + [rng.getrandbits(256) for _ in range(10000)]
    got = decode_all(sf, form, values)
    for a, k in zip(values, got):
        assert k < m, hex(a)
        assert k == a * rinv % m, hex(a)
    assert got[5] == 1 and got[0] == 0 and got[3] == 0      # 2^256 mod m -> 1; 0 and m -> 0


def test_generated_scalar_constants(sf):
    for form, m in MODULI.items():
        w = (ctypes.c_uint32 * 8)()
        ninv = ctypes.c_uint32()
        sf.sf_modulus(form, w, ctypes.byref(ninv))
        assert sum(int(w[i]) << (32 * i) for i in range(8)) == m
        assert ninv.value == (-pow(m, -1, 1 << 32)) % (1 << 32)


def limbs_value(words):
    return sum(int(w) << (29 * i) for i, w in enumerate(words))


def test_generated_point_constants(sf):
    te_c = (ctypes.c_uint32 * 18)()
    q_c = (ctypes.c_uint32 * 42)()
    sf.sf_point_constants(te_c, q_c)
    half = RE * RE * pow(RA, -1, P) * pow(2, -1, P) % P
    assert limbs_value(te_c[0:9]) == half and limbs_value(te_c[9:18]) == 2 * half % P
    assert all(w < 1 << 29 for w in te_c) and all(w < 1 << 29 for w in q_c)          # class N: canonical residues, normalised limbs
    s = 10189023633222963290707194929886294091415157242906428298294512798502806398782149227503530278436336312243746741931
    f = 23560188534917577818843641916571445935985386319233886518929971599490231428764380923487987729215299304184915158756
    assert 3 * s * s % Q == 1
    k = RE377 * RE377 * pow(RA377, -1, Q) % Q
    assert limbs_value(q_c[0:14]) == s * k % Q and limbs_value(q_c[14:28]) == k and limbs_value(q_c[28:42]) == f * k % Q


def te_record(sf, mont, x, y):
    out = (ctypes.c_uint32 * 27)()
    sf.sf_from_affine(mont, x.to_bytes(32, "little") + y.to_bytes(32, "little"), out)
    return [limbs_value(out[9 * k:9 * k + 9]) % P for k in range(3)]


def test_te_conversion_from_montgomery_coordinates(sf):
    rng = random.Random(77)
    pts = [(0, 1), (1, 0), (P - 1, P - 1)] + [(rng.randrange(P), rng.randrange(P)) for _ in range(200)]
    inv2 = pow(2, -1, P)
    for x, y in pts:
        want = te_record(sf, 0, x, y)
        assert want == [(y - x) * inv2 * RE % P, (y + x) * inv2 * RE % P, -D_TE * x * y * RE % P]
        xa, ya = x * RA % P, y * RA % P
        assert te_record(sf, 1, xa, ya) == want
        # non-canonical encodings stand for their residue (any value below 2^256)
        for kx, ky in ((1, 0), (0, 1), (3, 5)):
            if xa + kx * P < RA and ya + ky * P < RA:
                assert te_record(sf, 1, xa + kx * P, ya + ky * P) == want
    assert te_record(sf, 1, RA - 1, RA - 1) == te_record(sf, 0, (RA - 1) * pow(RA, -1, P) % P, (RA - 1) * pow(RA, -1, P) % P)


def sw_record(sf, mont, x, y):
    out = (ctypes.c_uint32 * 56)()
    sf.sf_from_sw377(mont, x.to_bytes(48, "little") + y.to_bytes(48, "little"), out)
    return [limbs_value(out[14 * k:14 * k + 14]) % Q for k in range(4)]


def test_377_conversion_from_montgomery_coordinates(sf):
    from oracle import oracle377
    pts = oracle377.gen_points(5, 40)
    rng = random.Random(78)
    coords = [(int.from_bytes(pts[96 * i:96 * i + 48], "little"), int.from_bytes(pts[96 * i + 48:96 * i + 96], "little")) for i in range(40)]
    coords += [(rng.randrange(Q), rng.randrange(Q)) for _ in range(60)]        # (the conversion is arithmetic: any pair will do)
    for x, y in coords:
        want = sw_record(sf, 0, x, y)
        xa, ya = x * RA377 % Q, y * RA377 % Q
        assert sw_record(sf, 1, xa, ya) == want
        for kx, ky in ((1, 0), (0, 1), (7, 100)):
            if xa + kx * Q < RA377 and ya + ky * Q < RA377:
                assert sw_record(sf, 1, xa + kx * Q, ya + ky * Q) == want


def test_standalone_program_under_sanitizers(tmp_path):
    """the shim is a program of its own: built with AddressSanitizer + UBSan as an executable and run once in the environment as it is.
    The runtimes are linked statically, so the program neither needs anything preloaded nor minds what the environment preloads."""
    exe = str(tmp_path / "scalarform_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", "-o", exe, SRC])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    assert re.search(r"scalarform: \d+ cases, 0 bad", r.stdout.decode()), r.stdout.decode()


def test_header_documents_the_options_and_is_still_c(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    assert '"scalars_montgomery"' in hdr and '"points_montgomery"' in hdr
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "te_msm.h"\nint (*f1)(te_ctx*, const char*, int64_t) = te_msm_set_option;\nint main(void) { return f1 ? 0 : 1; }\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "use.o"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


def test_library_knows_the_options_and_holds_the_kernels(pkg):
    blob = open(pkg.library_path(), "rb").read()
    assert b"scalars_montgomery" in blob and b"points_montgomery" in blob
    # the Montgomery instantiations of the digit kernels (template arguments C, FORM) and of the bind conversions are in the code object
    for c in (4, 13, 16):
        for form in (1, 2):
            assert (b"k_digitsILi%dELi%dE" % (c, form)) in blob and (b"k_digits_raggedILi%dELi%dE" % (c, form)) in blob
    assert b"k_fb_digitsILi16ELi1E" in blob and b"k_fb_digitsILi21ELi1E" in blob
    assert b"k_prep_pointsILb1E" in blob and b"k_prep_points377ILb1E" in blob
    assert b"k_check_formILi0ELb1E" in blob and b"k_check_subgroupILi1ELb1E" in blob


def test_package_passes_the_options_through(pkg):
    assert "montgomery" in inspect.signature(pkg.MsmContext.bind_points).parameters
    assert inspect.signature(pkg.MsmContext.bind_points).parameters["montgomery"].default is False
    assert "montgomery" in inspect.signature(pkg.MsmContext.bind_points_device).parameters


def test_addon_has_the_montgomery_switches():
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    assert re.search(r"module\.exports\s*=\s*\{[^}]*\bsetScalarsMontgomery\b", open(os.path.join(js, "compute_msm.js")).read())
    dts = open(os.path.join(js, "submission.d.ts")).read()
    assert "setScalarsMontgomery" in dts and "montgomery" in dts
    addon = open(os.path.join(js, "addon.cc")).read()
    assert '"setScalarsMontgomery"' in addon and '"scalars_montgomery"' in addon and '"points_montgomery"' in addon
