"""MSMs over an indexed subset of a bound point set (te_msm_run_scalars_indexed*), without a GPU: the new names are in the C header, the
cross-compiled library, the package and the addon; the header still compiles as C; and the HIP-free plan header (csrc/indexed_plan.hpp,
compiled for the host by tests/csrc/indexedplan.cpp) keeps its rules -- packed entries exactly when the SET's count is at most 2^23,
everything else planned for m, pieces and device slices that tile [0, m)."""
import ctypes
import os
import random
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCS = ("te_msm_run_scalars_indexed", "te_msm_run_scalars_indexed_device", "te_msm_submit_scalars_indexed", "te_msm_submit_scalars_indexed_device")
u64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def ip(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("indexedplan") / "libindexedplan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", so, os.path.join(ROOT, "tests", "csrc", "indexedplan.cpp")])
    L = ctypes.CDLL(so)
    L.ip_plan.argtypes = [u64, u64, ctypes.c_int, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_uint32)]
    L.ip_plan.restype = None
    L.ip_pieces.argtypes = [u64, ctypes.c_int]
    L.ip_pieces.restype = ctypes.c_int
    L.ip_piece_lo.argtypes = [u64, ctypes.c_int, ctypes.c_int]
    L.ip_piece_lo.restype = u64
    for name, n in (("ip_devices_for", 3), ("ip_slice_lo", 3), ("ip_slice_max", 2), ("ip_packed_limit", 0)):
        getattr(L, name).argtypes = [u64] * n
        getattr(L, name).restype = u64
    return L


def plan(ip, m, count, opt_packed=1):
    n, pk = u64(), ctypes.c_uint32()
    ip.ip_plan(m, count, opt_packed, ctypes.byref(n), ctypes.byref(pk))
    return n.value, pk.value


M_VALUES = (0, 1, 2, 3, 255, 4097, 1 << 16, (1 << 20) + 5, 1 << 23, (1 << 23) + 1, 3 << 23, (1 << 31) - 1)


def test_packed_follows_the_sets_count_not_m(ip):
    lim = ip.ip_packed_limit()
    assert lim == 1 << 23
    for count in (1, 5, 1 << 14, 1 << 20, lim - 1, lim, lim + 1, lim + 4099, 1 << 24, (1 << 31) - 1):
        for m in M_VALUES:          # m below, at and above the count (m > count: repeats)
            _, pk = plan(ip, m, count)
            assert pk == (1 if count <= lim else 0), (m, count)
            assert plan(ip, m, count, opt_packed=0)[1] == 0, "option packed_sort = 0 always gives the general form"


def test_the_plan_follows_m(ip):
    for count in (1, 1 << 20, (1 << 23) + 4099):
        for m in M_VALUES:
            assert plan(ip, m, count)[0] == m, "window bits, segment length and buffers are sized from the entries"


def test_pieces_tile_the_pairs(ip):
    r = random.Random(5)
    ms = list(M_VALUES[1:]) + [r.randint(1, 1 << 22) for _ in range(200)]
    for m in ms:
        for opt in (0, 1, 2, 3, 7, 64):
            K = ip.ip_pieces(m, opt)
            assert 1 <= K <= m
            if opt:
                assert K == min(opt, m)
            else:
                assert K == (3 if m >= 3 << 18 else 2 if m >= 1 << 18 else 1), "the thresholds of te_msm_run_scalars, from m"
            lo = [ip.ip_piece_lo(m, K, i) for i in range(K + 2)]
            assert lo[0] == 0 and lo[K] == m and lo[K + 1] == m
            sizes = [lo[i + 1] - lo[i] for i in range(K)]
            assert sum(sizes) == m and min(sizes) >= 1 and max(sizes) - min(sizes) <= 1


def test_piece_boundaries_equal_the_retired_floating_rule_up_to_nine_pieces(ip):
    """Host-point MSMs used to cut their pieces at (uint64_t)((double)n * ((double)i / K)); now every host-buffer form cuts at piece_lo.
    Python's int(float(n) * (i / K)) is that rule in the same double arithmetic.  Up to nine pieces -- the engine picks 1 to 3 -- the two
    agree; from ten pieces on (option "host_chunks" only) they may differ by one point, and the old rule could leave a piece empty."""
    r = random.Random(0x9137)
    for K in range(1, 10):
        ns = set(range(K, 4097))
        for e in range(12, 31):
            ns.update(((1 << e) - 1, 1 << e, (1 << e) + 1))
        for base in (1 << 17, 3 << 18, (1 << 31) - 1):
            ns.update((base - 1, base, base + 1))
        ns.update(K * r.randrange(1, ((1 << 31) - 1) // K + 1) for _ in range(2000))
        for n in ns:
            for i in range(K + 1):
                assert ip.ip_piece_lo(n, K, i) == int(float(n) * (i / K)), (n, K, i)
    # the two known differences beyond nine pieces (host-buffer pieces)
    assert int(float(90) * (7 / 10)) == 62 and ip.ip_piece_lo(90, 10, 7) == 63
    assert int(float(22) * (15 / 22)) == 14 and ip.ip_piece_lo(22, 22, 15) == 15
    assert int(float(22) * (14 / 22)) == 14, "the retired rule's empty piece"


def test_device_slices_tile_the_pairs(ip):
    r = random.Random(6)
    ms = list(M_VALUES[1:]) + [r.randint(1, 1 << 18) for _ in range(300)]
    for m in ms:
        for n_dev in (1, 2, 3, 4, 8):
            for shard_min in (1, 7, 4096, 1 << 16):
                D = ip.ip_devices_for(m, n_dev, shard_min)
                assert 1 <= D <= n_dev
                assert D == max(1, min(n_dev, m // shard_min))
                lo = [ip.ip_slice_lo(m, D, i) for i in range(D + 2)]
                assert lo[0] == 0 and lo[D] == m and lo[D + 1] == m
                sizes = [lo[i + 1] - lo[i] for i in range(D)]
                assert sum(sizes) == m and min(sizes) >= 1, "no empty device slice"
                assert max(sizes) - min(sizes) <= 1 and max(sizes) == ip.ip_slice_max(m, D)
                if D > 1:
                    assert min(sizes) >= shard_min, "no device works on fewer pairs than host_shard_min"
                else:
                    assert m < 2 * shard_min or n_dev == 1


def test_empty_call(ip):
    assert plan(ip, 0, 1 << 20) == (0, 1) and plan(ip, 0, (1 << 23) + 1) == (0, 0)
    assert ip.ip_pieces(0, 0) == 1 and ip.ip_pieces(0, 3) == 1
    assert ip.ip_piece_lo(0, 1, 0) == 0 and ip.ip_piece_lo(0, 1, 1) == 0
    for n_dev in (1, 4):
        assert ip.ip_devices_for(0, n_dev, 4096) == 1
        assert ip.ip_slice_lo(0, 1, 0) == 0 and ip.ip_slice_lo(0, 1, 1) == 0 and ip.ip_slice_max(0, 1) == 0


def test_header_declares_the_indexed_entry_points_and_is_still_c(tmp_path):
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name in NEW_FUNCS:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
    assert '"bad_index_position"' in hdr
    if not shutil.which("gcc"):
        pytest.skip("no gcc")
    src = tmp_path / "use.c"
    src.write_text('#include "te_msm.h"\n#include <stddef.h>\n'
                   "int (*f1)(te_ctx*, te_bases*, const uint32_t*, const uint8_t*, uint64_t, uint8_t*) = te_msm_run_scalars_indexed;\n"
                   "int (*f2)(te_ctx*, te_bases*, const void*, const void*, uint64_t, uint8_t*) = te_msm_run_scalars_indexed_device;\n"
                   "int (*f3)(te_ctx*, te_bases*, const uint32_t*, const uint8_t*, uint64_t, uint64_t*) = te_msm_submit_scalars_indexed;\n"
                   "int (*f4)(te_ctx*, te_bases*, const void*, const void*, uint64_t, uint64_t*) = te_msm_submit_scalars_indexed_device;\n"
                   "int main(void) { return f1 && f2 && f3 && f4 ? 0 : 1; }\n")
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "use.o"), str(src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()


def test_library_exports_the_indexed_entry_points(pkg):
    r = subprocess.run(["nm", "-D", "--defined-only", pkg.library_path()], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0, r.stdout.decode()
    syms = set(re.findall(r"\bT\s+(\w+)", r.stdout.decode()))
    for name in NEW_FUNCS:
        assert name in syms, name


def test_binding_has_the_indexed_methods_and_argtypes(pkg):
    for meth in ("run_scalars_indexed", "run_scalars_indexed_device", "submit_scalars_indexed", "submit_scalars_indexed_device"):
        assert callable(getattr(pkg.MsmContext, meth, None)), meth
    src = open(os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "binding.py")).read()
    for name in NEW_FUNCS:
        assert "L.%s.argtypes" % name in src and "L.%s.restype" % name in src, name
    binding = __import__("importlib").import_module("webgpu-msm-twisted-edwards_amd.binding")
    L = binding._lib()                                  # loading the library needs no device
    vp, cp, u = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64
    assert L.te_msm_run_scalars_indexed.argtypes == [vp, vp, vp, cp, u, cp]
    assert L.te_msm_run_scalars_indexed_device.argtypes == [vp, vp, vp, vp, u, cp]
    assert L.te_msm_submit_scalars_indexed.argtypes == [vp, vp, vp, cp, u, ctypes.POINTER(u)]
    assert L.te_msm_submit_scalars_indexed_device.argtypes == [vp, vp, vp, vp, u, ctypes.POINTER(u)]
    assert "index" in binding.MsmError(-1, "x", 7).__dict__ and binding.MsmError(-1, "x", 7).index == 7


def test_addon_exports_msm_indexed():
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    assert re.search(r"module\.exports\s*=\s*\{[^}]*\bmsmIndexed\b", open(os.path.join(js, "compute_msm.js")).read())
    assert "export declare const msmIndexed: (indices: Uint32Array, scalars: Buffer) => Promise<{ x: bigint; y: bigint }>;" in open(os.path.join(js, "submission.d.ts")).read()
    addon = open(os.path.join(js, "addon.cc")).read()
    assert '{"msmIndexed", MsmIndexed}' in addon and "te_msm_run_scalars_indexed(" in addon
