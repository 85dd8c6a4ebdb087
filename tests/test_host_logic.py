"""CPU-side tests of the product's host logic and of the device arithmetic headers compiled for the
host (tests/csrc/fpcheck.cpp).  No GPU, no compute calls into libtemsm.so beyond the host tail."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

import devcheck
from oracle.gen_golden import edge_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 1 << 261            # device Montgomery radix: 9 limbs of 29 bits
NL, LB = 9, 29
LM = (1 << LB) - 1


def limbs(v):
    """integer -> 9 normalised 29-bit limbs (ctypes array)"""
    return (ctypes.c_uint32 * NL)(*[(v >> (LB * i)) & LM if i < NL - 1 else v >> (LB * i) for i in range(NL)])


def raw(ls):
    return (ctypes.c_uint32 * NL)(*ls)


def val(a):
    return sum(int(a[i]) << (LB * i) for i in range(NL))


def test_field_constants(fpcheck, model):
    out = (ctypes.c_uint32 * 81)()
    fpcheck.fpc_constants(out)
    got = [[int(out[9 * k + i]) for i in range(9)] for k in range(9)]
    P = model.P
    vals = [sum(l << (LB * i) for i, l in enumerate(g)) for g in got]
    assert vals[:6] == [R % P, R * R % P, model.D * R % P, 2 * model.D * R % P, 1, P]
    for g in got[:6]:
        assert all(l <= LM for l in g)
    out2 = (ctypes.c_uint32 * 27)()
    fpcheck.fpc_constants2(out2)
    got2 = [[int(out2[9 * k + i]) for i in range(9)] for k in range(3)]
    assert [sum(l << (LB * i) for i, l in enumerate(g)) for g in got2[:2]] == [R * R * pow(2, -1, P) % P, (-model.D * pow(R, 3, P)) % P]
    assert all(l <= LM for g in got2[:2] for l in g)
    for k, g in zip((2, 4, 8, 16), got[6:] + got2[2:]):   # offset forms: same value as K*p, every lower limb >= 2^29 - 1
        assert sum(l << (LB * i) for i, l in enumerate(g)) == k * P
        assert all(LM <= l < (1 << 30) for l in g[:8]) and g[8] > 0
    assert 16 * P > 1 << 256                              # y - x + 16p >= 0 for any 256-bit x


def test_small_constant_product(fpcheck, model):
    """fp_mul_k2d (csrc/fp.hpp): a * 2d as  6042 a - q p  with q estimated from a's top 32 bits -- the residue, the value bound
    (below 1.0001 p + nothing) and the limb class for random class-N operands below 2^254 and for the operands at which the
    estimate is tightest; the estimate's constant re-derived from p."""
    P, rnd = model.P, random.Random(21)
    K = 2 * model.D
    assert K == 6042
    fpcheck.fpc_k2d_q.restype = ctypes.c_uint32
    assert int(fpcheck.fpc_k2d_q()) == (K << 49) // ((P >> 222) + 1) < 1 << 32
    out = (ctypes.c_uint32 * NL)()

    def lim(v):                                            # class N: 8 limbs of 29 bits, the rest in the top limb
        return [(v >> (29 * i)) & LM for i in range(8)] + [v >> 232]

    def check(v):
        fpcheck.fpc_mul_k2d(raw(lim(v)), out)
        r = val(out)
        assert r % P == K * v % P
        assert 0 <= r < P + (P >> 13)                      # below 1.0002 p: offset subtractions with 2p are safe
        assert all(int(out[i]) <= LM for i in range(NL - 1)) and int(out[NL - 1]) < 1 << 22

    vals = devcheck.small_product_values(K, n_random=20000, n_product=5000)     # the device tests run a few hundred of the same set
    assert len(vals) > 25000 and {0, P, 2 * P, (1 << 254) - 1, (P + K - 1) // K} <= set(vals)
    for v in vals:
        check(v)


def test_mont_mul_values_and_limb_classes(fpcheck, model):
    """exactness for normalised operands and for the widest limb classes the formulas use (S x D)"""
    P, rnd = model.P, random.Random(11)
    rinv = pow(R, -1, P)
    out = (ctypes.c_uint32 * NL)()

    def check(la, lb):
        fpcheck.fpc_mont_mul(raw(la), raw(lb), out)
        a, b, r = val(la), val(lb), val(out)
        assert r % P == a * b * rinv % P
        assert r < a * b // R + P + 1                       # value bound every caller relies on
        assert all(int(out[i]) <= LM for i in range(NL - 1))  # class N

    # limb-magnitude edge: D-class limbs (2^29 - 1 + largest offset limb) against S-class limbs (2 * (2^29 - 1))
    offs = (ctypes.c_uint32 * 81)()
    fpcheck.fpc_constants(offs)
    assert [int(offs[9 * 6 + i]) for i in range(9)] == devcheck.FIELDS[9].offset(2)
    max_off = max(int(offs[9 * 6 + i]) for i in range(8))
    d_max, s_max = LM + max_off, 2 * LM
    assert 9 * d_max * s_max + 8 * (1 << 58) + (1 << 36) < (1 << 64)      # the accumulator bound stated in fp.hpp
    # random values below 8p / 16p; D x S and S x S at their maximum and at random; the carry-folded quotient (fp.hpp): columns whose
    # value is 0 or -1 modulo 2^29, zero operands, sparse operands; a_0 * b_0 = 0 (mod 2^29), where column 0 takes q_0 = 2^29
    pairs = devcheck.mont_mul_pairs(9, n_random=2000, n_wide=500, n_col0=300)
    assert ([d_max] * 8 + [1 << 22], [s_max] * 8 + [1 << 22]) in pairs and ([0] * 9, list(limbs(P))) in pairs and len(pairs) == 2000 + 3 + 500 + 90 + 300
    for la, lb in pairs:
        check(la, lb)


def test_field_helpers(fpcheck, model):
    P, rnd = model.P, random.Random(12)
    out = (ctypes.c_uint32 * NL)()
    for ls, x, y, w in devcheck.helper_operands(9, 500):
        fpcheck.fpc_norm(raw(ls), out)
        assert val(out) == val(ls) and all(int(out[i]) <= LM for i in range(8))
        fpcheck.fpc_sub2(limbs(x), limbs(y), out)
        assert val(out) == x - y + 2 * P
        fpcheck.fpc_from_words32((ctypes.c_uint32 * 8)(*[(w >> (32 * i)) & 0xFFFFFFFF for i in range(8)]), out)
        assert val(out) == w and all(int(out[i]) <= LM for i in range(NL))


def _ete_affine(model, b):
    P = model.P
    rinv = pow(R, -1, P)
    coords = []
    for c in range(4):
        ws = [int.from_bytes(b[36 * c + 4 * i:36 * c + 4 * i + 4], "little") for i in range(NL)]
        coords.append(sum(w << (LB * i) for i, w in enumerate(ws)) * rinv % P)
    x, y, z, t = coords
    zi = pow(z, -1, P)
    assert t * z % P == x * y % P           # T = XY/Z stays consistent
    return (x * zi % P, y * zi % P)


def test_point_formulas(fpcheck, model, ora):
    pts = [model.xy_from_bytes(ora.gen_points(21, 12)[64 * i:64 * i + 64]) for i in range(12)]
    ident = ctypes.create_string_buffer(144)
    fpcheck.fpc_identity(ident)
    acc, exp = ident.raw, model.ZERO
    recs = []
    for p in pts:
        rec = ctypes.create_string_buffer(128)
        fpcheck.fpc_prep_point(model.points_to_bytes([p]), rec)
        recs.append(rec.raw)
    for i, p in enumerate(pts + pts[:3]):             # the last three re-add points: P + P through the unified law
        neg = i % 3 == 1
        out = ctypes.create_string_buffer(144)
        fpcheck.fpc_madd(acc, recs[i % 12], int(neg), out)
        acc = out.raw
        exp = model.add(exp, model.neg(p) if neg else p)
        assert _ete_affine(model, acc) == exp
    out = ctypes.create_string_buffer(144)
    fpcheck.fpc_add(acc, acc, out)                    # doubling through ete_add
    assert _ete_affine(model, out.raw) == model.add(exp, exp)
    fpcheck.fpc_add(out.raw, ident.raw, out)
    assert _ete_affine(model, out.raw) == model.add(exp, exp)
    assert fpcheck.fpc_bound_violations() == 0


@pytest.mark.parametrize("n,c,mode", [(1, 4, "chain"), (2, 16, "chain"), (33, 5, "chain"), (64, 16, "edge"),
                                       (300, 8, "chain"), (1000, 13, "chain"), (257, 16, "fixed"), (100, 7, "edge"),
                                       (500, 12, "fixed"), (4096, 11, "chain")])
def test_emulated_stages_plus_host_tail(fpcheck, pkg, model, ora, n, c, mode):
    """device-stage emulation (same limb code as the kernels) -> partial rows -> the product's host tail
    == oracle.  Covers the row format, the row/column weighting and Horner's split."""
    seed = 1000 + n + c
    pts = ora.gen_points_fixed(n) if mode == "fixed" else ora.gen_points(seed, n)
    sc = model.scalars_to_bytes(edge_scalars(seed, n)) if mode == "edge" else ora.gen_scalars(seed, n)
    W = (256 + c - 1) // c
    buf = ctypes.create_string_buffer(W * 720)
    assert fpcheck.fpc_partial_rows(pts, sc, n, c, 0, 1, buf) == 0
    assert pkg.finalize_host(buf.raw, c, W) == ora.msm(pts, sc, threads=4)
    assert fpcheck.fpc_bound_violations() == 0


def test_host_tail_forms_agree(fpcheck, pkg, model, ora, tmp_path):
    """The host tail has two accumulators -- scalar (mulx / adcx products) and AVX-512 IFMA (the point's coordinates in vector
    lanes) -- chosen by the CPU.  Whatever this machine chooses is what the tests above ran; here the OTHER choices run in fresh
    processes (the choice is made once per process) on rows with edge scalars and must return the same 64 bytes as the oracle."""
    import subprocess, sys
    n, c = 300, 16
    pts, sc = ora.gen_points(77, n), model.scalars_to_bytes(edge_scalars(77, n))
    W = (256 + c - 1) // c
    buf = ctypes.create_string_buffer(W * 720)
    assert fpcheck.fpc_partial_rows(pts, sc, n, c, 0, 1, buf) == 0
    exp = ora.msm(pts, sc, threads=4)
    assert pkg.finalize_host(buf.raw, c, W) == exp
    rows = tmp_path / "rows.bin"
    rows.write_bytes(buf.raw)
    prog = ("import importlib, sys; sys.path.insert(0, %r); p = importlib.import_module('webgpu-msm-twisted-edwards_amd'); "
            "print(p.host_tail_features(), p.finalize_host(open(%r, 'rb').read(), %d, %d).hex())" % (ROOT, str(rows), c, W))
    seen = {pkg.host_tail_features()}
    for env in ({"TE_MSM_HOST_TAIL": "scalar"}, {"TE_MSM_HOST_MUL": "c", "TE_MSM_HOST_TAIL": "scalar"}, {"TE_MSM_HOST_MUL": "c"}, {}):
        r = subprocess.run([sys.executable, "-c", prog], env={**os.environ, **env}, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()[-400:]
        feat, hexout = r.stdout.decode().split()
        assert bytes.fromhex(hexout) == exp, (env, feat)
        seen.add(int(feat))
    assert 0 in seen                                  # the portable form ran


def test_window_shards_merge(fpcheck, pkg, ora):
    n, c = 200, 9
    pts, sc = ora.gen_points(9, n), ora.gen_scalars(9, n)
    W = (256 + c - 1) // c
    exp = ora.msm(pts, sc)
    for world in (1, 2, 3, 8, 40):                    # 40 > W: some ranks own no window
        bufs = []
        for r in range(world):
            first, step = pkg.window_shard_for_rank(r, world)
            b = ctypes.create_string_buffer(W * 720)
            assert fpcheck.fpc_partial_rows(pts, sc, n, c, first, step, b) == 0
            bufs.append(b.raw)
        assert pkg.finalize_host(pkg.merge_partials(bufs, W, world), c, W) == exp
        flat = ctypes.create_string_buffer(b"".join(bufs), world * W * 720)        # what an all-gather leaves in host memory
        assert pkg.finalize_gathered(ctypes.addressof(flat), world, c, W) == exp


def test_point_shards_merge(fpcheck, pkg, ora):
    """Point sharding (te_msm_run on a multi-device context; SURVEY 8e "point sharding"): every slice of the points runs
    ALL windows, the host tail folds the SUM of the slices' rows -- te_msm_finalize_sum_curve, the code the multi-device
    te_msm_run ends in.  Slices of unequal size, an empty slice (all-zero rows), one slice."""
    n, c = 230, 9
    pts, sc = ora.gen_points(19, n), ora.gen_scalars(19, n)
    W = (256 + c - 1) // c
    exp = ora.msm(pts, sc)
    for cuts in ([0, n], [0, 100, n], [0, 1, 2, 50, 50, n], [0] + [29 * k for k in range(1, 8)] + [n]):
        sets = []
        for lo, hi in zip(cuts, cuts[1:]):
            b = ctypes.create_string_buffer(W * 720)                   # an empty slice leaves its rows all zero
            if hi > lo:
                assert fpcheck.fpc_partial_rows(pts[64 * lo:64 * hi], sc[32 * lo:32 * hi], hi - lo, c, 0, 1, b) == 0
            sets.append(b.raw)
        assert pkg.finalize_sum(sets, c, W) == exp, cuts
    with pytest.raises(pkg.MsmError):
        pkg.finalize_sum([], c, W)


def test_synth_random_points_match_the_oracle(pkg, model, ora):
    """SURVEY 8d set (R): the engine's harness generator (fixed-base table, threads) and the oracle's independent restatement
    (plain double-and-add) produce the same n independent points a_i * G; the pure-Python model agrees on the first few; the
    output does not depend on the thread split (n above and below the threading threshold); scalars are unchanged"""
    for n in (1, 7, 5000):
        p, s = pkg.synth_inputs(0xABCDE, n, "random")
        assert p == ora.gen_points_random(0xABCDE, n) and s == ora.gen_scalars(0xABCDE, n)
    p5000 = pkg.synth_inputs(0xABCDE, 5000, "random", scalars=False)[0]
    assert pkg.synth_inputs(0xABCDE, 7, "random", scalars=False)[0] == p5000[:7 * 64]
    assert model.points_to_bytes(model.gen_points_random(0xABCDE, 3)) == p5000[:3 * 64]
    assert len({p5000[64 * i:64 * i + 64] for i in range(5000)}) == 5000
    assert all(ora.on_curve(p5000[64 * i:64 * i + 64]) for i in range(0, 5000, 97))
    assert pkg.synth_inputs(3, 10, "chain")[0] == ora.gen_points(3, 10) and pkg.synth_inputs(3, 10, True)[0] == ora.gen_points_fixed(10)
    with pytest.raises(pkg.MsmError):
        pkg.synth_inputs(3, 10, 7)


def test_csv_export_format(pkg):
    """ui/CSVExportButton.tsx:9-11: every cell quoted, ',' between cells, newline between rows; header of ui/AllBenchmarks.tsx:45"""
    import importlib
    fb = importlib.import_module(pkg.__name__ + ".full_benchmarks")
    res = {17: {"first_run_elapsed": 3.5, "subsequent_runs": [1.25, 1.5]}, 16: {"first_run_elapsed": 9.0, "subsequent_runs": [0.5]}}
    assert fb.to_csv(fb.csv_rows(res)) == ('"InputSize","MSM Func","Time (MS)"\n"16","Submission","9.0"\n"16","Submission","0.5"\n'
                                           '"17","Submission","3.5"\n"17","Submission","1.25"\n"17","Submission","1.5"')


def test_devices_from_env(pkg, monkeypatch):
    monkeypatch.delenv("TE_MSM_DEVICES", raising=False)
    assert pkg.devices_from_env() == (0,)
    monkeypatch.setenv("TE_MSM_DEVICES", "0,2, 3")
    assert pkg.devices_from_env() == (0, 2, 3)
    monkeypatch.setenv("TE_MSM_DEVICES", "1")
    assert pkg.devices_from_env() == (1,)


def test_final_carry_detected_by_emulation(fpcheck, model, ora):
    pts = ora.gen_points(1, 2)
    sc = model.scalars_to_bytes([5, (1 << 256) - 1])
    buf = ctypes.create_string_buffer(16 * 720)
    assert fpcheck.fpc_partial_rows(pts, sc, 2, 16, 0, 1, buf) == -3


def test_host_tail_identity_and_args(pkg):
    ident = bytes(32) + (1).to_bytes(32, "little")
    assert pkg.finalize_host(bytes(16 * 720), 16, 16) == ident
    with pytest.raises(pkg.MsmError):
        pkg.finalize_host(bytes(720), 99, 1)


# ---------------------------------------------------------------- C-ABI surface
def test_synthetic_inputs_equal_the_oracle_generator(pkg, ora):
    """te_msm_synth_inputs (product side, used by bench.py and full_benchmarks.py) == the oracle's generator, so golden
    fixtures, tests and the bench all speak about the same inputs"""
    for seed, n in ((1, 1), (7, 2), (3, 1000), (0x5EED0014, 4097)):
        pts, sc = pkg.synth_inputs(seed, n)
        assert pts == ora.gen_points(seed, n) and sc == ora.gen_scalars(seed, n)
    assert pkg.synth_inputs(9, 3, fixed_point=True)[0] == ora.gen_points_fixed(3)
    assert pkg.synth_inputs(9, 0) == (b"", b"")
    assert pkg.synth_inputs(9, 4, points=False)[0] is None
    from oracle import oracle377
    for seed, n in ((1, 1), (7, 2), (3, 300)):
        pts, sc = pkg.synth_inputs(seed, n, curve=pkg.CURVE_BLS12_377_G1)
        assert pts == oracle377.gen_points(seed, n) and sc == oracle377.gen_scalars(seed, n)


def _declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(te_msm_\w+)\s*\(", hdr)))


def test_abi_exports_every_declared_symbol(pkg):
    L = ctypes.CDLL(pkg.library_path())
    syms = _declared_symbols()
    assert len(syms) >= 14
    for s in syms:
        assert hasattr(L, s), f"{s} declared in include/te_msm.h but not exported"
    # ... and nothing else: the functions the library defines for the dynamic linker are exactly the declared ones, beside the kernels'
    # launch stubs (te::__device_stub__*).  An engine internal exported under a plain name (tmp_alloc, pick_device, owner_of ...) could
    # be pre-empted by any other object of the host process that defines the name.
    import shutil
    nm = shutil.which("nm") or shutil.which("llvm-nm") or shutil.which("llvm-nm", path="/opt/rocm/llvm/bin")
    if not nm:
        pytest.skip("nm is not installed")
    out = subprocess.run([nm, "-D", "--defined-only", pkg.library_path()], stdout=subprocess.PIPE, check=True, universal_newlines=True).stdout
    text = [l.split()[-1] for l in out.splitlines() if len(l.split()) >= 3 and l.split()[-2] == "T"]
    exported = sorted(s for s in text if "__device_stub__" not in s)
    assert exported == syms, {"exported, not declared": sorted(set(exported) - set(syms)), "declared, not exported": sorted(set(syms) - set(exported))}


def test_library_has_gfx950_code_object(pkg):
    data = open(pkg.library_path(), "rb").read()
    assert b"gfx950" in data and b"k_accumulate" in data


def test_no_cpu_fallback_without_device(pkg):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the loud-failure path is not reachable")
    with pytest.raises(pkg.MsmError) as e:
        pkg.MsmContext((0,))
    assert "no CPU fallback" in str(e.value)
    with pytest.raises(pkg.MsmError):
        pkg.compute_msm(bytes(64), bytes(32), log_result=False)


def test_product_does_not_touch_the_oracle():
    """The oracle is test infrastructure: nothing under the package or include/ may reference it."""
    bad = []
    for base in ("webgpu-msm-twisted-edwards_amd", "include"):
        for dp, _, files in os.walk(os.path.join(ROOT, base)):
            for f in files:
                if f.endswith((".py", ".hpp", ".hip", ".h", ".inc", ".js", ".cc", ".cpp", "Makefile")):
                    txt = open(os.path.join(dp, f), errors="ignore").read()
                    if re.search(r"te_oracle|oracle/|from oracle|import oracle|ora_msm", txt):
                        bad.append(os.path.join(dp, f))
    assert not bad, bad


def test_zprize_expected_results_are_the_reference_constants(pkg, kats):
    import importlib
    td = importlib.import_module("webgpu-msm-twisted-edwards_amd.testdata")
    assert {str(k): {"x": str(v["x"]), "y": str(v["y"])} for k, v in td.EXPECTED.items()} == kats["zprize_expected"]
    assert td.expected_result(16)["x"] == int(kats["zprize_expected"]["16"]["x"]) and td.expected_result(15) is None


def test_zprize_ingestion_format(pkg, model, tmp_path):
    import importlib
    td = importlib.import_module("webgpu-msm-twisted-edwards_amd.testdata")
    pts = [(model.GX, model.GY), (model.HX, model.HY)]
    ptxt = "\n".join('{"x": "%d", "y": "%d", "t": "%d", "z": "1"}' % (x, y, x * y % model.P) for x, y in pts) + "\n"
    stxt = "5\n%d\n" % (model.P - 1)
    (tmp_path / "p.txt").write_text(ptxt)
    (tmp_path / "s.txt").write_text(stxt)
    bp, bs = td.load_test_case(str(tmp_path / "p.txt"), str(tmp_path / "s.txt"))
    assert bp == model.points_to_bytes(pts) and bs == model.scalars_to_bytes([5, model.P - 1])


# ---------------------------------------------------------------- N > 1 path on CPU (gloo, world_size 2)
_WORKER = r"""
import ctypes, importlib, os, sys
sys.path.insert(0, {root!r})
import torch, torch.distributed as dist
from oracle import oracle as o
pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:{port}", rank=int(sys.argv[1]), world_size=2)
rank, world = dist.get_rank(), dist.get_world_size()
L = ctypes.CDLL(os.path.join({root!r}, "tests", "csrc", "libfpcheck.so"))
L.fpc_partial_rows.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_char_p]
n, c = 300, 10
W = (256 + c - 1) // c
pts, sc = o.gen_points(77, n), o.gen_scalars(77, n)
first, step = pkg.window_shard_for_rank(rank, world)
buf = ctypes.create_string_buffer(W * 720)
assert L.fpc_partial_rows(pts, sc, n, c, first, step, buf) == 0       # stands in for the GPU stage
t = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8)
merged = pkg.exchange_partials(t, W, dist)
res = pkg.finalize_host(merged, c, W)
assert res == o.msm(pts, sc), "rank %d mismatch" % rank
# a launch sequence carrying three MSMs (te_msm_partial_device_batch): rows [MSM][W] per rank, ONE all-gather, the gathered
# finalize per MSM -- what ShardedPipeline.collect_batch does with the GPU's rows
batch, blk = 3, W * 720
ins = [(o.gen_points(80 + m, n), o.gen_scalars(90 + m, n)) for m in range(batch)]
mine = bytearray()
for p_, s_ in ins:
    assert L.fpc_partial_rows(p_, s_, n, c, first, step, buf) == 0
    mine += buf.raw
gathered = torch.empty(world * batch * blk, dtype=torch.uint8)
dist.all_gather_into_tensor(gathered, torch.frombuffer(mine, dtype=torch.uint8))
for m, (p_, s_) in enumerate(ins):
    rows = pkg.rows_of_batched_msm(gathered, world, batch, m)
    assert pkg.finalize_gathered(rows.data_ptr(), world, c, W) == o.msm(p_, s_), "rank %d, MSM %d of the batch" % (rank, m)
# inputs for the window-sharded form arrive once (SURVEY 8e "Inputs"): every rank contributes its slice of the host buffers,
# one all-gather per buffer assembles the whole on every rank -- ragged n (the last slice is padded), and the MSM over the
# assembled buffers is the oracle's
for n2 in (301, 2, 1):
    p2, s2 = o.gen_points(91, n2), o.gen_scalars(92, n2)
    dp, ds, got_n = pkg.distribute_inputs(p2, s2, dist, device="cpu")
    assert got_n == n2 and dp.numpy().tobytes() == p2 and ds.numpy().tobytes() == s2, "rank %d: assembled inputs differ (n = %d)" % (rank, n2)
    assert L.fpc_partial_rows(dp.numpy().tobytes(), ds.numpy().tobytes(), n2, c, first, step, buf) == 0
    t2 = torch.frombuffer(bytearray(buf.raw), dtype=torch.uint8)
    assert pkg.finalize_host(pkg.exchange_partials(t2, W, dist), c, W) == o.msm(p2, s2), "rank %d: MSM over distributed inputs" % rank
# the ranks must agree on n: a rank that brings another size gets a real exception -- on EVERY rank, before the all-gathers whose
# buffer sizes depend on it (round-5 advisor: an assert behind the collective, stripped under -O)
n3 = 40 + rank
try:
    pkg.distribute_inputs(o.gen_points(93, n3), o.gen_scalars(94, n3), dist, device="cpu")
    raise SystemExit("rank %d: mismatching n was accepted" % rank)
except ValueError as e:
    assert "disagree on n" in str(e), e
try:
    pkg.distribute_inputs(bytes(64 * 3 + 1), bytes(32 * 3), dist, device="cpu")
    raise SystemExit("a ragged point buffer was accepted")
except ValueError:
    pass
dist.barrier(); dist.destroy_process_group()
print("rank", rank, "ok")
"""


def test_gloo_two_rank_window_sharding(fpcheck, pkg, tmp_path):
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(_WORKER.format(root=ROOT, port=port))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


# ---------------------------------------------------------------- N-API addon (the reference's host language)
def _node():
    import shutil
    return shutil.which("node")


def test_napi_addon_loads_and_fails_loudly_without_gpu(pkg, tmp_path):
    import json
    import torch
    if not _node():
        pytest.skip("node is not installed")
    js = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js")
    if not os.path.exists(os.path.join(js, "te_msm_napi.node")):
        subprocess.check_call(["make", "-C", js, "-s"])
    (tmp_path / "p.bin").write_bytes(bytes(64))
    (tmp_path / "s.bin").write_bytes(bytes(32))
    r = subprocess.run([_node(), os.path.join(js, "run_msm.js"), str(tmp_path / "p.bin"), str(tmp_path / "s.bin")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    if torch.cuda.is_available():
        assert "x" in out
    else:
        assert "no CPU fallback" in out["error"]          # promise rejected, as the reference throws (gpu.ts:19-22)
    # argument validation rejects synchronously-thrown errors too
    bad = subprocess.run([_node(), "-e", "require(%r).compute_msm(Buffer.alloc(10), Buffer.alloc(32), false).catch(e => { console.log('rejected:' + e.message); })"
                          % os.path.join(js, "compute_msm.js")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert b"rejected:" in bad.stdout
    # the device list: TE_MSM_DEVICES and setDevices (no context is created until the first MSM)
    q = subprocess.run([_node(), "-e", "const m = require(%r); const a = m.getDevices(); m.setDevices([0, 1, 1]); const b = m.getDevices(); m.setDevices([]);"
                        "console.log(JSON.stringify([a, b, m.getDevices()]));" % os.path.join(js, "compute_msm.js")],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=dict(os.environ, TE_MSM_DEVICES="2,3"))
    assert json.loads(q.stdout.decode().strip().splitlines()[-1]) == [[2, 3], [0, 1, 1], [2, 3]], (q.stdout, q.stderr)
