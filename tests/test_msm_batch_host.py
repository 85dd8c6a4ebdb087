"""Batched MSMs over prefixes of a bound point set (te_msm_run_scalars_batch*): the planner (csrc/batch_plan.hpp, compiled for the host by
tests/csrc/batchplan.cpp) places every MSM exactly once, keeps the length-class bound, the per-sequence cap and the byte budget, splits
by device within one MSM's length and is deterministic; and the new names are in the C header and the package."""
import ctypes
import os
import random
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
u32p, u64p, i32p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int32)

# the harness's cost model: W windows, bytes per digit cell, fixed bytes per MSM
W, CELL, FIXED = 20, 10, 4 << 20


@pytest.fixture(scope="module")
def bp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("batchplan") / "libbatchplan.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-o", so, os.path.join(ROOT, "tests", "csrc", "batchplan.cpp")])
    L = ctypes.CDLL(so)
    L.bp_plan.argtypes = [u64p, ctypes.c_uint32, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64,
                          ctypes.c_uint64, ctypes.c_int, u32p, i32p, u64p, i32p, u64p, u32p, u32p, u32p, u64p]
    L.bp_plan.restype = ctypes.c_int
    L.bp_length_class.argtypes = [ctypes.c_uint64]
    return L


def plan(bp, lens, n_dev=1, small_max=1 << 15, cap=64, budget=1 << 30):
    count = len(lens)
    mx = count + 64
    lv = (ctypes.c_uint64 * max(1, count))(*lens)
    size, dev, nmax, shared, mb = (ctypes.c_uint32 * mx)(), (ctypes.c_int32 * mx)(), (ctypes.c_uint64 * mx)(), (ctypes.c_int32 * mx)(), (ctypes.c_uint64 * mx)()
    members, empty, ne, load = (ctypes.c_uint32 * max(1, count))(), (ctypes.c_uint32 * max(1, count))(), ctypes.c_uint32(), (ctypes.c_uint64 * max(1, n_dev))()
    k = bp.bp_plan(lv, count, n_dev, small_max, cap, budget, W, CELL, FIXED, mx, size, dev, nmax, shared, mb, members, empty, ctypes.byref(ne), load)
    assert k >= 0
    seqs, at = [], 0
    for s in range(k):
        seqs.append({"msms": list(members[at:at + size[s]]), "dev": dev[s], "nmax": nmax[s], "shared": bool(shared[s]), "msm_bytes": mb[s]})
        at += size[s]
    return seqs, list(empty[:ne.value]), list(load[:n_dev])


def random_lens(seed, count, top=1 << 20):
    r = random.Random(seed)
    out = []
    for _ in range(count):
        e = r.random()
        out.append(0 if e < 0.03 else r.randint(1, 1 << r.randint(0, 15)) if e < 0.85 else r.randint((1 << 15) + 1, top))
    return out


def check_plan(lens, seqs, empty, n_dev, small_max=1 << 15, cap=64, budget=1 << 30):
    placed = [m for s in seqs for m in s["msms"]] + empty
    assert sorted(placed) == list(range(len(lens))), "every MSM exactly once"
    assert all(lens[m] == 0 for m in empty) and all(lens[m] > 0 for s in seqs for m in s["msms"])
    for s in seqs:
        ls = [lens[m] for m in s["msms"]]
        assert s["nmax"] == max(ls)
        assert 0 <= s["dev"] < n_dev
        if not s["shared"]:
            assert len(ls) == 1 and ls[0] > small_max
            continue
        assert max(ls) <= small_max
        assert max(ls) < 2 * min(ls), "length class: the largest length below twice the smallest"
        assert len(ls) <= cap
        assert len(ls) == 1 or len(ls) * s["msm_bytes"] <= budget, "byte budget"
        stride = (s["nmax"] + 7) & ~7
        assert len(ls) * W * stride < (1 << 31)


def test_every_msm_placed_once_and_classes(bp):
    lens = [0, 1, 2, 3, 7, 8, 9, 255, 256, 257, 65535, 65536, 1, 1, 3, 3, 40000, 1 << 20] + random_lens(1, 300)
    seqs, empty, _ = plan(bp, lens)
    check_plan(lens, seqs, empty, 1)
    assert sorted(empty) == [i for i, x in enumerate(lens) if x == 0]


def test_cap_holds_and_small_msms_share(bp):
    lens = [300] * 1000
    seqs, empty, _ = plan(bp, lens, cap=64)
    check_plan(lens, seqs, empty, 1, cap=64)
    assert len(seqs) == -(-1000 // 64)
    assert max(len(s["msms"]) for s in seqs) - min(len(s["msms"]) for s in seqs) <= 1, "near-equal parts"
    seqs, empty, _ = plan(bp, lens, cap=7)
    check_plan(lens, seqs, empty, 1, cap=7)
    assert len(seqs) == -(-1000 // 7)
    assert bp.bp_length_class(1) == 0 and bp.bp_length_class(255) == 7 and bp.bp_length_class(256) == 8


def test_large_msms_run_alone_longest_first(bp):
    lens = [1 << 18, 5, 1 << 20, 1 << 16, 6]
    seqs, empty, _ = plan(bp, lens)
    check_plan(lens, seqs, empty, 1)
    big = [s for s in seqs if not s["shared"]]
    assert [s["msms"] for s in big] == [[2], [0], [3]]
    assert seqs[:3] == big
    seqs, empty, _ = plan(bp, lens, small_max=0)
    assert all(not s["shared"] for s in seqs) and len(seqs) == 5


@pytest.mark.parametrize("count", [1, 10, 1000, 10000])
def test_byte_budget_for_any_count(bp, count):
    r = random.Random(count)
    lens = [r.randint(1 << 12, 1 << 15) for _ in range(count)]
    for budget in (1 << 30, 64 << 20, 1 << 20):
        seqs, empty, _ = plan(bp, lens, budget=budget)
        check_plan(lens, seqs, empty, 1, budget=budget)
        # the budget bounds every sequence, so the scratch does not grow with count
        assert max(len(s["msms"]) * s["msm_bytes"] for s in seqs) <= max(budget, max(s["msm_bytes"] for s in seqs))


def test_windows_times_stride_limit(bp):
    lens = [1 << 15] * 200
    seqs, empty, _ = plan(bp, lens, budget=1 << 40)
    check_plan(lens, seqs, empty, 1, budget=1 << 40)
    per = ((1 << 31) - 1) // (W * (1 << 15))
    assert max(len(s["msms"]) for s in seqs) <= per


@pytest.mark.parametrize("n_dev", [1, 2, 3, 4, 8])
def test_device_split_balanced(bp, n_dev):
    for seed in range(5):
        lens = random_lens(100 + seed, 200)
        seqs, empty, load = plan(bp, lens, n_dev=n_dev)
        check_plan(lens, seqs, empty, n_dev)
        per = [0] * n_dev
        for s in seqs:
            for m in s["msms"]:
                per[s["dev"]] += lens[m]
        assert per == load
        assert sum(per) == sum(lens)
        assert max(per) - min(per) <= max(lens), "balanced within one MSM's length"


def test_deterministic(bp):
    lens = random_lens(7, 2000)
    a = plan(bp, lens, n_dev=4)
    for _ in range(3):
        assert plan(bp, lens, n_dev=4) == a
    assert plan(bp, [], n_dev=2) == ([], [], [0, 0])


def test_new_names_in_header_and_package():
    hdr = open(os.path.join(ROOT, "include", "te_msm.h")).read()
    for name in ("te_msm_run_scalars_batch", "te_msm_run_scalars_batch_device"):
        assert re.search(r"\bint %s\(" % name, hdr), name
    assert "TE_MSM_BATCH_SEQ_MAX" in hdr and '"batch_sequences"' in hdr and '"batch_small_max"' in hdr
    src = open(os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "binding.py")).read()
    for name in ("def run_scalars_batch(", "def run_scalars_batch_device(", "te_msm_run_scalars_batch_device.argtypes"):
        assert name in src, name
    import importlib
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    assert pkg.BATCH_SEQ_MAX == 64 and hasattr(pkg.MsmContext, "run_scalars_batch") and hasattr(pkg.MsmContext, "run_scalars_batch_device")
    js = open(os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js", "compute_msm.js")).read()
    assert "msmBatch" in js and "msmBatch" in open(os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "js", "submission.d.ts")).read()
