"""Host time per call of the point operations of csrc/points.hip where a call is bound by its launches and its one synchronise
(small n) and where it is not, for A/B runs of two builds of the library (profiles/points_plumbing_ab.txt):
    python tools/points_host_cost.py --also parent=PATH/libtemsm.so [--runs 5] [--out FILE]
        the in-tree build and every --also build alternate through TE_MSM_LIB, every run a process of its own under its own time limit:
        te_msm_mul_base_device at 2^10 and 2^20, te_msm_mul_device at 2^16, te_msm_add_device at 2^20 pairs, te_msm_sum_device at 2^16
        (Twisted-Edwards curve, device buffers, ms per call), the addition on BLS12-377 as well, and -- behind all of them -- bench.py's
        headline as a control; then the table and the rule of profiles/engine_split_ab.txt: a figure passes when a build's median
        lies within the first --also build's own spread (max - min of its runs) of that build's median
    python tools/points_host_cost.py --step one
        one run of the calls with the library TE_MSM_LIB names: one JSON line"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
IN_TREE = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd", "libtemsm.so")
BENCH = ["bench.py", "--gpus", "1", "--steps", "40", "--warmup", "5", "--no-cpu-baseline", "--no-sizes", "--no-configs"]
FIGURES = ("mul_base_device_n2^10_ms", "mul_base_device_n2^20_ms", "mul_device_n2^16_ms", "add_device_n2^20_ms", "sum_device_n2^16_ms", "add_device_bls12_377_n2^20_ms",
           "bench_value_msm_per_s")


def step_one(pkg):
    import torch
    from group_add_cost import operands, timed
    from mul_base_cost import rand_scalars
    n = 1 << 20
    a, b, da, db = operands(pkg, 0, n)
    ds = torch.frombuffer(bytearray(rand_scalars(n, 32)), dtype=torch.uint8).cuda()
    dout = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = {}
    with pkg.MsmContext((0,)) as c:
        base = c.bind_base(a[:64])
        for logn, reps in ((10, 2000), (20, 20)):
            res["mul_base_device_n2^%d_ms" % logn] = timed(lambda: c.mul_base_device(base, ds.data_ptr(), 1 << logn, dout.data_ptr()), reps)
        res["mul_device_n2^16_ms"] = timed(lambda: c.mul_device(da.data_ptr(), ds.data_ptr(), 1 << 16, dout.data_ptr()), 10)
        res["add_device_n2^20_ms"] = timed(lambda: c.add_device(da.data_ptr(), db.data_ptr(), n, dout.data_ptr()), 50)
        res["sum_device_n2^16_ms"] = timed(lambda: c.sum_device(da.data_ptr(), 1 << 16), 200)
    del da, db, dout
    a, b, da, db = operands(pkg, 1, n)                                      # the addition on the second curve as well: its kernels are the longest
    dout = torch.empty(96 * n, dtype=torch.uint8, device="cuda")
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", 1)
        res["add_device_bls12_377_n2^20_ms"] = timed(lambda: c.add_device(da.data_ptr(), db.data_ptr(), n, dout.data_ptr()), 50)
    print(json.dumps({k: round(v, 4) for k, v in res.items()}), flush=True)


def child(cmd, lib, limit):
    p = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable] + cmd, stdout=subprocess.PIPE, env=dict(os.environ, TE_MSM_LIB=lib), cwd=ROOT)
    if p.returncode:
        raise SystemExit("%s failed (%s): exit %d" % (cmd[0], lib, p.returncode))
    return json.loads([ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("one",), default=None)
    ap.add_argument("--also", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        return step_one(importlib.import_module("webgpu-msm-twisted-edwards_amd"))
    builds = {name: os.path.abspath(path) for name, _, path in (item.partition("=") for item in a.also)}
    builds["in_tree"] = IN_TREE
    yard = next(iter(builds))                                               # the build whose spread is the yardstick
    runs = {b: {f: [] for f in FIGURES} for b in builds}
    # (the calls first, the benchmark runs behind them: a large allocation costs a later process on the same device more once bench.py
    # has run there -- te_msm_add_device at 2^20, which allocates 112 MB per call, went from 0.72 to 3.2 ms per call for both builds alike)
    for cmd, limit in (([os.path.abspath(__file__), "--step", "one"], 240), (BENCH, 300)):
        for r in range(a.runs):
            for b, lib in builds.items():
                one = child(cmd, lib, limit)
                if cmd is BENCH:
                    one = {"bench_value_msm_per_s": round(one["value"], 2)}
                for f in one:
                    runs[b][f].append(one[f])
                print(json.dumps({"run": r + 1, "build": b, **one}), flush=True)
    lines = []
    for f in FIGURES:
        med, spread = statistics.median(runs[yard][f]), max(runs[yard][f]) - min(runs[yard][f])
        for b in builds:
            m = statistics.median(runs[b][f])
            verdict = "" if b == yard else ("passes" if abs(m - med) <= spread else "FAILS")
            lines.append("%-26s %-8s %-52s median %-10.4f %s %s" % (f, b, " ".join("%.4f" % v for v in runs[b][f]), m,
                                                                  ("spread %.4f" % spread) if b == yard else "", verdict))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
