"""Cost of fixed-base batch scalar multiplication (te_msm_bind_base, te_msm_mul_base_device) against what a
caller had before it: te_msm_mul_device over the point replicated n times, in the same process and library.  One box, the two sides
alternating inside every round, at least three rounds, ranges reported and no means.

  1. cost     per curve: for n in 2^10, 2^14, 2^18, 2^20 and W in 6, 8, 10, 12 -- the bind (wall clock, table bytes) once per W, then
              ROUNDS rounds of [baseline, W = 6, 8, 10, 12], every entry the wall clock of `reps` synchronous calls on device buffers
              divided by reps (a call returns with its output complete; reps makes every timed window at least 2^20 scalars long).
              The results of the bound call and of the baseline are compared byte for byte at every n before anything is timed.
              Acceptance line at 2^20: every round of the bound call below every round of the baseline.
  2. kernels  the workload for a profiler run of its own, which splits k_mul_base from the affine pass:
                  rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/mul_base_cost.py --step kernels
  3. parent   (only with --parent-lib PATH: a libtemsm.so built from the parent commit's csrc/) the default bench.py line of this build
              against the parent's, three rounds each, alternating, through TE_MSM_LIB: the MSM paths did not move.

    python tools/mul_base_cost.py [--only cost,parent] [--parent-lib /path/to/parent/libtemsm.so] [--out FILE]"""
import argparse
import importlib
import json
import os
import shlex
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1 << 10, 1 << 14, 1 << 18, 1 << 20)
WINDOWS = (6, 8, 10, 12)
ROUNDS = 3
BENCH_LIMIT = 300


def rand_scalars(n, sb):
    """n random 256-bit scalars in records of sb bytes (the top 16 bytes of a 48-byte record zero)"""
    import numpy as np
    raw = np.random.default_rng(n).integers(0, 256, size=(n, 32), dtype=np.uint8)
    if sb == 48:
        raw = np.concatenate([raw, np.zeros((n, 16), dtype=np.uint8)], axis=1)
    return raw.tobytes()


def timed(fn, reps):
    t = time.perf_counter()
    for _ in range(reps):
        fn()                                                                # (synchronous: returns with the output complete)
    return (time.perf_counter() - t) * 1e3 / reps


def step_cost(pkg, curve):
    import torch
    name = "bls12_377" if curve == pkg.CURVE_BLS12_377_G1 else "te"
    pb, sb = (96, 48) if curve == pkg.CURVE_BLS12_377_G1 else (64, 32)
    point, _ = pkg.synth_inputs(17, 1, scalars=False, curve=curve)
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", curve)
        bases = {}
        for W in WINDOWS:
            c.set_option("mul_base_window", W)
            before = c.get_option("mul_base_bytes")
            t = time.perf_counter()
            bases[W] = c.bind_base(point)
            ms = (time.perf_counter() - t) * 1e3
            t = time.perf_counter()
            again = c.bind_base(point)                                      # (the first bind of a process also loads the kernels' code)
            ms2 = (time.perf_counter() - t) * 1e3
            c.release_base(again)
            print(json.dumps({"step": "bind", "curve": name, "W": W, "first_bind_ms": round(ms, 2), "second_bind_ms": round(ms2, 2),
                              "table_bytes": c.get_option("mul_base_bytes") - before}), flush=True)
        for n in SIZES:
            sc = rand_scalars(n, sb)
            dp = torch.frombuffer(bytearray(point * n), dtype=torch.uint8).cuda()
            ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
            dref = torch.empty(pb * n, dtype=torch.uint8, device="cuda")
            dout = torch.empty(pb * n, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            baseline = lambda: c.mul_device(dp.data_ptr(), ds.data_ptr(), n, dref.data_ptr())
            calls = {W: (lambda b=bases[W]: c.mul_base_device(b, ds.data_ptr(), n, dout.data_ptr())) for W in WINDOWS}
            baseline()                                                      # warm-up of every shape, and the same bytes
            for W in WINDOWS:
                calls[W]()
                if not torch.equal(dout, dref):
                    raise SystemExit("W = %d, n = %d: the bound call differs from te_msm_mul_device" % (W, n))
            reps = max(1, (1 << 20) // n)
            rounds = {"baseline": [], **{W: [] for W in WINDOWS}}
            for _ in range(ROUNDS):
                rounds["baseline"].append(round(timed(baseline, reps), 4))
                for W in WINDOWS:
                    rounds[W].append(round(timed(calls[W], reps), 4))
            rec = {"step": "cost", "curve": name, "n": n, "reps_per_round": reps, "unit": "ms per call, one entry per round",
                   "te_msm_mul_device_replicated": rounds["baseline"]}
            for W in WINDOWS:
                rec["mul_base_device_W%d" % W] = rounds[W]
            if n == 1 << 20:
                rec["every_round_below_every_baseline_round"] = {"W%d" % W: max(rounds[W]) < min(rounds["baseline"]) for W in WINDOWS}
                rec["baseline_lowest_over_bound_highest"] = {"W%d" % W: round(min(rounds["baseline"]) / max(rounds[W]), 2) for W in WINDOWS}
            print(json.dumps(rec), flush=True)


def step_kernels(pkg):
    import torch
    n = 1 << 20
    for curve in (pkg.CURVE_TE_BLS12, pkg.CURVE_BLS12_377_G1):
        pb, sb = (96, 48) if curve == pkg.CURVE_BLS12_377_G1 else (64, 32)
        point, _ = pkg.synth_inputs(17, 1, scalars=False, curve=curve)
        ds = torch.frombuffer(bytearray(rand_scalars(n, sb)), dtype=torch.uint8).cuda()
        dout = torch.empty(pb * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            for W in WINDOWS:
                c.set_option("mul_base_window", W)
                base = c.bind_base(point)
                for _ in range(4):
                    c.mul_base_device(base, ds.data_ptr(), n, dout.data_ptr())
                c.release_base(base)
    print("kernels done: per curve, W = 6, 8, 10, 12 in this order, 4 calls of 4 pieces each")


def step_parent(parent_lib):
    """one bench.py headline per child; this build and the parent's alternate"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "5"]
    rounds = {"this_build": [], "parent": []}
    for _ in range(3):
        for who in ("this_build", "parent"):
            env = dict(os.environ)
            if who == "parent":
                env["TE_MSM_LIB"] = parent_lib
            else:
                env.pop("TE_MSM_LIB", None)
            p = subprocess.run(["timeout", "-k", "10", str(BENCH_LIMIT)] + cmd, stdout=subprocess.PIPE, env=env, cwd=ROOT)
            if p.returncode:
                raise SystemExit("bench.py failed (%s): exit %d" % (who, p.returncode))
            line = [ln for ln in p.stdout.decode().splitlines() if ln.startswith("{")][-1]
            rounds[who].append(round(json.loads(line)["value"], 2))
            print(json.dumps({"step": "parent", "round": len(rounds[who]), "build": who, "msm_per_s": rounds[who][-1]}), flush=True)
    par, new = rounds["parent"], rounds["this_build"]
    spread = max(par) - min(par)
    print(json.dumps({"step": "parent", "bench": "bench.py --gpus 1 --steps 100 --warmup 5, MSM/s, rounds alternating",
                      "this_build": new, "parent": par, "parent_spread": round(spread, 2),
                      "lowest_round_of_this_build_minus_parents_lowest": round(min(new) - min(par), 2),
                      "inside_parents_spread": min(new) >= min(par) - spread}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("cost", "kernels", "parent"), default=None)
    ap.add_argument("--curve", type=int, default=0)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default="cost,parent", help="the steps of this run; their outputs joined are one run's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        if a.step == "parent":
            return step_parent(a.parent_lib)
        pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
        return step_kernels(pkg) if a.step == "kernels" else step_cost(pkg, a.curve)
    # every step in a child of its own, under its own time limit, chained: a step that fails ends the run
    only = set(a.only.split(","))
    me = "%s %s" % (shlex.quote(sys.executable), shlex.quote(os.path.abspath(__file__)))
    steps = ["timeout -k 10 420 %s --step cost --curve 0" % me, "timeout -k 10 420 %s --step cost --curve 1" % me] if "cost" in only else []
    if a.parent_lib and "parent" in only:
        steps.append("timeout -k 10 %d %s --step parent --parent-lib %s" % (6 * BENCH_LIMIT + 60, me, shlex.quote(os.path.abspath(a.parent_lib))))
    p = subprocess.Popen(["bash", "-c", "set -o pipefail; " + " && ".join(steps)], stdout=subprocess.PIPE, cwd=ROOT, text=True)
    text = ""
    for line in p.stdout:                                                  # (as they come: a long run shows its progress)
        sys.stdout.write(line)
        sys.stdout.flush()
        text += line
    if p.wait():
        raise SystemExit("a step failed: exit %d" % p.returncode)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
