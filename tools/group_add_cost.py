"""Cost of batched group addition and point-set sums (te_msm_add_device, te_msm_sum_device).  One box, the sides of
every comparison alternating inside every round, three rounds, lowest .. highest reported and no means.

  1. add      te_msm_add_device at 2^20 pairs on both curves.  With --also NAME=PATH (repeatable: other builds of the same library, e.g.
              one whose affine pass is a different normaliser) every build runs in a child of its own through TE_MSM_LIB, the builds
              alternating inside every round, after each child has hashed its first 4101 results (the builds must agree).  This is how
              the block-wide batch inversion was measured against te_msm_mul's chains of eight before it was removed (DESIGN.md
              section 19): decision line per build -- lower than the in-tree library in every round, or not.
  2. link     the host path the call replaces, at 2^20 pairs: both operands read back, the result uploaded again (pinned memory).  The
              library has no batched host addition to time between the two (its host tails fold window rows, not point pairs): the link
              time alone is the floor of that path.
  3. sum      te_msm_sum_device at 2^16 and 2^20 points against te_msm_run_device with all-ones scalars over the same points (the only
              way to sum a point buffer on the device before), results compared first.
  4. copy     the yardstick of measuring-on-mi355x: a device-to-device copy_ of the bytes each kernel of an add call moves.
  5. kernels  the workload for a profiler run of its own, which splits the kernels of a call:
                  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -o run -- python tools/group_add_cost.py --step kernels
  6. parent   (only with --parent-lib PATH: a libtemsm.so built from the parent commit's csrc/) the default bench.py line of this build
              against the parent's, three rounds each, alternating, through TE_MSM_LIB: the MSM paths did not move.

    python tools/group_add_cost.py [--only add,link,sum,copy,parent] [--also NAME=PATH ...] [--parent-lib PATH] [--out FILE]"""
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
PKG_DIR = os.path.join(ROOT, "webgpu-msm-twisted-edwards_amd")
IN_TREE = os.path.join(PKG_DIR, "libtemsm.so")
N = 1 << 20
ROUNDS = 3
REPS = 10
BENCH_LIMIT = 300


def timed(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()                                                                # (synchronous: returns with the output complete)
    return (time.perf_counter() - t) * 1e3 / reps


def operands(pkg, curve, n):
    import torch
    a, _ = pkg.synth_inputs(0x6C0 + curve, n, scalars=False, curve=curve)
    b, _ = pkg.synth_inputs(0x6C1 + curve, n, scalars=False, curve=curve)
    da, db = (torch.frombuffer(bytearray(v), dtype=torch.uint8).cuda() for v in (a, b))
    torch.cuda.synchronize()
    return a, b, da, db


def step_add_one(pkg, build):
    """one build (TE_MSM_LIB names it), both curves: ms per te_msm_add_device call of 2^20 pairs"""
    import torch
    for curve in (pkg.CURVE_TE_BLS12, pkg.CURVE_BLS12_377_G1):
        pb = 96 if curve == pkg.CURVE_BLS12_377_G1 else 64
        a, b, da, db = operands(pkg, curve, N)
        dout = torch.empty(pb * N, dtype=torch.uint8, device="cuda")
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            c.add_device(da.data_ptr(), db.data_ptr(), 4101, dout.data_ptr())
            head = bytes(dout[:pb * 4101].cpu().numpy())
            ms = timed(lambda: c.add_device(da.data_ptr(), db.data_ptr(), N, dout.data_ptr()), REPS)
        print(json.dumps({"step": "add_one", "build": build, "curve": curve, "ms": round(ms, 4), "head": __import__("hashlib").sha256(head).hexdigest()}), flush=True)


def step_add(also):
    builds = {"in_tree": IN_TREE}
    for item in also:
        name, _, path = item.partition("=")
        builds[name] = os.path.abspath(path)
    rounds = {b: {0: [], 1: []} for b in builds}
    heads = {}
    me = [sys.executable, os.path.abspath(__file__)]
    for _ in range(ROUNDS):
        for build, lib in builds.items():
            if not os.path.exists(lib):
                raise SystemExit("%s is missing" % lib)
            p = subprocess.run(["timeout", "-k", "10", "240"] + me + ["--step", "add_one", "--build", build], stdout=subprocess.PIPE,
                               env=dict(os.environ, TE_MSM_LIB=lib), cwd=ROOT)
            if p.returncode:
                raise SystemExit("add_one failed (%s): exit %d" % (build, p.returncode))
            for ln in p.stdout.decode().splitlines():
                if ln.startswith("{"):
                    r = json.loads(ln)
                    rounds[build][r["curve"]].append(r["ms"])
                    heads.setdefault(r["curve"], set()).add(r["head"])
    for curve, name in ((0, "te"), (1, "bls12_377")):
        if len(heads[curve]) != 1:
            raise SystemExit("the builds disagree on the first 4101 results (%s)" % name)
        rec = {"step": "add", "curve": name, "pairs": N, "reps_per_round": REPS, "unit": "ms per te_msm_add_device call, one entry per round, builds alternating"}
        for b in builds:
            rec[b] = rounds[b][curve]
            rec[b + "_lowest_highest"] = [min(rounds[b][curve]), max(rounds[b][curve])]
            if b != "in_tree":
                rec[b + "_lower_than_in_tree_in_every_round"] = all(x < y for x, y in zip(rounds[b][curve], rounds["in_tree"][curve]))
        print(json.dumps(rec), flush=True)


def step_link(pkg):
    import torch
    for curve, name in ((pkg.CURVE_TE_BLS12, "te"), (pkg.CURVE_BLS12_377_G1, "bls12_377")):
        pb = 96 if curve == pkg.CURVE_BLS12_377_G1 else 64
        da = torch.zeros(pb * N, dtype=torch.uint8, device="cuda")
        db = torch.zeros(pb * N, dtype=torch.uint8, device="cuda")
        ha, hb = (torch.empty(pb * N, dtype=torch.uint8).pin_memory() for _ in range(2))

        def trip():
            ha.copy_(da, non_blocking=True)
            hb.copy_(db, non_blocking=True)
            torch.cuda.synchronize()
            da.copy_(ha, non_blocking=True)
            torch.cuda.synchronize()
        rounds = [round(timed(trip, 5), 3) for _ in range(ROUNDS)]
        print(json.dumps({"step": "link", "curve": name, "pairs": N, "bytes_down": 2 * pb * N, "bytes_up": pb * N,
                          "unit": "ms: both operands to pinned host memory, then the result back; no host addition in between (the library has none)",
                          "rounds": rounds}), flush=True)


def step_sum(pkg):
    import torch
    for curve, name in ((pkg.CURVE_TE_BLS12, "te"), (pkg.CURVE_BLS12_377_G1, "bls12_377")):
        sb = 48 if curve == pkg.CURVE_BLS12_377_G1 else 32
        for n in (1 << 16, 1 << 20):
            pts, _ = pkg.synth_inputs(0x6C2 + curve, n, scalars=False, curve=curve)
            dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
            ds = torch.frombuffer(bytearray((1).to_bytes(sb, "little") * n), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
            with pkg.MsmContext((0,)) as c:
                c.set_option("curve", curve)
                if c.sum_device(dp.data_ptr(), n) != c.run_device(dp.data_ptr(), ds.data_ptr(), n):
                    raise SystemExit("n = %d: te_msm_sum_device differs from the MSM over all-ones scalars" % n)
                reps = 20 if n < 1 << 20 else 10
                rs, rm = [], []
                for _ in range(ROUNDS):
                    rs.append(round(timed(lambda: c.sum_device(dp.data_ptr(), n), reps), 4))
                    rm.append(round(timed(lambda: c.run_device(dp.data_ptr(), ds.data_ptr(), n), reps), 4))
            print(json.dumps({"step": "sum", "curve": name, "n": n, "unit": "ms per call, one entry per round, alternating",
                              "te_msm_sum_device": rs, "te_msm_run_device_all_ones": rm,
                              "sum_lower_in_every_round": all(x < y for x, y in zip(rs, rm))}), flush=True)


def step_copy(pkg):
    """device-to-device copy_ of the bytes each kernel of a 2^20-pair add call moves (read + written), timed with events"""
    import torch
    for curve, name, pb, jb in ((0, "te", 64, 112), (1, "bls12_377", 96, 176)):
        for kernel, moved in (("k_group_add", (2 * pb + jb) * N), ("affine pass", (jb + pb) * N + pb * N // 8 * 2)):
            half = moved // 2                                               # a copy_ of h bytes moves 2 h
            src = torch.zeros(half, dtype=torch.uint8, device="cuda")
            dst = torch.empty_like(src)
            rounds = []
            for _ in range(ROUNDS):
                dst.copy_(src)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(10):
                    dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                rounds.append(round(e0.elapsed_time(e1) / 10, 4))
            print(json.dumps({"step": "copy", "curve": name, "kernel": kernel, "bytes_moved": moved, "unit": "ms per copy_ of the same bytes", "rounds": rounds}), flush=True)


def step_kernels(pkg):
    import torch
    for curve in (pkg.CURVE_TE_BLS12, pkg.CURVE_BLS12_377_G1):
        pb = 96 if curve == pkg.CURVE_BLS12_377_G1 else 64
        a, b, da, db = operands(pkg, curve, N)
        dout = torch.empty(pb * N, dtype=torch.uint8, device="cuda")
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            for _ in range(4):
                c.add_device(da.data_ptr(), db.data_ptr(), N, dout.data_ptr())
            for _ in range(4):
                c.sum_device(da.data_ptr(), N)
    print("kernels done: per curve, 4 te_msm_add_device calls and 4 te_msm_sum_device calls of 2^20")


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
    par, new = rounds["parent"], rounds["this_build"]
    spread = max(par) - min(par)
    print(json.dumps({"step": "parent", "bench": "bench.py --gpus 1 --steps 100 --warmup 5, MSM/s, rounds alternating",
                      "this_build": new, "parent": par, "parent_spread": round(spread, 2),
                      "lowest_round_of_this_build_minus_parents_lowest": round(min(new) - min(par), 2),
                      "inside_parents_spread": min(new) >= min(par) - spread}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=("add", "add_one", "link", "sum", "copy", "kernels", "parent"), default=None)
    ap.add_argument("--build", default="in_tree")
    ap.add_argument("--also", action="append", default=[], metavar="NAME=PATH")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--only", default="add,link,sum,copy,parent", help="the steps of this run; their outputs joined are one run's")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.step:
        if a.step == "parent":
            return step_parent(a.parent_lib)
        if a.step == "add":
            return step_add(a.also)
        pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
        return {"add_one": lambda: step_add_one(pkg, a.build), "link": lambda: step_link(pkg), "sum": lambda: step_sum(pkg),
                "copy": lambda: step_copy(pkg), "kernels": lambda: step_kernels(pkg)}[a.step]()
    # every step in a child of its own, under its own time limit, chained: a step that fails ends the run
    only = a.only.split(",")
    me = "%s %s" % (shlex.quote(sys.executable), shlex.quote(os.path.abspath(__file__)))
    limits = {"add": 3 * (1 + len(a.also)) * 250, "link": 120, "sum": 300, "copy": 120}
    also = "".join(" --also %s" % shlex.quote(x) for x in a.also)
    steps = ["timeout -k 10 %d %s --step %s%s" % (limits[s], me, s, also if s == "add" else "") for s in only if s in limits]
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
