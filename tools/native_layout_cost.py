"""What the native-layout options cost: "scalar_record_bytes" = 32 for BLS12-377 scalars from host memory, a bind at "point_stride" = 104
with "point_infinity_flag", and whether the default path kept its speed
(include/te_msm.h).  Needs one GPU.  Without --step it runs every step as a child process of its own, each under
`timeout -k 10`, chained with `&&` (a step that fails or hangs ends the run), and collects their JSON lines in --out:

  1. scalars  BLS12-377, a bound set of 2^log2n points, te_msm_run_scalars from HOST memory over the same values in 48-byte and in 32-byte
              records: the lone call (lowest of 9) and four tickets in flight (te_msm_submit_scalars, ms per MSM over --steps MSMs); three
              rounds, the two sizes alternating inside every round; every result compared with the first one.
  2. bind     BLS12-377, te_msm_bind_points of 2^log2n points from host memory: packed canonical x || y (96 bytes a point) against arkworks'
              image -- Montgomery coordinates, stride 104, the flag option on, one record in 1024 flagged; lowest of 3 binds a round, three
              rounds, alternating; one MSM over each set compared.
  3. parent   (only with --parent-lib PATH: a libtemsm.so built from the parent commit's csrc/) the default bench.py line
              (`--gpus 1 --steps 100 --warmup 5`) on this build against the parent's library through TE_MSM_LIB: three rounds, alternating.

    python tools/native_layout_cost.py [--log2n 20] [--steps 32] [--only scalars,bind,parent] [--parent-lib /path/to/parent/libtemsm.so] [--out FILE]"""
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
DEPTH = 4
BENCH_LIMIT = 300                           # seconds for one bench.py child of step 3; the step's own limit covers all six


def in_flight_ms(c, submit, steps):
    """ms per MSM of one pass of `steps` MSMs with DEPTH tickets in flight; the last result"""
    t1 = time.perf_counter()
    tk, last = [], None
    for _ in range(steps):
        tk.append(submit())
        if len(tk) >= DEPTH:
            last = c.collect(tk.pop(0))
    while tk:
        last = c.collect(tk.pop(0))
    return (time.perf_counter() - t1) * 1e3 / steps, last


def lone_ms(call, reps=9):
    ts, r = [], None
    for _ in range(reps):
        t1 = time.perf_counter()
        r = call()
        ts.append((time.perf_counter() - t1) * 1e3)
    return min(ts), r


def step_scalars(a):
    import numpy as np
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    n = 1 << a.log2n
    pts, sc48 = pkg.synth_inputs(7, n, curve=pkg.CURVE_BLS12_377_G1)
    sc32 = np.frombuffer(sc48, dtype=np.uint8).reshape(-1, 48)[:, :32].tobytes()
    sc = {48: sc48, 32: sc32}
    rounds = {"lone": {48: [], 32: []}, "in_flight": {48: [], 32: []}}
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        b = c.bind_points(pts)
        first = c.run_scalars(b, sc48)
        for rec in (48, 32):                                                     # warm both sizes: buffers, upload lanes
            c.set_option("scalar_record_bytes", rec)
            assert c.run_scalars(b, sc[rec]) == first
            assert in_flight_ms(c, lambda: c.submit_scalars(b, sc[rec]), 8)[1] == first
        for r in range(3):
            for rec in ((48, 32) if r % 2 == 0 else (32, 48)):
                c.set_option("scalar_record_bytes", rec)
                ms, got = lone_ms(lambda: c.run_scalars(b, sc[rec]))
                assert got == first
                rounds["lone"][rec].append(round(ms, 4))
                ms, got = in_flight_ms(c, lambda: c.submit_scalars(b, sc[rec]), a.steps)
                assert got == first
                rounds["in_flight"][rec].append(round(ms, 4))
        c.release_points(b)
    out = {"step": "scalars", "curve": "BLS12-377 G1", "n": n, "steps": a.steps, "depth": DEPTH,
           "bytes_per_msm": {"48": 48 * n, "32": 32 * n}}
    for form in ("lone", "in_flight"):
        for rec in (48, 32):
            out["%s_ms_%d_sorted" % (form, rec)] = sorted(rounds[form][rec])
    print(json.dumps(out), flush=True)


def step_bind(a):
    import numpy as np
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    n = 1 << a.log2n
    Q = 258664426012969094010652733694893533536393512754914660539884262666720468348340822774968888139573360124440321458177
    pts, sc = pkg.synth_inputs(9, n, curve=pkg.CURVE_BLS12_377_G1)
    flagged = np.arange(0, n, 1024)
    # the image: coordinates as x 2^384 mod q, 104-byte records, flag byte, filled padding
    mont = b"".join((int.from_bytes(pts[48 * i:48 * i + 48], "little") * (1 << 384) % Q).to_bytes(48, "little") for i in range(2 * n))
    img = np.full((n, 104), 0xA5, dtype=np.uint8)
    img[:, :96] = np.frombuffer(mont, dtype=np.uint8).reshape(n, 96)
    img[:, 96] = 0
    img[flagged, :96] = 0
    img[flagged, 96] = 1
    img = img.tobytes()
    sc0 = np.frombuffer(sc, dtype=np.uint8).reshape(n, 48).copy()
    sc0[flagged] = 0                                                             # the packed set cannot hold infinity: those scalars are zero there
    rounds = {"packed": [], "arkworks": []}
    with pkg.MsmContext((0,)) as c:
        c.set_option("curve", pkg.CURVE_BLS12_377_G1)
        binds = {"packed": lambda: c.bind_points(pts), "arkworks": lambda: c.bind_points(img, montgomery=True, stride=104, infinity_flag=True)}
        results = {}
        for who in ("packed", "arkworks"):                                       # warm, and one MSM over each set
            b = binds[who]()
            results[who] = c.run_scalars(b, sc0.tobytes() if who == "packed" else sc)
            c.release_points(b)
        assert results["packed"] == results["arkworks"]
        for r in range(3):
            for who in (("packed", "arkworks") if r % 2 == 0 else ("arkworks", "packed")):
                ts = []
                for _ in range(3):
                    t1 = time.perf_counter()
                    b = binds[who]()
                    ts.append((time.perf_counter() - t1) * 1e3)
                    c.release_points(b)
                rounds[who].append(round(min(ts), 4))
    print(json.dumps({"step": "bind", "curve": "BLS12-377 G1", "n": n, "bytes": {"packed": 96 * n, "arkworks": 104 * n}, "flagged": int(len(flagged)),
                      "packed_ms_sorted": sorted(rounds["packed"]), "arkworks_ms_sorted": sorted(rounds["arkworks"])}), flush=True)


def bench_line(lib, steps, warmup):
    env = dict(os.environ)
    if lib:
        env["TE_MSM_LIB"] = lib
    r = subprocess.run(["timeout", "-k", "10", str(BENCH_LIMIT), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT)
    if r.returncode:
        raise SystemExit("bench.py failed (%d): %s" % (r.returncode, r.stderr.decode()[-800:]))
    return json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1])


def step_parent(a):
    lines = {"this": [], "parent": []}
    for r in range(3):
        for who in (("this", "parent") if r % 2 == 0 else ("parent", "this")):
            lines[who].append(bench_line(a.parent_lib if who == "parent" else None, a.bench_steps, a.bench_warmup))
    out = {"step": "parent", "bench": "--gpus 1 --steps %d --warmup %d" % (a.bench_steps, a.bench_warmup), "metric": lines["this"][0].get("metric")}
    for who in ("this", "parent"):
        for key in ("value", "ms_per_step", "latency_ms"):
            out["%s_%s_sorted" % (who, key)] = sorted(round(ln[key], 4) for ln in lines[who])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["scalars", "bind", "parent"])
    ap.add_argument("--only", default="scalars,bind,parent")
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--bench-steps", type=int, default=100)
    ap.add_argument("--bench-warmup", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    if a.step:
        return {"scalars": step_scalars, "bind": step_bind, "parent": step_parent}[a.step](a)
    me = [sys.executable, os.path.abspath(__file__), "--log2n", str(a.log2n), "--steps", str(a.steps), "--bench-steps", str(a.bench_steps),
          "--bench-warmup", str(a.bench_warmup)]
    steps = []
    if "scalars" in a.only:
        steps.append(("scalars", 240, []))
    if "bind" in a.only:
        steps.append(("bind", 300, []))
    if "parent" in a.only and a.parent_lib:
        steps.append(("parent", 6 * BENCH_LIMIT + 30, ["--parent-lib", a.parent_lib]))
    cmd = " && ".join("timeout -k 10 %d %s" % (limit, " ".join(shlex.quote(x) for x in me + ["--step", name] + extra)) for name, limit, extra in steps)
    r = subprocess.run(["bash", "-c", "set -o pipefail; " + cmd], stdout=subprocess.PIPE, cwd=ROOT)
    text = r.stdout.decode()
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
