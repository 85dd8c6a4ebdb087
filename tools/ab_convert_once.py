"""A/B of the record conversion once per occupancy run of a shared slab, child processes alternating, three rounds:
  parent   the build named by --parent (TE_MSM_LIB: the previous commit's libtemsm.so -- every call converts, four products per point)
  convert  this build with "share_records" = 2 (TE_MSM_SHARE_RECORDS=2: every call converts, three products per point)
  once     this build as it ships (one conversion per occupancy run)
Per variant: bench.py's headline (--steps 100, default settings; 4 tickets in flight over ONE point buffer) and the same pipelined pass over
four DISTINCT copies of the points (every ticket converts in every variant: what the three-product conversion alone is worth there),
plus record_conversions per MSM and the accumulation's clock in flight (te_msm_stage_ms, profile level 1).
python tools/ab_convert_once.py --parent webgpu-msm-twisted-edwards_amd/libtemsm_parent.so [--rounds 3]"""
import argparse, importlib, json, os, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path.insert(0, ROOT)
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    import torch
    n, depth, steps = 1 << 20, 4, 100
    pts, sc = pkg.synth_inputs(0x5EED0014, n, fixed_point="random")
    copies = [torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda() for _ in range(depth)]
    ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()

    def passes(c, bufs):
        def one():
            tk, t0 = [], time.perf_counter()
            for i in range(steps):
                tk.append(c.submit_device(bufs[i % len(bufs)].data_ptr(), ds.data_ptr(), n))
                if len(tk) >= depth:
                    c.collect(tk.pop(0))
            while tk:
                c.collect(tk.pop(0))
            return (time.perf_counter() - t0) * 1e3 / steps
        one()
        return [one() for _ in range(3)]

    with pkg.MsmContext((0,)) as c:
        want = c.run_device(copies[0].data_ptr(), ds.data_ptr(), n)
        assert all(c.collect(c.submit_device(b.data_ptr(), ds.data_ptr(), n)) == want for b in copies)
        out = {}
        try:
            conv0 = c.get_option("record_conversions")
        except Exception:
            conv0 = None
        out["shared_ms"] = passes(c, copies[:1])
        if conv0 is not None:
            out["shared_conversions_per_msm"] = (c.get_option("record_conversions") - conv0) / (4 * steps)
        out["distinct_ms"] = passes(c, copies)
        c.set_option("profile", 1)
        clk = []
        tk = [c.submit_device(copies[0].data_ptr(), ds.data_ptr(), n) for _ in range(depth)]
        for _ in range(24):
            c.collect(tk.pop(0))
            st = c.stage_ms()
            clk.append(st.get("accumulate_core_clock_ghz", -1.0))
            tk.append(c.submit_device(copies[0].data_ptr(), ds.data_ptr(), n))
        for t in tk:
            c.collect(t)
        out["clock_in_flight_ghz"] = sum(clk) / len(clk)
    print(json.dumps(out), flush=True)


def bench(env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "100", "--no-cpu-baseline", "--no-sizes", "--no-host-buffers",
                        "--no-configs"], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if not lines:
        raise SystemExit("bench failed: " + r.stderr[-1500:])
    d = json.loads(lines[-1])
    return d["value"], d["passes_ms_per_step"], d["roofline"].get("timed_region", {}).get("core_clock_ghz")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "child":
        child()
        sys.exit(0)
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    variants = (("parent", {"TE_MSM_LIB": os.path.abspath(a.parent)}), ("convert", {"TE_MSM_SHARE_RECORDS": "2"}), ("once", {}))
    for rnd in range(a.rounds):
        for name, extra in variants:
            env = dict(os.environ, **extra)
            v, ps, ghz = bench(env)
            r = subprocess.run([sys.executable, __file__, "child"], env=env, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                raise SystemExit("child failed (%d): %s" % (r.returncode, r.stderr[-1500:]))
            c = json.loads(r.stdout.strip().splitlines()[-1])
            print("round %d %-8s bench %7.1f MSM/s (pass %s ms, clock %s GHz)  shared %s  distinct %s ms/MSM  conversions/MSM %s  clock in flight %.3f GHz" % (
                rnd, name, v, " ".join("%.4f" % x for x in ps), "%.3f" % ghz if ghz else "-", " ".join("%.4f" % x for x in c["shared_ms"]),
                " ".join("%.4f" % x for x in c["distinct_ms"]), c.get("shared_conversions_per_msm", "-"), c["clock_in_flight_ghz"]), flush=True)
