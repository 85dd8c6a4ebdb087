"""Cost of x-only points (te_msm_points_from_x*, te_msm_bind_points_x, te_msm_run_x).
Two runs, as profiles/points_from_x_cost.txt records them:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/points_from_x_cost.py --kernels
        k_points_from_x at 2^16 and 2^20 for both curves (device x -> device points; a few repetitions each), and
        k_check_subgroup at 2^20 (Twisted-Edwards) as the yardstick; the kernel times come from rocprofv3's stats
    python tools/points_from_x_cost.py [--out FILE]
        wall-clock times (profiler off) of run_x against run and of bind_points_x against bind_points, both curves, one JSON line"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def xs_of(pkg, pts, curve):
    """x-only form; BLS12-377 with the larger-root flag (the synthesized points' y decides)"""
    import numpy as np
    pb, xb = (96, 48) if curve == pkg.CURVE_BLS12_377_G1 else (64, 32)
    a = np.frombuffer(pts, dtype=np.uint8).reshape(-1, pb)
    xs = a[:, :xb].copy()
    if curve == pkg.CURVE_BLS12_377_G1:
        from oracle import model377 as b
        half, ys = (b.Q - 1) // 2, a[:, 48:].tobytes()
        larger = np.fromiter((int.from_bytes(ys[48 * i:48 * i + 48], "little") > half for i in range(len(a))), dtype=bool, count=len(a))
        xs[larger, 47] |= 0x80
    return xs.tobytes()


def kernels(pkg):
    import torch
    for curve in (pkg.CURVE_TE_BLS12, pkg.CURVE_BLS12_377_G1):
        pb = 96 if curve == pkg.CURVE_BLS12_377_G1 else 64
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            for n in (1 << 16, 1 << 20):
                pts, _ = pkg.synth_inputs(11, n, scalars=False, curve=curve)
                dx = torch.frombuffer(bytearray(xs_of(pkg, pts, curve)), dtype=torch.uint8).cuda()
                dout = torch.empty(pb * n, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                for _ in range(4):
                    c.points_from_x_device(dx.data_ptr(), n, dout.data_ptr())
                assert bytes(dout.cpu().numpy()) == pts
                if n == 1 << 20 and curve == pkg.CURVE_TE_BLS12:
                    dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
                    torch.cuda.synchronize()
                    for _ in range(4):
                        assert c.check_points_device(dp.data_ptr(), n, 2) is None
    print("kernels done")


def wall(pkg, out):
    res = {}
    for curve, name in ((pkg.CURVE_TE_BLS12, "te"), (pkg.CURVE_BLS12_377_G1, "bls12_377")):
        n = 1 << 20
        pts, sc = pkg.synth_inputs(12, n, curve=curve)
        xs = xs_of(pkg, pts, curve)
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            want = c.run(pts, sc)
            assert c.run_x(xs, sc) == want                                      # warm-up, and the same answer
            for key, fn in (("run", lambda: c.run(pts, sc)), ("run_x", lambda: c.run_x(xs, sc)),
                            ("bind_points", lambda: c.release_points(c.bind_points(pts))),
                            ("bind_points_x", lambda: c.release_points(c.bind_points_x(xs)))):
                ts = []
                for _ in range(3):
                    t = time.perf_counter()
                    fn()
                    ts.append((time.perf_counter() - t) * 1e3)
                res["%s_%s_n%d_ms" % (name, key, n)] = min(ts)
    line = json.dumps({k: round(v, 3) for k, v in res.items()})
    print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true", help="the kernel workload for rocprofv3 (no timing printed)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    if a.kernels:
        kernels(pkg)
    else:
        wall(pkg, a.out)


if __name__ == "__main__":
    main()
