"""Cost of batch scalar multiplication (te_msm_mul[_device], te_msm_mul_x).
Two runs, as profiles/scalar_mul_cost.txt records them:
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/scalar_mul_cost.py --kernels
        k_scalar_mul (per-point and shared scalars) and k_scalar_mul_affine at 2^16 and 2^20 for both curves (device buffers, a few
        repetitions each), and k_check_subgroup of the same curve at 2^20 as the yardstick; the kernel times come from rocprofv3's stats
    python tools/scalar_mul_cost.py [--out FILE]
        wall-clock times (profiler off) of mul (both modes) and mul_x with host buffers at 2^20, both curves, one JSON line"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rand_scalars(n, sb):
    """n random 256-bit scalars in records of sb bytes (the top 16 bytes of a 48-byte record zero)"""
    import numpy as np
    raw = np.random.default_rng(n).integers(0, 256, size=(n, 32), dtype=np.uint8)
    if sb == 48:
        raw = np.concatenate([raw, np.zeros((n, 16), dtype=np.uint8)], axis=1)
    return raw.tobytes()


def kernels(pkg):
    import torch
    for curve in (pkg.CURVE_TE_BLS12, pkg.CURVE_BLS12_377_G1):
        pb, sb = (96, 48) if curve == pkg.CURVE_BLS12_377_G1 else (64, 32)
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            for n in (1 << 16, 1 << 20):
                pts, _ = pkg.synth_inputs(11, n, scalars=False, curve=curve)
                sc = rand_scalars(n, sb)
                dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
                ds = torch.frombuffer(bytearray(sc), dtype=torch.uint8).cuda()
                dout = torch.empty(pb * n, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                for shared in (False, True):
                    for _ in range(4):
                        c.mul_device(dp.data_ptr(), ds.data_ptr(), n, dout.data_ptr(), shared=shared)
                assert bytes(dout.cpu().numpy()[:pb]) == c.mul(pts[:pb], sc[:sb])
                if n == 1 << 20:
                    for _ in range(4):
                        assert c.check_points_device(dp.data_ptr(), n, 2) is None
    print("kernels done")


def wall(pkg, out):
    res = {}
    for curve, name in ((pkg.CURVE_TE_BLS12, "te"), (pkg.CURVE_BLS12_377_G1, "bls12_377")):
        n = 1 << 20
        pb, sb, xb = (96, 48, 48) if curve == pkg.CURVE_BLS12_377_G1 else (64, 32, 32)
        pts, _ = pkg.synth_inputs(12, n, scalars=False, curve=curve)
        sc = rand_scalars(n, sb)
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            xs = None
            if curve == pkg.CURVE_TE_BLS12:
                import numpy as np
                xs = np.frombuffer(pts, dtype=np.uint8).reshape(-1, pb)[:, :xb].copy().tobytes()
                assert c.mul_x(xs, sc) == c.mul(pts, sc)                       # warm-up, and the same answer
            else:
                c.mul(pts, sc)
            calls = [("mul", lambda: c.mul(pts, sc)), ("mul_shared", lambda: c.mul(pts, sc[:sb])),
                     ("run", lambda: c.run(pts, (1).to_bytes(sb, "little") * n))]
            if xs is not None:
                calls.append(("mul_x", lambda: c.mul_x(xs, sc)))
            for key, fn in calls:
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
