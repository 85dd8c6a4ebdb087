"""Cost of input-point validation (option "check_points", te_msm_check_points; DESIGN.md "Input-point validation").
Run under `rocprofv3 --kernel-trace --stats` for the kernel times of k_check_form / k_check_subgroup; prints wall-clock times
of the stand-alone device check and of te_msm_bind_points at levels 0, 1 and 2 as one JSON line.
    python tools/check_points_cost.py [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    res = {}
    for curve, name in ((pkg.CURVE_TE_BLS12, "te"), (pkg.CURVE_BLS12_377_G1, "bls12_377")):
        n = 1 << 20
        pts, _ = pkg.synth_inputs(11, n, scalars=False, curve=curve)
        dp = torch.frombuffer(bytearray(pts), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            for level, m in ((1, n), (2, 1 << 16), (2, n)):
                assert c.check_points_device(dp.data_ptr(), m, level) is None          # warm-up (module load, buffers)
                t = time.perf_counter()
                assert c.check_points_device(dp.data_ptr(), m, level) is None
                res["%s_check_device_l%d_n%d_ms" % (name, level, m)] = (time.perf_counter() - t) * 1e3
            for level in (0, 1, 2):
                c.set_option("check_points", level)
                c.release_points(c.bind_points(pts))
                t = time.perf_counter()
                bs = c.bind_points(pts)
                res["%s_bind_l%d_n%d_ms" % (name, level, n)] = (time.perf_counter() - t) * 1e3
                c.release_points(bs)
    line = json.dumps({k: round(v, 3) for k, v in res.items()})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
