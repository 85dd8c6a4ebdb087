"""What MSMs over an indexed subset of a bound point set buy (te_msm_run_scalars_indexed*): a sparse scalar vector
over a bound set of 2^20 points, given as (index, scalar) pairs, against the way a caller has without them -- te_msm_run_scalars* over
the zero-padded vector -- in the same build and process, alternating.  Densities 1 (the identity index list: the price of the
translation and of 4 more bytes per entry), 1/2, 1/8, 1/64 (sorted random positions); both curves; three shapes:
    lone       host buffers, one call at a time (te_msm_run_scalars_indexed / te_msm_run_scalars): best of 7
    host x4    host buffers, four tickets in flight (te_msm_submit_scalars_indexed / te_msm_submit_scalars): ms per MSM, best of 3 passes
    device x4  device-resident buffers, four tickets in flight (..._indexed_device / te_msm_submit_scalars_device): the same
Timing as bench.py's bases_resident_figures: every shape is warmed first, a pass is `--steps` MSMs so that filling and draining the
pipeline stay a few per cent of it, the host clock stops after the last collect.  The two ways' results are compared once per density.
    python tools/indexed_sparse.py [--log2n 20] [--steps 32] [--out profiles/indexed_subset_sparse.txt]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEPTH = 4


def in_flight(c, submit, steps, want):
    """ms per MSM with DEPTH tickets in flight: best of 3 passes of `steps` MSMs (one warming round first)"""
    for t in [submit() for _ in range(DEPTH)]:
        assert c.collect(t) == want
    passes = []
    for _ in range(3):
        t1 = time.perf_counter()
        tk = []
        for _ in range(steps):
            tk.append(submit())
            if len(tk) >= DEPTH:
                c.collect(tk.pop(0))
        while tk:
            last = c.collect(tk.pop(0))
        passes.append((time.perf_counter() - t1) * 1e3 / steps)
        assert last == want
    return min(passes), max(passes) / min(passes)


def lone(call, want):
    assert call() == want
    ts = []
    for _ in range(7):
        t1 = time.perf_counter()
        r = call()
        ts.append((time.perf_counter() - t1) * 1e3)
    assert r == want
    return min(ts), max(ts) / min(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    n = 1 << a.log2n
    lines = []
    dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
    for curve in (0, 1):
        sb = 32 if curve == 0 else 48
        # independent random points on the Twisted-Edwards curve; the BLS12-377 generator of the harness makes distinct chain points
        pts, _ = pkg.synth_inputs(11, n, fixed_point="random" if curve == 0 else False, scalars=False, curve=curve)
        rng = np.random.default_rng(100 + curve)
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            b = c.bind_points(pts)
            for inv in (1, 2, 8, 64):
                m = n // inv
                idx = np.arange(n, dtype="<u4") if inv == 1 else np.sort(rng.choice(n, size=m, replace=False)).astype("<u4")
                raw = rng.integers(0, 256, size=(m, sb), dtype=np.uint8)
                raw[:, 31] &= 0x0F                                               # below 2^252: every digit form accepts it
                raw[:, 32:] = 0
                padded = np.zeros((n, sb), dtype=np.uint8)
                padded[idx] = raw
                vals, padded = raw.tobytes(), padded.tobytes()
                d_idx, d_vals, d_pad = dev(idx.tobytes()), dev(vals), dev(padded)
                torch.cuda.synchronize()
                want = c.run_scalars(b, padded)
                res = {}
                # the two ways alternate, shape by shape
                res["lone"] = (lone(lambda: c.run_scalars_indexed(b, idx, vals), want), lone(lambda: c.run_scalars(b, padded), want))
                res["host_x4"] = (in_flight(c, lambda: c.submit_scalars_indexed(b, idx, vals), a.steps, want),
                                  in_flight(c, lambda: c.submit_scalars(b, padded), a.steps, want))
                res["device_x4"] = (in_flight(c, lambda: c.submit_scalars_indexed_device(b, d_idx.data_ptr(), d_vals.data_ptr(), m), a.steps, want),
                                    in_flight(c, lambda: c.submit_scalars_device(b, d_pad.data_ptr()), a.steps, want))
                rec = {"curve": "TE" if curve == 0 else "BLS12-377", "bound_points": n, "density": "1/%d" % inv, "m": m,
                       "bytes_over_pcie": {"indexed": m * (sb + 4), "padded": n * sb}}
                for shape, ((ti, si), (tp, sp)) in res.items():
                    rec[shape] = {"indexed_ms": round(ti, 4), "padded_ms": round(tp, 4), "padded_over_indexed": round(tp / ti, 3),
                                  "spread": [round(si, 3), round(sp, 3)]}
                print(json.dumps(rec), flush=True)
                lines.append(json.dumps(rec))
            c.release_points(b)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
