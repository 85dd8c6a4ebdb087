"""Cost of batched MSMs over prefixes of a bound point set (te_msm_run_scalars_batch_device) against the two
existing ways, alternating in one process, device-resident scalars:
    (A) te_msm_submit_scalars_device tickets with zero-padded scalars, up to 8 in flight
    (B) te_msm_submit_device tickets on the point prefix, up to 8 in flight
Shapes: TE 64 x 2^12, 32 x 2^14, 16 x 2^16, 8 x 2^20 and a seeded prover mix over a 2^18 set (2 x 2^18, 6 x 2^16, 12 x 2^14,
24 x 2^10); BLS12-377 the first three and the mix.  Best and spread (max / best) of --reps repeats, ms per call and ms per MSM; the
batch's results are checked against (A) once per shape.
    python tools/batch_msm_cost.py [--reps 5] [--out profiles/batch_msm_cost.txt] [--quick]
    rocprofv3 --kernel-trace --stats -d OUT -o run -- python tools/batch_msm_cost.py --reps 1 --quick   (kernel times, a run of its own)"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes(quick):
    mix = [1 << 18] * 2 + [1 << 16] * 6 + [1 << 14] * 12 + [1 << 10] * 24
    te = [("64x2^12", [1 << 12] * 64), ("32x2^14", [1 << 14] * 32), ("16x2^16", [1 << 16] * 16)]
    if not quick:
        te.append(("8x2^20", [1 << 20] * 8))
    return [(0, name, lens) for name, lens in te + [("mix2^18", mix)]] + [(1, name, lens) for name, lens in te[:3] + [("mix2^18", mix)]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="leave out 8 x 2^20")
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    lines = []
    for curve, name, lens in shapes(a.quick):
        n = max(lens)
        pb, sb = (64, 32) if curve == 0 else (96, 48)
        pts, _ = pkg.synth_inputs(7, n, scalars=False, curve=curve)
        rng = np.random.default_rng(len(lens) * 1000 + curve)
        lens = list(rng.permutation(lens)) if name.startswith("mix") else lens
        lens = [int(x) for x in lens]
        scs = []
        for m, L in enumerate(lens):
            raw = rng.integers(0, 256, size=(L, sb), dtype=np.uint8)
            raw[:, 31] &= 0x0F                                                   # below 2^252: every digit form accepts it
            if sb == 48:
                raw[:, 32:] = 0
            scs.append(raw.tobytes())
        with pkg.MsmContext((0,)) as c:
            c.set_option("curve", curve)
            b = c.bind_points(pts)
            dev = lambda x: torch.frombuffer(bytearray(x), dtype=torch.uint8).cuda()
            d_packed = dev(b"".join(scs))
            d_pad = [dev(s + bytes(sb * (n - L))) for s, L in zip(scs, lens)]
            d_pts = dev(pts)
            torch.cuda.synchronize()

            def run_batch():
                return c.run_scalars_batch_device(b, d_packed.data_ptr(), lens)

            def tickets(submit):
                out, q = [None] * len(lens), []
                for m in range(len(lens)):
                    if len(q) == pkg.WORKSETS:
                        k, t = q.pop(0)
                        out[k] = c.collect(t)
                    q.append((m, submit(m)))
                for k, t in q:
                    out[k] = c.collect(t)
                return out

            run_a = lambda: tickets(lambda m: c.submit_scalars_device(b, d_pad[m].data_ptr()))
            run_b = lambda: tickets(lambda m: c.submit_device(d_pts.data_ptr(), d_pad[m].data_ptr(), lens[m]))
            want = run_a()
            assert run_batch() == want, name
            assert run_b() == want, name
            seqs = c.get_option("batch_sequences")
            t = {"batch": [], "A": [], "B": []}
            for _ in range(a.reps):
                for key, fn in (("batch", run_batch), ("A", run_a), ("B", run_b)):
                    t0 = time.perf_counter()
                    fn()
                    t[key].append((time.perf_counter() - t0) * 1e3)
            c.release_points(b)
        best = {k: min(v) for k, v in t.items()}
        rec = {"curve": "TE" if curve == 0 else "BLS12-377", "shape": name, "count": len(lens), "sum_len": sum(lens), "batch_sequences": seqs,
               "best_ms": {k: round(v, 3) for k, v in best.items()}, "spread": {k: round(max(v) / min(v), 3) for k, v in t.items()},
               "ms_per_msm": {k: round(v / len(lens), 4) for k, v in best.items()},
               "speedup_vs_better_baseline": round(min(best["A"], best["B"]) / best["batch"], 3)}
        print(json.dumps(rec), flush=True)
        lines.append(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
