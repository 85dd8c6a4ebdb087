"""Cost of MSMs over narrow scalars (options "scalar_record_bytes" = 8 / 16 and "scalar_bits"; DESIGN.md, "Narrow scalars") against the
best way to run the same vector without them: the values zero-extended into 32-byte records, both options at 0 -- the code every call
ran before the options existed (profiles/narrow_scalars_isa.txt: the wide digit kernels kept their instructions).  One box, one process,
one library; the sides alternate inside every round, three rounds, ranges reported and no means.

Per n in 2^20, 2^16 and width in u64, u128, over a bound point set on the Twisted-Edwards curve:
  padded      32-byte records, options at 0
  narrow          8- / 16-byte records: W = ceil((b + 2) / c0) windows of the size c0 the padded call runs
  narrow_shrunk   the same records with "window_bits" forced to max(4, ceil((b + 2) / W)), the smallest size with that window count --
                  as many accumulated entries, fewer buckets to reduce: the alternative rule the choice of c = c0 was measured against
in three forms: a lone host call (te_msm_run_scalars), four host tickets in flight (te_msm_submit_scalars x 4, then their collects;
reported per MSM) and the device-resident call (te_msm_run_scalars_device).  Every variant's result is compared with the padded one
before anything is timed.

    python tools/narrow_scalars_cost.py [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (1 << 20, 1 << 16)
WIDTHS = ((8, "u64"), (16, "u128"))
ROUNDS = 3
IN_FLIGHT = 4


def narrow_values(n, size):
    import numpy as np
    return np.random.default_rng(n + size).integers(0, 256, size=(n, size), dtype=np.uint8)


def timed(fn, reps):
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    lines = []

    def emit(rec):
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    with pkg.MsmContext((0,)) as c:
        for n in SIZES:
            pts, _ = pkg.synth_inputs(11, n, scalars=False)
            bases = c.bind_points(pts)
            c0, W0 = c.plan(n)
            for size, name in WIDTHS:
                raw = narrow_values(n, size)
                narrow = raw.tobytes()
                padded = np.concatenate([raw, np.zeros((n, 32 - size), dtype=np.uint8)], axis=1).tobytes()
                d_narrow = torch.frombuffer(bytearray(narrow), dtype=torch.uint8).cuda()
                d_padded = torch.frombuffer(bytearray(padded), dtype=torch.uint8).cuda()
                torch.cuda.synchronize()
                W = -(-(8 * size + 2) // c0)
                shrunk = max(4, -(-(8 * size + 2) // W))
                variants = {"padded": (0, 0, padded, d_padded), "narrow": (size, 0, narrow, d_narrow), "narrow_shrunk": (size, shrunk, narrow, d_narrow)}

                def select(v):
                    rec_bytes, wb, host, dev = variants[v]
                    c.set_option("scalar_record_bytes", 0)
                    c.set_option("scalar_bits", 8 * rec_bytes)              # (16-byte records need the width declared first)
                    c.set_option("scalar_record_bytes", rec_bytes)
                    c.set_option("window_bits", wb)
                    return host, dev

                def lone(v):
                    host, _ = select(v)
                    return lambda: c.run_scalars(bases, host)

                def tickets(v):
                    host, _ = select(v)

                    def f():
                        ts = [c.submit_scalars(bases, host) for _ in range(IN_FLIGHT)]
                        return [c.collect(t) for t in ts][-1]
                    return f

                def device(v):
                    _, dev = select(v)
                    return lambda: c.run_scalars_device(bases, dev.data_ptr())

                plans, want = {}, None
                for v in variants:                                          # the same bytes from every variant and form, and a warm-up of every shape
                    got = {lone(v)(), tickets(v)(), device(v)()}
                    plans[v] = c.plan(n)
                    want = want or got
                    if len(got) != 1 or got != want:
                        raise SystemExit("n = %d, %s, %s: results differ" % (n, name, v))
                reps = 20 if n >= 1 << 20 else 60
                forms = (("lone_host_call", lone, 1), ("four_host_tickets_in_flight_per_msm", tickets, IN_FLIGHT), ("device_resident_call", device, 1))
                for form, make, per in forms:
                    rounds = {v: [] for v in variants}
                    for _ in range(ROUNDS):
                        for v in variants:
                            f = make(v)
                            rounds[v].append(round(timed(f, max(1, reps // per)) / per, 4))
                    rec = {"n": n, "scalars": name, "form": form, "unit": "ms per MSM, one entry per round",
                           "plan_c_W": {v: list(plans[v]) for v in variants}, "scalar_bytes": {"padded": 32 * n, "narrow": size * n}}
                    rec.update(rounds)
                    rec["padded_lowest_over_narrow_highest"] = round(min(rounds["padded"]) / max(rounds["narrow"]), 2)
                    rec["narrow_slower_than_padded_in_a_round"] = any(x > y for x, y in zip(rounds["narrow"], rounds["padded"]))
                    rec["narrow_shrunk_lowest_over_narrow_highest"] = round(min(rounds["narrow_shrunk"]) / max(rounds["narrow"]), 2)
                    emit(rec)
                c.set_option("scalar_record_bytes", 0)
                c.set_option("scalar_bits", 0)
                c.set_option("window_bits", 0)
            c.release_points(bases)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
