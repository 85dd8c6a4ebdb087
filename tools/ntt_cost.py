"""Cost of batched NTTs (te_msm_ntt_device).  One box, one process, the sides of every comparison alternating
inside every round, three rounds, lowest .. highest reported and no means.  A call is synchronous (it returns with the output complete),
so a host clock around it is the call's time.

  1. ntt    te_msm_ntt_device, forward and inverse, in place, at 2^10 x 1024, 2^16 x 16, 2^20 and 2^24 -- and, in the same rounds, its
            two yardsticks:
              copy   a device copy_ of the same bytes, times the passes of the plan: the bandwidth floor of the plan
              mul    te_msm_field_op_device(MUL) over n log_n / 2 elements per transform: the butterflies' products at the map kernel's rate
            with the ratio of the call to each (of the lowest times) and which of the two is the larger, i.e. binds.
  2. shift  the same calls with a coset shift (22) at 2^20: what the two extra products per element and the call's table build cost.
  3. link   the host round trip the device form replaces: the same bytes down and up over the link from pinned memory.

    python tools/ntt_cost.py [--only ntt,shift,link] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 3
SHAPES = ((10, 1024), (16, 16), (20, 1), (24, 1))                   # (log_n, count)
OUT = []


def emit(rec):
    print(json.dumps(rec), flush=True)
    OUT.append(rec)


def timed(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) * 1e3 / reps


def spread(v):
    return [round(min(v), 4), round(max(v), 4)]


def passes_of(log_n):
    return 1 if log_n <= 10 else 2 if log_n <= 16 else 3          # csrc/ntt_plan.hpp, passes_for


def random_elements(seed, n):
    import numpy as np
    import torch
    d = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=n * 32, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    return d


def step_ntt(pkg, c, shapes, shift=None, step="ntt"):
    import torch
    for log_n, count in shapes:
        total = count << log_n
        da, src = random_elements(log_n, total), torch.zeros(32 * total, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        m = min(total * log_n // 2, 1 << 27)                        # the butterflies' products (capped: 4 GiB an operand; scaled below)
        fa = random_elements(100 + log_n, min(m, 1 << 24))
        per = min(m, 1 << 24)                                       # MUL calls of at most 2^24 elements, in place
        calls_mul = (m + per - 1) // per
        passes = passes_of(log_n)

        def fwd():
            c.ntt_device(da.data_ptr(), log_n, count, da.data_ptr(), shift=shift)

        def inv():
            c.ntt_device(da.data_ptr(), log_n, count, da.data_ptr(), inverse=True, shift=shift)

        def copy():
            for _ in range(passes):
                dst.copy_(src)
            torch.cuda.synchronize()

        def mul():
            for _ in range(calls_mul):
                c.field_op_device(pkg.FIELD_MUL, fa.data_ptr(), fa.data_ptr(), per, fa.data_ptr())
        reps = 3 if log_n >= 24 else 10
        calls = {"forward": (fwd, reps), "inverse": (inv, reps), "copy_x_passes": (copy, reps), "mul_butterflies": (mul, reps)}
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, (fn, r) in calls.items():
                ms[k].append(timed(fn, r))
        scale = (total * log_n / 2) / (calls_mul * per)             # (1 unless the cap above cut the yardstick short)
        mul_ms = [x * scale for x in ms["mul_butterflies"]]
        lo = {k: min(v) for k, v in ms.items()}
        lo["mul_butterflies"] = min(mul_ms)
        emit({"step": step, "log_n": log_n, "count": count, "passes": passes, "shift": shift, "unit": "ms per call, lowest .. highest of %d rounds" % ROUNDS,
              "forward": spread(ms["forward"]), "inverse": spread(ms["inverse"]), "copy_x_passes": spread(ms["copy_x_passes"]),
              "mul_butterflies": spread(mul_ms), "mul_elements": total * log_n // 2,
              "forward_over_copy": round(lo["forward"] / lo["copy_x_passes"], 2), "forward_over_mul": round(lo["forward"] / lo["mul_butterflies"], 2),
              "inverse_over_copy": round(lo["inverse"] / lo["copy_x_passes"], 2), "inverse_over_mul": round(lo["inverse"] / lo["mul_butterflies"], 2),
              "binds": "mul" if lo["mul_butterflies"] >= lo["copy_x_passes"] else "copy"})
        del da, src, dst, fa
        torch.cuda.empty_cache()


def step_link():
    import torch
    for log_n, count in SHAPES:
        nbytes = 32 * (count << log_n)
        pin = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")

        def trip():
            dev.copy_(pin, non_blocking=True)
            pin.copy_(dev, non_blocking=True)
            torch.cuda.synchronize()
        emit({"step": "link", "log_n": log_n, "count": count, "bytes_each_way": nbytes, "unit": "ms for the same bytes down and up over the link, pinned memory",
              "ms": spread([timed(trip, 3 if log_n >= 24 else 10) for _ in range(ROUNDS)])})
        del pin, dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ntt,shift,link")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/ntt_cost.py needs a GPU: nothing here is measured without one")
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    emit({"step": "setup", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS})
    only = args.only.split(",")
    with pkg.MsmContext((0,)) as c:
        if "ntt" in only:
            step_ntt(pkg, c, SHAPES)
        if "shift" in only:
            step_ntt(pkg, c, ((20, 1),), shift=22, step="shift")
        if "link" in only:
            step_link()
    if args.out:
        with open(args.out, "w") as f:
            for rec in OUT:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
