"""Cost of prefix sums and products (te_msm_field_scan_device).  One box, one process, the sides of every comparison
alternating inside every round, three rounds, lowest .. highest reported and no means.  A call is synchronous (it returns with out
complete and the totals on the host), so a host clock around it is the call's time.

  1. call   te_msm_field_scan_device in place, sum and product, with out and totals only, at 1024 x 2^10, 16 x 2^16, 2^20 and 2^24 -- and,
            in the same rounds, its three yardsticks:
              copy   a device copy_ of the bytes the call moves: two reads and a write (one and a half copies), or one read (half a copy)
              mul    te_msm_field_op_device(MUL) over the same n elements: the map kernel's rate for one product an element
              link   the same 32 n bytes down and up over the link from pinned memory: what the call replaces
  2. chunk  the candidates 4, 8 and 16 of TE_MSM_SCAN_CHUNK at 2^20 and 16 x 2^16, sum and product with out, alternating.

    python tools/scan_cost.py [--only call,chunk] [--out FILE]"""
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
CANDIDATES = (4, 8, 16)
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


def random_elements(seed, n):
    import numpy as np
    import torch
    d = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=n * 32, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    return d


def step_call(pkg, c):
    import torch
    for log_n, count in SHAPES:
        n, total = 1 << log_n, count << log_n
        da, fa = random_elements(log_n, total), random_elements(50 + log_n, total)
        src, dst = torch.zeros(32 * total, dtype=torch.uint8, device="cuda"), torch.empty(32 * total, dtype=torch.uint8, device="cuda")
        pin = torch.empty(32 * total, dtype=torch.uint8).pin_memory()

        def scan(op, out):
            return lambda: c.field_scan_device(op, da.data_ptr(), n, count, da.data_ptr() if out else None, exclusive=True)

        def copy_rrw():                                              # two reads and a write: a copy and half a copy
            dst.copy_(src)
            dst[:16 * total].copy_(src[:16 * total])
            torch.cuda.synchronize()

        def copy_r():                                                # one read (and half a write): half a copy
            dst[:16 * total].copy_(src[:16 * total])
            torch.cuda.synchronize()

        def mul():
            c.field_op_device(pkg.FIELD_MUL, fa.data_ptr(), fa.data_ptr(), total, fa.data_ptr())

        def link():
            da.copy_(pin, non_blocking=True)
            pin.copy_(da, non_blocking=True)
            torch.cuda.synchronize()
        reps = 3 if log_n >= 24 else 10
        calls = {"sum": scan(pkg.SCAN_SUM, True), "sum_totals_only": scan(pkg.SCAN_SUM, False), "product": scan(pkg.SCAN_PRODUCT, True),
                 "product_totals_only": scan(pkg.SCAN_PRODUCT, False), "copy_2r1w": copy_rrw, "copy_1r": copy_r, "mul_n": mul, "link_down_up": link}
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                ms[k].append(timed(fn, reps))
        lo = {k: min(v) for k, v in ms.items()}
        rec = {"step": "call", "log_n": log_n, "count": count, "chunk": c.get_option("scan_chunk"), "unit": "ms per call, lowest .. highest of %d rounds" % ROUNDS}
        rec.update({k: spread(v) for k, v in ms.items()})
        rec.update({"sum_over_copy": round(lo["sum"] / lo["copy_2r1w"], 2), "sum_over_mul": round(lo["sum"] / lo["mul_n"], 2),
                    "product_over_copy": round(lo["product"] / lo["copy_2r1w"], 2), "product_over_mul": round(lo["product"] / lo["mul_n"], 2),
                    "sum_totals_over_copy": round(lo["sum_totals_only"] / lo["copy_1r"], 2), "product_totals_over_mul": round(lo["product_totals_only"] / lo["mul_n"], 2),
                    "below_link_in_every_round": all(max(s, p) < l for s, p, l in zip(ms["sum"], ms["product"], ms["link_down_up"])),
                    "scratch_bytes": c.get_option("scan_scratch_bytes")})
        emit(rec)
        del da, fa, src, dst, pin
        torch.cuda.empty_cache()


def step_chunk(pkg, c):
    import torch
    for log_n, count in ((20, 1), (16, 16)):
        n, total = 1 << log_n, count << log_n
        da = random_elements(log_n, total)
        for name, op in (("sum", pkg.SCAN_SUM), ("product", pkg.SCAN_PRODUCT)):
            ms, used = {k: [] for k in CANDIDATES}, {}
            for _ in range(ROUNDS):
                for k in CANDIDATES:
                    os.environ["TE_MSM_SCAN_CHUNK"] = str(k)
                    used[k] = c.get_option("scan_chunk")
                    ms[k].append(timed(lambda: c.field_scan_device(op, da.data_ptr(), n, count, da.data_ptr(), exclusive=True), 10))
            os.environ.pop("TE_MSM_SCAN_CHUNK", None)
            lowest = [min(CANDIDATES, key=lambda k: ms[k][r]) for r in range(ROUNDS)]
            median = {str(k): round(sorted(v)[len(v) // 2], 4) for k, v in ms.items()}
            emit({"step": "chunk", "op": name, "log_n": log_n, "count": count, "unit": "ms per call with out, lowest .. highest of %d rounds" % ROUNDS,
                  "ms": {str(k): spread(v) for k, v in ms.items()}, "every_round": {str(k): [round(x, 4) for x in v] for k, v in ms.items()}, "median": median,
                  "chunk_in_force": {str(k): used[k] for k in CANDIDATES}, "lowest_of_each_round": lowest})
        del da
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="call,chunk")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/scan_cost.py needs a GPU: nothing here is measured without one")
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    emit({"step": "setup", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS})
    only = args.only.split(",")
    with pkg.MsmContext((0,)) as c:
        if "chunk" in only:
            step_chunk(pkg, c)
        if "call" in only:
            step_call(pkg, c)
    if args.out:
        with open(args.out, "w") as f:
            for rec in OUT:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
