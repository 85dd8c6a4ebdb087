"""Cost of sparse matrix-vector products (te_msm_spmv_device).  One box, one process, the sides of every comparison
alternating inside every round, three rounds, lowest .. highest reported and no means.  A call is synchronous (it returns with out
complete), so a host clock around it is the call's time.

  1. call   te_msm_spmv_device, one vector, at
              r1cs       2^20 x 2^20, 3 random entries a row and the constant's column in every row (4 x 2^20 entries)
              r1cs_t     the same matrix transposed: one row of 2^20 entries, the others short
              banded     2^20 x 2^20, columns r .. r + 3 (the same number of entries)
              rows22     2^22 x 2^22 like r1cs (2^24 entries)
            and, in the same rounds, its three yardsticks:
              copy   a device copy_ that moves the bytes the call moves (72 an entry read -- value, indices, gathered x -- and 32 a row written)
              mul    te_msm_field_op_device(MUL) over nnz elements
              link   32 cols bytes down and 32 rows bytes up over the link from pinned memory: what the call replaces
  2. chunk  the candidates 4, 8 and 16 of TE_MSM_SPMV_CHUNK at r1cs and r1cs_t, alternating.

    python tools/spmv_cost.py [--only call,chunk] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ROUNDS = 3
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


def matrix(kind, log_rows, seed):
    """(rows, cols, row_ptr, col_idx, vals) as numpy arrays: 4 entries a row"""
    import numpy as np
    rng = np.random.default_rng(seed)
    rows = cols = 1 << log_rows
    ptr = np.arange(rows + 1, dtype=np.uint64) * 4
    if kind == "banded":
        col = (np.arange(rows, dtype=np.uint64)[:, None] + np.arange(4, dtype=np.uint64)[None, :]) % cols
    else:
        col = rng.integers(1, cols, size=(rows, 4), dtype=np.uint64)
        col[:, 0] = 0                                                # the constant's column in every row
    vals = rng.integers(0, 256, size=rows * 4 * 32, dtype=np.uint8)
    return rows, cols, ptr.tobytes(), col.astype(np.uint32).tobytes(), vals.tobytes()


def random_elements(seed, n):
    import numpy as np
    import torch
    d = torch.from_numpy(np.random.default_rng(seed).integers(0, 256, size=n * 32, dtype=np.uint8)).cuda()
    torch.cuda.synchronize()
    return d


def step_call(pkg, c, shapes):
    import torch
    for name, kind, log_rows, tr in shapes:
        rows, cols, ptr, col, vals = matrix(kind, log_rows, log_rows)
        nnz = 4 * rows
        t0 = time.perf_counter()
        mat = c.bind_matrix(rows, cols, ptr, col, vals, transpose=tr)
        bind_s = time.perf_counter() - t0
        del ptr, col, vals
        dx, dout, fa = random_elements(1, cols), torch.zeros(32 * rows, dtype=torch.uint8, device="cuda"), random_elements(2, nnz)
        moved = 72 * nnz + 32 * rows
        src, dst = torch.zeros(moved // 2, dtype=torch.uint8, device="cuda"), torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
        pin_x, pin_o = torch.empty(32 * cols, dtype=torch.uint8).pin_memory(), torch.empty(32 * rows, dtype=torch.uint8).pin_memory()

        def call():
            c.spmv_device(mat, dx.data_ptr(), 1, dout.data_ptr(), transpose=tr)

        def copy():
            dst.copy_(src)
            torch.cuda.synchronize()

        def mul():
            c.field_op_device(pkg.FIELD_MUL, fa.data_ptr(), fa.data_ptr(), nnz, fa.data_ptr())

        def link():
            dx.copy_(pin_x, non_blocking=True)
            pin_o.copy_(dout, non_blocking=True)
            torch.cuda.synchronize()
        reps = 3 if log_rows >= 22 else 10
        calls = {"spmv": call, "copy_moved_bytes": copy, "mul_nnz": mul, "link_down_up": link}
        ms = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, fn in calls.items():
                ms[k].append(timed(fn, reps))
        lo = {k: min(v) for k, v in ms.items()}
        rec = {"step": "call", "shape": name, "rows": rows, "cols": cols, "nnz": nnz, "transpose": tr, "chunk": c.get_option("spmv_chunk"),
               "unit": "ms per call, lowest .. highest of %d rounds" % ROUNDS, "bind_seconds": round(bind_s, 2)}
        rec.update({k: spread(v) for k, v in ms.items()})
        rec.update({"spmv_over_copy": round(lo["spmv"] / lo["copy_moved_bytes"], 2), "spmv_over_mul": round(lo["spmv"] / lo["mul_nnz"], 2),
                    "spmv_below_link_in_every_round": all(a < b for a, b in zip(ms["spmv"], ms["link_down_up"])),
                    "matrix_bytes": c.get_option("matrix_bytes"), "scratch_bytes": c.get_option("spmv_scratch_bytes")})
        emit(rec)
        mat.release()
        del dx, dout, fa, src, dst, pin_x, pin_o
        torch.cuda.empty_cache()


def step_chunk(pkg, c):
    import torch
    rows, cols, ptr, col, vals = matrix("r1cs", 20, 20)
    mat = c.bind_matrix(rows, cols, ptr, col, vals, transpose=True)
    dx, dout = random_elements(1, cols), torch.zeros(32 * rows, dtype=torch.uint8, device="cuda")
    for tr in (False, True):
        ms, used = {k: [] for k in CANDIDATES}, {}
        for _ in range(ROUNDS):
            for k in CANDIDATES:
                os.environ["TE_MSM_SPMV_CHUNK"] = str(k)
                used[k] = c.get_option("spmv_chunk")
                ms[k].append(timed(lambda: c.spmv_device(mat, dx.data_ptr(), 1, dout.data_ptr(), transpose=tr), 10))
        os.environ.pop("TE_MSM_SPMV_CHUNK", None)
        lowest = [min(CANDIDATES, key=lambda k: ms[k][r]) for r in range(ROUNDS)]
        emit({"step": "chunk", "shape": "r1cs_t" if tr else "r1cs", "unit": "ms per call, lowest .. highest of %d rounds" % ROUNDS,
              "ms": {str(k): spread(v) for k, v in ms.items()}, "every_round": {str(k): [round(x, 4) for x in v] for k, v in ms.items()},
              "chunk_in_force": {str(k): used[k] for k in CANDIDATES}, "lowest_of_each_round": lowest})
    mat.release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="chunk,call")
    ap.add_argument("--shapes", default="r1cs,r1cs_t,banded,rows22")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/spmv_cost.py needs a GPU: nothing here is measured without one")
    pkg = importlib.import_module("webgpu-msm-twisted-edwards_amd")
    emit({"step": "setup", "device": torch.cuda.get_device_name(0), "rounds": ROUNDS})
    only = args.only.split(",")
    every = {"r1cs": ("r1cs", "r1cs", 20, False), "r1cs_t": ("r1cs_t", "r1cs", 20, True), "banded": ("banded", "banded", 20, False), "rows22": ("rows22", "r1cs", 22, False)}
    with pkg.MsmContext((0,)) as c:
        if "chunk" in only:
            step_chunk(pkg, c)
        if "call" in only:
            step_call(pkg, c, [every[s] for s in args.shapes.split(",")])
    if args.out:
        with open(args.out, "w") as f:
            for rec in OUT:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
