"""Writes tests/golden/field_ops_wasm_golden.json: what the reference's own field arithmetic (the Aleo WASM behind bulkAddFields,
bulkSubFields, bulkMulFields, bulkDoubleFields, bulkInvertFields, bulkPowFields / bulkPowFields17 and bulkSqrtFields) answers on about
40 cases per op -- data only.  tools/field_golden_wasm.js runs the WASM under node, where the reference tree is present
(TE_REFERENCE_ROOT); tests/test_field_ops_host.py compares te_msm_field_op's arithmetic with the file and needs neither.
usage: TE_REFERENCE_ROOT=<reference tree> python tools/gen_field_golden.py"""
import json
import os
import random
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.model import P  # noqa: E402


def cases():
    rnd = random.Random(0xF1E1D)
    edge = [0, 1, P - 1, P, P + 1]                      # (the reference reads P and P + 1 as 0 and 1)
    vals = edge + [rnd.randrange(P) for _ in range(35)]
    out = []
    for op in ("add", "sub", "mul"):
        others = edge[::-1] + [rnd.randrange(P) for _ in range(35)]
        out += [dict(op=op, a=str(a), b=str(b)) for a, b in zip(vals, others)]
    out += [dict(op="double", a=str(a)) for a in vals]
    out += [dict(op="inv", a=str(a)) for a in vals]                       # 0 and P: recorded as "traps"
    exps = [0, 1, 17, P - 2, P - 1]
    out += [dict(op="pow", a=str(a), b=str(e)) for a in (0, 1, P - 1, vals[5], vals[6]) for e in exps]      # 0^0 among them
    out += [dict(op="pow", a=str(a), b="17") for a in vals[7:22]]
    squares = [0, 1, 3, 4] + [pow(v, 2, P) for v in vals[5:30]]
    out += [dict(op="sqrt", a=str(a)) for a in squares + [11, 11 * 4 % P] + [11 * pow(v, 2, P) % P for v in vals[5:14]]]     # 11: the smallest non-square
    return out


def main():
    with tempfile.TemporaryDirectory() as d:
        src, dst = os.path.join(d, "cases.json"), os.path.join(d, "out.json")
        json.dump(cases(), open(src, "w"))
        subprocess.check_call(["node", os.path.join(ROOT, "tools", "field_golden_wasm.js"), src, dst])
        done = json.load(open(dst))
    path = os.path.join(ROOT, "tests", "golden", "field_ops_wasm_golden.json")
    with open(path, "w") as f:
        json.dump({"source": "Address.*_field* of the reference's Aleo WASM (tools/gen_field_golden.py)", "modulus": str(P), "cases": done}, f, indent=0)
        f.write("\n")
    print(path, len(done), "cases,", sum(c["out"] == "traps" for c in done), "trap")


if __name__ == "__main__":
    main()
