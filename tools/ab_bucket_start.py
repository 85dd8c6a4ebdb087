"""A/B of k_accumulate's segment start and record ping-pong: bench.py as child processes, alternating, on one box
in one session:
  parent   the build named by --parent (TE_MSM_LIB: the previous commit's libtemsm.so -- every segment starts with a conversion,
           3 + 7 products for its first two entries; the loop rotates one record pair)
  new      this build as it ships (1 + 7 products; two named records per pass)
  before   optional third build (--before: an older commit's libtemsm.so), run first in every round and reported beside the two; the
           verdict stays new against parent
Per round and variant: bench.py's `value` (MSM/s), `latency_ms`, every `configs.*.value` and the accumulation's clock in the timed region.
Then medians, the parent's own spread between rounds, and the verdict by the rule of profiles/convert_once_ab.txt: a gain only if EVERY
round of the new build lies above EVERY round of the parent, and no side config below the parent's lowest round.
python tools/ab_bucket_start.py --parent /path/to/parent/libtemsm.so [--before older.so] [--rounds 3] [--budget seconds] [--out rounds.jsonl]
                                [-- extra bench.py arguments]"""
import argparse, json, os, statistics, subprocess, sys, time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(env, extra, timeout):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, env=env, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        raise SystemExit("bench failed (%d): %s" % (r.returncode, r.stderr[-1500:]))
    return json.loads(lines[-1])


def figures(d):
    cfg = {k: v.get("value") for k, v in (d.get("configs") or {}).items() if isinstance(v, dict) and v.get("value") is not None}
    return {"value": d["value"], "latency_ms": d.get("latency_ms"), "configs": cfg, "parity": d.get("parity"),
            "clock_ghz": (d.get("roofline") or {}).get("timed_region", {}).get("core_clock_ghz")}


if __name__ == "__main__":
    argv, extra = sys.argv[1:], []
    if "--" in argv:
        extra, argv = argv[argv.index("--") + 1:], argv[:argv.index("--")]
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--before", default=None, help="a third, older build, measured in every round as well")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--budget", type=float, default=0.0, help="seconds: no new round starts unless one more of the longest so far still fits (0 = no limit)")
    ap.add_argument("--out", default=None, help="append one JSON line per run (round, variant, bench.py's whole result)")
    ap.add_argument("--timeout", type=int, default=900, help="seconds per bench.py run")
    a = ap.parse_args(argv)
    if not os.path.exists(a.parent):
        raise SystemExit("--parent %s does not exist" % a.parent)
    variants = (("parent", {"TE_MSM_LIB": os.path.abspath(a.parent)}), ("new", {}))
    if a.before:
        if not os.path.exists(a.before):
            raise SystemExit("--before %s does not exist" % a.before)
        variants = (("before", {"TE_MSM_LIB": os.path.abspath(a.before)}),) + variants
    t_start, longest = time.time(), 0.0
    runs = {name: [] for name, _ in variants}
    print("# bench.py %s; %d rounds, parent and new alternating" % (" ".join(extra) or "(default arguments)", a.rounds), flush=True)
    for rnd in range(a.rounds):
        if a.budget and rnd and time.time() - t_start + longest > a.budget:
            print("# budget: %d of %d rounds run" % (rnd, a.rounds), flush=True)
            break
        t_round = time.time()
        for name, env_extra in variants:
            env = dict(os.environ, **env_extra)
            if not env_extra:
                env.pop("TE_MSM_LIB", None)
            d = bench(env, extra, a.timeout)
            f = figures(d)
            runs[name].append(f)
            if a.out:
                with open(a.out, "a") as fh:
                    fh.write(json.dumps({"round": rnd, "variant": name, "result": d}) + "\n")
            print("round %d %-6s %8.1f MSM/s  latency %s ms  clock %s GHz  parity %s  configs %s" % (
                rnd, name, f["value"], "%.4f" % f["latency_ms"] if f["latency_ms"] else "-", "%.3f" % f["clock_ghz"] if f["clock_ghz"] else "-",
                f["parity"], " ".join("%s %.1f" % kv for kv in sorted(f["configs"].items()))), flush=True)
        longest = max(longest, time.time() - t_round)
    pv, nv = [f["value"] for f in runs["parent"]], [f["value"] for f in runs["new"]]
    mp, mn = statistics.median(pv), statistics.median(nv)
    print("# value: parent median %.1f (rounds %.1f .. %.1f, spread %.1f), new median %.1f (rounds %.1f .. %.1f): %+.2f %%" % (
        mp, min(pv), max(pv), max(pv) - min(pv), mn, min(nv), max(nv), 100.0 * (mn / mp - 1.0)))
    if a.before:
        bv = [f["value"] for f in runs["before"]]
        print("# value: before median %.1f (rounds %.1f .. %.1f)" % (statistics.median(bv), min(bv), max(bv)))
    lp, ln = [f["latency_ms"] for f in runs["parent"] if f["latency_ms"]], [f["latency_ms"] for f in runs["new"] if f["latency_ms"]]
    if lp and ln:
        print("# latency_ms: parent median %.4f, new median %.4f" % (statistics.median(lp), statistics.median(ln)))
    separated = min(nv) > max(pv)
    below = []
    for k in sorted(runs["parent"][0]["configs"]):
        cp, cn = [f["configs"][k] for f in runs["parent"] if k in f["configs"]], [f["configs"][k] for f in runs["new"] if k in f["configs"]]
        if not cp or not cn:
            continue
        print("# configs.%s: parent median %.1f (lowest %.1f), new median %.1f (lowest %.1f)" % (k, statistics.median(cp), min(cp), statistics.median(cn), min(cn)))
        if min(cn) < min(cp):
            below.append(k)
    print("# verdict: %s; side configs below the parent's lowest round: %s" % (
        "every round of the new build above every round of the parent" if separated else "NOT separated from the parent's rounds",
        ", ".join(below) or "none"))
