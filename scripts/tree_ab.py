#!/usr/bin/env python3
"""A/B of whole trees for host-side changes (the batcher, the pool): each
workload is run as its own command from every tree given, one tree after the
other, round after round, each round starting one tree further on so that no
tree always runs in the same place of a round (as lib_ab.py does for kernels
in one process).  The trees are checkouts with their own build; `old2`, a
second copy of `old`'s, is the A/A control.

Workloads (--set bench: the first three; --set site: the rest):
  c3q, crcq, c5  bench.py --config ... : the line's value, and `drained`
  asio      scripts/asio_scale.py --matrix threads (the tree's own library
            through LD_LIBRARY_PATH): latency p50 and thread CPU per call at
            8 / 64 / 256 callers, registered and pageable, batcher and pool
  latency   scripts/latency_probe.py: median us per synchronous device call
  submit    scripts/probes/submit_cost.py: the C call's cost per 79 K-chunk
            device submission (reserve_device)
  poollat   scripts/pool_latency_probe.py: median us per synchronous submit
            through a batcher, a pool over one device and one over four

Per figure: every tree's values and median, the old-vs-old2 gap, new against
old (positive = new worse), and whether that is within twice the gap.  Stops
at the first command that fails.  Writes --out (merging into it when it
exists, so the sets may run as separate calls) and prints each run.
--points reruns single points of the asio matrix instead (the same command
asio_scale.py makes for them).
usage: tree_ab.py --tree old=DIR --tree old2=DIR --tree new=DIR [--rounds 5]
                  [--set bench|site] [--only c3q,asio] [--secs 1]
                  [--points pageable:pool:256,...] --out FILE"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

PY = sys.executable
BENCH = ["--gpus", "1", "--steps", "10", "--warmup", "3"]


def last_json(text):
    for line in reversed(text.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise ValueError("no JSON line in the output")


def bench_figs(name):
    def figs(rec, _):
        out = {f"{name}.value": (rec["value"], +1)}
        if "drained" in rec:
            out[f"{name}.drained"] = (rec["drained"]["value"], +1)
        return out
    return figs


def asio_figs(_, tmp):
    out = {}
    with open(tmp) as f:
        res = json.load(f)
    assert res["all_digests_equal_oracle"], "asio_scale: a digest differs from the oracle"
    for r in res["runs"]:
        key = f"asio.{r['mode']}.{r['target']}.T{r['threads']}"
        out[key + ".lat_p50_us"] = (r["lat_us"]["p50"], -1)
        out[key + ".thread_cpu_us"] = (r["thread_cpu_us_per_call"]["mean"], -1)
    return out


def latency_figs(rec, _):
    return {f"latency.{shape}.median_us": (v["product"]["median_us"], -1) for shape, v in rec.items()}


def submit_figs(rec, _):
    return {f"submit.{mode}.c_call_us": (statistics.median(x["c_call"] for x in runs), -1)
            for mode, runs in rec["us_median"].items()}


def poollat_figs(rec, _):
    return {f"poollat.{shape}.{k}.median_us": (v[k]["median_us"], -1)
            for shape, v in rec.items() for k in ("batcher", "pool1", "pool4")}


def point_figs(rec, _):
    assert rec.get("mismatches", 1) == 0, "asio_scale: a digest differs from the oracle"
    key = f"asio.{rec['mode']}.{rec['target']}.T{rec['threads']}"
    return {key + ".lat_p50_us": (rec["lat_us"]["p50"], -1),
            key + ".thread_cpu_us": (rec["thread_cpu_us_per_call"]["mean"], -1)}


def workloads(secs, points=()):
    if points:      # single points of the asio matrix (a rerun): the tree's build/c/asio_scale itself
        return {p: ("site", ["./build/c/asio_scale", p.split(":")[1], p.split(":")[2], "64", "16384", str(secs),
                             p.split(":")[0]], point_figs) for p in points}
    return {
        "c3q": ("bench", [PY, "bench.py", *BENCH, "--config", "c3q"], bench_figs("c3q")),
        "crcq": ("bench", [PY, "bench.py", *BENCH, "--config", "crcq"], bench_figs("crcq")),
        "c5": ("bench", [PY, "bench.py", *BENCH, "--config", "c5"], bench_figs("c5")),
        "asio": ("site", [PY, "scripts/asio_scale.py", "--matrix", "threads", "--secs", str(secs), "--out", "{tmp}"],
                 asio_figs),
        "latency": ("site", [PY, "scripts/latency_probe.py", "--iters", "200"], latency_figs),
        "submit": ("site", [PY, "scripts/probes/submit_cost.py", "--bursts", "8"], submit_figs),
        "poollat": ("site", [PY, "scripts/pool_latency_probe.py", "--iters", "200", "--secs", "0.5"], poollat_figs),
    }


def summarize(fig):
    """fig: {"better": +1|-1, "values": {tree: [..]}} -> medians, gap, verdict"""
    med = {k: statistics.median(v) for k, v in fig["values"].items() if v}
    fig["median"] = med
    if not {"old", "old2", "new"} <= set(med) or not med["old"]:
        return
    fig["aa_gap"] = round(abs(med["old2"] - med["old"]) / med["old"], 5)
    fig["new_worse_by"] = round(-fig["better"] * (med["new"] - med["old"]) / med["old"], 5)
    fig["margin"] = round(2 * fig["aa_gap"], 5)
    fig["within"] = fig["new_worse_by"] <= fig["margin"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", action="append", required=True, help="name=directory (old, old2, new)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--set", choices=["bench", "site", "all"], default="all")
    ap.add_argument("--only", default="", help="comma list of workloads")
    ap.add_argument("--secs", type=float, default=1.0, help="asio: seconds per run")
    ap.add_argument("--points", default="", help="only these points of the asio matrix, as mode:target:threads,...")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per command")
    ap.add_argument("--tag", default="", help="suffix of this call's figures in --out (a rerun)")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    trees = dict(t.split("=", 1) for t in a.tree)
    names = list(trees)
    only = set(a.only.split(",")) if a.only else None
    todo = {k: v for k, v in workloads(a.secs, [p for p in a.points.split(",") if p]).items()
            if (a.set == "all" or v[0] == a.set) and (only is None or k in only)}
    figures = {}
    rc = 0
    for wname, (_, cmd, figs) in todo.items():
        for r in range(a.rounds):
            for j in range(len(names)):
                tree = names[(r + j) % len(names)]
                root = os.path.abspath(trees[tree])
                with tempfile.NamedTemporaryFile(suffix=".json") as tmp:
                    argv = [c.replace("{tmp}", tmp.name) for c in cmd]
                    env = dict(os.environ, LD_LIBRARY_PATH=os.path.join(root, "sproxy_amd", "lib") + ":" +
                               os.environ.get("LD_LIBRARY_PATH", ""))
                    t0 = time.time()
                    try:
                        p = subprocess.run(argv, cwd=root, env=env, capture_output=True, text=True,
                                           timeout=a.timeout)
                        rc, err = p.returncode, p.stderr[-2000:]
                    except subprocess.TimeoutExpired:
                        rc, err = 124, "timed out"
                    if rc == 0:
                        got = figs(last_json(p.stdout) if "{tmp}" not in cmd else None, tmp.name)
                if rc:
                    print(json.dumps({"failed": wname, "tree": tree, "round": r, "exit": rc, "stderr": err}),
                          flush=True)
                    break
                for key, (val, better) in got.items():
                    f = figures.setdefault(key + a.tag, {"better": better, "values": {n: [] for n in names}})
                    f["values"][tree].append(val)
                print(json.dumps({"workload": wname, "tree": tree, "round": r, "run_s": round(time.time() - t0, 1),
                                  **{k: v for k, (v, _) in got.items()}}), flush=True)
            if rc:
                break
        if rc:
            break
    for f in figures.values():
        summarize(f)
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.setdefault("figures", {}).update(figures)
    res["rule"] = ("new may be worse than old by at most twice the old-vs-old2 gap of the same figure "
                   "(medians over the rounds, relative to old)")
    res["outside"] = sorted(k for k, f in res["figures"].items() if f.get("within") is False)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({"figures": len(res["figures"]), "outside": res["outside"]}), flush=True)
    return rc


if __name__ == "__main__":
    sys.exit(main())
