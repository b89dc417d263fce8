#!/usr/bin/env python3
"""Device-resident blocks laid out as page lists: gather-then-hash against
hashing the pages where they lie.

The blocks' 16 KiB pages sit at a random permutation of a page pool.  Three
legs, MD5, alternated within one run -- `--rounds` rounds of `--launches`
launches each after a warm-up, each round timed with device events on the
launch stream:
  A  what a caller has to do without md5hip_digest_pages: one gather of the
     pages into a contiguous buffer (a single index_select over the pool,
     rows viewed as int64), then md5hip_digest_fixed
  B  md5hip_digest_pages over the pages where they lie
  C  md5hip_digest_fixed over bytes that are contiguous already: the floor
Two shapes: 1,048,576 x 16 KiB (one page each: the indirection alone) and
262,144 x 64 KiB (four pages each: the page crossings).
Reported per leg: every round's ms per launch, their median, min and max;
A's min-max spread, whether B's median is below A's by more than that, and
B / C.  B's digests must equal C's over the whole batch in both shapes.

usage: pages_ab.py [--rounds 7] [--launches 20] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
from sproxy_amd import md5 as m  # noqa: E402

PAGE = 16384


def stats(v):
    return {"rounds_ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4),
            "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def shape_ab(a, n, L):
    ppc = L // PAGE                                      # pages per chunk
    E = n * ppc
    contig = m.arena_empty(n * L)
    m.fill_synthetic(contig, seed=0xA9E5 + ppc)
    perm = torch.randperm(E, device="cuda", generator=torch.Generator(device="cuda").manual_seed(ppc))
    pool = torch.empty(E * PAGE, dtype=torch.uint8, device="cuda")
    pool.view(torch.int64).view(E, PAGE // 8)[perm] = contig.view(torch.int64).view(E, PAGE // 8)
    gathered = torch.empty(E * PAGE, dtype=torch.uint8, device="cuda")
    pool_rows, gath_rows = pool.view(torch.int64).view(E, PAGE // 8), gathered.view(torch.int64).view(E, PAGE // 8)
    pages = pool.data_ptr() + perm * PAGE                # page j of the blocks' bytes lies at pool page perm[j]
    first = torch.arange(n, dtype=torch.int64, device="cuda") * ppc
    lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
    dig = {k: torch.empty((n, 16), dtype=torch.uint8, device="cuda") for k in "ABC"}
    s = torch.cuda.current_stream()

    def leg_a():
        torch.index_select(pool_rows, 0, perm, out=gath_rows)
        m.digest_fixed(gathered, n, L, out=dig["A"])

    def leg_b():
        m.digest_pages(m.Batcher.MD5, pages, first, lens, PAGE, out=dig["B"])

    def leg_c():
        m.digest_fixed(contig, n, L, out=dig["C"])

    legs = {"A": leg_a, "B": leg_b, "C": leg_c}
    for _ in range(3):                                   # warm-up, every leg
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for r in range(a.rounds):
        for k in ("ABC", "BCA", "CAB")[r % 3]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.launches):
                legs[k]()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    out = {"n": n, "len": L, "page_bytes": PAGE, "pages_per_chunk": ppc, "rounds": a.rounds,
           "launches_per_round": a.launches, "A_gather_then_fixed": stats(ms["A"]),
           "B_digest_pages": stats(ms["B"]), "C_fixed_contiguous": stats(ms["C"])}
    ma, mb, mc = out["A_gather_then_fixed"], out["B_digest_pages"], out["C_fixed_contiguous"]
    out["A_spread_ms"] = round(ma["max_ms"] - ma["min_ms"], 4)
    out["B_over_A_median"] = round(mb["median_ms"] / ma["median_ms"], 4)
    out["B_below_A_by_more_than_A_spread"] = bool(ma["median_ms"] - mb["median_ms"] > out["A_spread_ms"])
    out["B_over_C_median"] = round(mb["median_ms"] / mc["median_ms"], 4)
    out["B_TBps"] = round(n * L / (mb["median_ms"] * 1e-3) / 1e12, 4)
    out["B_equals_C"] = bool(torch.equal(dig["B"], dig["C"]))
    out["A_equals_C"] = bool(torch.equal(dig["A"], dig["C"]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pages_ab.py measures on the GPU: no HIP device is visible")
    out = {"one_page_16KiB": shape_ab(a, 1 << 20, 16384)}
    torch.cuda.empty_cache()
    out["four_pages_64KiB"] = shape_ab(a, 1 << 18, 65536)
    print(json.dumps(out))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    sys.exit(0 if all(v["B_equals_C"] and v["A_equals_C"] for v in out.values()) else 1)


if __name__ == "__main__":
    main()
