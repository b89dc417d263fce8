#!/usr/bin/env python3
"""Batched MD5Update over blocks laid out as page lists, against the gather a
caller needs without it and against contiguous bytes.

Rate.  One context per block; the blocks' 16 KiB pages sit at a random
permutation of a page pool; no context has pending bytes (every update is a
whole number of pages).  Three arms, each with contexts of its own, alternated
within one run -- `--rounds` rounds of `--launches` launches each after a
warm-up, each round timed with device events on the launch stream:
  A  the only route without md5hip_update_ctx_pages: one gather of the pages
     into a contiguous buffer (a single index_select over the pool, rows
     viewed as int64), then md5hip_update_ctx
  B  md5hip_update_ctx_pages over the pages where they lie
  C  md5hip_update_ctx over bytes that are contiguous already: the floor
Two shapes: 1,048,576 contexts x 16 KiB (one page an update) and 262,144 x
64 KiB (four pages an update).  Reported per arm: every round's ms per launch,
their median, min and max; A's min-max spread, whether B's median is below A's
by more than that, B / A, B / C and B's rate.  Every arm makes the same number
of updates, so after each shape a copy of each arm's contexts is finalised:
A's, B's and C's digests must be equal over the whole batch, and those of the
first contexts equal hashlib.md5 of the block repeated once per update.

Call site.  One synchronous update of 64 contexts x 16 KiB, timed on the host
clock around the call and the synchronise behind it: the paged entry beside
md5hip_update_ctx over the same blocks contiguous (which runs fed pairs at
this size).  `--calls` calls an arm and round, arms alternated; microseconds
per call.

Writes profiles/ctx_pages/ab.json unless --out names another file.

usage: ctx_pages_ab.py [--rounds 7] [--launches 20] [--calls 200] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from sproxy_amd import md5 as m  # noqa: E402

PAGE = 16384
WARMUP = 3


def stats(v, unit="ms"):
    return {f"rounds_{unit}": [round(x, 4) for x in v], f"median_{unit}": round(float(np.median(v)), 4),
            f"min_{unit}": round(min(v), 4), f"max_{unit}": round(max(v), 4)}


def scattered(n, L):
    """n blocks of L bytes: contiguous, and their pages at a random permutation
    of a pool (page j of the blocks' bytes lies at pool page perm[j])."""
    ppc = L // PAGE
    E = n * ppc
    contig = m.arena_empty(n * L)
    m.fill_synthetic(contig, seed=0xC7A5 + ppc)
    perm = torch.randperm(E, device="cuda", generator=torch.Generator(device="cuda").manual_seed(ppc))
    pool = torch.empty(E * PAGE, dtype=torch.uint8, device="cuda")
    pool.view(torch.int64).view(E, PAGE // 8)[perm] = contig.view(torch.int64).view(E, PAGE // 8)
    return contig, pool, perm


def fresh(n):
    return m.init_ctx(torch.zeros((n, 88), dtype=torch.uint8, device="cuda"))


def rate_ab(a, n, L):
    ppc = L // PAGE
    E = n * ppc
    contig, pool, perm = scattered(n, L)
    gathered = torch.empty(E * PAGE, dtype=torch.uint8, device="cuda")
    pool_rows, gath_rows = pool.view(torch.int64).view(E, PAGE // 8), gathered.view(torch.int64).view(E, PAGE // 8)
    pages = pool.data_ptr() + perm * PAGE
    first = torch.arange(n, dtype=torch.int64, device="cuda") * ppc
    lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
    step = torch.arange(n, dtype=torch.int64, device="cuda") * L
    ptrs_gathered, ptrs_contig = gathered.data_ptr() + step, contig.data_ptr() + step
    ctx = {k: fresh(n) for k in "ABC"}
    s = torch.cuda.current_stream()

    def arm_a():
        torch.index_select(pool_rows, 0, perm, out=gath_rows)
        m.update_ctx(ctx["A"], ptrs_gathered, lens)

    def arm_b():
        m.update_ctx_pages(ctx["B"], pages, first, lens, PAGE)

    def arm_c():
        m.update_ctx(ctx["C"], ptrs_contig, lens)

    arms = {"A": arm_a, "B": arm_b, "C": arm_c}
    for _ in range(WARMUP):                              # warm-up, every arm
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for r in range(a.rounds):
        for k in ("ABC", "BCA", "CAB")[r % 3]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.launches):
                arms[k]()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    updates = WARMUP + a.rounds * a.launches
    out = {"n": n, "len": L, "page_bytes": PAGE, "pages_per_update": ppc, "rounds": a.rounds,
           "launches_per_round": a.launches, "updates_per_context": updates,
           "A_gather_then_update_ctx": stats(ms["A"]), "B_update_ctx_pages": stats(ms["B"]),
           "C_update_ctx_contiguous": stats(ms["C"])}
    ma, mb, mc = out["A_gather_then_update_ctx"], out["B_update_ctx_pages"], out["C_update_ctx_contiguous"]
    out["A_spread_ms"] = round(ma["max_ms"] - ma["min_ms"], 4)
    out["B_over_A_median"] = round(mb["median_ms"] / ma["median_ms"], 4)
    out["B_below_A_by_more_than_A_spread"] = bool(ma["median_ms"] - mb["median_ms"] > out["A_spread_ms"])
    out["B_over_C_median"] = round(mb["median_ms"] / mc["median_ms"], 4)
    out["B_over_C_rounds"] = [round(x / y, 4) for x, y in zip(ms["B"], ms["C"])]
    out["B_GiB_per_s"] = round(n * L / 2**30 / (mb["median_ms"] * 1e-3), 1)
    out["C_GiB_per_s"] = round(n * L / 2**30 / (mc["median_ms"] * 1e-3), 1)
    dig = {k: m.final_ctx(ctx[k].clone()) for k in arms}
    torch.cuda.synchronize()
    out["B_equals_C"] = bool(torch.equal(dig["B"], dig["C"]))
    out["A_equals_C"] = bool(torch.equal(dig["A"], dig["C"]))
    k = 8
    head = contig[:k * L].cpu().numpy().reshape(k, L)
    want = np.array([np.frombuffer(hashlib.md5(bytes(row) * updates).digest(), np.uint8) for row in head])
    out["C_equals_hashlib_first_8"] = bool(np.array_equal(dig["C"][:k].cpu().numpy(), want))
    return out


def call_site(a, n=64, L=16384):
    contig, pool, perm = scattered(n, L)
    pages = pool.data_ptr() + perm * PAGE
    first = torch.arange(n, dtype=torch.int64, device="cuda")
    lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
    ptrs = contig.data_ptr() + torch.arange(n, dtype=torch.int64, device="cuda") * L
    ctx = {"paged": fresh(n), "contiguous": fresh(n)}
    torch.cuda.synchronize()

    def paged():
        m.update_ctx_pages(ctx["paged"], pages, first, lens, PAGE)
        torch.cuda.synchronize()

    def contiguous():
        m.update_ctx(ctx["contiguous"], ptrs, lens)
        torch.cuda.synchronize()

    arms = {"paged": paged, "contiguous": contiguous}
    for f in arms.values():                              # warm-up
        for _ in range(20):
            f()
    us = {k: [] for k in arms}
    for r in range(a.rounds):
        for k in (("paged", "contiguous"), ("contiguous", "paged"))[r % 2]:
            t0 = time.perf_counter()
            for _ in range(a.calls):
                arms[k]()
            us[k].append((time.perf_counter() - t0) / a.calls * 1e6)
    out = {"n": n, "len": L, "calls_per_round": a.calls, "rounds": a.rounds,
           "update_ctx_pages": stats(us["paged"], "us"), "update_ctx_fed_pairs": stats(us["contiguous"], "us")}
    out["paged_over_contiguous_median"] = round(out["update_ctx_pages"]["median_us"] /
                                                out["update_ctx_fed_pairs"]["median_us"], 4)
    out["paged_equals_contiguous"] = bool(torch.equal(m.final_ctx(ctx["paged"]), m.final_ctx(ctx["contiguous"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ctx_pages", "ab.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ctx_pages_ab.py measures on the GPU: no HIP device is visible")
    out = {"rate": {"one_page_16KiB": rate_ab(a, 1 << 20, 16384)}}
    torch.cuda.empty_cache()
    out["rate"]["four_pages_64KiB"] = rate_ab(a, 1 << 18, 65536)
    torch.cuda.empty_cache()
    out["call_site"] = call_site(a)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    right = all(v["B_equals_C"] and v["A_equals_C"] and v["C_equals_hashlib_first_8"] for v in out["rate"].values())
    sys.exit(0 if right and out["call_site"]["paged_equals_contiguous"] else 1)


if __name__ == "__main__":
    main()
