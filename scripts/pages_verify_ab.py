#!/usr/bin/env python3
"""fastcrc windows of blocks laid out as page lists, and the paged verify at a
call site's size.

Windows.  The blocks' 16 KiB pages sit at a random permutation of a page
pool; fastcrc = 128.  Four arms, alternated within one run -- `--rounds`
rounds of `--launches` launches each after a warm-up, each round timed with
device events on the launch stream:
  A  the only correct route without crc32hip_pages: one gather of the pages
     into a contiguous buffer (a single index_select over the pool, rows
     viewed as int64), then crc32hip_fixed(fastcrc=128)
  B  crc32hip_pages over the pages where they lie
  C  crc32hip_fixed(fastcrc=128) over bytes that are contiguous already: the
     floor
  D  crc32hip_pages over the contiguous bytes taken as pages in address order
     (a reading, not a route: B's kernel and tables on C's placement, so
     D / C is what the table costs and B / D what the scattered placement does)
Two shapes: 1,048,576 x 16 KiB (one page each) and 262,144 x 64 KiB (four
pages each: the tail window's table entry is the chunk's fourth).  Reported
per arm: every round's ms per launch, their median, min and max; A's min-max
spread, whether B's median is below A's by more than that, B / C, D / C and
B / D.  A's, B's and D's values must equal C's over the whole batch in both
shapes.

Call site.  One synchronous verify of 64 blocks of 16 KiB, all values right,
timed on the host clock around the call (it ends when the results are back):
verify_device_pages under MD5 and under CRC-32 with fastcrc = 128, beside
md5_batch_verify_device of the same blocks contiguous.  `--calls` calls an
arm and round, arms alternated; microseconds per call.

Writes profiles/pages_verify/ab.json unless --out names another file.

usage: pages_verify_ab.py [--rounds 7] [--launches 20] [--calls 200] [--out FILE]"""
import argparse
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
F = 128


def stats(v, unit="ms"):
    return {f"rounds_{unit}": [round(x, 4) for x in v], f"median_{unit}": round(float(np.median(v)), 4),
            f"min_{unit}": round(min(v), 4), f"max_{unit}": round(max(v), 4)}


def scattered(n, L):
    """n blocks of L bytes: contiguous, and their pages at a random permutation
    of a pool (page j of the blocks' bytes lies at pool page perm[j])."""
    ppc = L // PAGE
    E = n * ppc
    contig = m.arena_empty(n * L)
    m.fill_synthetic(contig, seed=0xA9E5 + ppc)
    perm = torch.randperm(E, device="cuda", generator=torch.Generator(device="cuda").manual_seed(ppc))
    pool = torch.empty(E * PAGE, dtype=torch.uint8, device="cuda")
    pool.view(torch.int64).view(E, PAGE // 8)[perm] = contig.view(torch.int64).view(E, PAGE // 8)
    return contig, pool, perm


def windows_ab(a, n, L):
    ppc = L // PAGE
    E = n * ppc
    contig, pool, perm = scattered(n, L)
    gathered = torch.empty(E * PAGE, dtype=torch.uint8, device="cuda")
    pool_rows, gath_rows = pool.view(torch.int64).view(E, PAGE // 8), gathered.view(torch.int64).view(E, PAGE // 8)
    pages = pool.data_ptr() + perm * PAGE
    pages_inorder = contig.data_ptr() + torch.arange(E, dtype=torch.int64, device="cuda") * PAGE
    first = torch.arange(n, dtype=torch.int64, device="cuda") * ppc
    lens = torch.full((n,), L, dtype=torch.int32, device="cuda")
    crc = {k: torch.empty(n, dtype=torch.int32, device="cuda") for k in "ABCD"}
    s = torch.cuda.current_stream()

    def arm_a():
        torch.index_select(pool_rows, 0, perm, out=gath_rows)
        m.crc32_fixed(gathered, n, L, fastcrc=F, out=crc["A"])

    def arm_b():
        m.crc32_pages(pages, first, lens, PAGE, F, out=crc["B"])

    def arm_c():
        m.crc32_fixed(contig, n, L, fastcrc=F, out=crc["C"])

    def arm_d():
        m.crc32_pages(pages_inorder, first, lens, PAGE, F, out=crc["D"])

    arms = {"A": arm_a, "B": arm_b, "C": arm_c, "D": arm_d}
    for _ in range(3):                                   # warm-up, every arm
        for f in arms.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for r in range(a.rounds):
        for k in ("ABCD", "BCDA", "CDAB", "DABC")[r % 4]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.launches):
                arms[k]()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    out = {"n": n, "len": L, "page_bytes": PAGE, "pages_per_chunk": ppc, "fastcrc": F, "rounds": a.rounds,
           "launches_per_round": a.launches, "A_gather_then_fixed": stats(ms["A"]),
           "B_crc32_pages": stats(ms["B"]), "C_fixed_contiguous": stats(ms["C"]),
           "D_crc32_pages_in_address_order": stats(ms["D"])}
    ma, mb, mc = out["A_gather_then_fixed"], out["B_crc32_pages"], out["C_fixed_contiguous"]
    out["A_spread_ms"] = round(ma["max_ms"] - ma["min_ms"], 4)
    out["B_over_A_median"] = round(mb["median_ms"] / ma["median_ms"], 4)
    out["B_below_A_by_more_than_A_spread"] = bool(ma["median_ms"] - mb["median_ms"] > out["A_spread_ms"])
    out["B_over_C_median"] = round(mb["median_ms"] / mc["median_ms"], 4)
    md = out["D_crc32_pages_in_address_order"]
    out["D_over_C_median"] = round(md["median_ms"] / mc["median_ms"], 4)
    out["B_over_D_median"] = round(mb["median_ms"] / md["median_ms"], 4)
    out["B_windows_per_us"] = round(2 * n / (mb["median_ms"] * 1e3), 2)
    out["B_equals_C"] = bool(torch.equal(crc["B"], crc["C"]))
    out["A_equals_C"] = bool(torch.equal(crc["A"], crc["C"]))
    out["D_equals_C"] = bool(torch.equal(crc["D"], crc["C"]))
    return out


def call_site(a, n=64, L=16384):
    contig, pool, perm = scattered(n, L)
    torch.cuda.synchronize()
    pages = (pool.data_ptr() + perm.cpu().numpy().astype(np.int64) * PAGE).astype(np.uint64)
    first = np.arange(n + 1, dtype=np.uint64)
    lens = np.full(n, L, dtype=np.uint32)
    ptrs = (contig.data_ptr() + np.arange(n, dtype=np.int64) * L).astype(np.uint64)
    out = {"n": n, "len": L, "calls_per_round": a.calls, "rounds": a.rounds}
    with m.Queue(device=0) as q:
        for name, kind, fast in (("md5", m.Batcher.MD5, 0), ("crc32_fastcrc128", m.Batcher.CRC32, F)):
            q.set_digest(kind, fast)
            want = q.submit_device(ptrs, lens) if fast == 0 else \
                m.crc32_fixed(contig, n, L, fastcrc=F).cpu().numpy().view(np.uint32)
            arms = {"paged": lambda: q.verify_device_pages(pages, first, lens, PAGE, want, after=None),
                    "contiguous": lambda: q.verify_device(ptrs, lens, want, after=None)}
            for f in arms.values():                      # warm-up; every value must be right
                for _ in range(20):
                    ok, nbad = f()
                    assert nbad == 0 and ok.all(), name
            us = {k: [] for k in arms}
            for r in range(a.rounds):
                for k in (("paged", "contiguous"), ("contiguous", "paged"))[r % 2]:
                    t0 = time.perf_counter()
                    for _ in range(a.calls):
                        arms[k]()
                    us[k].append((time.perf_counter() - t0) / a.calls * 1e6)
            out[name] = {"verify_device_pages": stats(us["paged"], "us"), "verify_device": stats(us["contiguous"], "us")}
            out[name]["paged_over_contiguous_median"] = round(
                out[name]["verify_device_pages"]["median_us"] / out[name]["verify_device"]["median_us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "pages_verify", "ab.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("pages_verify_ab.py measures on the GPU: no HIP device is visible")
    out = {"windows": {"one_page_16KiB": windows_ab(a, 1 << 20, 16384)}}
    torch.cuda.empty_cache()
    out["windows"]["four_pages_64KiB"] = windows_ab(a, 1 << 18, 65536)
    torch.cuda.empty_cache()
    out["call_site"] = call_site(a)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    sys.exit(0 if all(v["B_equals_C"] and v["A_equals_C"] and v["D_equals_C"] for v in out["windows"].values()) else 1)


if __name__ == "__main__":
    main()
