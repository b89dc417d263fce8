#!/usr/bin/env python3
"""MD5 + CRC-32 of the same blocks: two launches against the one-pass kind.

Device (shape C2: 1,048,576 x 16 KiB device-resident, md5hip_fill_synthetic):
  A  md5hip_digest_fixed then crc32hip_fixed on one stream
  B  md5crc32hip_fixed
alternated within one run, `--rounds` rounds of `--launches` launches each
after a warm-up, each round timed with device events on the launch stream.
Reported per side: every round's ms per launch, their median, min and max;
for B the algorithmic bytes n * (len + 32) over the median.  The yardstick
for B is A in the same run.  After timing, 4,096 random chunks plus the first
and the last are checked against the oracle (tests/gen.py), and B's records
against A's digests over the whole batch.

Host (1 GiB of pinned memory through Batcher.host_fixed, 65,536 x 16 KiB):
once under the kind, once as an MD5 call plus a CRC-32 call, alternated;
GiB/s of payload (wall clock around the synchronous calls).

usage: dual_ab.py [--rounds 7] [--launches 20] [--n 1048576] [--len 16384] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import gen  # noqa: E402
from sproxy_amd import md5 as m  # noqa: E402


def stats(v):
    return {"rounds_ms": [round(x, 4) for x in v], "median_ms": round(float(np.median(v)), 4),
            "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def device_ab(a):
    n, L = a.n, a.len
    data = m.arena_empty(n * L)
    m.fill_synthetic(data, seed=0xC2)
    md5 = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    crc = torch.empty(n, dtype=torch.int32, device="cuda")
    rec = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    s = torch.cuda.current_stream()

    def side_a():
        m.digest_fixed(data, n, L, out=md5)
        m.crc32_fixed(data, n, L, out=crc)

    def side_b():
        m.md5crc32_fixed(data, n, L, out=rec)

    sides = {"A": side_a, "B": side_b}
    for _ in range(3):                                   # warm-up, both sides
        side_a()
        side_b()
    torch.cuda.synchronize()
    ms = {"A": [], "B": []}
    for r in range(a.rounds):
        for k in (("A", "B") if r % 2 == 0 else ("B", "A")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(s)
            for _ in range(a.launches):
                sides[k]()
            e1.record(s)
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.launches)
    out = {"n": n, "len": L, "rounds": a.rounds, "launches_per_round": a.launches,
           "A_md5_then_crc32": stats(ms["A"]), "B_md5crc32": stats(ms["B"])}
    ma, mb = out["A_md5_then_crc32"], out["B_md5crc32"]
    out["B_alg_bytes"] = n * (L + 32)
    out["B_alg_TBps"] = round(n * (L + 32) / (mb["median_ms"] * 1e-3) / 1e12, 4)
    out["A_spread_ms"] = round(ma["max_ms"] - ma["min_ms"], 4)
    out["B_over_A_median"] = round(mb["median_ms"] / ma["median_ms"], 4)
    out["B_below_A_by_more_than_A_spread"] = bool(ma["median_ms"] - mb["median_ms"] > out["A_spread_ms"])
    # results: B against A over the whole batch, a sample against the oracle
    gm, gc = rec[:, :16], rec[:, 16:20].contiguous().view(torch.int32).reshape(n)
    out["B_equals_A"] = bool(torch.equal(gm, md5) and torch.equal(gc, crc) and not bool(rec[:, 20:].any()))
    rng = np.random.default_rng(0xAB)
    idx = np.unique(np.concatenate([rng.integers(0, n, 4096), [0, n - 1]]))
    host = data.view(n, L)[torch.from_numpy(idx).cuda()].cpu().numpy().reshape(-1)
    offs = np.arange(idx.size, dtype=np.uint64) * L
    wm, wc = gen.oracle_digests(host, offs, [L] * idx.size), gen.oracle_crc32_batch(host, offs, [L] * idx.size)
    sm, sc = m.split_records(rec[torch.from_numpy(idx).cuda()])
    out["oracle_sample"] = int(idx.size)
    out["oracle_sample_ok"] = bool(np.array_equal(sm, wm) and np.array_equal(sc, wc))
    return out


def host_ab(a):
    n, L = (1 << 30) // a.len, a.len
    pinned = torch.empty(n * L, dtype=torch.uint8).pin_memory()
    dev = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    m.fill_synthetic(dev, seed=0xB05)
    pinned.copy_(dev)
    torch.cuda.synchronize()
    del dev
    src = pinned.numpy()
    B = m.Batcher
    gib = n * L / 2.0**30
    t = {"one_pass": [], "md5_then_crc32": []}
    with B(device=0) as b1, B(device=0) as b2:
        def one_pass():
            b1.set_digest(B.MD5_CRC32)
            return b1.host_fixed(src, n, L)

        def two_calls():
            b2.set_digest(B.MD5)
            d = b2.host_fixed(src, n, L)
            b2.set_digest(B.CRC32)
            return d, b2.host_fixed(src, n, L)

        rec = one_pass()                                 # warm-up
        d, c = two_calls()
        for r in range(a.host_rounds):
            for k, fn in ((("one_pass", one_pass), ("md5_then_crc32", two_calls))[::1 if r % 2 == 0 else -1]):
                t0 = time.perf_counter()
                fn()
                t[k].append(time.perf_counter() - t0)
    gm, gc = m.split_records(rec)
    return {"n": n, "len": L, "payload_GiB": gib,
            "one_pass_GiBps": {"rounds": [round(gib / x, 3) for x in t["one_pass"]],
                               "median": round(gib / float(np.median(t["one_pass"])), 3)},
            "md5_then_crc32_GiBps": {"rounds": [round(gib / x, 3) for x in t["md5_then_crc32"]],
                                     "median": round(gib / float(np.median(t["md5_then_crc32"])), 3)},
            "records_equal_two_calls": bool(np.array_equal(gm, d) and np.array_equal(gc, c))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--len", type=int, default=16384)
    ap.add_argument("--host-rounds", type=int, default=5)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dual_ab.py measures on the GPU: no HIP device is visible")
    out = {"device": device_ab(a)}
    if not a.skip_host:
        out["host_fixed"] = host_ab(a)
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ok = out["device"]["oracle_sample_ok"] and out["device"]["B_equals_A"] and \
        (a.skip_host or out["host_fixed"]["records_equal_two_calls"])
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
