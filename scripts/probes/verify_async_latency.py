"""The cache-read verify at the call site, both ways in one process: the
synchronous md5hip_batch_verify_iov (digests to the host, compared there)
against md5hip_batch_verify_iov_async + md5_batch_wait (compared on the
device), 64 x 16 KiB blocks from registered pages, calls alternated, the median
of each.  The device-to-host bytes per call are what the slot's copies carry:
dsz x n digests for the synchronous call, one count per compare range plus one
ok byte per block for the ticket form (md5_submit.c enqueue_digests /
enqueue_verify; counted on the stand-in runtime by tests/c/verify_check.c).

    python scripts/probes/verify_async_latency.py --out profiles/verify_async/latency.json
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

import gen  # noqa: E402
import sproxy_amd.md5 as m  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--block-bytes", type=int, default=16384)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, B = a.blocks, a.block_bytes
    heap = gen.xorshift_array(n * B, seed=77).copy()
    chunks = [[heap[i * B + 4096 * p:i * B + 4096 * (p + 1)] for p in range(B // 4096)] for i in range(n)]   # 4 KiB pages
    offs = [i * B for i in range(n)]
    res = {"blocks": n, "block_bytes": B, "calls": a.calls, "source": "registered pages, 4 KiB segments",
           "what": "median wall time of one call, calls of the two forms alternated in one process", "kinds": {}}
    m.register_host(heap)
    try:
        with m.Batcher(device=0) as b:
            for name, kind, dsz in (("md5", b.MD5, 16), ("crc32", b.CRC32, 4)):
                b.set_digest(kind, 0)
                if kind == b.MD5:
                    exp = gen.oracle_digests(heap, offs, [B] * n)
                else:
                    exp = np.array([zlib.crc32(heap[o:o + B].tobytes()) for o in offs], dtype="<u4").view(np.uint8).reshape(n, 4)
                exp = exp.copy()
                exp[n // 2, 0] ^= 1                         # one mismatch: both forms must find it
                ts, ta = [], []
                for k in range(a.warmup + a.calls):
                    t0 = time.perf_counter()
                    ok_s, bad_s = b.verify_iov(chunks, exp)
                    t1 = time.perf_counter()
                    ok_a, bad_a = b.verify_iov_async(chunks, exp).wait()
                    t2 = time.perf_counter()
                    assert bad_s == 1 and bad_a == 1 and np.array_equal(ok_s, ok_a) and not ok_a[n // 2]
                    if k >= a.warmup:
                        ts.append((t1 - t0) * 1e6)
                        ta.append((t2 - t1) * 1e6)
                q = lambda v, p: sorted(v)[int(p * (len(v) - 1))]   # noqa: E731
                res["kinds"][name] = {
                    "sync_verify_iov_us": {"median": statistics.median(ts), "p10": q(ts, 0.1), "p90": q(ts, 0.9)},
                    "verify_iov_async_wait_us": {"median": statistics.median(ta), "p10": q(ta, 0.1), "p90": q(ta, 0.9)},
                    "d2h_bytes_per_call": {"sync_verify_iov": dsz * n, "verify_iov_async": 8 * ((n + 4095) // 4096) + n},
                }
    finally:
        m.unregister_host(heap)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
