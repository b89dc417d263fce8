#!/usr/bin/env python3
"""MD5 + CRC-32 of a small vector of blocks: the throughput kernel of the
one-pass kind against its small-batch kernel and against two launches.

Device legs, per shape (n x len, device-resident, md5hip_fill_synthetic):
  A  md5crc32hip_fixed_variant XDMA16    (md5crc32_fixed_xdma16)
  B  md5crc32hip_fixed_variant FEDSPLIT  (md5crc32_fedsplit)
  C  md5hip_digest_fixed then crc32hip_fixed on one stream
alternated within one run: `--rounds` rounds, the legs in an order that
rotates by one each round, each leg `launches` launches between two device
events on the launch stream (as many as fill ~30 ms of leg A, 3 to 20).
Reported per leg: every round's us per launch, their median, min and max;
per shape md5crc32hip_plan's choice, A's min-max spread, and whether B's
median lies below A's by more than that spread.  Every leg's output over the
whole batch is compared with the oracle (tests/gen.py).

Call site: md5hip_batch_upgrade_iov of 64 x 16 KiB blocks in registered
16 KiB pages, the library before the change (--old, a build of the parent
commit) against the current one, both loaded side by side, each with its own
batcher and its own registered copy of the pages; `--site-calls` synchronous
calls per round, wall clock, rounds alternated.

usage: dual_small_ab.py [--rounds 7] [--old build/ab/libmd5hip_old.so] [--out FILE]"""
import argparse
import ctypes
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
from sproxy_amd import _lib  # noqa: E402
from sproxy_amd import md5 as m  # noqa: E402

SHAPES = [(64, 16384), (1024, 16384), (16384, 16384), (64, 128 << 10), (64, 1 << 20), (1024, 2048), (1024, 1024),
          # around the rule's edges: n = CUs x len / 256 and past it, and below MD5CRC32HIP_FEDSPLIT_MIN_LEN
          (64, 1024), (2048, 2048), (4096, 2048), (16384, 2048), (8192, 8192), (16384, 8192), (16384, 1024),
          (64, 512), (512, 512), (1024, 512), (1024, 256), (1024, 128)]


def stats(v):
    return {"rounds_us": [round(x, 2) for x in v], "median_us": round(float(np.median(v)), 2),
            "min_us": round(min(v), 2), "max_us": round(max(v), 2)}


def shape_ab(n, L, rounds):
    data = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    m.fill_synthetic(data, seed=0xD5 + n + L)
    rec = {k: torch.full((n, 32), 0xAA, dtype=torch.uint8, device="cuda") for k in "AB"}
    md5 = torch.full((n, 16), 0xAA, dtype=torch.uint8, device="cuda")
    crc = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream()

    def leg_c():
        m.digest_fixed(data, n, L, out=md5)
        m.crc32_fixed(data, n, L, out=crc)

    legs = {"A": lambda: m.md5crc32_fixed(data, n, L, out=rec["A"], variant="xdma16"),
            "B": lambda: m.md5crc32_fixed(data, n, L, out=rec["B"], variant="fedsplit"),
            "C": leg_c}

    def timed(k, launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        for _ in range(launches):
            legs[k]()
        e1.record(s)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / launches

    for _ in range(3):                                   # warm-up, every leg
        for k in legs:
            legs[k]()
    torch.cuda.synchronize()
    launches = int(min(20, max(3, round(30e3 / timed("A", 3)))))
    us = {k: [] for k in legs}
    names = list(legs)
    for r in range(rounds):
        for j in range(len(names)):
            k = names[(r + j) % len(names)]
            us[k].append(timed(k, launches))
    out = {"n": n, "len": L, "rounds": rounds, "launches_per_round": launches,
           "plan": m.md5crc32_plan(n, L),
           "A_xdma16": stats(us["A"]), "B_fedsplit": stats(us["B"]), "C_md5_then_crc32": stats(us["C"])}
    a, b, c = out["A_xdma16"], out["B_fedsplit"], out["C_md5_then_crc32"]
    out["A_spread_us"] = round(a["max_us"] - a["min_us"], 2)
    out["B_over_A_median"] = round(b["median_us"] / a["median_us"], 4)
    out["B_over_C_median"] = round(b["median_us"] / c["median_us"], 4)
    out["B_below_A_by_more_than_A_spread"] = bool(a["median_us"] - b["median_us"] > out["A_spread_us"])
    # every leg's whole output against the oracle
    host = data.cpu().numpy()
    offs = np.arange(n, dtype=np.uint64) * L
    wm, wc = gen.oracle_digests(host, offs, [L] * n), gen.oracle_crc32_batch(host, offs, [L] * n)
    ok = {}
    for k in "AB":
        r = rec[k].cpu().numpy()
        gm, gc = m.split_records(r)
        ok[k] = bool(np.array_equal(gm, wm) and np.array_equal(gc, wc) and not r[:, 20:].any())
    ok["C"] = bool(np.array_equal(md5.cpu().numpy(), wm) and
                   np.array_equal(crc.cpu().numpy().view(np.uint32), wc))
    out["oracle_ok"] = ok
    return out


# ---------------------------------------------------------------- the call site, old library against new
vp, u64, u32, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int


def load(path):
    L = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    L.md5hip_batcher_create.argtypes = [ci, u64, u32, ctypes.POINTER(vp)]
    L.md5hip_batcher_destroy.argtypes = [vp]
    L.md5hip_batcher_destroy.restype = None
    L.md5hip_host_register.argtypes = [vp, u64]
    L.md5hip_host_unregister.argtypes = [vp]
    L.md5hip_batch_upgrade_iov.argtypes = [vp, vp, vp, u64, vp, vp, vp]
    return L


class Site:
    """One library's batcher and its registered copy of the 64 x 16 KiB pages."""

    def __init__(self, lib, pages_src, n, L):
        self.lib, self.n = lib, n
        raw = np.empty(n * L + 4096, dtype=np.uint8)
        skip = (-raw.ctypes.data) % 4096
        self.pages = raw[skip:skip + n * L]
        self.pages[:] = pages_src
        self._raw = raw
        rc = lib.md5hip_host_register(self.pages.ctypes.data, n * L)
        assert rc == 0, rc
        self.h = vp()
        rc = lib.md5hip_batcher_create(0, 0, 0, ctypes.byref(self.h))
        assert rc == 0, rc
        self.segs = (_lib.MD5HipIov * n)()
        for i in range(n):
            self.segs[i].base = self.pages.ctypes.data + i * L
            self.segs[i].len = L
        self.first = np.arange(n + 1, dtype=np.uint64)
        self.ok = np.empty(n, dtype=np.uint8)
        self.md5 = np.empty((n, 16), dtype=np.uint8)

    def call(self, want):
        return self.lib.md5hip_batch_upgrade_iov(self.h, self.segs, self.first.ctypes.data, self.n,
                                                 want.ctypes.data, self.ok.ctypes.data, self.md5.ctypes.data)

    def close(self):
        self.lib.md5hip_batcher_destroy(self.h)
        self.lib.md5hip_host_unregister(self.pages.ctypes.data)


def site_ab(old_path, rounds, calls):
    n, L = 64, 16384
    src = gen.xorshift_array(n * L, seed=0x517E)
    offs = np.arange(n, dtype=np.uint64) * L
    wm, wc = gen.oracle_digests(src, offs, [L] * n), gen.oracle_crc32_batch(src, offs, [L] * n)
    want = np.ascontiguousarray(wc, dtype=np.uint32).copy()
    want[5] ^= 1                                          # one stored CRC wrong
    sites = {"old": Site(load(old_path), src, n, L), "new": Site(load(_lib.LIB_PATH), src, n, L)}
    ok = {}
    for k, st in sites.items():
        for _ in range(20):                               # warm-up
            rc = st.call(want)
        ok[k] = bool(rc == 1 and np.array_equal(st.md5, wm) and np.flatnonzero(st.ok == 0).tolist() == [5])
    us = {k: [] for k in sites}
    for r in range(rounds):
        for k in (("old", "new") if r % 2 == 0 else ("new", "old")):
            st = sites[k]
            t0 = time.perf_counter()
            for _ in range(calls):
                st.call(want)
            us[k].append((time.perf_counter() - t0) * 1e6 / calls)
    for st in sites.values():
        st.close()
    o, w = stats(us["old"]), stats(us["new"])
    return {"n": n, "len": L, "rounds": rounds, "calls_per_round": calls, "gather": "default (registered pages)",
            "old_parent_build": o, "new": w, "old_spread_us": round(o["max_us"] - o["min_us"], 2),
            "new_over_old_median": round(w["median_us"] / o["median_us"], 4), "oracle_ok": ok}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--site-calls", type=int, default=200)
    ap.add_argument("--old", default="build/ab/libmd5hip_old.so", help="a build of the parent commit")
    ap.add_argument("--skip-site", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dual_small_ab.py measures on the GPU: no HIP device is visible")
    out = {"min_len": m.MD5CRC32_FEDSPLIT_MIN_LEN, "shapes": []}
    for n, L in SHAPES:
        out["shapes"].append(shape_ab(n, L, a.rounds))
        print(json.dumps(out["shapes"][-1]), flush=True)
    if not a.skip_site:
        out["upgrade_iov_site"] = site_ab(os.path.join(REPO, a.old), a.rounds, a.site_calls)
        print(json.dumps(out["upgrade_iov_site"]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
    ok = all(all(s["oracle_ok"].values()) for s in out["shapes"]) and \
        (a.skip_site or all(out["upgrade_iov_site"]["oracle_ok"].values()))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
