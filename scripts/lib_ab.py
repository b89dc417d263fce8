#!/usr/bin/env python3
"""In-process A/B of two builds of libmd5hip.so on the same device buffers:
OLD (build/ab/libmd5hip_old.so, the library before a change) against NEW
(sproxy_amd/lib/libmd5hip.so).  Both are loaded with ctypes side by side;
every workload runs both, interleaved, and their outputs are compared.

Workloads:
  c2        md5hip_digest_fixed_variant xdma1nt on 1,048,576 x 16 KiB (bench C2)
  ctx       md5hip_update_ctx on 1,048,576 contexts x 16 KiB (bench --config ctx)
  ragged16  md5hip_digest_desc_variant XDMA, netcache blocks packed at 16 B
  ragged16_lines  the same batch under LINES
  crc_fixed, crc_fast128, crc_fast4096, md5crc32_fixed, small_fed  (fixed_more_ab)
  c3k3_balanced, c3k6_balanced  BALANCED on 3 / 6 coalesced C3 batches (bench --config c3 coalesced leg)
  c3_hybrid  HYBRID on one C3 batch
An A/A control is a second copy of the old build: --extra old2=build/ab/libmd5hip_old2.so.
Prints one JSON object (ms per launch, hipEvent, interleaved rounds).
usage: lib_ab.py [--rounds R] [--extra name=path ...]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import bench  # noqa: E402
from sproxy_amd import md5 as m  # noqa: E402

vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int


def load(path):
    L = ctypes.CDLL(path, mode=ctypes.RTLD_LOCAL)
    L.md5hip_update_ctx.argtypes = [vp, vp, vp, u64, vp]
    L.md5hip_init_ctx.argtypes = [vp, u64, vp]
    L.md5hip_digest_desc_variant.argtypes = [vp, vp, vp, vp, u64, vp, vp, ci]
    L.md5hip_digest_fixed_variant.argtypes = [vp, u64, ctypes.c_uint32, u64, vp, vp, ci]
    L.crc32hip_fixed_variant.argtypes = [vp, u64, ctypes.c_uint32, u64, ctypes.c_uint32, vp, vp, ci]
    L.md5crc32hip_fixed.argtypes = [vp, u64, ctypes.c_uint32, u64, vp, vp]
    return L


def batch(K, seed0):
    """K C3 batches (bench.py's lengths) in one arena: (arena, lens, offsets,
    longest-first order, planned variant)."""
    lk = [bench.c3_lens(16 << 30, seed0 + 31 * j) for j in range(K)]
    ok_ = [bench.c3_offsets(x)[0] for x in lk]
    spans = [(bench.c3_offsets(x)[1] + 15) // 16 * 16 for x in lk]
    starts = np.concatenate([[0], np.cumsum(spans)[:-1]])
    big = m.arena_empty(int(sum(spans)))
    m.fill_synthetic(big, seed=0xC3D)
    L = np.concatenate(lk)
    O = np.concatenate([o + s for o, s in zip(ok_, starts)])
    order, var = m.plan_desc(L.astype(np.uint32))
    return big, L, O, order, var


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = f()
    e1.record()
    torch.cuda.synchronize()
    assert rc == 0, rc
    return e0.elapsed_time(e1)


def ab(libs, run, out, rounds):
    """run(lib) -> rc; out() -> tensor to compare; returns ms lists and equality"""
    res = {}
    for name, L in libs.items():
        assert run(L) == 0
        torch.cuda.synchronize()
        res[name] = out().clone()
    eq = all(bool(torch.equal(res["old"], v)) for v in res.values())
    for _ in range(3):                   # clocks settle
        for L in libs.values():
            run(L)
    torch.cuda.synchronize()
    ms = {k: [] for k in libs}
    names = list(libs)
    for r in range(rounds):              # each round starts one build further on: no build
        for j in range(len(names)):      # always runs in the same place of the round
            k = names[(r + j) % len(names)]
            ms[k].append(round(timed(lambda: run(libs[k])), 4))
    return {"ms": ms, "equal": eq, "median_ms": {k: sorted(v)[rounds // 2] for k, v in ms.items()},
            "best_new_vs_old": round(min(ms["old"]) / min(ms["new"]), 4),
            "median_new_vs_old": round(sorted(ms["old"])[rounds // 2] / sorted(ms["new"])[rounds // 2], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--extra", nargs="*", default=[], help="name=path of more builds to compare")
    ap.add_argument("--old", default="build/ab/libmd5hip_old.so", help="the baseline build")
    ap.add_argument("--only", default="", help="comma list of workloads (see the module docstring)")
    a = ap.parse_args()
    only = set(a.only.split(",")) if a.only else None
    libs = {"old": load(os.path.join(REPO, a.old))}
    for extra in a.extra:               # name=path, between old and new
        k, v = extra.split("=", 1)
        libs[k] = load(os.path.join(REPO, v))
    libs["new"] = load(os.path.join(REPO, "sproxy_amd", "lib", "libmd5hip.so"))
    st = torch.cuda.current_stream().cuda_stream
    res = {}

    if only is None or "c2" in only:
        c2_ab(libs, st, res, a.rounds)
    # ctx: 1 M contexts x 16 KiB (one update launch; contexts re-initialised per run)
    if only is None or "ctx" in only:
        ctx_ab(libs, st, res, a.rounds)
    for name, var in (("ragged16", 4), ("ragged16_lines", 7)):
        if only is None or name in only:
            ragged_ab(libs, st, res, a.rounds, name, var)
    if only is None or only & set(FIXED_MORE):
        fixed_more_ab(libs, st, res, a.rounds, only)
    for K, name, var in ((3, "c3k3_balanced", 5), (6, "c3k6_balanced", 5), (1, "c3_hybrid", 3)):
        if only is None or name in only:
            c3_ab(libs, st, res, a.rounds, K, name, var)
    print(json.dumps(res))


def c2_ab(libs, st, res, rounds):
    """C2: 1,048,576 x 16 KiB fixed-length, md5_fixed_xdma1nt (variant 10)"""
    n, L = 1 << 20, 16384
    data = m.arena_empty(n * L)
    m.fill_synthetic(data, seed=0xC2)
    dig = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
    run = lambda Lb: Lb.md5hip_digest_fixed_variant(data.data_ptr(), n, L, L, dig.data_ptr(), st, 10)  # noqa
    res["c2"] = ab(libs, run, lambda: dig, rounds)
    print(json.dumps({"c2": res["c2"]}), flush=True)
    del data, dig
    torch.cuda.empty_cache()


def ctx_ab(libs, st, res, rounds):
    """1 M contexts x 16 KiB (one update launch; contexts re-initialised per run)"""
    n, L = 1 << 20, 16384
    data = torch.empty(n * L, dtype=torch.uint8, device="cuda")
    m.fill_synthetic(data, seed=0xC7)
    ctx = torch.zeros((n, 88), dtype=torch.uint8, device="cuda")
    ptrs = torch.arange(n, dtype=torch.int64, device="cuda") * L + data.data_ptr()
    lens = torch.full((n,), L, dtype=torch.int32, device="cuda")

    def run_ctx(Lb):
        rc = Lb.md5hip_init_ctx(ctx.data_ptr(), n, st)
        return rc or Lb.md5hip_update_ctx(ctx.data_ptr(), ptrs.data_ptr(), lens.data_ptr(), n, st)
    res["ctx"] = ab(libs, run_ctx, lambda: ctx, rounds)
    print(json.dumps({"ctx": res["ctx"]}), flush=True)
    del data, ctx, ptrs, lens
    torch.cuda.empty_cache()


FIXED_MORE = ("crc_fixed", "crc_fast128", "crc_fast4096", "md5crc32_fixed", "small_fed")


def fixed_more_ab(libs, st, res, rounds, only):
    """The other fixed-length kernels on bench.py's 1,048,576 x 16 KiB: whole-chunk
    CRC-32 (crc32_fixed_xdma16), fastcrc 128 (crc32_fast_pipe) and 4096
    (crc32_fast_xdma16), MD5 + CRC-32 records (md5crc32_fixed_xdma16), and a
    4,096-chunk MD5 batch that AUTO sends to fed pairs (md5_desc_fed; 20
    launches per sample, ms per launch)."""
    n, L = 1 << 20, 16384
    data = m.arena_empty(n * L)
    m.fill_synthetic(data, seed=0xC2)
    out = torch.empty((n, 32), dtype=torch.uint8, device="cuda")
    d, o = data.data_ptr(), out.data_ptr()

    def fed20(Lb):
        rc = 0
        for _ in range(20):
            rc = rc or Lb.md5hip_digest_fixed_variant(d, 4096, L, L, o, st, 0)
        return rc
    runs = {"crc_fixed": lambda Lb: Lb.crc32hip_fixed_variant(d, n, L, L, 0, o, st, 0),
            "crc_fast128": lambda Lb: Lb.crc32hip_fixed_variant(d, n, L, L, 128, o, st, 0),
            "crc_fast4096": lambda Lb: Lb.crc32hip_fixed_variant(d, n, L, L, 4096, o, st, 0),
            "md5crc32_fixed": lambda Lb: Lb.md5crc32hip_fixed(d, n, L, L, o, st),
            "small_fed": fed20}
    for name in FIXED_MORE:
        if only is not None and name not in only:
            continue
        out.zero_()
        res[name] = ab(libs, runs[name], lambda: out, rounds)
        if name == "small_fed":
            res[name]["ms"] = {k: [round(x / 20, 5) for x in v] for k, v in res[name]["ms"].items()}
            res[name]["median_ms"] = {k: round(x / 20, 5) for k, x in res[name]["median_ms"].items()}
        print(json.dumps({name: res[name]}), flush=True)
    del data, out
    torch.cuda.empty_cache()


def ragged_ab(libs, st, res, rounds, name="ragged16", var=4):
    """ragged netcache blocks packed at 16 B (descriptor XDMA, or LINES: var 7)"""
    rng = np.random.default_rng(5)
    S, nb = 16384, 983040                       # ~15 GiB
    bl = np.full(nb, S, dtype=np.int64)
    tail = rng.integers(0, 8, nb) == 0
    bl[tail] = rng.integers(1, S, int(tail.sum()))
    offs = np.concatenate([[0], np.cumsum((bl + 15) // 16 * 16)[:-1]]).astype(np.int64)
    arena = m.arena_empty(int(offs[-1] + bl[-1] + 64))
    m.fill_synthetic(arena, seed=0x16)
    order, _ = m.plan_desc(bl.astype(np.uint32))
    dO = torch.from_numpy(offs).cuda()
    dL = torch.from_numpy(bl.astype(np.int32)).cuda()
    dR = torch.from_numpy(order.astype(np.int32)).cuda()
    dig = torch.empty((nb, 16), dtype=torch.uint8, device="cuda")
    run_r = lambda Lb: Lb.md5hip_digest_desc_variant(arena.data_ptr(), dO.data_ptr(), dL.data_ptr(),  # noqa
                                                     dR.data_ptr(), nb, dig.data_ptr(), st, var)
    res[name] = ab(libs, run_r, lambda: dig, rounds)
    print(json.dumps({name: res[name]}), flush=True)
    del arena, dO, dL, dR, dig
    torch.cuda.empty_cache()


def c3_ab(libs, st, res, rounds, K, name, var):
    """K coalesced C3 batches (bench.py's lengths) launched with `var`
    (5 = BALANCED, the queue's choice for coalesced batches; 3 = HYBRID for one)"""
    big, Lk, O, order, _ = batch(K, 1000)
    nk = Lk.size
    dO = torch.from_numpy(O).cuda()
    dL = torch.from_numpy(Lk.astype(np.int32)).cuda()
    dR = torch.from_numpy(order.astype(np.int32)).cuda()
    dig = torch.empty((nk, 16), dtype=torch.uint8, device="cuda")
    run_b = lambda Lb: Lb.md5hip_digest_desc_variant(big.data_ptr(), dO.data_ptr(), dL.data_ptr(),  # noqa
                                                     dR.data_ptr(), nk, dig.data_ptr(), st, var)
    res[name] = ab(libs, run_b, lambda: dig, rounds)
    res[name]["payload_bytes"] = int(Lk.sum())
    print(json.dumps({name: res[name]}), flush=True)
    del big, dO, dL, dR, dig
    torch.cuda.empty_cache()


if __name__ == "__main__":
    sys.exit(main())
