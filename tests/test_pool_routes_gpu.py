"""Every pool route of tests/pool_cases.py, run: each case goes through
md5hip_pool_* on a pool of sproxy_amd.md5.Pool(devices=(0, 0, 0, 0),
slice_bytes=1 << 20, nslots=2) -- a device may be listed more than once, so
one device serves -- and every digest, CRC or 32-byte record is compared bit
for bit with hashlib.md5 and zlib.crc32 of the host bytes (head ^ tail for a
chunk longer than the window).  tests/test_pool_routes.py proves on the CPU
that a case takes the route the table names; this proves the route right at
every part boundary on the device.

Only what does not depend on timing is asserted: the return code of every
call, the digests of every kind, the 0xAA guards before the first and after
the last record of every submission, the pool's counters, the chunks each
device took for one split as a multiset equal to the planned part sizes, even
spreading on the idle pool, the ticket rules, health and failovers.  A device
fails by md5hip_pool_inject_fault, the library's own control: a launch that
really finished is reported as failed, no device fault occurs."""
import ctypes
import hashlib
import zlib

import numpy as np
import pytest

import pool_cases as pc
from sproxy_amd import md5 as m
from sproxy_amd._lib import MD5HipIov, lib

pytestmark = pytest.mark.gpu

CASES = {c.id: c for c in pc.cases() if c.only != "cpu"}
GUARD = 64
SPREAD = [(100 * i, 100) for i in range(4)]


class World:
    """The arena and the references."""

    def __init__(self):
        self.H = pc.arena()
        self._ref = {}

    def want(self, kind, fastcrc, segments):
        """the record of one chunk, given as [(arena offset, length)]"""
        k = (kind, fastcrc, tuple(segments))
        if k not in self._ref:
            b = b"".join(bytes(self.H[o:o + ln]) for o, ln in segments)
            out = b""
            if kind != pc.CRC32:
                out += hashlib.md5(b).digest()
            if kind != pc.MD5:
                whole = fastcrc == 0 or len(b) <= fastcrc          # md5hip.h: 'fastcrc == 0 || len_i <= fastcrc'
                crc = zlib.crc32(b) if whole else zlib.crc32(b[:fastcrc]) ^ zlib.crc32(b[len(b) - fastcrc:])
                out += crc.to_bytes(4, "little")
            self._ref[k] = out.ljust(pc.DSZ[kind], b"\0")
        return self._ref[k]

    def wants(self, kind, fastcrc, chunks):
        return np.frombuffer(b"".join(self.want(kind, fastcrc, c) for c in chunks), dtype=np.uint8)


@pytest.fixture(scope="module")
def world(cuda):
    return World()


def test_the_table_names_its_one_sided_cases():
    table = pc.cases()
    assert sorted(c.id for c in table if c.only == "cpu") == sorted(pc.CPU_ONLY)
    assert sorted(c.id for c in table if c.only == "gpu") == sorted(pc.GPU_ONLY)
    assert sorted(CASES) == sorted(c.id for c in table if c.id not in pc.CPU_ONLY)


class Made:
    """a submission made: its arrays (alive until the case ends), its ticket and what its digests must be"""

    def __init__(self, s, kind, fastcrc, want, keep):
        self.s, self.kind, self.fastcrc, self.want, self.keep = s, kind, fastcrc, want, keep
        self.out = np.full(2 * GUARD + want.size, 0xAA, dtype=np.uint8)
        self.ticket = ctypes.c_uint64(0xdead)

    def check(self, what):
        dsz = pc.DSZ[self.kind]
        have = self.out[GUARD:GUARD + self.want.size].reshape(-1, dsz)
        bad = np.flatnonzero((have != self.want.reshape(-1, dsz)).any(axis=1))
        assert bad.size == 0, f"{what}: chunks {bad[:8].tolist()} ({bad.size} of {self.s.n})"

    def guards(self, what):
        assert (self.out[:GUARD] == 0xAA).all() and (self.out[GUARD + self.want.size:] == 0xAA).all(), \
            f"{what}: written outside its records"


class Run:
    def __init__(self, world, pool, id):
        self.w, self.p, self.h, self.id = world, pool, pool._h, id
        self.kind, self.fastcrc, self.made = pc.MD5, 0, []

    def chunks_taken(self):
        return [self.p.device_stats(g)["chunks"] for g in range(pc.NDEV)]

    def taken(self):
        return [self.p.device_stats(g)["submissions"] for g in range(pc.NDEV)]

    def sources(self, chunks):
        """(ptrs, lens) or (segs, seg_first) for chunks = [[(offset, length)]]"""
        base = self.w.H.ctypes.data
        nseg = sum(len(c) for c in chunks)
        segs, first, at = (MD5HipIov * max(nseg, 1))(), np.zeros(len(chunks) + 1, dtype=np.uint64), 0
        for i, c in enumerate(chunks):
            for o, ln in c:
                segs[at].base, segs[at].len = base + o, ln
                at += 1
            first[i + 1] = at
        return segs, first

    def sub(self, s, k):
        L, what = lib(), f"{self.id}: submission {k}"
        chunks = [s.segments(i) for i in range(s.n)]
        base = self.w.H.ctypes.data
        if s.entry in ("verify", "upgrade"):
            segs, first = self.sources(chunks)
            ok = np.full(s.n, 7, dtype=np.uint8)
            if s.entry == "verify":
                exp = self.w.wants(self.kind, self.fastcrc, chunks).copy()
                if s.bad >= 0:
                    exp[pc.DSZ[self.kind] * s.bad] ^= 1
                rc = L.md5hip_pool_verify_iov(self.h, segs, first.ctypes.data, s.n, exp.ctypes.data, ok.ctypes.data)
            else:
                exp = self.w.wants(pc.CRC32, 0, chunks).copy()
                if s.bad >= 0:
                    exp[4 * s.bad] ^= 1
                md5s = np.zeros((s.n, 16), dtype=np.uint8)
                rc = L.md5hip_pool_upgrade_iov(self.h, segs, first.ctypes.data, s.n, exp.ctypes.data, ok.ctypes.data,
                                               md5s.ctypes.data)
                assert np.array_equal(md5s.reshape(-1), self.w.wants(pc.MD5, 0, chunks)), what
            assert rc == s.rc, f"{what}: {rc}"
            assert ok.tolist() == [int(i != s.bad) for i in range(s.n)], what
            self.made.append(None)
            return
        want = self.w.wants(self.kind, self.fastcrc, chunks)
        before = self.chunks_taken()
        if s.entry == "fixed":
            mk = Made(s, self.kind, self.fastcrc, want, None)
            rc = L.md5hip_pool_host_fixed(self.h, base, s.n, s.chunks[1], s.chunks[2], mk.out.ctypes.data + GUARD)
        elif s.entry == "ptrs":
            ptrs = np.array([base + c[0][0] for c in chunks], dtype=np.uint64)
            lens = np.array(s.lens, dtype=np.uint32)
            mk = Made(s, self.kind, self.fastcrc, want, (ptrs, lens))
            args = (self.h, ptrs.ctypes.data, lens.ctypes.data, s.n, mk.out.ctypes.data + GUARD)
            rc = L.md5hip_pool_submit(*args) if s.sync else L.md5hip_pool_submit_async(*args, ctypes.byref(mk.ticket))
        else:
            segs, first = self.sources(chunks)
            mk = Made(s, self.kind, self.fastcrc, want, (segs, first))
            args = (self.h, segs, first.ctypes.data, s.n, mk.out.ctypes.data + GUARD)
            rc = L.md5hip_pool_submit_iov(*args) if s.sync else \
                L.md5hip_pool_submit_iov_async(*args, ctypes.byref(mk.ticket))
        self.made.append(mk)
        assert rc == s.rc, f"{what}: {rc}"
        if s.sync:
            if rc == 0:
                mk.check(what)
                if s.all_taken():                          # one device submission per part, of the planned sizes
                    got = sorted(a - b for a, b in zip(self.chunks_taken(), before) if a != b)
                    firsts = s.cuts if s.tie else [s.cuts]
                    assert got in [sorted(hi - lo for lo, hi in s.ranges(f)) if s.k > 1 else [s.n] for f in firsts], \
                        f"{what}: devices took {got} chunks"
            return
        t = mk.ticket.value
        if s.ticket() == "0":
            assert t == 0, f"{what}: ticket {t:#x}"
        elif s.ticket() == "w":
            assert t and not t >> 63 and (t & 63) < pc.NDEV, f"{what}: ticket {t:#x}"
        else:
            assert t >> 63, f"{what}: ticket {t:#x}"

    def spread(self, n, mode):
        chunks = [[c] for c in SPREAD]
        s = pc.Sub("ptrs", [ln for _, ln in SPREAD])
        before = self.taken()
        ptrs = np.array([self.w.H.ctypes.data + o for o, _ in SPREAD], dtype=np.uint64)
        lens = np.array(s.lens, dtype=np.uint32)
        for r in range(n):
            mk = Made(s, pc.MD5, 0, self.w.wants(pc.MD5, 0, chunks), None)
            rc = lib().md5hip_pool_submit(self.h, ptrs.ctypes.data, lens.ctypes.data, 4, mk.out.ctypes.data + GUARD)
            assert rc == 0, f"{self.id}: whole submission {r} of {n}: {rc}"
            mk.check(f"{self.id}: whole submission {r} of {n}")
            mk.guards(f"{self.id}: whole submission {r} of {n}")
        counts = [a - b for a, b in zip(self.taken(), before)]
        healthy = [lib().md5hip_pool_device_health(self.h, g) == 0 for g in range(pc.NDEV)]
        if mode in ("even", "healthy"):
            assert all(c == 0 for c, h in zip(counts, healthy) if not h) and sum(counts) == n, f"{self.id}: {counts}"
            if mode == "even":
                assert len({c for c, h in zip(counts, healthy) if h}) == 1, f"{self.id}: {counts}"
        elif mode != "*":
            assert counts == [int(x) for x in mode.split(",")], f"{self.id}: {counts}"

    def step(self, s):
        L, op = lib(), s[0]
        if op == "split":
            assert L.md5hip_pool_set_split(self.h, s[1]) == 0
        elif op == "digest":
            assert L.md5hip_pool_set_digest(self.h, s[1], s[2]) == s[3], f"{self.id}: {s}"
            if s[3] == 0:
                self.kind, self.fastcrc = s[1], s[2]
        elif op == "fault":
            assert L.md5hip_pool_inject_fault(self.h, s[1], s[2]) == 0
        elif op == "kill":
            assert L.md5hip_pool_inject_fault(self.h, s[1], 1) == 0
            self.spread(8, "*")
        elif op in ("wait", "poll", "waitnext"):
            mk = self.made[s[1]]
            t = mk.ticket.value + (op == "waitnext")
            rc = L.md5hip_pool_poll(self.h, t) if op == "poll" else L.md5hip_pool_wait(self.h, t)
            assert rc == s[2], f"{self.id}: {s}: {rc}"
            if op == "wait" and rc == 0:
                mk.check(f"{self.id}: submission {s[1]} after its wait")
        elif op in ("twait", "tpoll"):
            rc = L.md5hip_pool_poll(self.h, s[1]) if op == "tpoll" else L.md5hip_pool_wait(self.h, s[1])
            assert rc == s[2], f"{self.id}: {op} {s[1]:#x}: {rc}"
        elif op == "stats":
            st, h = self.p.stats(), self.p.health()
            got = dict(st, nfailed=h["nfailed"], mask=h["failed_mask"], failovers=h["failovers"])
            want = {k: v for k, v in s[1].items() if v is not None}
            assert {k: got[k] for k in want} == want and h["ndev"] == pc.NDEV, f"{self.id}: {got}"
        elif op == "spread":
            self.spread(s[1], s[2])
        else:
            raise AssertionError(f"{self.id}: step {op} is the fake's")


@pytest.mark.parametrize("id", sorted(CASES))
def test_route(world, id):
    c = CASES[id]
    with m.Pool(devices=(0,) * pc.NDEV, slice_bytes=pc.SLICE, nslots=2) as p:
        run, k = Run(world, p, id), 0
        try:
            for s in c.steps:
                if isinstance(s, pc.Sub):
                    run.sub(s, k)
                    k += 1
                else:
                    run.step(s)
        finally:
            for mk in run.made:                            # nothing may still write when the arrays go
                if mk is not None and not mk.s.sync:
                    lib().md5hip_pool_wait(run.h, mk.ticket.value if mk.ticket.value != 0xdead else 0)
        for k, mk in enumerate(run.made):
            if mk is not None:
                mk.guards(f"{id}: submission {k}")
