"""Every slot route of the batcher, run: each case of tests/slot_cases.py goes
through sproxy_amd.md5 on the device with the same creation arguments, digest
kind, window, gather mode, registered ranges and submissions, and every
digest, CRC or 32-byte record is compared bit for bit with hashlib.md5 and
zlib.crc32 of the host copy (head ^ tail for a chunk longer than the window).
tests/test_slot_routes.py proves on the CPU that a case takes the route the
table names; this proves the route right at its edge.

Device outputs lie in one 0xAA arena: after a case every byte outside the
submissions' own records must still be 0xAA.  The counters are the table's.
A coalesced case queues behind one 8 MiB chain at in-flight target 1, as
test_queue_coalesces_pending_submissions does; its counters show that its
submissions did share one launch.  `gather_shapes` adds what the table alone
would not give the gather kernel: every source residue of 16, destinations on
and off 16 B, lengths around 16 B and around one unrolled trip."""
import hashlib
import zlib

import numpy as np
import pytest
import torch

import gen
import slot_cases as sc
from sproxy_amd import md5 as m

pytestmark = pytest.mark.gpu

CASES = {c.id: c for c in sc.cases() if c.only != "cpu"}


class World:
    """The arenas and the references."""

    def __init__(self, cuda):
        self.cuda = cuda
        raw = np.empty(sc.H_BYTES + sc.PAGE, dtype=np.uint8)
        skew = -raw.ctypes.data % sc.PAGE
        self.H = raw[skew:skew + sc.H_BYTES]
        self.H[:] = gen.xorshift_array(sc.H_BYTES, seed=0x5107)
        self.Dh = gen.xorshift_array(sc.D_BYTES, seed=0x5108)
        self.D = torch.from_numpy(self.Dh).to(cuda)
        self.O = torch.empty(sc.O_BYTES, dtype=torch.uint8, device=cuda)
        self._ref = {}

    def want(self, kind, fastcrc, pieces):
        """the digest of one chunk, given as [(arena, offset, length)]"""
        k = (kind, fastcrc, tuple(pieces))
        if k not in self._ref:
            b = b"".join(bytes((self.H if a == "H" else self.Dh)[o:o + ln]) for a, o, ln in pieces)
            out = b""
            if kind != sc.CRC32:
                out += hashlib.md5(b).digest()
            if kind != sc.MD5:
                whole = fastcrc == 0 or len(b) <= fastcrc          # md5hip.h: 'fastcrc == 0 || len_i <= fastcrc'
                crc = zlib.crc32(b) if whole else zlib.crc32(b[:fastcrc]) ^ zlib.crc32(b[len(b) - fastcrc:])
                out += crc.to_bytes(4, "little")
            self._ref[k] = out.ljust(sc.DSZ[kind], b"\0")
        return self._ref[k]


@pytest.fixture(scope="module")
def world(cuda):
    return World(cuda)


def test_the_table_names_its_one_sided_cases():
    table = sc.cases()
    assert sorted(c.id for c in table if c.only == "cpu") == sorted(sc.CPU_ONLY)
    assert sorted(c.id for c in table if c.only == "gpu") == sorted(sc.GPU_ONLY)
    assert sorted(CASES) == sorted(c.id for c in table if c.id not in sc.CPU_ONLY)


def _submit(w, b, s, dsz, sync):
    """submission `s`: (pending or None, result or None)"""
    out = None if s.out == "h" else w.O[s.out:s.out + dsz * s.n]
    if s.entry == "ptrs":
        bufs = [w.H[o:o + ln] for o, ln in s.chunks]
        return (None, b.submit(bufs)) if sync else (b.submit_async(bufs), None)
    if s.entry == "iov":
        segs = [[w.H[o:o + ln] for o, ln in c] for c in s.chunks]
        return (None, b.submit_iov(segs)) if sync else (b.submit_iov_async(segs), None)
    if s.entry == "dev":
        ptrs = np.array([w.D.data_ptr() + o for o, _ in s.chunks], dtype=np.uint64)
        lens = np.array([ln for _, ln in s.chunks], dtype=np.uint32)
        if sync:
            return None, b.submit_device(ptrs, lens, out=out, after=None)
        return b.submit_device_async(ptrs, lens, out=out, after=None), None
    base, n, length, stride = s.fixed
    if s.entry == "hostfixed":
        return None, b.host_fixed(w.H[base:], n, length, stride)
    return b.submit_device_fixed_async(w.D[base:], n, length, stride, out=out, after=None), None


@pytest.mark.parametrize("id", sorted(CASES))
def test_route(world, id):
    w, c = world, CASES[id]
    dsz = sc.DSZ[c.kind]
    w.O.fill_(0xAA)
    torch.cuda.synchronize()
    how, a, nslots = c.create
    b = m.Batcher(0, a, nslots) if how == "B" else m.Queue(0, a, nslots)
    regs = []
    try:
        if c.kind != sc.MD5 or c.fastcrc:
            b.set_digest(c.kind, c.fastcrc)
        if c.gather is not None:
            b.set_gather(c.gather)
        for off, nbytes in c.regs:
            m.register_host(w.H[off:off + nbytes])
            regs.append(w.H[off:off + nbytes])
        subs = list(c.subs)
        if c.coalesced:
            b.set_inflight(1)
            subs.insert(0, sc.Sub("dev", [sc.BLOCKER]))
        done = [_submit(w, b, s, dsz, not c.coalesced) for s in subs]
        got = [r if p is None else p.wait() for p, r in done]
        st = b.stats()
    finally:
        b.close()
        for r in regs:
            m.unregister_host(r)
    torch.cuda.synchronize()
    O = w.O.cpu().numpy()
    ours = np.zeros(sc.O_BYTES, dtype=bool)
    for s, g in zip(subs, got):
        want = np.frombuffer(b"".join(w.want(c.kind, c.fastcrc, s.pieces(i)) for i in range(s.n)),
                             dtype=np.uint8).reshape(s.n, dsz)
        if s.out == "h":
            have = np.ascontiguousarray(g).view(np.uint8).reshape(s.n, dsz)
        else:
            have = O[s.out:s.out + dsz * s.n].reshape(s.n, dsz)
            ours[s.out:s.out + dsz * s.n] = True
        bad = np.flatnonzero((have != want).any(axis=1))
        assert bad.size == 0, f"{id}: chunks {bad[:8].tolist()} ({bad.size} of {s.n}) of a {s.entry} submission"
    hurt = np.flatnonzero(~ours & (O != 0xAA))
    assert hurt.size == 0, f"{id}: output arena written at {hurt[:8].tolist()}, outside every submission's records"
    if c.stats:
        want = dict(c.stats, submissions=len(subs), chunks=sum(s.n for s in subs))
        assert {k: st[k] for k in want} == want, f"{id}: {st}"
