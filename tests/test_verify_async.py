"""Asynchronous verify and upgrade on the GPU: the digest-compare kernel alone
(md5hip_digest_compare, numpy records against a numpy compare), then the
ticket entries of the batcher, the queue and the pool: page lists of every
kind against hashlib / zlib, coalescing behind a running launch, device-resident
chunks over several slots with expected / ok on the host and on the device,
agreement with the synchronous verify_iov / upgrade_iov, an injected fault, and
a pool that cuts the submission over two batchers."""
import ctypes
import errno
import hashlib
import zlib

import numpy as np
import pytest
import torch

import gen
from sproxy_amd import md5 as m

pytestmark = pytest.mark.gpu

PIECE = 4096                                   # MD5HIP_CMP_PIECE: records per workgroup of the public entry
SHAPES = [(4, 0, 4), (16, 0, 16), (32, 0, 32), (32, 16, 4)]          # (gsz, goff, wsz); the last: upgrade


@pytest.mark.parametrize("gsz,goff,wsz", SHAPES)
def test_digest_compare_alone(cuda, gsz, goff, wsz):
    rng = np.random.default_rng(1000 + gsz + goff)
    for n in (1, 63, 64, 65, 257, PIECE - 1, PIECE, PIECE + 1):
        got = rng.integers(0, 256, (n, gsz), dtype=np.uint8)
        want = got[:, goff:goff + wsz].copy()
        bad = sorted({i for i in (0, 63, 64, n - 1) if i < n})
        for i in bad:
            want[i, rng.integers(0, wsz)] ^= 0x10
        want[0] = got[0, goff:goff + wsz]
        want[0, 0] ^= 1                                        # only the first compared byte
        if n > 1:
            want[n - 1] = got[n - 1, goff:goff + wsz]
            want[n - 1, wsz - 1] ^= 0x80                       # only the last compared byte
        if n > 2 and wsz < gsz:                                # differs only outside the compared field: ok
            assert 2 not in bad
            got[2, :goff] ^= 0xFF
            got[2, goff + wsz:] ^= 0xFF
        ref = (got[:, goff:goff + wsz] == want).all(axis=1)
        assert int((~ref).sum()) == len(bad)
        d_got = torch.from_numpy(got).to(cuda)
        wbuf = torch.zeros(n * wsz + 1, dtype=torch.uint8, device=cuda)
        wbuf[1:] = torch.from_numpy(want.reshape(-1)).to(cuda)
        okbuf = torch.full((n + 18,), 0xAA, dtype=torch.uint8, device=cuda)
        d_want, d_ok = wbuf[1:], okbuf[1:1 + n]                # both 1 byte off alignment
        assert d_want.data_ptr() % 2 == 1 and d_ok.data_ptr() % 2 == 1
        nbad = torch.tensor([1000], dtype=torch.int64, device=cuda)
        out = m.digest_compare(d_got, d_want, gsz, goff, wsz, n=n, ok=d_ok, nbad=nbad)
        torch.cuda.synchronize()
        okh = okbuf.cpu().numpy()
        assert set(np.unique(okh[1:1 + n])) <= {0, 1}, (n, "ok bytes are exactly 0 or 1")
        assert np.array_equal(okh[1:1 + n].astype(bool), ref), n
        assert okh[0] == 0xAA and (okh[1 + n:] == 0xAA).all(), (n, "guard bytes")
        assert int(nbad.item()) == 1000 + len(bad), n
        assert out.data_ptr() == d_ok.data_ptr()
    # no counter; ok made by the call; n == 0
    ok = m.digest_compare(d_got, d_want, gsz, goff, wsz)
    torch.cuda.synchronize()
    assert np.array_equal(ok.cpu().numpy().astype(bool), ref)
    assert m.digest_compare(d_got, d_want, gsz, goff, wsz, n=0).numel() == 0


# ---------------------------------------------------------------- page lists
LENS = [0, 1, 55, 56, 63, 64, 65, 1000, 4096, 16389, 119, 120, 127, 128, 129, 4095, 4097, 8192, 30000, 777]
BAD = (0, 63, 64, 69)


def _page_lists(heap, n=70, seed=5):
    """n chunks of LENS' lengths packed into `heap`, each as 1-4 segments: (chunks, bytes of each)."""
    rng = np.random.default_rng(seed)
    chunks, raw, cur = [], [], 0
    for i in range(n):
        L = LENS[i % len(LENS)] + (i // len(LENS))
        cuts = sorted(int(x) for x in rng.integers(0, L + 1, int(rng.integers(0, 4))))
        edges = [0] + cuts + [L]
        chunks.append([heap[cur + a:cur + b] for a, b in zip(edges[:-1], edges[1:])])
        raw.append(heap[cur:cur + L].tobytes())
        cur += L
    assert cur <= heap.size
    return chunks, raw


def _crc(b, F=0):
    return zlib.crc32(b) if F == 0 or len(b) <= F else zlib.crc32(b[:F]) ^ zlib.crc32(b[-F:])


def _expected(raw, kind, F=0):
    """[n, dsz] uint8: the digests of `kind` from hashlib / zlib."""
    md5 = np.array([np.frombuffer(hashlib.md5(b).digest(), np.uint8) for b in raw])
    crc = np.array([_crc(b, F) for b in raw], dtype="<u4")
    if kind == m.Batcher.MD5:
        return md5
    if kind == m.Batcher.CRC32:
        return crc.view(np.uint8).reshape(-1, 4).copy()
    rec = np.zeros((len(raw), 32), dtype=np.uint8)
    rec[:, :16] = md5
    rec[:, 16:20] = crc.view(np.uint8).reshape(-1, 4)
    return rec


def _corrupt(exp, bad):
    exp = exp.copy()
    for k, i in enumerate(bad):
        exp[i, (5 * k) % exp.shape[1]] ^= 1 << (k % 8)
    return exp


@pytest.fixture(scope="module")
def pages():
    heap = gen.xorshift_array(1 << 19, seed=4242).copy()
    chunks, raw = _page_lists(heap)
    return heap, chunks, raw


@pytest.mark.parametrize("registered", [False, True])
def test_host_page_lists_every_kind(cuda, pages, registered):
    heap, chunks, raw = pages
    n = len(chunks)
    ref_ok = np.array([i not in BAD for i in range(n)])
    md5 = _expected(raw, m.Batcher.MD5)
    if registered:
        m.register_host(heap)
    try:
        with m.Batcher(device=0, slice_bytes=1 << 20, nslots=3) as b:
            for kind, F in ((b.MD5, 0), (b.CRC32, 0), (b.CRC32, 64), (b.MD5_CRC32, 0)):
                b.set_digest(kind, F)
                exp = _corrupt(_expected(raw, kind, F), BAD)
                pend = b.verify_iov_async(chunks, exp)
                exp[:] = 0xEE                                   # copied by the call
                ok, nbad = pend.wait()
                assert np.array_equal(ok, ref_ok) and nbad == 4, (kind, F, nbad)
                # the untouched synchronous path agrees
                ok_s, nbad_s = b.verify_iov(chunks, _corrupt(_expected(raw, kind, F), BAD))
                assert np.array_equal(ok_s, ok) and nbad_s == nbad
            # upgrade, whatever kind is set (CRC-32 with a window here)
            b.set_digest(b.CRC32, 64)
            want = np.array([_crc(x) for x in raw], dtype=np.uint32)
            for k, i in enumerate(BAD):
                want[i] ^= np.uint32(1 << (7 * k))
            keep = want.copy()
            pend = b.upgrade_iov_async(chunks, want)
            want[:] = 0xEEEEEEEE
            ok, got_md5, nbad = pend.wait()
            assert np.array_equal(ok, ref_ok) and nbad == 4 and np.array_equal(got_md5, md5)
            ok_s, md5_s = b.upgrade_iov(chunks, keep)
            assert np.array_equal(ok_s, ok) and np.array_equal(md5_s, md5)
            assert b.kind == b.CRC32
            # empty
            assert b.verify_iov_async([], np.empty((0, 4), np.uint8)).wait()[1] == 0
    finally:
        if registered:
            m.unregister_host(heap)


def _arena(lens, seed, cuda, align=1):
    offs, total = gen.pack_offsets(lens, align=align)
    host = gen.xorshift_array(total + 64, seed=seed)
    dev = torch.from_numpy(host.copy()).to(cuda)
    ptrs = np.asarray(offs, dtype=np.uint64) + np.uint64(dev.data_ptr())
    return dev, host, ptrs, np.asarray(lens, dtype=np.uint32), gen.oracle_digests(host, offs, lens)


def test_coalesced_behind_a_running_launch(cuda, pages):
    """One long launch in flight at inflight target 1: verify tickets and plain
    tickets submitted meanwhile share ONE launch (and one compare launch);
    every ticket gets its own results, waited on in reverse order."""
    heap, chunks, raw = pages
    md5 = _expected(raw, m.Batcher.MD5)
    blocker_bytes, _, pl, Ll, wl = _arena([32 << 20] * 2, 9, cuda, align=16)    # held until the test ends
    dev, _, ps, Ls, ws = _arena([int(x) for x in np.random.default_rng(3).integers(0, 50000, 90)], 19, cuda)
    with m.Queue(device=0, nslots=4) as q:
        q.set_inflight(1)
        assert q.verify_device(ps[:1], Ls[:1], ws[:1])[1] == 0      # the feature's buffers exist from here on
        st0 = q.stats()
        blocker = q.submit_device_async(pl, Ll)
        pend, want = [], []
        for r in range(6):
            lo, hi = 10 * r, 10 * r + 10
            bad = (lo, hi - 1) if r % 2 else (lo + 3,)
            ok_ref = np.array([i not in bad for i in range(lo, hi)])
            if r < 2:                                           # verify from page lists
                pend.append(q.verify_iov_async(chunks[lo:hi], _corrupt(md5[lo:hi], [i - lo for i in bad])))
                want.append((ok_ref, len(bad)))
            elif r < 4:                                         # verify of device-resident chunks, host expected
                pend.append(q.verify_device_async(ps[lo:hi], Ls[lo:hi], _corrupt(ws[lo:hi], [i - lo for i in bad])))
                want.append((ok_ref, len(bad)))
            else:                                               # plain digests
                pend.append(q.submit_device_async(ps[lo:hi], Ls[lo:hi]) if r == 4 else q.submit_iov_async(chunks[lo:hi]))
                want.append(ws[lo:hi] if r == 4 else md5[lo:hi])
        outs = [p.wait() for p in reversed(pend)][::-1]
        assert np.array_equal(blocker.wait(), wl)
        st = q.stats()
    assert st["launches"] - st0["launches"] == 2 and st["max_tickets_per_launch"] == 6, (st0, st)
    for r, (got, w) in enumerate(zip(outs, want)):
        if r < 4:
            assert np.array_equal(got[0], w[0]) and got[1] == w[1], r
        else:
            assert np.array_equal(got, w), r


def test_device_resident_over_several_slots(cuda):
    """700 chunks at 1-byte alignment through 256-chunk slots, written by a
    producer on torch's current stream with no host sync; expected / ok on the
    host, then as device tensors with ok not 16-B aligned."""
    lens = [int(x) for x in np.random.default_rng(23).integers(0, 20000, 693)] + [0, 1, 55, 56, 63, 64, 65]
    n = len(lens)
    offs, total = gen.pack_offsets(lens, align=1)
    host = torch.from_numpy(gen.xorshift_array(total + 64, seed=231).copy()).pin_memory()
    digests = gen.oracle_digests(host.numpy(), offs, lens)
    bad = (0, 100, 255, 256, 400, 511, 512, 699)              # every slot
    exp = _corrupt(digests, bad)
    ref = np.array([i not in bad for i in range(n)])
    L = np.asarray(lens, dtype=np.uint32)
    with m.Queue(device=0, max_chunks=256, nslots=4) as q:
        dev = torch.empty(total + 64, dtype=torch.uint8, device=cuda)
        ptrs = np.asarray(offs, dtype=np.uint64) + np.uint64(dev.data_ptr())
        dev.copy_(host, non_blocking=True)                      # the producer: no sync before the submission
        pend = q.verify_device_async(ptrs, L, exp.copy(), after="current")
        ok, nbad = pend.wait()
        assert np.array_equal(ok, ref) and nbad == len(bad)
        assert q.stats()["launches"] >= 3
        # expected and ok on the device
        d_exp = torch.zeros(16 * n + 1, dtype=torch.uint8, device=cuda)
        raw_ok = torch.full((n + 16,), 0xAA, dtype=torch.uint8, device=cuda)
        d_ok = raw_ok[3:3 + n]
        assert d_ok.data_ptr() % 16 != 0
        dev.zero_()
        dev.copy_(host, non_blocking=True)
        d_exp[1:].copy_(torch.from_numpy(exp.reshape(-1)), non_blocking=False)
        ok2, nbad2 = q.verify_device_async(ptrs, L, d_exp[1:], ok=d_ok, after="current").wait()
        torch.cuda.synchronize()
        okh = raw_ok.cpu().numpy()
        assert ok2.data_ptr() == d_ok.data_ptr() and nbad2 == len(bad)
        assert np.array_equal(okh[3:3 + n].astype(bool), ref) and set(np.unique(okh[3:3 + n])) <= {0, 1}
        assert (okh[:3] == 0xAA).all() and (okh[3 + n:] == 0xAA).all()
        # the synchronous form
        ok3, nbad3 = q.verify_device(ptrs, L, exp)
        assert np.array_equal(ok3, ref) and nbad3 == len(bad)


def test_injected_fault(cuda, pages):
    heap, chunks, raw = pages
    n = 20
    exp = _expected(raw[:n], m.Batcher.MD5)
    with m.Batcher(device=0, slice_bytes=1 << 20, nslots=3) as b:
        assert b.verify_iov_async(chunks[:n], exp).wait()[1] == 0
        arr, fa, keep = b._iov(chunks[:n])
        ok = np.full(n, 0xAA, dtype=np.uint8)
        nbad = np.full(1, 77, dtype=np.uint64)
        t = ctypes.c_uint64()
        b.inject_fault(1)
        bad = _corrupt(exp, (1, 2))
        name, rc = b._call("verify_iov_async", arr, fa.ctypes.data, n, bad.ctypes.data, ok.ctypes.data,
                           nbad.ctypes.data, ctypes.byref(t))
        assert rc == 0 and t.value and nbad[0] == 0            # zeroed by the call
        assert b._call("wait", ctypes.c_uint64(t.value))[1] == -errno.EIO
        assert (ok == 0xAA).all() and nbad[0] == 0, "a failed launch delivered results"
        with pytest.raises(m.MD5HipError) as e:
            b.verify_iov_async(chunks[:n], exp)
        assert e.value.rc == -errno.ENODEV
        with pytest.raises(m.MD5HipError) as e:
            b.upgrade_iov_async(chunks[:n], np.zeros(n, np.uint32))
        assert e.value.rc == -errno.ENODEV
        del keep


def test_pool_cut_over_two_batchers(cuda, pages):
    heap, chunks, raw = pages
    n = len(chunks)
    md5 = _expected(raw, m.Batcher.MD5)
    bad = (0, 1, 34, 35, 68, 69)                               # both halves, whatever the cut
    ref = np.array([i not in bad for i in range(n)])
    with m.Pool(devices=(0, 0), slice_bytes=1 << 20, nslots=3) as p:
        p.set_split(32 << 10)
        ok, nbad = p.verify_iov_async(chunks, _corrupt(md5, bad)).wait()
        assert np.array_equal(ok, ref) and nbad == len(bad)
        want = np.array([_crc(x) for x in raw], dtype=np.uint32)
        for i in bad:
            want[i] += 1
        ok, got_md5, nbad = p.upgrade_iov_async(chunks, want).wait()
        assert np.array_equal(ok, ref) and nbad == len(bad) and np.array_equal(got_md5, md5)
        st = p.stats()
        assert st["split"] == 2 and st["parts"] == 4, st
        assert all(p.device_stats(g)["submissions"] == 2 for g in range(2))
        with pytest.raises(NotImplementedError):
            p.verify_device_async([], [], np.empty((0, 16), np.uint8))
