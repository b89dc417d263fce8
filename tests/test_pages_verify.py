"""fastcrc windows over page lists (crc32hip_pages) and verify / upgrade of
paged blocks on the device (md5_batch_verify_device_pages,
md5_batch_upgrade_device_pages).

The window values are blk_make_crc's with g__need_fastcrc = F, computed here
with zlib: crc32(c) for a chunk of at most F bytes, else crc32(c[:F]) ^
crc32(c[-F:]); the mid-size batch is also held against the library's own
contiguous entry (crc32hip_desc with the same window).

A batch is tests/test_pages.py's: a pool of slots of page_bytes + 128 bytes;
table entry e is the page at slot slot[e], `skew[e]` bytes in (0: on the
128-B line).  The slots are a random permutation unless a test places them.
A 64-row group of the window kernel is 32 chunks (a head and a tail row
each)."""
import errno
import hashlib
import zlib

import numpy as np
import pytest
import torch

import sproxy_amd.md5 as m
import trips

pytestmark = pytest.mark.gpu

MD5, CRC32, DUAL = m.Batcher.MD5, m.Batcher.CRC32, m.Batcher.MD5_CRC32
PAD = 128
FAST_PIPE = (16, 32)          # the window kernel's frame: waves per CU, chunks per group (trips.py)


def pages_of(length, P):
    return (length + P - 1) // P


def window_crc(c, F):
    """blk_make_crc's value of the bytes c under fastcrc = F (0: the whole chunk)."""
    return zlib.crc32(c) if F == 0 or len(c) <= F else zlib.crc32(c[:F]) ^ zlib.crc32(c[-F:])


def records(kind, F, chunks):
    """The stored values of `chunks` under digest kind `kind` with window F."""
    if kind == CRC32:
        return np.array([window_crc(c, F) for c in chunks], dtype="<u4")
    md5 = np.array([np.frombuffer(hashlib.md5(c).digest(), dtype=np.uint8) for c in chunks],
                   dtype=np.uint8).reshape(len(chunks), 16)
    if kind == MD5:
        return md5
    rec = np.zeros((len(chunks), 32), dtype=np.uint8)
    rec[:, :16] = md5
    rec[:, 16:20] = np.array([zlib.crc32(c) for c in chunks], dtype="<u4").view(np.uint8).reshape(-1, 4)
    return rec


class Paged:
    """A paged batch on the device and its chunks' bytes on the host.

    lens: chunk lengths; P: page_bytes.  owned[i] (default: what the length
    needs) table entries belong to chunk i; slot / skew per table entry place
    the pages (default: a random permutation, on the line)."""

    def __init__(self, lens, P, seed, cuda, owned=None, slot=None, skew=None):
        rng = np.random.default_rng(seed)
        self.P, self.lens = P, np.asarray(lens, dtype=np.uint32)
        need = [pages_of(int(x), P) for x in lens]
        owned = need if owned is None else owned
        self.first = np.concatenate([[0], np.cumsum(owned)]).astype(np.uint64)
        E = int(self.first[-1])
        self.slot = rng.permutation(E) if slot is None else np.asarray(slot)
        self.skew = np.zeros(E, dtype=np.int64) if skew is None else np.asarray(skew, dtype=np.int64)
        S = P + PAD
        nslots = int(self.slot.max()) + 1 if E else 1
        self.host = rng.integers(0, 256, nslots * S + PAD, dtype=np.uint8)
        self.pool = torch.from_numpy(self.host).to(cuda)
        self.at = self.slot.astype(np.int64) * S + self.skew            # byte offset of entry e's page
        self.pages = (self.pool.data_ptr() + self.at).astype(np.uint64)
        self.need = need
        self.chunks = self.chunks_of(self.host)
        self.d_pages = torch.from_numpy(self.pages.view(np.int64)).to(cuda)
        self.d_first = torch.from_numpy(self.first[:-1].view(np.int64).copy()).to(cuda)
        self.d_lens = torch.from_numpy(self.lens.view(np.int32)).to(cuda)

    def chunks_of(self, host):
        """The chunks' bytes when the pool holds `host`."""
        out = []
        for i, L in enumerate(int(x) for x in self.lens):
            f = int(self.first[i])
            parts = [host[self.at[f + p]:self.at[f + p] + min(self.P, L - p * self.P)] for p in range(self.need[i])]
            out.append(b"".join(bytes(x) for x in parts))
        return out

    def crcs(self, F, order=None, out=None):
        o = None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).to(self.pool.device)
        got = m.crc32_pages(self.d_pages, self.d_first, self.d_lens, self.P, F, order=o, out=out)
        torch.cuda.synchronize()
        return got.cpu().numpy().view("<u4")

    def check(self, F, order=None):
        got = self.crcs(F, order)
        want = records(CRC32, F, self.chunks)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"F {F}: chunks {bad[:8].tolist()} (lens {self.lens[bad[:8]].tolist()}) differ"
        return got


def edge_lengths(P, F):
    cand = [0, 1, F - 1, F, F + 1, 2 * F - 4, 2 * F, 2 * F + 1, P - 1, P, P + 1, P + F - 1, P + F, P + F + 1,
            2 * P + 1, 2 * P + F - 4, 2 * P + 63, 2 * P + 64, 3 * P + 191]
    return sorted({x for x in cand if x >= 0})


@pytest.mark.parametrize("F", (4, 64, 128, 132, 1000))
@pytest.mark.parametrize("P", (128, 256, 16384))
def test_window_edges(P, F, cuda):
    """One chunk per length in one launch: a chunk no longer than F,
    overlapping windows (F < L < 2F), a tail with one byte in the last page
    (2P + 1), tails starting 1, 2 and 3 bytes off the dword grid, windows
    spanning several pages (P = 128 under F = 132 and 1000), F no multiple of
    64."""
    Paged(edge_lengths(P, F), P, 7, cuda).check(F)


@pytest.mark.parametrize("F", (64, 128, 200))
def test_window_alignment(F, cuda):
    """Group 1 (chunks 32..63): every page 16-B aligned, off the 128-B line;
    group 2: two pages 4 bytes off the 16-B grid that hold a tail window (of
    128 and 200 bytes: straddling them, 70 bytes in the last); group 4: a page
    1 byte off that holds a whole tail window; groups 0 and 3 on the line with
    every window of 64 and 128 bytes inside one page on the 16-B grid, in the
    same launch."""
    P = 256
    rng = np.random.default_rng(17)
    lens = rng.integers(0, 3 * P + 1, 5 * 32)
    for g in (0, 3):                                                  # whole 16-B granules, tails inside one page
        lens[32 * g:32 * g + 32] = P * rng.integers(1, 4, 32) - 16 * rng.integers(0, 8, 32)
    lens[2 * 32 + 9], lens[4 * 32 + 30] = 2 * P + 70, 3 * P
    first = np.concatenate([[0], np.cumsum([pages_of(int(x), P) for x in lens])])
    skew = np.zeros(int(first[-1]), dtype=np.int64)
    skew[first[32]:first[64]] = rng.choice([16, 48, 80, 112], int(first[64] - first[32]))
    skew[first[2 * 32 + 9] + 1:first[2 * 32 + 9] + 3] = 4
    skew[first[4 * 32 + 30] + 2] = 1
    Paged(lens.tolist(), P, 19, cuda, skew=skew).check(F)


@pytest.mark.parametrize("F", (128, 300))
def test_scattered_pages(F, cuda):
    """Chunk 0's pages descend in address and interleave with chunk 1's; one
    page is shared by chunks 0 and 2; chunk 3 owns more entries than its
    length needs; chunk 5 has six pages, of which the middle ones (never read
    under F = 128; F = 300 reads into pages 1 and 4) are other chunks' pages."""
    P = 256
    lens = [3 * P + 77, 3 * P, P + 5, P + 1, 2 * P, 6 * P]
    owned = [4, 3, 2, 5, 2, 6]
    #        chunk 0        chunk 1    chunk 2   chunk 3           chunk 4   chunk 5
    slot = [9, 7, 5, 3,     8, 6, 4,   5, 10,    12, 11, 0, 0, 0,  2, 1,     13, 9, 7, 8, 6, 14]
    Paged(lens, P, 11, cuda, owned=owned, slot=slot).check(F)


@pytest.mark.parametrize("n", (1, 31, 32, 33, 63, 64, 65, 130))
def test_rows_and_order(n, cuda):
    """32 chunks fill a 64-row group: its ragged edges, with and without a
    reversed d_order -- the same values either way, which are the right ones."""
    P = 128
    rng = np.random.default_rng(n)
    b = Paged(rng.integers(0, 3 * P + 2, n).tolist(), P, 13 + n, cuda)
    for F in (64, 100):
        plain = b.check(F)
        assert np.array_equal(b.check(F, order=np.arange(n)[::-1].copy()), plain)


@pytest.mark.parametrize("n", (1, 32, 33))
def test_output_bounds(n, cuda):
    """Canaries before and after the n CRCs (n = 33: the ragged second group's
    one value is the last)."""
    P, F, guard = 128, 64, 64
    b = Paged(np.random.default_rng(n).integers(1, 3 * P, n).tolist(), P, 23, cuda)
    buf = torch.full((guard + 4 * n + guard,), 0xA5, dtype=torch.uint8, device=cuda)
    b.crcs(F, out=buf[guard:guard + 4 * n].view(torch.int32))
    h = buf.cpu().numpy()
    assert (h[:guard] == 0xA5).all() and (h[guard + 4 * n:] == 0xA5).all()
    assert np.array_equal(h[guard:guard + 4 * n].view("<u4"), records(CRC32, F, b.chunks))


def test_grid_stride_trips(cuda):
    """One-page chunks for 2.25 trips of the per-CU frame (16 waves, 32 chunks
    a group), the last group ragged: every wave hashes a group while the next
    one's windows are in flight, and on from there.  Two thirds of the groups
    hold whole 128-B pages alone (pipelined, F = 64), the others lengths that
    end off the 16-B grid (lane by lane), so a wave's successive groups take
    both paths in either order."""
    P, F = 128, 64
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    wpc, cpg = FAST_PIPE
    G = trips.ngroups_for(cus, wpc, 2.25)
    assert trips.trip_of(G - 1, cus, wpc) == 2
    n = (G - 1) * cpg + trips.RAGGED[cpg]
    rng = np.random.default_rng(29)
    lens = np.full((G, cpg), P, dtype=np.int64)
    odd = rng.random(G) < 1 / 3
    lens[odd] = rng.integers(0, P + 1, (int(odd.sum()), cpg))
    lens = lens.reshape(-1)[:n]
    S = P + PAD
    perm = rng.permutation(n)
    host = rng.integers(0, 256, (n, S), dtype=np.uint8)
    pool = torch.from_numpy(host).to(cuda)
    pages = torch.from_numpy(pool.data_ptr() + perm.astype(np.int64) * S).to(cuda)
    first = torch.arange(n, dtype=torch.int64, device=cuda)
    got = m.crc32_pages(pages, first, torch.from_numpy(lens.astype(np.int32)).to(cuda), P, F)
    torch.cuda.synchronize()
    want = np.array([window_crc(host[perm[i], :lens[i]].tobytes(), F) for i in range(n)], dtype="<u4")
    bad = np.flatnonzero(got.cpu().numpy().view("<u4") != want)
    assert bad.size == 0, f"{bad.size} of {n} differ, first at chunks {bad[:8].tolist()} (groups {(bad[:8] // cpg).tolist()})"


def scattered_copy(cuda, n=4096, P=16384, seed=31):
    """n chunks of 0 .. 5 pages, the pages a random permutation of a contiguous
    copy: (contig, its offsets, lens, pages, first), all on the device."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 5 * P + 1, n).astype(np.uint32)
    need = (lens.astype(np.int64) + P - 1) // P
    first = np.concatenate([[0], np.cumsum(need)])
    E = int(first[-1])
    g = torch.Generator(device=cuda).manual_seed(37)
    contig = torch.randint(0, 256, (E, P), dtype=torch.uint8, device=cuda, generator=g)
    perm = rng.permutation(E)
    pool = torch.empty_like(contig)
    pool[torch.from_numpy(perm).to(cuda)] = contig                   # page j of the copy lies at pool page perm[j]
    pages = torch.from_numpy((pool.data_ptr() + perm.astype(np.int64) * P)).to(cuda)
    d_first = torch.from_numpy(first[:-1].copy()).to(cuda)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    return contig, pool, d_first * P, d_lens, pages, d_first, lens


@pytest.fixture(scope="module")
def scattered(cuda):
    return scattered_copy(cuda)


@pytest.mark.parametrize("F", (128, 4096))
def test_against_the_contiguous_entry(F, scattered, cuda):
    """4,096 chunks of 0 .. 5 pages of 16 KiB, pages permuted: every value
    equals crc32hip_desc's with the same window over the contiguous copy."""
    contig, _pool, d_offs, d_lens, pages, d_first, lens = scattered
    order = torch.from_numpy(m.plan_order(lens).astype(np.int32)).to(cuda)
    ref = m.crc32_desc(contig, d_offs, d_lens, order, fastcrc=F)
    for o in (order, None):
        got = m.crc32_pages(pages, d_first, d_lens, 16384, F, order=o)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32))


def test_fastcrc_zero_is_the_whole_chunk_kernel(scattered, cuda):
    _contig, _pool, _offs, d_lens, pages, d_first, lens = scattered
    order = torch.from_numpy(m.plan_order(lens).astype(np.int32)).to(cuda)
    for o in (order, None):
        a = m.crc32_pages(pages, d_first, d_lens, 16384, 0, order=o)
        b = m.digest_pages(CRC32, pages, d_first, d_lens, 16384, order=o)
        torch.cuda.synchronize()
        assert torch.equal(a, b)


# ------------------------------------------------------------------ the queue
BAD = (0, 63, 64, 199)
KINDS = ((MD5, 0), (CRC32, 0), (CRC32, 128), (DUAL, 0))
KIND_IDS = ("md5", "crc32", "crc32-f128", "md5crc32")


@pytest.fixture(scope="module")
def qbatch(cuda):
    lens = np.random.default_rng(41).integers(0, 4 * 256 + 1, 200).tolist()
    return Paged(lens, 256, 42, cuda)


def spoiled(want):
    """`want` as bytes per record with one bit flipped in the records BAD,
    each at another byte offset of the record; and the ok bytes that gives."""
    rec = want.view(np.uint8).reshape(len(want), -1).copy()
    dsz = rec.shape[1]
    for i, off in zip(BAD, (0, 1, dsz - 2, dsz - 1)):
        rec[i, off] ^= 1 << (i % 8)
    ok = np.ones(len(want), dtype=bool)
    ok[list(BAD)] = False
    return rec, ok


def verify_forms(q, b, exp, ok_want, cuda):
    """The four forms of one verify: synchronous and by ticket, host and
    device `expected` / `ok`."""
    n = len(ok_want)
    ok, nbad = q.verify_device_pages(b.pages, b.first, b.lens, b.P, exp)
    assert np.array_equal(ok, ok_want) and nbad == len(BAD)
    scratch = exp.copy()
    pend = q.verify_device_pages_async(b.pages, b.first, b.lens, b.P, scratch)
    scratch[:] = 0xEE                                                 # copied by the call
    ok, nbad = pend.wait()
    assert np.array_equal(ok, ok_want) and nbad == len(BAD)
    d_exp = torch.from_numpy(exp).to(cuda)
    ok, nbad = q.verify_device_pages(b.pages, b.first, b.lens, b.P, d_exp)
    assert ok.is_cuda and np.array_equal(ok.cpu().numpy()[:n].astype(bool), ok_want) and nbad == len(BAD)
    d_ok = torch.full((n,), 7, dtype=torch.uint8, device=cuda)
    ok, nbad = q.verify_device_pages_async(b.pages, b.first, b.lens, b.P, d_exp, ok=d_ok).wait()
    assert ok is d_ok and np.array_equal(d_ok.cpu().numpy(), ok_want.astype(np.uint8)) and nbad == len(BAD)


@pytest.mark.parametrize("max_chunks", (0, 64), ids=("one-launch", "four-launches"))
@pytest.mark.parametrize("kind,F", KINDS, ids=KIND_IDS)
def test_queue_verify(kind, F, max_chunks, qbatch, cuda):
    """200 blocks of 0 .. 4 pages of 256 B under every kind; four expected
    values are wrong by one bit.  max_chunks 64: four launches a call, nbad
    summed across them, ok in submission order.  No block byte is staged."""
    exp, ok_want = spoiled(records(kind, F, qbatch.chunks))
    with m.Queue(device=0, max_chunks=max_chunks) as q:
        q.set_digest(kind, F)
        torch.cuda.synchronize()
        s0 = q.stats()
        verify_forms(q, qbatch, exp, ok_want, cuda)
        s1 = q.stats()
        assert s1["launches"] - s0["launches"] == 4 * (4 if max_chunks else 1)
        assert s1["chunks"] - s0["chunks"] == 4 * 200 and s1["bytes_staged"] == 0


def test_queue_verify_after_current_orders_behind_the_writer(cuda):
    """The pages are rewritten by a torch kernel on the current stream just
    before the call: after="current" orders the launch behind it."""
    b = Paged(np.random.default_rng(43).integers(0, 4 * 256 + 1, 96).tolist(), 256, 44, cuda)
    with m.Queue(device=0) as q:
        q.set_digest(CRC32, 128)
        torch.cuda.synchronize()
        big = torch.ones(1 << 26, dtype=torch.float32, device=cuda)
        for _ in range(4):
            big = big * 1.0001                                        # keeps the stream busy ahead of the write
        b.pool.bitwise_xor_(0x3C)
        exp = records(CRC32, 128, b.chunks_of(b.host ^ 0x3C))
        ok, nbad = q.verify_device_pages(b.pages, b.first, b.lens, b.P, exp, after="current")
    assert ok.all() and nbad == 0


@pytest.mark.parametrize("max_chunks", (0, 64), ids=("one-launch", "four-launches"))
def test_queue_upgrade(max_chunks, qbatch, cuda):
    """want_crc wrong at blocks 1 and 65; the MD5 of every block comes back,
    whatever kind the queue is set to."""
    n = len(qbatch.chunks)
    want = np.array([zlib.crc32(c) for c in qbatch.chunks], dtype=np.uint32)
    want[[1, 65]] ^= 0x10000
    ok_want = np.ones(n, dtype=bool)
    ok_want[[1, 65]] = False
    md5_want = records(MD5, 0, qbatch.chunks)
    with m.Queue(device=0, max_chunks=max_chunks) as q:
        q.set_digest(CRC32, 64)
        torch.cuda.synchronize()
        ok, md5, nbad = q.upgrade_device_pages(qbatch.pages, qbatch.first, qbatch.lens, qbatch.P, want)
        assert np.array_equal(ok, ok_want) and nbad == 2 and np.array_equal(md5, md5_want)
        ok, md5, nbad = q.upgrade_device_pages_async(qbatch.pages, qbatch.first, qbatch.lens, qbatch.P, want).wait()
        assert np.array_equal(ok, ok_want) and nbad == 2 and np.array_equal(md5, md5_want)
        assert q.stats()["bytes_staged"] == 0


def test_queue_injected_fault(qbatch):
    """The library's injected report on a paged verify launch: the ticket is
    -EIO, host ok keeps its fill bytes and nbad stays 0; the next call is
    -ENODEV with no launch."""
    b = qbatch
    exp, _ = spoiled(records(CRC32, 128, b.chunks))
    with m.Queue(device=0) as q:
        q.set_digest(CRC32, 128)
        torch.cuda.synchronize()
        assert q.verify_device_pages(b.pages, b.first, b.lens, b.P, exp)[1] == len(BAD)
        q.inject_fault(1)
        ok = np.full(200, 0x5A, dtype=np.uint8)
        pend = q.verify_device_pages_async(b.pages, b.first, b.lens, b.P, exp, ok=ok)
        nbad = pend._nbad
        with pytest.raises(m.MD5HipError) as e:
            pend.wait()
        assert e.value.rc == -errno.EIO and (ok == 0x5A).all() and int(nbad[0]) == 0
        launches = q.stats()["launches"]
        with pytest.raises(m.MD5HipError) as e:
            q.verify_device_pages(b.pages, b.first, b.lens, b.P, exp)
        assert e.value.rc == -errno.ENODEV and q.stats()["launches"] == launches


def test_pool_refuses_paged_verify(cuda):
    with m.Pool(devices=(0,)) as p:
        for f in (p.verify_device_pages, p.verify_device_pages_async, p.upgrade_device_pages,
                  p.upgrade_device_pages_async):
            with pytest.raises(NotImplementedError):
                f([1], [0, 1], [1], 128, np.zeros(16, dtype=np.uint8))
