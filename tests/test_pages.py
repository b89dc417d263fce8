"""Digests of device-resident chunks laid out as page lists
(md5hip_digest_pages, md5_batch_submit_device_pages): the three kinds against
hashlib.md5 / zlib.crc32 over each chunk's bytes concatenated on the host,
and, for the mid-size batch, against the library's own descriptor entries over
a contiguous copy.

A batch here is a pool of slots of page_bytes + 128 bytes; table entry e is
the page at slot slot[e], `skew[e]` bytes in (0: on the 128-B line).  The
slots of a batch are a random permutation unless a test places them."""
import errno
import hashlib
import zlib

import numpy as np
import pytest
import torch

import sproxy_amd.md5 as m

pytestmark = pytest.mark.gpu

MD5, CRC32, DUAL = m.Batcher.MD5, m.Batcher.CRC32, m.Batcher.MD5_CRC32
KINDS = (MD5, CRC32, DUAL)
KIND_IDS = ("md5", "crc32", "md5crc32")
PAD = 128


def pages_of(length, P):
    return (length + P - 1) // P


def records(kind, chunks):
    """The expected output of `kind` for the byte strings `chunks`."""
    md5 = np.array([np.frombuffer(hashlib.md5(c).digest(), dtype=np.uint8) for c in chunks],
                   dtype=np.uint8).reshape(len(chunks), 16)
    crc = np.array([zlib.crc32(c) for c in chunks], dtype="<u4")
    if kind == MD5:
        return md5
    if kind == CRC32:
        return crc
    rec = np.zeros((len(chunks), 32), dtype=np.uint8)
    rec[:, :16] = md5
    rec[:, 16:20] = crc.view(np.uint8).reshape(-1, 4)
    return rec


def as_host(kind, out):
    a = out.cpu().numpy()
    return a.view("<u4").reshape(-1) if kind == CRC32 else a


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
        host = rng.integers(0, 256, nslots * S + PAD, dtype=np.uint8)
        self.pool = torch.from_numpy(host).to(cuda)
        self.at = self.slot.astype(np.int64) * S + self.skew            # byte offset of entry e's page
        self.pages = (self.pool.data_ptr() + self.at).astype(np.uint64)
        self.chunks = []
        for i, L in enumerate(int(x) for x in lens):
            f = int(self.first[i])
            parts = [host[self.at[f + p]:self.at[f + p] + min(P, L - p * P)] for p in range(need[i])]
            self.chunks.append(b"".join(bytes(x) for x in parts))
        self.d_pages = torch.from_numpy(self.pages.view(np.int64)).to(cuda)
        self.d_first = torch.from_numpy(self.first[:-1].view(np.int64).copy()).to(cuda)
        self.d_lens = torch.from_numpy(self.lens.view(np.int32)).to(cuda)

    def digest(self, kind, order=None, out=None):
        o = None if order is None else torch.from_numpy(np.asarray(order, dtype=np.int32)).to(self.pool.device)
        got = m.digest_pages(kind, self.d_pages, self.d_first, self.d_lens, self.P, order=o, out=out)
        torch.cuda.synchronize()
        return got

    def check(self, kind, order=None):
        got = as_host(kind, self.digest(kind, order))
        want = records(kind, self.chunks)
        bad = np.flatnonzero((got != want).reshape(len(self.chunks), -1).any(axis=1))
        assert bad.size == 0, f"chunks {bad[:8].tolist()} (lens {self.lens[bad[:8]].tolist()}) differ"


def edge_lengths(P):
    return [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, P - 1, P, P + 1, P + 63, P + 64, P + 65,
            2 * P - 1, 2 * P, 2 * P + 64, 2 * P + 127, 3 * P + 191]


@pytest.mark.parametrize("P", (128, 256, 16384))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_edge_lengths(kind, P, cuda):
    """One chunk per length in one launch, so the lanes of the wave run out on
    different pages: an empty chunk, a remainder alone on a new page (P + 1), a
    last page exactly full (P, 2P), an odd block at the end of the last page."""
    Paged(edge_lengths(P), P, 7, cuda).check(kind)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_scattered_pages(kind, cuda):
    """Chunk 0's pages descend in address and interleave with chunk 1's; one
    page is shared by chunks 0 and 2; chunk 3 owns more entries than its
    length needs (its spare entries name another chunk's page: reading one
    would show in the digest)."""
    P = 256
    lens = [3 * P + 77, 3 * P, P + 5, P + 1, 2 * P]
    owned = [4, 3, 2, 5, 2]
    #        chunk 0        chunk 1    chunk 2   chunk 3           chunk 4
    slot = [9, 7, 5, 3,     8, 6, 4,   5, 10,    12, 11, 0, 0, 0,  2, 1]
    Paged(lens, P, 11, cuda, owned=owned, slot=slot).check(kind)


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_launch_order(n, cuda):
    """With and without d_order (reversed: a non-trivial permutation), every
    kind; lengths differ by chunk, so a lane index taken for a chunk shows."""
    P = 128
    rng = np.random.default_rng(n)
    b = Paged(rng.integers(0, 3 * P + 2, n).tolist(), P, 13 + n, cuda)
    for kind in KINDS:
        b.check(kind)
        b.check(kind, order=np.arange(n)[::-1].copy())


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_page_alignment(kind, cuda):
    """Group 1: every page 16-B aligned, off the 128-B line; group 2: one page
    4 bytes off the 16-B grid; group 4: one page 1 byte off (both lane-direct
    at that page index); groups 0 and 3 on the line, in the same launch."""
    P = 256
    rng = np.random.default_rng(17)
    lens = rng.integers(0, 3 * P + 1, 5 * 64)
    lens[2 * 64 + 9], lens[4 * 64 + 30] = 2 * P + 70, 3 * P
    first = np.concatenate([[0], np.cumsum([pages_of(int(x), P) for x in lens])])
    skew = np.zeros(int(first[-1]), dtype=np.int64)
    skew[first[64]:first[128]] = rng.choice([16, 48, 80, 112], int(first[128] - first[64]))
    skew[first[2 * 64 + 9] + 1] = 4
    skew[first[4 * 64 + 30] + 2] = 1
    Paged(lens.tolist(), P, 19, cuda, skew=skew).check(kind)


@pytest.mark.parametrize("n", (1, 64, 65))
@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_output_bounds(kind, n, cuda):
    """Canaries before and after the n records (n = 65: the ragged second
    group's one record is the last): nothing outside them is written, and all
    32 bytes of an MD5_CRC32 record are defined, 20..31 zero."""
    P, dsz, guard = 128, {MD5: 16, CRC32: 4, DUAL: 32}[kind], 64
    b = Paged(np.random.default_rng(n).integers(1, 2 * P, n).tolist(), P, 23, cuda)
    buf = torch.full((guard + n * dsz + guard,), 0xA5, dtype=torch.uint8, device=cuda)
    rec = buf[guard:guard + n * dsz]
    b.digest(kind, out=rec.view(torch.int32) if kind == CRC32 else rec.view(n, dsz))
    h = buf.cpu().numpy()
    assert (h[:guard] == 0xA5).all() and (h[guard + n * dsz:] == 0xA5).all()
    got = h[guard:guard + n * dsz]
    want = records(kind, b.chunks)
    assert np.array_equal(got.view("<u4") if kind == CRC32 else got.reshape(n, dsz), want)
    if kind == DUAL:
        assert not got.reshape(n, 32)[:, 20:].any()


@pytest.mark.parametrize("kind", (CRC32, DUAL), ids=KIND_IDS[1:])
def test_grid_stride_trips(kind, cuda):
    """64 x 12 x CUs + 65 one-page chunks of 128 bytes: every wave of the
    per-CU frame makes a second trip, and the last group is ragged."""
    P = 128
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    n = 64 * 12 * cus + 65
    Paged([P] * n, P, 29, cuda).check(kind)


def test_mixed_batch_against_descriptor_entries(cuda):
    """4,096 chunks of 0 .. 5 pages of 16 KiB, pages randomly permuted: every
    record of the three kinds equals the descriptor entries' over the
    contiguous copy the pages were scattered from."""
    P, n = 16384, 4096
    rng = np.random.default_rng(31)
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
    d_offs = d_first * P
    d_lens = torch.from_numpy(lens.view(np.int32)).to(cuda)
    order = torch.from_numpy(m.plan_order(lens).astype(np.int32)).to(cuda)
    for kind, ref in ((MD5, m.digest_desc(contig, d_offs, d_lens, order)),
                      (CRC32, m.crc32_desc(contig, d_offs, d_lens, order)),
                      (DUAL, m.md5crc32_desc(contig, d_offs, d_lens, order))):
        for o in (order, None):
            got = m.digest_pages(kind, pages, d_first, d_lens, P, order=o)
            torch.cuda.synchronize()
            assert torch.equal(got.view(torch.uint8).reshape(n, -1), ref.view(torch.uint8).reshape(n, -1)), kind


# ------------------------------------------------------------------ the queue
def queue_batch(cuda, n=200, P=256, seed=41):
    lens = np.random.default_rng(seed).integers(0, 4 * P + 1, n).tolist()
    return Paged(lens, P, seed + 1, cuda)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_queue_sync_async_host_and_device_digests(kind, cuda):
    b = queue_batch(cuda)
    n, want = len(b.chunks), records(kind, b.chunks)
    with m.Queue(device=0) as q:
        q.set_digest(kind)
        torch.cuda.synchronize()
        assert np.array_equal(q.submit_device_pages(b.pages, b.first, b.lens, b.P), want)
        assert np.array_equal(q.submit_device_pages_async(b.pages, b.first, b.lens, b.P).wait(), want)
        dev = torch.zeros(n * q.dsz, dtype=torch.uint8, device=cuda)
        q.submit_device_pages(b.pages, b.first, b.lens, b.P, out=dev)
        pend = q.submit_device_pages_async(b.pages, b.first, b.lens, b.P, out=torch.zeros_like(dev))
        dev2 = pend.wait()
        for d in (dev, dev2):
            assert np.array_equal(as_host(kind, d.view(torch.int32) if kind == CRC32 else d.view(n, -1)), want)
        assert q.stats()["bytes_staged"] == 0


def test_queue_after_current_orders_behind_the_writer(cuda):
    """The pages are written by a torch kernel on the current stream just
    before the submission: after="current" orders the launch behind it."""
    b = queue_batch(cuda, n=96)
    host = b.pool.cpu().numpy()
    with m.Queue(device=0) as q:
        torch.cuda.synchronize()
        big = torch.ones(1 << 26, dtype=torch.float32, device=cuda)
        for _ in range(4):
            big = big * 1.0001                                        # keeps the stream busy ahead of the write
        b.pool.bitwise_xor_(0x3C)
        got = q.submit_device_pages(b.pages, b.first, b.lens, b.P, after="current")
    flipped = host ^ 0x3C
    chunks = []
    for i, L in enumerate(int(x) for x in b.lens):
        f = int(b.first[i])
        chunks.append(b"".join(bytes(flipped[b.at[f + p]:b.at[f + p] + min(b.P, L - p * b.P)])
                               for p in range(pages_of(L, b.P))))
    assert np.array_equal(got, records(MD5, chunks))


def test_queue_slices_in_order(cuda):
    """max_chunks 64: 200 chunks cut into four launches (64, 64, 64, 8), the
    digests in submission order; a table smaller than one chunk is -E2BIG."""
    b = queue_batch(cuda)
    with m.Queue(device=0, max_chunks=64) as q:
        torch.cuda.synchronize()
        s0 = q.stats()
        got = q.submit_device_pages(b.pages, b.first, b.lens, b.P)
        s1 = q.stats()
        assert np.array_equal(got, records(MD5, b.chunks))
        assert s1["launches"] - s0["launches"] == 4 and s1["chunks"] - s0["chunks"] == 200
        assert s1["max_chunks_per_launch"] == 64 and s1["bytes_staged"] == 0
        cap = max(4 * 64, 65536)                                      # MD5HIP_PAGES_PER_SLOT(64)
        with pytest.raises(m.MD5HipError) as e:
            q.submit_device_pages(np.full(cap + 1, b.pages[0]), [0, cap + 1], [(cap + 1) * 128], 128)
        assert e.value.rc == -errno.E2BIG and q.stats()["launches"] == s1["launches"]


def test_queue_injected_fault(cuda):
    """The library's injected report on a paged launch: the ticket is -EIO,
    the host array untouched, the next call -ENODEV."""
    b = queue_batch(cuda, n=64)
    with m.Queue(device=0) as q:
        torch.cuda.synchronize()
        assert np.array_equal(q.submit_device_pages(b.pages, b.first, b.lens, b.P), records(MD5, b.chunks))
        q.inject_fault(1)
        out = np.full((64, 16), 0x5A, dtype=np.uint8)
        with pytest.raises(m.MD5HipError) as e:
            q.submit_device_pages(b.pages, b.first, b.lens, b.P, out=out)
        assert e.value.rc == -errno.EIO and (out == 0x5A).all()
        launches = q.stats()["launches"]
        with pytest.raises(m.MD5HipError) as e:
            q.submit_device_pages(b.pages, b.first, b.lens, b.P)
        assert e.value.rc == -errno.ENODEV and q.stats()["launches"] == launches


def test_pool_refuses_paged_submissions(cuda):
    with m.Pool(devices=(0,)) as p:
        for f in (p.submit_device_pages, p.submit_device_pages_async):
            with pytest.raises(NotImplementedError):
                f([1], [0, 1], [1], 128)
