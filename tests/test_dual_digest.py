"""MD5 + CRC-32 in one pass (MD5HIP_DIGEST_MD5_CRC32): the two device entries
(md5crc32hip_fixed / md5crc32hip_desc), and the kind through every submit
path of the batcher, the device queue and the pool, verify_iov and
upgrade_iov.  Expected values come from the oracle (oracle/md5_oracle.c,
oracle/crc32_oracle.c through tests/gen.py), never from the library's own
MD5 or CRC entries; one assertion compares against those as well.  A record
is 32 bytes: MD5 at 0..15, the CRC-32 little-endian at 16..19, bytes 20..31
written as zero."""
import numpy as np
import pytest
import torch

import gen
import sproxy_amd.md5 as m

pytestmark = pytest.mark.gpu

LENS = [0, 1, 3, 4, 7, 8, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 191, 192, 193, 4096, 16384, 16385]
COUNTS = [1, 63, 64, 65, 200]
NMAX = max(COUNTS)


def _want(buf, offs, lens):
    """Oracle (md5 [n, 16], crc [n]) of the chunks of a host buffer."""
    return gen.oracle_digests(buf, offs, lens), gen.oracle_crc32_batch(buf, offs, lens)


def _check(rec, md5, crc, what):
    """rec: (n, 32) uint8 records (host array or device tensor)."""
    r = rec.cpu().numpy() if isinstance(rec, torch.Tensor) else np.asarray(rec)
    assert r.shape == (len(crc), 32), what
    gm, gc = m.split_records(r)
    assert np.array_equal(gm, md5), f"{what}: md5"
    assert np.array_equal(gc, crc), f"{what}: crc"
    assert not r[:, 20:].any(), f"{what}: bytes 20..31 of a record not zero"


@pytest.fixture(scope="module")
def blob(cuda):
    """One random host buffer and its device copy, shared by the fixed-length cases."""
    host = gen.xorshift_array(NMAX * (16640 + 16) + 256, seed=0xD0A1)
    return host, torch.from_numpy(host.copy()).to(cuda)


def _fixed_cases(blob, cuda, stride_of, skew=0):
    host, dev = blob
    for L in LENS:
        stride = stride_of(L)
        offs = [skew + i * stride for i in range(NMAX)]
        md5, crc = _want(host, offs, [L] * NMAX)
        for n in COUNTS:
            out = torch.full((n + 1, 32), 0xAA, dtype=torch.uint8, device=cuda)
            m.md5crc32_fixed(dev[skew:], n, L, stride, out=out)
            torch.cuda.synchronize()
            _check(out[:n], md5[:n], crc[:n], f"len {L} n {n} stride {stride} skew {skew}")
            assert bool((out[n] == 0xAA).all()), f"len {L} n {n}: wrote past record n - 1"


def test_fixed_on_the_line(blob, cuda):
    """stride = len rounded up to 256: every chunk on a 128-B line (nt loads)."""
    _fixed_cases(blob, cuda, lambda L: max((L + 255) // 256 * 256, 256))


def test_fixed_off_the_line(blob, cuda):
    """the same + 16: on the 16-B grid, off the line (default cache policy)."""
    _fixed_cases(blob, cuda, lambda L: max((L + 255) // 256 * 256, 256) + 16)


def test_fixed_off_the_grid(blob, cuda):
    """stride = len + 5 from base + 3: the descriptor kernel with implicit offsets."""
    _fixed_cases(blob, cuda, lambda L: L + 5, skew=3)


def test_fixed_second_grid_trip(cuda):
    """12 * CUs * 64 + 65 chunks of 192 B: the grid-stride loop's second trip."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, L = 12 * cus * 64 + 65, 192
    host = gen.xorshift_array(n * L, seed=0x192)
    md5, crc = _want(host, np.arange(n, dtype=np.uint64) * L, [L] * n)
    out = m.md5crc32_fixed(torch.from_numpy(host).to(cuda), n, L)
    torch.cuda.synchronize()
    _check(out, md5, crc, "second trip")


def test_fixed_one_mib_chunks(cuda):
    n, L = 65, 1 << 20
    host = gen.xorshift_array(n * L, seed=0x100000)
    md5, crc = _want(host, np.arange(n, dtype=np.uint64) * L, [L] * n)
    dev = torch.from_numpy(host).to(cuda)
    out = m.md5crc32_fixed(dev, n, L)
    torch.cuda.synchronize()
    _check(out, md5, crc, "65 x 1 MiB")
    # (the one comparison with the library's own entries)
    assert np.array_equal(m.digest_fixed(dev, n, L).cpu().numpy(), md5)
    assert np.array_equal(m.crc32_fixed(dev, n, L).cpu().numpy().view(np.uint32), crc)


@pytest.mark.parametrize("align", [1, 4, 16, 128])
def test_desc(cuda, align):
    lens = gen.mixed_lengths(1000, seed=40 + align, max_len=1 << 16) + [0]
    offs, total = gen.pack_offsets(lens, align=align)
    host = gen.xorshift_array(total + 64, seed=0xDE5C + align)
    md5, crc = _want(host, offs, lens)
    dev = torch.from_numpy(host).to(cuda)
    for n in (1, 64, 65, 1001):
        # the first n - 1 chunks and the empty one (n = 1: the longest chunk alone)
        sl = list(range(n - 1)) + [len(lens) - 1] if n > 1 else [int(np.argmax(lens))]
        sub = [lens[i] for i in sl]
        o = torch.tensor([offs[i] for i in sl], dtype=torch.int64, device=cuda)
        ln = torch.tensor(sub, dtype=torch.int32, device=cuda)
        order = torch.from_numpy(m.plan_order(sub).astype(np.int32)).to(cuda)
        for od in (None, order):
            out = torch.full((n + 1, 32), 0xAA, dtype=torch.uint8, device=cuda)
            m.md5crc32_desc(dev, o, ln, od, out=out)
            torch.cuda.synchronize()
            _check(out[:n], md5[sl], crc[sl], f"align {align} n {n} order {od is not None}")
            assert bool((out[n] == 0xAA).all())


# ---------------------------------------------------------------- batcher, queue, pool
@pytest.fixture(scope="module")
def chunks():
    """~300 chunks of 1..40,000 bytes (and an empty one) in one host buffer."""
    rng = np.random.default_rng(23)
    lens = [int(x) for x in rng.integers(1, 40001, 300)] + [0, 1, 63, 64, 65]
    offs, total = gen.pack_offsets(lens, align=1)
    host = gen.xorshift_array(total + 64, seed=0xC4)
    md5, crc = _want(host, offs, lens)
    rec = np.zeros((len(lens), 32), dtype=np.uint8)
    rec[:, :16] = md5
    rec[:, 16:20] = crc.astype("<u4").view(np.uint8).reshape(-1, 4)
    bufs = [host[o:o + L] for o, L in zip(offs, lens)]
    pages = [[b[:len(b) // 3], b[len(b) // 3:]] for b in bufs]       # two segments per chunk
    return dict(host=host, offs=offs, lens=lens, md5=md5, crc=crc, rec=rec, bufs=bufs, pages=pages)


def test_batcher_host_paths(chunks, cuda):
    c = chunks
    with m.Batcher(device=0, kind=m.Batcher.MD5_CRC32) as b:
        for what, got in (("ptrs", b.submit(c["bufs"])), ("iov", b.submit_iov(c["pages"])),
                          ("async", b.submit_async(c["bufs"]).wait()),
                          ("iov async", b.submit_iov_async(c["pages"]).wait())):
            _check(got, c["md5"], c["crc"], what)


def test_queue_device_paths(chunks, cuda):
    c = chunks
    n = len(c["lens"])
    dev = torch.from_numpy(c["host"].copy()).to(cuda)
    ptrs = np.asarray(c["offs"], dtype=np.uint64) + np.uint64(dev.data_ptr())
    L = np.asarray(c["lens"], dtype=np.uint32)
    with m.Queue(device=0) as q:
        q.set_digest(m.Batcher.MD5_CRC32)
        _check(q.submit_device(ptrs, L), c["md5"], c["crc"], "device, records to host")
        out = torch.full((n, 32), 0xAA, dtype=torch.uint8, device=cuda)
        q.submit_device(ptrs, L, out=out)
        torch.cuda.synchronize()
        _check(out, c["md5"], c["crc"], "device, records on device")
        _check(q.submit_device_async(ptrs, L).wait(), c["md5"], c["crc"], "device async")
        # two submissions sharing a slot: device records go through the scatter
        halves = [torch.full((k, 32), 0xAA, dtype=torch.uint8, device=cuda) for k in (100, n - 100)]
        p1 = q.submit_device_async(ptrs[:100], L[:100], out=halves[0])
        p2 = q.submit_device_async(ptrs[100:], L[100:], out=halves[1])
        p1.wait()
        p2.wait()
        torch.cuda.synchronize()
        _check(torch.cat(halves), c["md5"], c["crc"], "two tickets, records on device")


def _fixed_batch(n, L, stride, seed):
    host = gen.xorshift_array(n * stride, seed=seed)
    offs = np.arange(n, dtype=np.uint64) * stride
    return host, _want(host, offs, [L] * n)


def test_device_fixed_and_host_fixed(cuda):
    n, L, stride = 1000, 5000, 5008
    host, (md5, crc) = _fixed_batch(n, L, stride, 0xF1)
    dev = torch.from_numpy(host.copy()).to(cuda)
    with m.Queue(device=0) as q:
        q.set_digest(m.Batcher.MD5_CRC32)
        out = torch.full((n, 32), 0xAA, dtype=torch.uint8, device=cuda)
        q.submit_device_fixed_async(dev, n, L, stride, out=out).wait()
        torch.cuda.synchronize()
        _check(out, md5, crc, "device_fixed, records on device")
        _check(q.submit_device_fixed_async(dev, n, L, stride).wait(), md5, crc, "device_fixed, records to host")
    pinned = torch.from_numpy(host.copy()).pin_memory()
    with m.Batcher(device=0, slice_bytes=1 << 20, kind=m.Batcher.MD5_CRC32) as b:     # several slices
        _check(b.host_fixed(pinned.numpy(), n, L, stride), md5, crc, "host_fixed pinned")
        _check(b.host_fixed(host, n, L, stride), md5, crc, "host_fixed pageable")


def test_host_fixed_stages_once(cuda):
    """A host_fixed call under the kind moves what ONE MD5 call over the same
    buffer moves (the point of the kind: not an MD5 call plus a CRC call)."""
    n, L, stride = 1000, 5000, 5008
    host, (md5, crc) = _fixed_batch(n, L, stride, 0xF2)
    pinned = torch.from_numpy(host.copy()).pin_memory().numpy()
    for src in (host, pinned):
        with m.Batcher(device=0, slice_bytes=1 << 20) as b:
            s0 = b.stats()
            assert np.array_equal(b.host_fixed(src, n, L, stride), md5)
            s1 = b.stats()
            b.set_digest(m.Batcher.MD5_CRC32)
            _check(b.host_fixed(src, n, L, stride), md5, crc, "host_fixed")
            s2 = b.stats()
        for k in ("bytes_staged", "launches", "chunks", "submissions"):
            assert s2[k] - s1[k] == s1[k] - s0[k], k


def test_kind_switches_on_one_handle(chunks, cuda):
    c = chunks
    B = m.Batcher
    with B(device=0) as b:
        assert np.array_equal(b.submit(c["bufs"]), c["md5"])
        b.set_digest(B.MD5_CRC32)
        _check(b.submit_iov(c["pages"]), c["md5"], c["crc"], "both")
        b.set_digest(B.CRC32)
        assert np.array_equal(b.submit(c["bufs"]), c["crc"])
        b.set_digest(B.MD5_CRC32)
        _check(b.submit(c["bufs"]), c["md5"], c["crc"], "both again")
        with pytest.raises(m.MD5HipError) as e:
            b.set_digest(B.MD5_CRC32, 64)                     # no fastcrc window under the kind
        assert e.value.rc == -22
        with pytest.raises(m.MD5HipError):
            b.set_digest(3)
        _check(b.submit(c["bufs"]), c["md5"], c["crc"], "kind kept after a refused switch")


def test_interleaved_kinds(chunks, cuda):
    """Async submissions of three kinds interleaved on one pool (its set_digest
    does not drain): every ticket comes back in its own kind."""
    c = chunks
    B = m.Batcher
    n = len(c["bufs"])
    with m.Pool(devices=(0, 0)) as p:
        pend = []
        for r in range(12):
            kind = (B.MD5, B.MD5_CRC32, B.CRC32)[r % 3]
            lo, hi = r * n // 12, (r + 1) * n // 12
            p.set_digest(kind)
            pend.append((kind, lo, hi, p.submit_async(c["bufs"][lo:hi])))
        for kind, lo, hi, t in reversed(pend):
            got = t.wait()
            if kind == B.MD5:
                assert np.array_equal(got, c["md5"][lo:hi])
            elif kind == B.CRC32:
                assert np.array_equal(got, c["crc"][lo:hi])
            else:
                _check(got, c["md5"][lo:hi], c["crc"][lo:hi], f"ticket {lo}:{hi}")


def test_pool_paths(chunks, cuda):
    c = chunks
    with m.Pool(devices=(0, 0), slice_bytes=1 << 20, kind=m.Batcher.MD5_CRC32) as p:
        for split in (1 << 40, 64 << 10):                    # whole to one device, then cut over both
            p.set_split(split)
            for what, got in (("ptrs", p.submit(c["bufs"])), ("iov", p.submit_iov(c["pages"])),
                              ("async", p.submit_async(c["bufs"]).wait()),
                              ("iov async", p.submit_iov_async(c["pages"]).wait())):
                _check(got, c["md5"], c["crc"], f"pool {what} split {split}")
        assert p.stats()["split"] > 0
        n, L, stride = 400, 4000, 4001
        host, (md5, crc) = _fixed_batch(n, L, stride, 0xF3)
        _check(p.host_fixed(host, n, L, stride), md5, crc, "pool host_fixed")


@pytest.mark.parametrize("make", [lambda: m.Batcher(device=0, kind=2), lambda: m.Pool(devices=(0, 0), kind=2)],
                         ids=["batcher", "pool"])
def test_verify_iov_over_records(chunks, cuda, make):
    c = chunks
    exp = c["rec"].copy()
    exp[3, 5] ^= 1            # an md5 byte
    exp[77, 17] ^= 0x80       # a crc byte
    exp[200, 27] = 1          # a padding byte
    with make() as b:
        ok, bad = b.verify_iov(c["pages"], exp)
        assert bad == 3 and sorted(np.flatnonzero(~ok)) == [3, 77, 200]
        ok, bad = b.verify_iov(c["pages"], c["rec"])
        assert bad == 0 and ok.all()


@pytest.mark.parametrize("make", [lambda: m.Batcher(device=0), lambda: m.Pool(devices=(0, 0), kind=1, fastcrc=64)],
                         ids=["batcher", "pool"])
def test_upgrade_iov(chunks, cuda, make):
    """The stored CRC-32 verified and the MD5 of every block in one pass,
    whatever kind the handle is set to."""
    c = chunks
    want = c["crc"].copy()
    want[0] ^= 1
    want[299] ^= 0x80000000
    with make() as b:
        kind = b.kind
        ok, md5 = b.upgrade_iov(c["pages"], want)
        assert sorted(np.flatnonzero(~ok)) == [0, 299]
        assert np.array_equal(md5, c["md5"])                 # the two mismatching blocks included
        name, rc = b._call("upgrade_iov", *_upgrade_args(b, c["pages"], want))
        assert rc == 2
        assert b.kind == kind
        got = b.submit(c["bufs"])                            # the handle's own kind still in force
        assert np.array_equal(got, c["md5"] if kind == 0 else gen.oracle_crc32_batch(c["host"], c["offs"], c["lens"], 64))


def _upgrade_args(b, pages, want):
    arr, fa, keep = b._iov(pages)
    n = len(pages)
    w = np.ascontiguousarray(want, dtype=np.uint32)
    ok = np.empty(n, dtype=np.uint8)
    md5 = np.empty((n, 16), dtype=np.uint8)
    _upgrade_args.keep = (arr, fa, keep, w, ok, md5)
    return arr, fa.ctypes.data, n, w.ctypes.data, ok.ctypes.data, md5.ctypes.data
