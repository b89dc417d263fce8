"""The small-batch kernel of the one-pass MD5 + CRC-32 kind (md5crc32_fedsplit,
sproxy_amd/csrc/md5_kernels.h): one launch whose first ceil(n / 64) workgroups
run the MD5s as fed pairs (or lane-direct, for a group off the 16-B grid or
without two whole blocks) and whose other workgroups cut each CRC-32 across a
wave, grid-striding over the chunks.

Expected values are hashlib.md5 and zlib.crc32 of the host copy.  Every device
output is a 0xAA canary with a guard record behind the last one, and every
case checks the MD5 at bytes 0..15, the CRC-32 little-endian at 16..19, zeros
at 20..31 and the guard untouched.  The sizes are the smallest that reach
each path: the group counts around 64, the CRC role's second grid trip
(2 x CUs + 3 chunks), the lane body (under two blocks), the fed pair from two
blocks on, a second split pass (16,385 B) and many passes with a short first
segment (262,221 B)."""
import hashlib
import zlib

import numpy as np
import pytest
import torch

import gen
import sproxy_amd.md5 as m

pytestmark = pytest.mark.gpu

FIXED_LENS = [0, 64, 127, 128, 255, 256, 257, 2048, 16384, 16385, 262221]
SHORT = 2048                      # the large n go with lengths up to here, the large lengths with n <= 65
DESC_LENS = [0, 1, 63, 64, 128, 200, 4096, 16385, 70001]
DESC_N = 130


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _counts(L):
    small = [1, 63, 64, 65]
    return small + [130, 2 * _cus() + 3] if L <= SHORT else small


def _want(host, offs, lens):
    """(md5 [n, 16] uint8, crc [n] uint32) of the chunks of a host array."""
    md5 = np.empty((len(lens), 16), dtype=np.uint8)
    crc = np.empty(len(lens), dtype=np.uint32)
    for i, (o, L) in enumerate(zip(offs, lens)):
        b = host[int(o):int(o) + int(L)].tobytes()
        md5[i] = np.frombuffer(hashlib.md5(b).digest(), dtype=np.uint8)
        crc[i] = zlib.crc32(b)
    return md5, crc


def _canary(n, cuda):
    return torch.full((n + 1, 32), 0xAA, dtype=torch.uint8, device=cuda)


def _check(out, n, md5, crc, what):
    """out: n + 1 records on the device, the last one the guard."""
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert a.shape == (n + 1, 32), what
    _check_records(a[:n], md5, crc, what)
    assert (a[n] == 0xAA).all(), f"{what}: wrote past record n - 1"
    return a[:n]


def _check_records(r, md5, crc, what):
    assert r.shape == (len(crc), 32), what
    bad = np.flatnonzero((r[:, :16] != md5).any(axis=1))
    assert bad.size == 0, f"{what}: md5 of chunks {bad[:8].tolist()}"
    got = r[:, 16:20].copy().view("<u4").reshape(-1)
    bad = np.flatnonzero(got != crc)
    assert bad.size == 0, f"{what}: crc of chunks {bad[:8].tolist()}"
    assert not r[:, 20:].any(), f"{what}: bytes 20..31 of a record not zero"


@pytest.fixture(scope="module")
def blob(cuda):
    """One random host buffer and its device copy for every fixed-length case."""
    nbytes = max(65 * ((max(FIXED_LENS) + 15) // 16 * 16 + 8), (2 * _cus() + 3) * (SHORT + 8)) + 256
    host = gen.xorshift_array(nbytes, seed=0x5A11)
    return host, torch.from_numpy(host.copy()).to(cuda)


def _fixed(blob, cuda, L, stride, skew, variant="fedsplit"):
    host, dev = blob
    counts = _counts(L)
    offs = skew + np.arange(max(counts), dtype=np.int64) * stride
    md5, crc = _want(host, offs, [L] * max(counts))
    for n in counts:
        out = _canary(n, cuda)
        m.md5crc32_fixed(dev[skew:], n, L, stride, out=out, variant=variant)
        _check(out, n, md5[:n], crc[:n], f"len {L} n {n} stride {stride} skew {skew}")


@pytest.mark.parametrize("L", FIXED_LENS)
def test_fixed_on_the_grid(blob, cuda, L):
    """stride = len rounded up to 16 (at least 16): every chunk on the 16-B grid."""
    _fixed(blob, cuda, L, max((L + 15) // 16 * 16, 16), 0)


@pytest.mark.parametrize("L", [257, 16385])
def test_fixed_off_the_grid(blob, cuda, L):
    """stride = len + 5 from base + 3: every group holds a chunk start off the
    16-B grid, so the MD5 role runs lane-direct; the CRC role splits as ever."""
    _fixed(blob, cuda, L, L + 5, 3)


def test_fixed_at_the_fed_edge(cuda):
    """64 x CUs chunks of 2 KiB, the most groups a fed-pair batch has: CUs MD5
    workgroups beside CUs CRC workgroups, the CRC role 32 grid trips deep.
    "auto" takes the same batch (so many chunks this short md5crc32_plan leaves
    to xdma16), and then the largest batch of 2 KiB chunks that it does send
    to the new kernel."""
    cus = _cus()
    n, L = 64 * cus, 2048
    host = gen.xorshift_array(n * L, seed=0xED6E)
    dev = torch.from_numpy(host).to(cuda)
    md5, crc = _want(host, np.arange(n, dtype=np.int64) * L, [L] * n)
    edge = cus * L // 256
    assert m.md5crc32_plan(edge, L) == "fedsplit" and m.md5crc32_plan(edge + 1, L) == "xdma16"
    for k, variant in ((n, "fedsplit"), (n, "auto"), (edge, "auto")):
        out = _canary(k, cuda)
        m.md5crc32_fixed(dev, k, L, out=out, variant=variant)
        _check(out, k, md5[:k], crc[:k], f"{variant} at {k} x {L}")


@pytest.fixture(scope="module")
def mixed(cuda):
    """The mixed group repeated to 130 chunks, packed at 128 B, 16 B and 1 B:
    lanes without a whole block beside long ones, dead lanes in the ragged
    last group, and (1 B) groups off the 16-B grid."""
    lens = (DESC_LENS * (DESC_N // len(DESC_LENS) + 1))[:DESC_N]
    packs = {}
    for align in (128, 16, 1):
        offs, total = gen.pack_offsets(lens, align=align)
        host = gen.xorshift_array(total + 64, seed=0xDE5C + align)
        packs[align] = (host, torch.from_numpy(host.copy()).to(cuda), offs, _want(host, offs, lens))
    return lens, packs


@pytest.mark.parametrize("align", [128, 16, 1])
def test_desc(mixed, cuda, align):
    lens, packs = mixed
    host, dev, offs, (md5, crc) = packs[align]
    o = torch.tensor([int(x) for x in offs], dtype=torch.int64, device=cuda)
    ln = torch.tensor(lens, dtype=torch.int32, device=cuda)
    order = torch.from_numpy(m.plan_desc(lens)[0].astype(np.int32)).to(cuda)
    for od in (None, order):
        out = _canary(DESC_N, cuda)
        m.md5crc32_desc(dev, o, ln, od, out=out, variant="fedsplit")
        got = _check(out, DESC_N, md5, crc, f"align {align} order {od is not None}")
        # the same batch through the throughput kernel: byte-equal records
        ref = _canary(DESC_N, cuda)
        m.md5crc32_desc(dev, o, ln, od, out=ref, variant="xdma16")
        torch.cuda.synchronize()
        assert np.array_equal(got, ref.cpu().numpy()[:DESC_N]), f"align {align}: fedsplit != xdma16"


def test_fixed_agrees_with_xdma16(blob, cuda):
    host, dev = blob
    n, L = 65, 16385
    stride = (L + 15) // 16 * 16
    a, b, c = _canary(n, cuda), _canary(n, cuda), _canary(n, cuda)
    m.md5crc32_fixed(dev, n, L, stride, out=a, variant="fedsplit")
    m.md5crc32_fixed(dev, n, L, stride, out=b, variant="xdma16")
    m.md5crc32_fixed(dev, n, L, stride, out=c)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(b, c)


# ---------------------------------------------------------------- through the call site
def _blocks(lens, seed, page=16384):
    """Blocks of the given lengths as lists of pages of one host buffer."""
    offs, total = gen.pack_offsets(lens, align=4096)
    host = gen.xorshift_array(total + 64, seed=seed)
    pages = [[host[o + p:o + min(p + page, L)] for p in range(0, L, page)] for o, L in zip(offs, lens)]
    return pages, _want(host, offs, lens)


@pytest.mark.parametrize("make", [lambda: m.Batcher(device=0, kind=m.Batcher.MD5_CRC32),
                                  lambda: m.Pool(devices=(0, 0), kind=m.Batcher.MD5_CRC32)],
                         ids=["batcher", "pool"])
def test_submit_iov_of_one_vector(cuda, make):
    """64 x 16 KiB in 16 KiB pages: the vector the kind was built for."""
    pages, (md5, crc) = _blocks([16384] * 64, 0x10F)
    with make() as b:
        _check_records(np.asarray(b.submit_iov(pages)), md5, crc, "submit_iov 64 x 16 KiB")


def test_upgrade_iov_of_mixed_blocks(cuda):
    rng = np.random.default_rng(0x0B6)
    lens = [int(x) for x in rng.integers(4096, 131073, 100)]
    pages, (md5, crc) = _blocks(lens, 0x0B7)
    want = crc.copy()
    for i, bit in ((0, 1), (41, 0x8000), (99, 0x80000000)):
        want[i] ^= bit
    with m.Batcher(device=0) as b:
        ok, got = b.upgrade_iov(pages, want)
        assert sorted(np.flatnonzero(~ok).tolist()) == [0, 41, 99]
        assert np.array_equal(got, md5)
        name, rc = b._call("upgrade_iov", *_upgrade_args(b, pages, want))
        assert rc == 3, name


def _upgrade_args(b, pages, want):
    arr, fa, keep = b._iov(pages)
    n = len(pages)
    w = np.ascontiguousarray(want, dtype=np.uint32)
    ok = np.empty(n, dtype=np.uint8)
    md5 = np.empty((n, 16), dtype=np.uint8)
    _upgrade_args.keep = (arr, fa, keep, w, ok, md5)
    return arr, fa.ctypes.data, n, w.ctypes.data, ok.ctypes.data, md5.ctypes.data
