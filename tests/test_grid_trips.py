"""The persistent per-CU kernels past their first grid trip.

Every throughput kernel launches one workgroup per CU and loops over 64-row
groups; the LDS-DMA image, the wave priority, the hasher's lane constants and
crc32_fast_pipe's two-slot register ring live on from one group to the next.
The batches here (tests/trips.py) are sized from the device's CU count so that
every wave hashes several groups of different shape, the ragged last group
lies on a later trip, and every expected value comes from the oracle over the
whole batch.  Every output tensor is one record longer than the batch, filled
with 0xAA, and that record is asserted untouched.

CPU tests (-m "not gpu") keep the coverage claim honest: the built batches
reach the trips and shape pairs they claim for 64, 256 and 304 CUs, and the
oracle agrees with hashlib / zlib on a sample of them."""
import hashlib
import zlib

import numpy as np
import pytest

import gen
import trips
import sproxy_amd.md5 as m

# (waves per CU, chunks per group) of the persistent kernels
XDMA16, FAST_XDMA, FAST_PIPE, BALANCED = (12, 64), (12, 32), (16, 32), (4, 64)
A_TRIPS, B_TRIPS = 2.25, 4.25          # batch A in the (12, 64) frame, batch B in (16, 32)
A_FAST = 1000                          # batch A's window: crc32_fast_xdma16
B_FAST = (64, 100, 128)                # batch B's: crc32_fast_pipe, crc32_fast_xdma16, crc32_fast_pipe
SEED_A, SEED_B = 0xA7219, 0xB7219


def build_a(cus):
    return trips.build(cus, *XDMA16, A_TRIPS, trips.SHAPES_A, SEED_A)


def build_b(cus):
    return trips.build(cus, *FAST_PIPE, B_TRIPS, trips.SHAPES_B, SEED_B)


# ----------------------------------------------------------------- CPU: the builder
def _group_shapes(cus, batch, cpg):
    """Shape index of every `cpg`-chunk group of batch 'A' / 'B'."""
    if batch == "A":
        gs = trips.group_shapes(trips.ngroups_for(cus, XDMA16[0], A_TRIPS), trips.SHAPES_A, SEED_A)
        return np.repeat(gs, 64 // cpg)            # a 32-chunk group has its 64-chunk group's shape
    assert cpg == 32
    return trips.group_shapes(trips.ngroups_for(cus, FAST_PIPE[0], B_TRIPS), trips.SHAPES_B, SEED_B)


@pytest.mark.parametrize("cus", [64, 256, 304])
@pytest.mark.parametrize("batch,frame,min_trip", [("A", XDMA16, 2), ("A", FAST_XDMA, 2), ("A", BALANCED, 2),
                                                  ("B", FAST_PIPE, 4), ("B", FAST_XDMA, 2)],
                         ids=["A-12x64", "A-12x32", "A-4x64", "B-16x32", "B-12x32"])
def test_builder_reaches_the_later_trips(cus, batch, frame, min_trip):
    """In every frame a batch is launched in: some wave reaches trip `min_trip`
    (4 for crc32_fast_pipe: its outer loop runs twice and hashes both ring
    slots in the second pass), the ragged last group lies past the first trip,
    and every ordered pair of shapes is some wave's consecutive trips."""
    wpc, cpg = frame
    lens, offs, total = (build_a if batch == "A" else build_b)(cus)
    n = lens.size
    ngroups = (n + cpg - 1) // cpg
    assert n % cpg in (trips.RAGGED[cpg], trips.RAGGED[64] % cpg), "the last group is ragged"
    assert trips.trip_of(ngroups - 1, cus, wpc) >= min_trip
    assert ngroups > min_trip * wpc * cus            # what the GPU tests assert
    assert trips.trip_of(ngroups - 1, cus, wpc) >= 1
    gs = _group_shapes(cus, batch, cpg)
    assert gs.size == ngroups
    k = len(trips.SHAPES_A if batch == "A" else trips.SHAPES_B)
    want = {(a, b) for a in range(k) for b in range(k)}
    assert trips.shape_pairs(gs, cus, wpc) == want


def test_builder_sizes_and_layout():
    lens, offs, total = build_a(256)
    assert lens.size == (trips.ngroups_for(256, 12, A_TRIPS) - 1) * 64 + 37 == 442405
    assert 100e6 <= total <= 170e6
    assert int((offs + lens).max()) + trips.PAD <= total
    lens, offs, total = build_b(256)
    assert lens.size == (trips.ngroups_for(256, 16, B_TRIPS) - 1) * 32 + 19 == 557075
    assert 100e6 <= total <= 170e6
    assert int((offs + lens).max()) + trips.PAD <= total
    assert np.all(np.diff(offs.astype(np.int64)) >= 0)


def _groups_of(lens, offs, gs, names, name, cpg):
    """(lens, offs) of the whole groups of one shape, as [k, cpg] arrays."""
    full = lens.size // cpg
    idx = np.flatnonzero(gs[:full] == names.index(name))
    assert idx.size, name
    sel = (idx[:, None] * cpg + np.arange(cpg)).reshape(-1)
    return lens[sel].reshape(-1, cpg).astype(np.int64), offs[sel].reshape(-1, cpg).astype(np.int64)


def test_builder_shapes_are_what_they_claim():
    """Each shape drives the kernel path it is named for (desc_xpose_group's
    conditions for batch A, fast_pipe_body's `simple` for batch B)."""
    cus = 64
    lens, offs, _ = build_a(cus)
    names = list(trips.SHAPES_A)
    gs = _group_shapes(cus, "A", 64)
    L, O = _groups_of(lens, offs, gs, names, "lined256", 64)
    assert np.all(L == 256) and np.all(O % 128 == 0)
    for name in ("offline", "skew4"):
        L, O = _groups_of(lens, offs, gs, names, name, 64)
        assert L.min() >= 384 and L.max() <= 640
        assert np.all((O % 128 != 0).any(axis=1)), "some chunk of every group off the line"
        off16 = (O % 16 != 0).sum(axis=1)
        assert np.all(off16 == (1 if name == "skew4" else 0))
        if name == "skew4":
            assert np.all((O % 16)[O % 16 != 0] == 4)
    L, O = _groups_of(lens, offs, gs, names, "tiny", 64)
    assert L.max() < 128 and np.all((L == 0).any(axis=1)) and np.all(O % 16 == 0)
    L, O = _groups_of(lens, offs, gs, names, "ragged", 64)
    assert L.max() <= 1536 and L.max() > 1400 and np.all(O % 16 == 0)
    assert np.all((L < 128).any(axis=1)), "a row without any 128-B stage"
    assert np.all(np.ptp(L // 128, axis=1) > 0), "clamped rows"
    for r in trips.RESIDUES:
        assert np.all((L % 64 == r).any(axis=1)), r
    L, O = _groups_of(lens, offs, gs, names, "long1", 64)
    assert np.all((L == trips.LONG_CHUNK).sum(axis=1) == 1) and np.all(O % 16 == 0)
    assert np.all(np.sort(L, axis=1)[:, -2] < 256) and (trips.LONG_CHUNK >> 6) >= 256
    # the ragged last group keeps its shape's special chunk
    last = names[gs[-1]]
    tail_l, tail_o = lens[-37:].astype(np.int64), offs[-37:].astype(np.int64)
    if last == "long1":
        assert (tail_l == trips.LONG_CHUNK).sum() == 1
    if last == "skew4":
        assert (tail_o % 16 != 0).sum() == 1

    lens, offs, _ = build_b(cus)
    names = list(trips.SHAPES_B)
    gs = _group_shapes(cus, "B", 32)
    fmax = max(f for f in B_FAST if f in (64, 128))
    L, O = _groups_of(lens, offs, gs, names, "simple", 32)
    assert L.min() > fmax and L.max() <= 400 and np.all(L % 16 == 0) and np.all(O % 16 == 0)
    L, O = _groups_of(lens, offs, gs, names, "short", 32)
    assert np.all(O % 16 == 0) and np.all((L == 0).sum(axis=1) == 1)
    assert np.all(((L > 0) & (L <= min(B_FAST))).sum(axis=1) == 1)
    L, O = _groups_of(lens, offs, gs, names, "oddlen", 32)
    assert L.min() > fmax and np.all(L % 16 != 0) and np.all(O % 16 == 0)
    L, O = _groups_of(lens, offs, gs, names, "pack4", 32)
    assert L.min() > fmax and np.all(L % 16 == 0) and np.all(O % 4 == 0)
    assert np.all((O % 16 != 0).any(axis=1))
    # "simple" carries about 60 % of the groups
    assert 0.55 < np.mean(gs == names.index("simple")) < 0.65


def _blk_crc(b: bytes, F: int) -> int:
    """blk_make_crc's rule (blk_io.c:408-424) over zlib."""
    if F == 0 or len(b) <= F:
        return zlib.crc32(b)
    return zlib.crc32(b[:F]) ^ zlib.crc32(b[-F:])


@pytest.mark.parametrize("batch", ["A", "B"])
def test_reference_on_samples(batch):
    """The oracle against hashlib.md5 and zlib.crc32 on 2,000 chunks of each batch."""
    lens, offs, total = (build_a if batch == "A" else build_b)(64)
    buf = gen.xorshift_array(total, seed=SEED_A if batch == "A" else SEED_B)
    rng = np.random.default_rng(2000)
    idx = np.unique(np.concatenate([rng.integers(0, lens.size, 1990), [0, lens.size - 1],
                                    np.flatnonzero(lens == lens.max())[:4],
                                    np.flatnonzero(lens == 0)[:4]]))
    sl, so = lens[idx], offs[idx]
    raw = [buf[int(o):int(o) + int(L)].tobytes() for o, L in zip(so, sl)]
    md5 = gen.oracle_digests(buf, so, sl)
    assert [bytes(d) for d in md5] == [hashlib.md5(b).digest() for b in raw]
    for F in (0,) + ((A_FAST,) if batch == "A" else B_FAST):
        crc = gen.oracle_crc32_batch(buf, so, sl, F)
        assert crc.tolist() == [_blk_crc(b, F) for b in raw], F


# ----------------------------------------------------------------- GPU
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _canary(n, width, cuda):
    """n + 1 records of `width` bytes, every byte 0xAA."""
    import torch
    return torch.full((n + 1, width), 0xAA, dtype=torch.uint8, device=cuda)


def _records(out, n, what):
    """The n records a launch wrote, once record n is seen untouched."""
    import torch
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert a.shape[0] == n + 1
    assert (a[n] == 0xAA).all(), f"{what}: wrote past record n - 1"
    return a[:n]


def _same(got, want, what, cpg=64):
    """Bit-exact, and on a mismatch which records and groups differ."""
    got = np.ascontiguousarray(got).view(np.uint8).reshape(len(want), -1)
    want = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        groups = np.unique(bad // cpg)
        untouched = int((got[bad] == 0xAA).all(axis=1).sum())
        pytest.fail(f"{what}: {bad.size} of {len(want)} records differ from the oracle "
                    f"({untouched} still 0xAA), first {int(bad[0])}; {groups.size} groups of {cpg}, "
                    f"first {groups[:8].tolist()}")


def _crcs(out, n, what):
    return _records(out, n, what).view("<u4")


class Batch:
    """A built batch on the host and the device, oracle values computed once."""

    def __init__(self, lens, offs, total, seed, cuda):
        import torch
        self.lens, self.offs, self.n = lens, offs, lens.size
        self.buf = gen.xorshift_array(total, seed=seed)
        self.d_buf = _dev(self.buf, cuda)
        self.d_offs = torch.from_numpy(offs.astype(np.int64)).to(cuda)
        self.d_lens = torch.from_numpy(lens.astype(np.int32)).to(cuda)
        self._order = None
        self._want = {}
        self.cuda = cuda

    def order(self):
        if self._order is None:
            self._order = _dev(m.plan_order(self.lens).astype(np.int32), self.cuda)
        return self._order

    def orders(self):
        return (("chunk order", None), ("longest first", self.order()))

    def md5(self):
        if "md5" not in self._want:
            w = gen.oracle_digests(self.buf, self.offs, self.lens)
            w.setflags(write=False)
            self._want["md5"] = w
        return self._want["md5"]

    def crc(self, fast=0):
        if fast not in self._want:
            w = gen.oracle_crc32_batch(self.buf, self.offs, self.lens, fast)
            w.setflags(write=False)
            self._want[fast] = w
        return self._want[fast]


@pytest.fixture(scope="module")
def batch_a(cuda):
    return Batch(*build_a(_cus()), SEED_A, cuda)


@pytest.fixture(scope="module")
def batch_b(cuda):
    return Batch(*build_b(_cus()), SEED_B, cuda)


def _assert_trips(n, frame, k):
    """More than k full trips of the frame on this device, or the test would
    pass without reaching the trips it is about."""
    wpc, cpg = frame
    ngroups = (n + cpg - 1) // cpg
    assert ngroups > k * wpc * _cus(), (ngroups, wpc, _cus())


@pytest.mark.gpu
def test_a_crc32_desc_xdma16(batch_a, cuda):
    """crc32_desc_xdma16: 2.25 trips of 12 waves per CU over groups of six shapes."""
    b = batch_a
    _assert_trips(b.n, XDMA16, 2)
    for what, od in b.orders():
        out = _canary(b.n, 4, cuda)
        m.crc32_desc(b.d_buf, b.d_offs, b.d_lens, od, out=out, variant="xdma16")
        _same(_crcs(out, b.n, what), b.crc(), f"crc32_desc xdma16, {what}")


@pytest.mark.gpu
def test_a_md5crc32_desc(batch_a, cuda):
    """md5crc32_desc_xdma16<false>, the same frame; bytes 20..31 of a record zero."""
    b = batch_a
    _assert_trips(b.n, XDMA16, 2)
    for what, od in b.orders():
        out = _canary(b.n, 32, cuda)
        m.md5crc32_desc(b.d_buf, b.d_offs, b.d_lens, od, out=out)
        r = _records(out, b.n, what)
        _same(r[:, :16], b.md5(), f"md5crc32_desc md5, {what}")
        _same(r[:, 16:20], b.crc(), f"md5crc32_desc crc, {what}")
        assert not r[:, 20:].any(), f"{what}: bytes 20..31 of a record not zero"


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(m.DESC_VARIANTS))
def test_a_digest_desc(batch_a, cuda, variant):
    """Every MD5 descriptor kernel on batch A.  BALANCED (4 waves per CU, groups
    from a counter) takes 6.75 trips with the shapes in arbitrary order; the
    others are one workgroup per group."""
    b = batch_a
    _assert_trips(b.n, BALANCED, 2)
    for what, od in b.orders():
        out = _canary(b.n, 16, cuda)
        m.digest_desc(b.d_buf, b.d_offs, b.d_lens, od, out=out, variant=variant)
        _same(_records(out, b.n, what), b.md5(), f"digest_desc {variant}, {what}")


@pytest.mark.gpu
def test_a_fastcrc_xdma16(batch_a, cuda):
    """crc32_fast_xdma16 (F = 1000) on batch A's 32-chunk window groups: 4.5 trips."""
    b = batch_a
    _assert_trips(b.n, FAST_XDMA, 2)
    for what, od in b.orders():
        out = _canary(b.n, 4, cuda)
        m.crc32_desc(b.d_buf, b.d_offs, b.d_lens, od, fastcrc=A_FAST, out=out)
        _same(_crcs(out, b.n, what), b.crc(A_FAST), f"crc32_desc fastcrc {A_FAST}, {what}", 32)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", B_FAST)
def test_b_fastcrc(batch_b, cuda, fast):
    """crc32_fast_pipe (F = 64, 128) at 4.25 trips of 16 waves per CU: the next
    group in flight, both ring slots reused, pipelined groups between groups
    that fall back; F = 100 takes the same batch through crc32_fast_xdma16."""
    b = batch_b
    pipe = fast in (64, 128)
    _assert_trips(b.n, FAST_PIPE if pipe else FAST_XDMA, 4)
    out = _canary(b.n, 4, cuda)
    m.crc32_desc(b.d_buf, b.d_offs, b.d_lens, fastcrc=fast, out=out)
    _same(_crcs(out, b.n, fast), b.crc(fast), f"crc32_desc fastcrc {fast}", 32)


@pytest.fixture(scope="module")
def fixed_blob(cuda):
    """Random bytes for batch B's chunk count at a 272-B stride."""
    n = build_b(_cus())[0].size
    host = gen.xorshift_array(n * 272 + trips.PAD, seed=0xF17ED)
    return n, host, _dev(host, cuda)


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [64, 128, 1000])
def test_fixed_fastcrc(fixed_blob, cuda, fast):
    """crc32_fixed with a window (FastWindows without descriptor arrays), batch
    B's trip count: 256 B on the line (pipelined for 64 and 128) and 250 B at
    a 272-B stride (a ragged tail window: every group falls back).  Chunks no
    longer than the window (F = 1000) are hashed whole by crc32_fixed_xdma16."""
    n, host, dev = fixed_blob
    _assert_trips(n, FAST_PIPE, 4)
    for L, stride in ((256, 256), (250, 272)):
        want = gen.oracle_crc32_batch(host, np.arange(n, dtype=np.uint64) * stride,
                                      np.full(n, L, dtype=np.uint32), fast)
        out = _canary(n, 4, cuda)
        m.crc32_fixed(dev, n, L, stride, fastcrc=fast, out=out)
        _same(_crcs(out, n, (L, stride)), want, f"crc32_fixed fastcrc {fast}, {L} B at stride {stride}", 32)


@pytest.mark.gpu
def test_fixed_dual_off_the_grid_later_trips(cuda):
    """md5crc32_desc_xdma16<true> past one trip: 192-B chunks at stride 197 from
    base + 3 (the off-grid twin of test_dual_digest.test_fixed_second_grid_trip)."""
    n, L = 12 * _cus() * 64 + 65, 192
    _assert_trips(n, XDMA16, 1)
    stride, skew = L + 5, 3
    host = gen.xorshift_array(skew + n * stride + trips.PAD, seed=0x197)
    offs = skew + np.arange(n, dtype=np.uint64) * stride
    lens = np.full(n, L, dtype=np.uint32)
    out = _canary(n, 32, cuda)
    m.md5crc32_fixed(_dev(host, cuda)[skew:], n, L, stride, out=out)
    r = _records(out, n, "off the grid")
    _same(r[:, :16], gen.oracle_digests(host, offs, lens), "md5crc32_fixed off the grid: md5")
    _same(r[:, 16:20], gen.oracle_crc32_batch(host, offs, lens), "md5crc32_fixed off the grid: crc")
    assert not r[:, 20:].any()


@pytest.mark.gpu
def test_fixed_dual_huge_stride(cuda):
    """md5crc32_fixed at a stride past the fixed loader's 32-bit group offsets
    (>= 2^31 / 64): the descriptor kernel with implicit offsets."""
    import torch
    n, L, stride = 5, 16384, 40 << 20
    assert stride >= (1 << 31) // 64
    dev = torch.empty((n - 1) * stride + L, dtype=torch.uint8, device=cuda)
    m.fill_synthetic(dev, seed=0x40)
    torch.cuda.synchronize()
    host = np.concatenate([dev[i * stride:i * stride + L].cpu().numpy() for i in range(n)])
    offs = np.arange(n, dtype=np.uint64) * L
    lens = np.full(n, L, dtype=np.uint32)
    out = _canary(n, 32, cuda)
    m.md5crc32_fixed(dev, n, L, stride, out=out)
    r = _records(out, n, "huge stride")
    _same(r[:, :16], gen.oracle_digests(host, offs, lens), "md5crc32_fixed huge stride: md5")
    _same(r[:, 16:20], gen.oracle_crc32_batch(host, offs, lens), "md5crc32_fixed huge stride: crc")
    assert not r[:, 20:].any()
    del dev
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_crc_split_past_one_trip(cuda):
    """crc32_split (2 workgroups of 4 waves per CU, a chunk per wave) past its
    8 * CUs-chunk trip: 0-3,000 B chunks at any alignment, ordered and not; and
    2 KiB windows over 2,049-6,000 B chunks."""
    import torch
    n = 20 * _cus() + 3
    assert n > 2 * 8 * _cus()
    rng = np.random.default_rng(0x5B117)
    for fast, lo, hi in ((0, 0, 3001), (2048, 2049, 6001)):
        lens = rng.integers(lo, hi, n).astype(np.uint32)
        offs = (np.cumsum(lens, dtype=np.uint64) - lens).astype(np.uint64)     # 1-B packing
        host = gen.xorshift_array(int(lens.sum()) + trips.PAD, seed=fast + 7)
        want = gen.oracle_crc32_batch(host, offs, lens, fast)
        dev = _dev(host, cuda)
        t_off = torch.from_numpy(offs.astype(np.int64)).to(cuda)
        t_len = torch.from_numpy(lens.astype(np.int32)).to(cuda)
        for od in (None, _dev(m.plan_order(lens).astype(np.int32), cuda)):
            out = _canary(n, 4, cuda)
            m.crc32_desc(dev, t_off, t_len, od, fastcrc=fast, out=out, variant="split")
            _same(_crcs(out, n, fast), want, f"crc32_split fastcrc {fast}, ordered {od is not None}", 1)


@pytest.mark.gpu
def test_balanced_counter_across_launches_and_streams(batch_a, cuda):
    """BALANCED's per-stream group counter on 3 trips of its 4-wave frame:
    three launches back to back on one stream (the middle one of 70 chunks
    leaves most waves nothing to take, and every launch must find the counter
    reset), then the same launch on two side streams before either is
    synchronised (each stream owns a counter)."""
    import torch
    b = batch_a
    n = 3 * BALANCED[0] * _cus() * 64 + 37
    assert n <= b.n
    _assert_trips(n, BALANCED, 2)

    def launch(k, stream=None):
        out = _canary(k, 16, cuda)
        m.digest_desc(b.d_buf, b.d_offs[:k], b.d_lens[:k], out=out, stream=stream, variant="balanced")
        return k, out

    outs = [launch(n), launch(70), launch(n)]
    for i, (k, out) in enumerate(outs):
        _same(_records(out, k, i), b.md5()[:k], f"balanced launch {i} of 3 ({k} chunks)")
    side = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    outs = [_canary(n, 16, cuda) for _ in side]
    for s in side:
        s.wait_stream(torch.cuda.current_stream())       # the canaries are filled on this one
    for s, out in zip(side, outs):
        m.digest_desc(b.d_buf, b.d_offs[:n], b.d_lens[:n], out=out, stream=s, variant="balanced")
    for s in side:
        s.synchronize()
    for i, out in enumerate(outs):
        _same(_records(out, n, i), b.md5()[:n], f"balanced on side stream {i}")


# ----------------------------------------------------------------- canary row, the other entries
CANARY_N = (1, 63, 65, 130)


@pytest.fixture(scope="module")
def small(cuda):
    """130 ragged chunks (1-B packed and 16-B packed) and a fixed-length blob."""
    import torch
    rng = np.random.default_rng(130)
    lens = np.concatenate([[0, 1, 55, 56, 63, 64, 65, 127, 128, 129, 300, 5000],
                           rng.integers(0, 2000, max(CANARY_N) - 12)]).astype(np.uint32)
    packs = {}
    for align in (1, 16):
        adv = (lens.astype(np.int64) + align - 1) // align * align
        offs = (np.cumsum(adv) - adv).astype(np.uint64)
        host = gen.xorshift_array(int(adv.sum()) + trips.PAD, seed=align)
        packs[align] = dict(host=host, dev=_dev(host, cuda), offs=offs,
                            d_offs=torch.from_numpy(offs.astype(np.int64)).to(cuda))
    d_lens = torch.from_numpy(lens.astype(np.int32)).to(cuda)
    blob = gen.xorshift_array(max(CANARY_N) * 1040 + trips.PAD, seed=0xB10B)
    return dict(lens=lens, d_lens=d_lens, packs=packs, blob=blob, d_blob=_dev(blob, cuda))


# (length, stride, skew): on the line, on the 16-B grid, off it
FIXED_CASES = [(256, 256, 0), (1000, 1008, 0), (100, 112, 0), (200, 203, 1), (0, 16, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(m.VARIANTS))
def test_canary_digest_fixed(small, cuda, variant):
    host, dev = small["blob"], small["d_blob"]
    for L, stride, skew in FIXED_CASES:
        for n in CANARY_N:
            offs = skew + np.arange(n, dtype=np.uint64) * stride
            want = gen.oracle_digests(host, offs, np.full(n, L, dtype=np.uint32))
            out = _canary(n, 16, cuda)
            m.digest_fixed(dev[skew:], n, L, stride, out=out, variant=variant)
            _same(_records(out, n, (L, n)), want, f"digest_fixed {variant} {L} B stride {stride} n {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(m.DESC_VARIANTS))
def test_canary_digest_desc(small, cuda, variant):
    lens = small["lens"]
    for align, p in small["packs"].items():
        want = gen.oracle_digests(p["host"], p["offs"], lens)
        for n in CANARY_N:
            for od in (None, _dev(m.plan_order(lens[:n]).astype(np.int32), cuda)):
                out = _canary(n, 16, cuda)
                m.digest_desc(p["dev"], p["d_offs"][:n], small["d_lens"][:n], od, out=out, variant=variant)
                _same(_records(out, n, (align, n)), want[:n],
                      f"digest_desc {variant} align {align} n {n} ordered {od is not None}")


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 128])
@pytest.mark.parametrize("variant", list(m.CRC_VARIANTS))
def test_canary_crc32(small, cuda, variant, fast):
    """crc32_fixed and crc32_desc: with a window, the pair-XOR store at c >> 1
    and the ragged last group of window rows."""
    host, dev = small["blob"], small["d_blob"]
    for L, stride, skew in FIXED_CASES:
        for n in CANARY_N:
            offs = skew + np.arange(n, dtype=np.uint64) * stride
            want = gen.oracle_crc32_batch(host, offs, np.full(n, L, dtype=np.uint32), fast)
            out = _canary(n, 4, cuda)
            m.crc32_fixed(dev[skew:], n, L, stride, fastcrc=fast, out=out, variant=variant)
            _same(_crcs(out, n, (L, n)), want, f"crc32_fixed {variant} fastcrc {fast} {L} B n {n}", 1)
    lens = small["lens"]
    for align, p in small["packs"].items():
        want = gen.oracle_crc32_batch(p["host"], p["offs"], lens, fast)
        for n in CANARY_N:
            for od in (None, _dev(m.plan_order(lens[:n]).astype(np.int32), cuda)):
                out = _canary(n, 4, cuda)
                m.crc32_desc(p["dev"], p["d_offs"][:n], small["d_lens"][:n], od, fastcrc=fast, out=out,
                             variant=variant)
                _same(_crcs(out, n, (align, n)), want[:n],
                      f"crc32_desc {variant} fastcrc {fast} align {align} n {n} ordered {od is not None}", 1)
