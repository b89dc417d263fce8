"""The batcher's slot routes as a table: what a slot of
sproxy_amd/csrc/md5_submit.c does with a submission -- how the bytes get in,
which descriptor arrays the kernel reads, which order is built, which kernel
runs and how the digests get out -- at every switch point, from both sides.

A case is a short script of public calls on one batcher or queue: how it is
created, the digest kind and fastcrc window, the gather mode, the registered
host ranges, and its submissions.  Every chunk is named by offset and length
in one of three arenas the runner owns: H (host memory, page aligned), D
(device memory) and O (device memory for digests, 0xAA before the case).
tests/test_slot_routes.py runs the table on the CPU against the recording
fake runtime (tests/c/slot_check.c) and holds `expect` against the records;
tests/test_slot_routes_gpu.py runs it through sproxy_amd.md5 on the device
and compares every digest with hashlib and zlib.

The expectations are written from include/md5hip.h and the comments of
md5_submit.c, never taken from a run.  A record names memory by the
allocation it lies in (tests/c/fake_hip.c): `dev:SIZE+OFF`, `mapped:SIZE+OFF`
(the descriptor arrays a small slot's kernel reads in place), `pin:SIZE+OFF`,
or `H+OFF`, `D+OFF`, `O+OFF`; class Names gives each of a slot's buffers its
name from the creation arguments.

Synchronous single submissions launch from the caller, so their records are
exact.  A coalesced case (`coalesced=True`) first sends BLOCKER, alone, as an
asynchronous submission at in-flight target 1 -- held in flight on the CPU by
fake_hip_hold, an 8 MiB chain on the device -- then its own submissions, which
share the open slot, then lets go.  Its records are those after the blocker's
launch, and because the progress thread may plan the open slot ahead the
expectation is on the final plan: of the planning records before the hash
launch (order builds, bucket and order copies, the LINES choice) only the
last plan's are compared.  `sum_desc` cases compare the descriptor copies by
their total, since a plan made ahead copies a first part early.
"""

MD5, CRC32, MD5_CRC32 = 0, 1, 2
DSZ = {MD5: 16, CRC32: 4, MD5_CRC32: 32}
GATHER_HOST, GATHER_DEVICE, GATHER_DMA, GATHER_AUTO = 0, 1, 2, 3
XDMA, LINES = 4, 7                         # enum md5hip_desc_variant
CRC_XDMA16, CRC_SPLIT = 6, 7               # enum crc32hip_variant
DUAL_XDMA16, DUAL_FEDSPLIT = 1, 2          # enum md5crc32hip_variant
FEDSPLIT_MIN_LEN = 1024                    # MD5CRC32HIP_FEDSPLIT_MIN_LEN
HIST_KMAX = 1 << 17                        # MD5HIP_HIST_KMAX
CUS = 256                                  # the fake planner's device

PAGE = 4096
SLICE = 1 << 20                            # maxn 16,384 and segcap 4,096
H_BYTES = (2 << 20) + PAGE
D_BYTES = 9 << 20
O_BYTES = 1 << 20
DS = 8 << 20                               # small device chunks live past the long one
LONG = 8 << 20
BLOCKER = (0, LONG - 64)                   # the chunk a coalesced case queues behind
B1 = ("B", SLICE, 2)


def key(length):
    return (length >> 6) + 1


def up128(x):
    return (x + 127) & ~127


class Names:
    """A slot's buffers by allocation (batcher_new): cap bytes of staging,
    maxn descriptors, segcap table entries."""

    def __init__(self, create):
        how, a, _ = create
        if how == "B":
            self.cap = (a + 4095) & ~4095
            self.maxn = min(max(4096, self.cap // 64), 1 << 20)
        else:
            self.cap, self.maxn = 16 << 20, a
        self.segcap = max(4096, self.cap // 1024)
        self.DATA, self.HDATA = f"dev:{self.cap}", f"pin:{self.cap}"
        self.MOFF, self.MLEN = f"mapped:{8 * self.maxn}", f"mapped:{4 * self.maxn}"
        self.DOFF, self.DLEN = f"dev:{8 * self.maxn}", f"dev:{4 * self.maxn}"
        self.DORD, self.HORD = f"dev:{4 * self.maxn}", f"pin:{4 * self.maxn}"
        self.DIG, self.HDIG = f"dev:{32 * self.maxn}", f"pin:{32 * self.maxn}"
        self.DTAB, self.HTAB = f"dev:{24 * self.segcap}", f"pin:{24 * self.segcap}"
        self.DBKT, self.HBKT = f"dev:{4 * (HIST_KMAX + 2)}", f"pin:{4 * (HIST_KMAX + 2)}"
        self.SORT = f"dev:{4 * self.maxn + 256}"


class Sub:
    """One submission.  entry: ptrs (chunks = [(H offset, length)]), iov
    (chunks = [[(H offset, length), ...]]), dev (chunks = [(D offset,
    length)]), hostfixed / devfixed (fixed = (base offset, n, length,
    stride)).  out: "h" = a host array, or the byte offset into O."""

    def __init__(self, entry, chunks=None, out="h", fixed=None):
        self.entry, self.chunks, self.out, self.fixed = entry, chunks, out, fixed
        self.n = fixed[1] if fixed else len(chunks)

    def pieces(self, i):
        """chunk i as [(arena, offset, length)]"""
        if self.fixed:
            base, _, length, stride = self.fixed
            return [("D" if self.entry == "devfixed" else "H", base + i * stride, length)]
        if self.entry == "iov":
            return [("H", o, ln) for o, ln in self.chunks[i]]
        return [("D" if self.entry == "dev" else "H",) + tuple(self.chunks[i])]

    def words(self, sync):
        w = ["sub", self.entry, int(sync), "h" if self.out == "h" else "d", 0 if self.out == "h" else self.out, self.n]
        if self.fixed:
            base, _, length, stride = self.fixed
            return w + [base, length, stride]
        for c in self.chunks:
            if self.entry == "iov":
                w.append(len(c))
                for o, ln in c:
                    w += [o, ln]
            else:
                w += list(c)
        return w


class Case:
    def __init__(self, id, subs, expect, stats, create=B1, kind=MD5, fastcrc=0, gather=None, regs=(),
                 coalesced=False, refuse=0, only=None, sum_desc=False):
        self.id, self.subs, self.expect, self.stats = id, subs, expect, stats
        self.create, self.kind, self.fastcrc, self.gather, self.regs = create, kind, fastcrc, gather, regs
        self.coalesced, self.refuse, self.only, self.sum_desc = coalesced, refuse, only, sum_desc

    def script(self):
        """the case for tests/c/slot_check.c"""
        w = ["case", self.id, "create", *self.create]
        if self.kind != MD5 or self.fastcrc:
            w += ["digest", self.kind, self.fastcrc]
        if self.gather is not None:
            w += ["gather", self.gather]
        if self.refuse:
            w += ["refuse", self.refuse]
        for off, nbytes in self.regs:
            w += ["reg", off, nbytes]
        if self.coalesced:
            w += ["inflight", 1, "hold", *Sub("dev", [BLOCKER]).words(False), "mark"]
        for s in self.subs:
            w += s.words(not self.coalesced)
        if self.coalesced:
            w += ["release"]
        return " ".join(str(x) for x in w + ["waitall", "end"])


# ------------------------------------------------------------------ what the header says
def lines_variant(unlined, payload):
    """md5hip_lines_choice: XDMA becomes LINES past half"""
    return LINES if 2 * unlined > payload else XDMA


def crc_variant(n, mean):
    """enum crc32hip_variant: SPLIT for up to 128 chunks per CU of >= 2 KiB, 12 per CU shorter"""
    return CRC_SPLIT if n <= (128 if mean >= 2048 else 12) * CUS else CRC_XDMA16


def dual_variant(n, mean):
    """md5crc32hip_plan: FEDSPLIT for at most one 64-chunk group per CU, mean_len >=
    MD5CRC32HIP_FEDSPLIT_MIN_LEN and n <= CUs x mean_len / 256"""
    return DUAL_FEDSPLIT if n and (n + 63) // 64 <= CUS and mean >= FEDSPLIT_MIN_LEN and n * 256 <= CUS * mean \
        else DUAL_XDMA16


def unlined_of(chunks):
    """payload in device-resident chunks that start on 16 B but not on 128 B"""
    return sum(ln for o, ln in chunks if o % 128 and o % 16 == 0)


def ends(seq):
    """the entries a hash record shows: the first four and the last"""
    n = len(seq)
    return [seq[k] for k in sorted({0, 1, 2, 3, n - 1} & set(range(n)))]


def copy(direction, nbytes, dst, src):
    return f"copy|{direction}|{nbytes}|{dst}|{src}"


def staged_at(nm, lens):
    """chunks packed on 128-B lines: (names, staging bytes used)"""
    at, used = [], 0
    for ln in lens:
        at.append(f"{nm.DATA}+{used}")
        used += up128(ln)
    return at, used


def order_device(nm, n, kmax, direct):
    """the bucket table first, then md5hip_order_device on the lengths the kernel will read"""
    return [copy("H2D", 4 * (kmax + 1), nm.DBKT + "+0", nm.HBKT + "+0"),
            f"order|device|{nm.MLEN if direct else nm.DLEN}+0|{n}|{kmax}|{nm.DBKT}+0|{nm.DORD}+0"]


def desc_copies(nm, lo, hi):
    """descriptor entries [lo, hi) to the device"""
    return [copy("H2D", 8 * (hi - lo), f"{nm.DOFF}+{8 * lo}", f"{nm.MOFF}+{8 * lo}"),
            copy("H2D", 4 * (hi - lo), f"{nm.DLEN}+{4 * lo}", f"{nm.MLEN}+{4 * lo}")]


def launch(nm, kind, fastcrc, lens, at, *, order=None, unlined=0, bytes_in=(), out=None, digests=(),
           copied=None):
    """One descriptor launch of `lens` (as staged) at `at`: descriptors, order,
    bytes in, kernel, digests out.  order: None (keys non-increasing), "device",
    "stable", "refused", "host", "host_sorted".  copied: the descriptor copies
    if not the whole slot at once."""
    n, payload = len(lens), sum(lens)
    direct = n <= 4096
    kmax = max(key(ln) for ln in lens)
    r = []
    if not direct:
        r += desc_copies(nm, 0, n) if copied is None else copied
    if order == "device":
        r += order_device(nm, n, kmax, direct)
    elif order in ("stable", "refused"):
        r.append(f"order|stable|{nm.DLEN}+0|{n}|{kmax}|{nm.SORT}+0|{nm.DORD}+0|{'done' if order == 'stable' else 'refused'}")
        if order == "refused":
            r += order_device(nm, n, kmax, direct)
    elif order in ("host", "host_sorted"):
        r.append(f"plan_desc|{nm.MLEN}+0|{n}|{nm.HORD}+0")
        if order == "host":
            r.append(copy("H2D", 4 * n, nm.DORD + "+0", nm.HORD + "+0"))
    r.append(f"choice|lines|{XDMA}|{unlined}|{payload}")
    r += list(bytes_in)
    mean = (payload + 64 * n) // n - 64                     # load / n - 64
    if kind == CRC32:
        cn, cm = (2 * n, fastcrc) if fastcrc else (n, mean)
        r.append(f"choice|crc|{cn}|{cm}")
        what, variant = "crc_desc", crc_variant(cn, cm)
    elif kind == MD5_CRC32:
        r.append(f"choice|dual|{n}|{mean}")
        what, variant = "dual_desc", dual_variant(n, mean)
    else:
        what, variant = "md5_desc", lines_variant(unlined, payload)
    arrays = f"{nm.MOFF}+0|{nm.MLEN}+0" if direct else f"{nm.DOFF}+0|{nm.DLEN}+0"
    ordered = order not in (None, "host_sorted")
    r.append(f"hash|{what}|{variant}|{n}|{fastcrc}|{nm.DATA}+0|{arrays}|{nm.DORD + '+0' if ordered else 'NULL'}|"
             f"{out or nm.DIG + '+0'}|at={','.join(ends(at))}|lens={','.join(str(x) for x in ends(lens))}")
    return r + list(digests)


def to_host(nm, kind, n):
    return [copy("D2H", DSZ[kind] * n, nm.HDIG + "+0", nm.DIG + "+0")]


def table(nm, segs, dst):
    """a gather table's copy and launch: segs = [(source, destination, length)]"""
    return [copy("H2D", 24 * len(segs), nm.DTAB + "+0", nm.HTAB + "+0"), f"gather|{len(segs)}|{nm.DTAB}+0|{dst}+0"] + \
           [f"seg|{s}|{d}|{ln}" for s, d, ln in segs]


def scatter(nm, segs):
    """digests out of the slot's array: segs = [(byte offset in it, O offset, length)]"""
    return table(nm, [(f"{nm.DIG}+{a}", f"O+{o}", ln) for a, o, ln in segs], nm.DIG)


def gathered(nm, segs):
    """registered pages into the staging: segs = [(H offset, staging offset, length)]"""
    return table(nm, [(f"H+{h}", f"{nm.DATA}+{d}", ln) for h, d, ln in segs], nm.DATA)


def dev_at(chunks):
    return [f"D+{o}" for o, _ in chunks]


def stats(launches=1, tickets=1, chunks=0, staged=0):
    return dict(launches=launches, coalesced_launches=int(tickets > 1), max_tickets_per_launch=tickets,
                max_chunks_per_launch=chunks, bytes_staged=staged)


def pages(first, count):
    return [(p * PAGE, PAGE) for p in range(first, first + count)]


def strided(n, length, step, first=DS):
    return [(first + step * i, length) for i in range(n)]


# ------------------------------------------------------------------ the cases
def _bytes_in():
    nm, c = Names(B1), []
    # staged: one H2D of `used` bytes, chunks on 128-B lines
    ch = [(5, 129), (1000, 128), (3001, 100)]
    lens = [ln for _, ln in ch]
    at, used = staged_at(nm, lens)
    assert (at, used) == ([f"{nm.DATA}+0", f"{nm.DATA}+256", f"{nm.DATA}+384"], 512)
    c.append(Case("staged_ptrs", [Sub("ptrs", ch)],
                  launch(nm, MD5, 0, lens, at, bytes_in=[copy("H2D", 512, nm.DATA + "+0", nm.HDATA + "+0")],
                         digests=to_host(nm, MD5, 3)),
                  stats(chunks=3, staged=512)))
    # zero-copy DEVICE: pieces merge while source and destination both run on, up to 64 KiB
    ch = [pages(0, 16), [(20 * PAGE, PAGE), (22 * PAGE, PAGE)],
          [(30 * PAGE, 128)], [(30 * PAGE + 128, 128)],          # both run on: one entry across two chunks
          [(31 * PAGE, 100)], [(31 * PAGE + 100, 100)]]          # the source runs on, the 128-B lines do not
    lens = [sum(ln for _, ln in x) for x in ch]
    at, used = staged_at(nm, lens)
    assert used == 74240
    segs = [(0, 0, 65536), (20 * PAGE, 65536, PAGE), (22 * PAGE, 69632, PAGE), (30 * PAGE, 73728, 256),
            (31 * PAGE, 73984, 100), (31 * PAGE + 100, 74112, 100)]
    c.append(Case("zc_device_64k_block", [Sub("iov", ch)],
                  launch(nm, MD5, 0, lens, at, bytes_in=gathered(nm, segs), digests=to_host(nm, MD5, 6)),
                  stats(chunks=6, staged=used), gather=GATHER_DEVICE, regs=[(0, 64 * PAGE)]))
    ch = [pages(0, 17)]
    c.append(Case("zc_device_64k_block_plus_page", [Sub("iov", ch)],
                  launch(nm, MD5, 0, [17 * PAGE], [nm.DATA + "+0"],
                         bytes_in=gathered(nm, [(0, 0, 65536), (65536, 65536, PAGE)]), digests=to_host(nm, MD5, 1)),
                  stats(chunks=1, staged=17 * PAGE), gather=GATHER_DEVICE, regs=[(0, 64 * PAGE)]))
    # zero-copy DMA: one copy per run, past 64 KiB, never across two registrations
    ch = [pages(20, 17), pages(14, 4)]
    lens = [17 * PAGE, 4 * PAGE]
    at, used = staged_at(nm, lens)
    dma = [copy("H2D", 17 * PAGE, nm.DATA + "+0", f"H+{20 * PAGE}"),
           copy("H2D", 2 * PAGE, f"{nm.DATA}+{17 * PAGE}", f"H+{14 * PAGE}"),
           copy("H2D", 2 * PAGE, f"{nm.DATA}+{19 * PAGE}", f"H+{16 * PAGE}")]
    c.append(Case("zc_dma_runs", [Sub("iov", ch)],
                  launch(nm, MD5, 0, lens, at, bytes_in=dma, digests=to_host(nm, MD5, 2)),
                  stats(chunks=2, staged=used), gather=GATHER_DMA, regs=[(0, 16 * PAGE), (16 * PAGE, 32 * PAGE)]))
    # AUTO: DMA while ndma * 256 KiB <= used
    K256 = 256 << 10
    for id, ch, runs in (("auto_runs_of_256k_dma", [[(0, K256)], [(2 * K256, K256)]], None),
                         ("auto_one_run_dma", [[(0, K256)], [(K256, K256)]], None),
                         ("auto_three_runs_device", [[(0, K256)], [(2 * K256, K256 // 2), (3 * K256, K256 // 2)]],
                          [(0, 0, K256), (2 * K256, K256, K256 // 2), (3 * K256, K256 + K256 // 2, K256 // 2)])):
        at, used = staged_at(nm, [K256, K256])
        if runs:
            bytes_in = gathered(nm, runs)
        elif id == "auto_one_run_dma":
            bytes_in = [copy("H2D", 2 * K256, nm.DATA + "+0", "H+0")]
        else:
            bytes_in = [copy("H2D", K256, nm.DATA + "+0", "H+0"), copy("H2D", K256, f"{nm.DATA}+{K256}", f"H+{2 * K256}")]
        c.append(Case(id, [Sub("iov", ch)],
                      launch(nm, MD5, 0, [K256, K256], at, bytes_in=bytes_in, digests=to_host(nm, MD5, 2)),
                      stats(chunks=2, staged=used), gather=GATHER_AUTO, regs=[(0, 1 << 20)]))
    # one unregistered segment: the whole call is staged
    c.append(Case("unregistered_segment_staged", [Sub("iov", [[(0, PAGE), (1 << 20, 100)]])],
                  launch(nm, MD5, 0, [PAGE + 100], [nm.DATA + "+0"],
                         bytes_in=[copy("H2D", up128(PAGE + 100), nm.DATA + "+0", nm.HDATA + "+0")],
                         digests=to_host(nm, MD5, 1)),
                  stats(chunks=1, staged=up128(PAGE + 100)), gather=GATHER_DEVICE, regs=[(0, 16 * PAGE)]))
    # a chunk of ns segments may take ns + 3 table entries: 4,093 fit segcap, 4,094 do not
    for ns, zc in ((4093, True), (4094, False)):
        ch = [[(16 * k, 16) for k in range(ns)]]
        bytes_in = gathered(nm, [(0, 0, 16 * ns)]) if zc else [copy("H2D", up128(16 * ns), nm.DATA + "+0", nm.HDATA + "+0")]
        c.append(Case(f"chunk_of_{ns}_segments_{'zero_copy' if zc else 'staged'}", [Sub("iov", ch)],
                      launch(nm, MD5, 0, [16 * ns], [nm.DATA + "+0"], bytes_in=bytes_in, digests=to_host(nm, MD5, 1)),
                      stats(chunks=1, staged=up128(16 * ns)), gather=GATHER_DEVICE, regs=[(0, 32 * PAGE)]))
    # a CRC-32 slot with window F: only 2F bytes of a chunk longer than 2F
    F = 128
    lens = [2 * F, 2 * F, F]                                  # as staged, of 2F + 1, 2F and F
    at, used = staged_at(nm, lens)
    c.append(Case("crc_window_staged", [Sub("ptrs", [(3, 2 * F + 1), (1001, 2 * F), (2002, F)])],
                  launch(nm, CRC32, F, lens, at, bytes_in=[copy("H2D", used, nm.DATA + "+0", nm.HDATA + "+0")],
                         digests=to_host(nm, CRC32, 3)),
                  stats(chunks=3, staged=used), kind=CRC32, fastcrc=F))
    segs = [(16, 0, F), (16 + F + 1, F, F), (1024, 256, 2 * F), (2048, 512, F)]
    c.append(Case("crc_window_zero_copy", [Sub("ptrs", [(16, 2 * F + 1), (1024, 2 * F), (2048, F)])],
                  launch(nm, CRC32, F, lens, at, bytes_in=gathered(nm, segs), digests=to_host(nm, CRC32, 3)),
                  stats(chunks=3, staged=used), kind=CRC32, fastcrc=F, gather=GATHER_DEVICE, regs=[(0, 16 * PAGE)]))
    # fixed slots: one copy (DMA in place from a wholly pinned source), the fixed entry of the kind
    fx = (64, 5, 100, 128)
    span = 4 * 128 + 100
    for id, regs, src, staged in (("host_fixed_pinned", [(0, 16 * PAGE)], "H+64", 0),
                                  ("host_fixed_pageable", [], nm.HDATA + "+0", span)):
        c.append(Case(id, [Sub("hostfixed", fixed=fx)],
                      [copy("H2D", span, nm.DATA + "+0", src), f"hash|md5_fixed|5|100|128|0|{nm.DATA}+0|{nm.DIG}+0",
                       *to_host(nm, MD5, 5)],
                      stats(chunks=5, staged=staged), regs=regs))
    c.append(Case("host_fixed_crc_window", [Sub("hostfixed", fixed=(64, 5, 200, 256))],
                  [copy("H2D", 4 * 256 + 200, nm.DATA + "+0", nm.HDATA + "+0"),
                   f"hash|crc_fixed|5|200|256|64|{nm.DATA}+0|{nm.DIG}+0", *to_host(nm, CRC32, 5)],
                  stats(chunks=5, staged=4 * 256 + 200), kind=CRC32, fastcrc=64))
    c.append(Case("device_fixed_dual_in_place", [Sub("devfixed", fixed=(DS + 16, 4, 1000, 1008), out=0)],
                  [f"hash|dual_fixed|4|1000|1008|0|D+{DS + 16}|O+0"], stats(chunks=4), kind=MD5_CRC32))
    c.append(Case("device_fixed_md5_to_host", [Sub("devfixed", fixed=(DS + 16, 4, 1000, 1008))],
                  [f"hash|md5_fixed|4|1000|1008|0|D+{DS + 16}|{nm.DIG}+0", *to_host(nm, MD5, 4)], stats(chunks=4)))
    return c


def _descriptors_and_order():
    nm, c = Names(B1), []
    # at most 4,096 chunks: the mapped host arrays, nothing copied; 4,097: copied
    for n in (4096, 4097):
        ch = strided(n, 64, 64)
        c.append(Case(f"device_{n}_chunks", [Sub("dev", ch)],
                      launch(nm, MD5, 0, [64] * n, dev_at(ch), unlined=unlined_of(ch), digests=to_host(nm, MD5, n)),
                      stats(chunks=n)))
    # a device-resident submission of >= 8,192 chunks copies early; the launch copies what followed
    a, b = strided(8192, 64, 64), strided(10, 64, 64)
    early = desc_copies(nm, 0, 8192) + desc_copies(nm, 8192, 8202)
    c.append(Case("early_copy_8192", [Sub("dev", a), Sub("dev", b)],
                  launch(nm, MD5, 0, [64] * 8202, dev_at(a + b), unlined=unlined_of(a + b), copied=early,
                         digests=to_host(nm, MD5, 8202)),
                  stats(launches=2, tickets=2, chunks=8202), coalesced=True))
    # with nothing appended after it the launch copies nothing
    c.append(Case("early_copy_8192_alone", [Sub("dev", a)],
                  launch(nm, MD5, 0, [64] * 8192, dev_at(a), unlined=unlined_of(a), digests=to_host(nm, MD5, 8192)),
                  stats(launches=2, chunks=8192), coalesced=True))
    a = strided(8191, 64, 64)
    c.append(Case("no_early_copy_8191", [Sub("dev", a), Sub("dev", b)],
                  launch(nm, MD5, 0, [64] * 8201, dev_at(a + b), unlined=unlined_of(a + b),
                         digests=to_host(nm, MD5, 8201)),
                  stats(launches=2, tickets=2, chunks=8201), coalesced=True, sum_desc=True))
    # keys non-increasing as reserved: no order; only the last chunk breaks it: order_device on the mapped lengths
    for id, lens, order in (("keys_non_increasing_no_order", [320] + [256] * 7, None),
                            ("last_chunk_breaks_order", [256] * 7 + [320], "device")):
        ch = [(DS + 512 * i, ln) for i, ln in enumerate(lens)]
        c.append(Case(id, [Sub("dev", ch)],
                      launch(nm, MD5, 0, lens, dev_at(ch), order=order, digests=to_host(nm, MD5, 8)), stats(chunks=8)))
    # unsorted and more than 4,096 chunks: the stable order; refused: order_device on the copied lengths
    ch = strided(4096, 64, 128) + [(DS, 128)]
    lens = [ln for _, ln in ch]
    for id, order, refuse, only in (("unsorted_4097_stable_order", "stable", 0, None),
                                    ("stable_order_refused", "refused", 1, "cpu")):
        c.append(Case(id, [Sub("dev", ch)],
                      launch(nm, MD5, 0, lens, dev_at(ch), order=order, digests=to_host(nm, MD5, 4097)),
                      stats(chunks=4097), refuse=refuse, only=only))
    # a key past MD5HIP_HIST_KMAX (a chunk of 8 MiB): the host plan and one order copy
    for id, ch, order in (("key_at_kmax_device_order", [(DS, 100), (0, LONG - 64)], "device"),
                          ("key_past_kmax_host_order", [(DS, 100), (0, LONG)], "host"),
                          ("key_past_kmax_sorted_no_order", [(0, LONG), (DS, 100)], "host_sorted")):
        c.append(Case(id, [Sub("dev", ch)],
                      launch(nm, MD5, 0, [ln for _, ln in ch], dev_at(ch), order=order, digests=to_host(nm, MD5, 2)),
                      stats(chunks=2)))
    return c


def _kernels():
    nm, c = Names(B1), []
    # LINES exactly past half the payload in chunks on 16 B but not on 128 B
    tie = [(DS + 16, 256), (DS + 1024, 192), (DS + 3003, 64)]         # a chunk off 16 B is not counted
    for id, ch in (("lines_tie_keeps_xdma", tie), ("lines_tie_plus_one_chunk", tie + [(DS + 2064, 64)])):
        c.append(Case(id, [Sub("dev", ch)],
                      launch(nm, MD5, 0, [ln for _, ln in ch], dev_at(ch), unlined=unlined_of(ch),
                             digests=to_host(nm, MD5, len(ch))),
                      stats(chunks=len(ch))))
    assert unlined_of(tie) == 256 and unlined_of(tie + [(DS + 2064, 64)]) == 320
    # CRC-32: the choice of (n, load / n - 64); 3,073 chunks are SPLIT only from a mean of 2,048
    for id, last in (("crc_mean_2048", 2048), ("crc_mean_2047", 2047)):
        ch = strided(3072, 2048, 16) + [(DS + 16 * 3072, last)]
        c.append(Case(id, [Sub("dev", ch)],
                      launch(nm, CRC32, 0, [ln for _, ln in ch], dev_at(ch), unlined=unlined_of(ch),
                             digests=to_host(nm, CRC32, 3073)),
                      stats(chunks=3073), kind=CRC32))
    assert crc_variant(3073, 2048) == CRC_SPLIT and crc_variant(3073, 2047) == CRC_XDMA16
    # one-pass: md5crc32hip_plan(n, mean) around MD5CRC32HIP_FEDSPLIT_MIN_LEN
    for id, last in (("dual_mean_1024", 1024), ("dual_mean_1023", 1023)):
        ch = [(DS, 1024), (DS + 1024, last)]
        c.append(Case(id, [Sub("dev", ch)],
                      launch(nm, MD5_CRC32, 0, [1024, last], dev_at(ch), digests=to_host(nm, MD5_CRC32, 2)),
                      stats(chunks=2), kind=MD5_CRC32))
    return c


def pieces(length, spare):
    """enqueue_digests: pieces of 64 KiB as the table has room, in 16-B multiples"""
    extra = min((length + 65535) // 65536 - 1, spare)
    piece = ((length + extra) // (extra + 1) + 15) & ~15
    return [(at, min(piece, length - at)) for at in range(0, length, piece)]


def _digests_out():
    nm, c = Names(B1), []
    name = {MD5: "md5", CRC32: "crc", MD5_CRC32: "dual"}
    ch = strided(3, 200, 256)
    for kind in (MD5, CRC32, MD5_CRC32):
        dsz = DSZ[kind]
        # one device ticket filling the slot from chunk 0, 16-B aligned: in place
        c.append(Case(f"{name[kind]}_device_ticket_in_place", [Sub("dev", ch, out=0)],
                      launch(nm, kind, 0, [200] * 3, dev_at(ch), out="O+0"), stats(chunks=3), kind=kind))
        # the same 4 B off: scatter
        c.append(Case(f"{name[kind]}_device_ticket_4_off", [Sub("dev", ch, out=4)],
                      launch(nm, kind, 0, [200] * 3, dev_at(ch), digests=scatter(nm, [(0, 4, 3 * dsz)])),
                      stats(chunks=3), kind=kind))
    # two device tickets in one slot: one entry each
    a, b = strided(3, 200, 256), strided(2, 200, 256, DS + 1024)
    c.append(Case("two_device_tickets", [Sub("dev", a, out=0), Sub("dev", b, out=64)],
                  launch(nm, MD5, 0, [200] * 5, dev_at(a + b), digests=scatter(nm, [(0, 0, 48), (48, 64, 32)])),
                  stats(launches=2, tickets=2, chunks=5), coalesced=True))
    # more than 64 KiB of digests in a shared slot: pieces of 16-B multiples
    assert pieces(65536, 4094) == [(0, 65536)] and pieces(65552, 4094) == [(0, 32784), (32784, 32768)]
    assert pieces(65568, 4094) == [(0, 32784), (32784, 32784)]
    for id, kind, n in (("md5_4096_digests_one_piece", MD5, 4096), ("md5_4097_digests_two_pieces", MD5, 4097),
                        ("dual_2049_records_two_pieces", MD5_CRC32, 2049)):
        dsz = DSZ[kind]
        a, b = strided(n, 64, 64), [(DS, 64)]
        segs = [(at, at, ln) for at, ln in pieces(dsz * n, 4096 - 2)] + [(dsz * n, 65600, dsz)]
        c.append(Case(id, [Sub("dev", a, out=0), Sub("dev", b, out=65600)],
                      launch(nm, kind, 0, [64] * (n + 1), dev_at(a + b), unlined=unlined_of(a + b),
                             digests=scatter(nm, segs)),
                      stats(launches=2, tickets=2, chunks=n + 1), kind=kind, coalesced=True, sum_desc=True))
    # the piece count clipped by the spare table room: 4,094 one-chunk tickets leave room for one
    # more piece, 4,095 for none (a slot takes segcap = 4,096 tickets)
    for small, only in ((4094, "cpu"), (4095, "cpu")):
        subs = [Sub("dev", [(DS, 64)], out=65600 + 16 * k) for k in range(small)]
        big = strided(4097, 64, 64)
        subs.append(Sub("dev", big, out=0))
        spare = 4096 - (small + 1)
        segs = [(16 * k, 65600 + 16 * k, 16) for k in range(small)] + \
               [(16 * small + at, at, ln) for at, ln in pieces(65552, spare)]
        allch = [(DS, 64)] * small + big
        c.append(Case(f"pieces_after_{small}_tickets", subs,
                      launch(nm, MD5, 0, [64] * len(allch), dev_at(allch), unlined=unlined_of(allch),
                             digests=scatter(nm, segs)),
                      stats(launches=2, tickets=small + 1, chunks=len(allch)), coalesced=True, sum_desc=True, only=only))
    assert len(pieces(65552, 1)) == 2 and len(pieces(65552, 0)) == 1
    # a CRC-32 device ticket across slots of 5 chunks: the second slot's output is 4-B aligned only
    q = ("Q", 5, 3)
    qn = Names(q)
    ch = strided(10, 100, 128)
    first = launch(qn, CRC32, 0, [100] * 5, dev_at(ch[:5]), out="O+0")
    second = launch(qn, CRC32, 0, [100] * 5, dev_at(ch[5:]), digests=scatter(qn, [(0, 20, 20)]))
    c.append(Case("crc_ticket_spans_slots", [Sub("dev", ch, out=0)], first + second,
                  stats(launches=2, chunks=5), create=q, kind=CRC32))
    # host and device tickets in one slot: one D2H of dsz * n beside the scatter
    a, b = strided(2, 200, 256), strided(2, 200, 256, DS + 1024)
    c.append(Case("host_and_device_tickets", [Sub("dev", a), Sub("dev", b, out=0)],
                  launch(nm, MD5, 0, [200] * 4, dev_at(a + b), digests=scatter(nm, [(32, 0, 32)]) + to_host(nm, MD5, 4)),
                  stats(launches=2, tickets=2, chunks=4), coalesced=True))
    return c


def gather_shapes():
    """GPU only: what the gather kernel is given beyond the table -- sources at
    every residue of 16, the destination on and 3 B off 16 B, lengths 0, 1, 15,
    16, 17 and one unrolled trip of 4 x 256 x 16 B, -16 and +16.  Chunk = a
    prefix segment (0 or 3 bytes, moving the destination) and the segment
    itself, from a place that does not run on from the prefix (the sources
    may overlap: nothing writes them)."""
    trip = 4 * 256 * 16
    return [[(8, pre), (64 * PAGE + r, length)]
            for length in (0, 1, 15, 16, 17, trip - 16, trip, trip + 16) for r in range(16) for pre in (0, 3)]


# One half only.  CPU: the refused sort is the fake's control; the clipped
# piece count needs 4,095 tickets in one open slot, which the fake holds open
# as long as it takes and one 8 MiB chain on the device (~75 ms) does not --
# its arithmetic is the same `pieces` the shared-slot cases run on the device.
# GPU: the gather kernel's shapes mean nothing to the fake's memmove.
CPU_ONLY = ["stable_order_refused", "pieces_after_4094_tickets", "pieces_after_4095_tickets"]
GPU_ONLY = ["gather_shapes"]


def cases():
    c = _bytes_in() + _descriptors_and_order() + _kernels() + _digests_out()
    c.append(Case("gather_shapes", [Sub("iov", gather_shapes())], None, None, gather=GATHER_DEVICE,
                  regs=[(0, H_BYTES - PAGE)], only="gpu"))
    assert len({x.id for x in c}) == len(c)
    return c
