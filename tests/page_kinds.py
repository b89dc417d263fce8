"""Constructed 64-lane groups for the paged kernels of
sproxy_amd/csrc/md5_pages.hip (tests/test_page_kinds.py).  Pure numpy: test
infrastructure, the product never imports this module.

pages_group walks a group's page index p and decides per p, wave-uniformly,
how page p of every lane is read: lane by lane (some lane's page is off the
16-B grid), not at all (no lane has a 128-B stage in it), or as an LDS-DMA
image, non-temporally when every staged row starts on a 128-B line.  Within
an image a row may be clamped, or stand in for a lane that has no stage at p:
one whose page holds under 128 bytes, one whose chunk ended on an earlier
page, a dead lane.  A lane's state is carried from one page index to the next
whatever their kinds, and what is left of its last page -- an odd 64-B block,
then len % 64 bytes -- is finished by the lane itself from wherever that page
lies.  md5_update_ctx_pages adds a route per group and the rebuild of in[];
crc32_pages_fast a pipelined path per 64-row group and the reasons a group
leaves it.  This module

  * restates those conditions in numpy (classify_pages, classify_ctx,
    classify_windows), with every address range the kernels read,
  * names the groups that reach each of them on purpose (KINDS, ctx_combos,
    window_kinds), every kind with the page kinds and flags it claims, and
  * packs kinds back to back into one batch per page size (Layout) in
    test_pages.Paged's layout -- slots of P + 128 bytes, a slot and a skew per
    table entry -- with two arrangements: the identity and one that shuffles
    whole groups and rotates the lanes inside each, so a group keeps its
    composition while mrow and the row-to-lane mapping move.

A lane is (length, skew of each of its pages); lengths are whole pages plus
128 * stages + extra, the extras cycling over loader_kinds.EXTRAS (the tail
residues 0, 1, 55, 56, 63 with both parities of the 64-B block count, and
100), one step further in every group.  Every skew is under 128, so whatever
a kernel reads of a page -- the 17th dword of a block off the dword grid, the
granule past a tail -- stays inside that page's slot."""
import numpy as np

import loader_kinds as lk

PAD = 128                    # test_pages.PAD: a slot is page_bytes + PAD
EXTRAS = lk.EXTRAS
OFF_SKEWS = (1, 2, 3, 4, 8, 12, 20, 33)         # off the 16-B grid: on the dword grid (4, 8, 12, 20) and off it
PAGE_KINDS = ("lane", "skip", "lined", "unlined")
STAGE_FLAGS = ("clamp", "standin_own", "standin_ended", "mrow_nz", "plain", "standin_dead", "smax1")
LANE_SUBS = ("ring", "alignbit0", "alignbit")


def pages_of(length, P):
    return (int(length) + P - 1) // P


def _align(addr):
    """How a lane reads from `addr`: 16-B loads, dwords with a zero funnel
    shift, dwords shifted."""
    return "a16" if addr % 16 == 0 else "a4" if addr % 4 == 0 else "odd"


def _block_reads(addr, nblk):
    """nblk 64-B blocks from addr: load_block, or load_block_unaligned's 16
    dwords from the dword at or before addr, a 17th when addr is off the
    dword grid."""
    if nblk == 0:
        return []
    if addr % 16 == 0:
        return [(addr, addr + 64 * nblk)]
    lo = addr - addr % 4
    return [(lo, lo + 64 * nblk + (4 if addr % 4 else 0))]


def _tail_reads(addr, r):
    """load_tail: the 16-B granules that hold the r bytes at addr, or, off the
    16-B grid, the dwords that do."""
    if r == 0:
        return []
    if addr % 16 == 0:
        return [(addr, addr + (r + 15) // 16 * 16)]
    lo = addr - addr % 4
    return [(lo, lo + 4 * ((addr % 4 + r + 3) // 4))]


def _range_reads(addr, n):
    """lane_range: n bytes from addr, blocks and tail."""
    return _block_reads(addr, n >> 6) + _tail_reads(addr + (n >> 6 << 6), n & 63)


# ----------------------------------------------------------------- pages_group
def classify_pages(lens, page_addrs, P, live):
    """What pages_group computes for one 64-lane group: lens[l] bytes in lane
    l (dead lanes, l >= live: 0), page_addrs[l] the addresses of its pages.

    pages[p]: kind ("lane", "skip", "lined", "unlined") and flags -- for
    "lane" the branches taken by lanes with a stage (LANE_SUBS), for stages
    STAGE_FLAGS and mrow.  chunks[l] (live lanes): the epilogue's class.
    reads: every (lo, hi) address range the group reads."""
    lens = np.asarray(lens, np.int64)
    lane = np.arange(64)
    lv = lane < live
    assert not lens[~lv].any()
    npg = (lens + P - 1) // P
    pmax = int(npg.max())
    pages, reads = [], []
    for p in range(pmax):
        own = p < npg
        addr = np.array([int(page_addrs[l][p]) if own[l] else 0 for l in range(64)], np.int64)
        rest = np.where(own, lens - p * P, 0)
        nbytes = np.minimum(rest, P)
        nst = nbytes >> 7
        if (own & (addr % 16 != 0)).any():
            subs = set()
            for l in np.flatnonzero(nst > 0):
                subs.add({"a16": "ring", "a4": "alignbit0", "odd": "alignbit"}[_align(int(addr[l]))])
                reads += _block_reads(int(addr[l]), 2 * int(nst[l]))
            pages.append(dict(kind="lane", flags=subs))
            continue
        smax = int(nst.max())
        if smax == 0:
            pages.append(dict(kind="skip", flags=set()))
            continue
        lined = not ((nst != 0) & (addr % 128 != 0)).any()
        mrow = int(np.flatnonzero(nst == smax)[0])
        rows = np.where(nst == 0, smax, nst)
        rmin = int(rows.min()) - 1
        f = set()
        if smax - 1 > rmin:
            f.add("clamp")
        if (own & (nst == 0)).any():
            f.add("standin_own")                   # a page of under 128 bytes: the chunk's last
        if (lv & ~own & (npg > 0)).any():
            f.add("standin_ended")                 # addr == 0, aliased to mrow
        if (lv & (npg == 0)).any():
            f.add("standin_empty")
        if live < 64:
            f.add("standin_dead")
        if mrow != 0:
            f.add("mrow_nz")
        if smax == 1:
            f.add("smax1")
        if not f & {"clamp", "standin_own", "standin_ended", "standin_empty", "mrow_nz"}:
            f.add("plain")
        # a row reads its own stages, clamped to its last; a stand-in row those of row mrow
        reads += [(int(addr[l]), int(addr[l]) + 128 * int(nst[l])) for l in np.flatnonzero(nst > 0)]
        pages.append(dict(kind="lined" if lined else "unlined", flags=f, mrow=mrow, smax=smax, rmin=rmin,
                          nst=nst.copy()))
    chunks = []
    for l in range(live):
        L = int(lens[l])
        if L == 0:
            chunks.append(dict(empty=True))
            continue
        last = int(page_addrs[l][npg[l] - 1])
        lastb = L - (int(npg[l]) - 1) * P
        nfull, r = lastb >> 6, L & 63
        if nfull & 1:
            reads += _block_reads(last + 64 * (nfull - 1), 1)
        reads += _tail_reads(last + 64 * nfull, r)
        chunks.append(dict(empty=False, align=_align(last), odd_block=bool(nfull & 1),
                           tail="r0" if r == 0 else "lt56" if r < 56 else "ge56",
                           lastpage="under64" if lastb < 64 else "full" if lastb == P else "between"))
    return dict(pmax=pmax, pages=pages, chunks=chunks, reads=reads, live=live)


def page_seq(g):
    return tuple(pg["kind"] for pg in g["pages"])


# ----------------------------------------------------------------- md5_update_ctx_pages
def classify_ctx(lens, page_addrs, P, live, pending):
    """md5_update_ctx_pages for one group of 64 contexts: pending[l] bytes wait
    in context l.  route: "loader" (pages_group's walk: `walk`) or "lane";
    lanes[l] (live, len > 0) on the loader route: where the block kept in
    in[] comes from -- "in" (len < 64: in[] itself), "last" or "prev" page --
    with the alignment class of the page it comes from and of the page the
    tail comes from.  reads as classify_pages."""
    lens, pending = np.asarray(lens, np.int64), np.asarray(pending, np.int64)
    if ((lens != 0) & (pending != 0)).any():
        reads, off = [], False
        for l in range(live):
            L, t = int(lens[l]), int(pending[l])
            if L == 0:
                continue
            pa = [int(a) for a in page_addrs[l][:pages_of(L, P)]]
            off |= any(a % 16 for a in pa)
            if t and L < 64 - t:
                reads.append((pa[0], pa[0] + L))
                continue
            pos = 64 - t if t else 0
            if t:
                reads.append((pa[0], pa[0] + pos))
            nblk = (L - pos) >> 6
            for b in range(nblk):                  # a block inside a page: block_words; else byte by byte
                s = pos + 64 * b
                e, q = divmod(s, P)
                if q + 64 <= P:
                    reads += _block_reads(pa[e] + q, 1)
                else:
                    reads += [(pa[e] + q, pa[e] + P), (pa[e + 1], pa[e + 1] + 64 - (P - q))]
            s = pos + 64 * nblk
            r = L - s
            if r:
                e, q = divmod(s, P)
                c1 = min(r, P - q)
                reads.append((pa[e] + q, pa[e] + q + c1))
                if r > c1:
                    reads.append((pa[e + 1], pa[e + 1] + r - c1))
        return dict(route="lane", off_grid=off, reads=reads, lanes={})
    walk = classify_pages(lens, page_addrs, P, live)
    lanes, reads = {}, list(walk["reads"])
    for l in range(live):
        L = int(lens[l])
        if L == 0:
            continue
        n = pages_of(L, P)
        last = int(page_addrs[l][n - 1])
        lastb = L - (n - 1) * P
        tail = last + (lastb >> 6 << 6)
        if L < 64:
            src, blk = "in", None
        elif lastb >= 64:
            src, blk = "last", tail - 64
        else:                                      # len = kP + 1 .. kP + 63: the previous page's last block
            src, blk = "prev", int(page_addrs[l][n - 2]) + P - 64
        if blk is not None:
            reads += _block_reads(blk, 1)
        reads += _tail_reads(tail, L & 63)
        lanes[l] = dict(src=src, blk_align=None if blk is None else _align(blk), tail_align=_align(tail))
    return dict(route="loader", walk=walk, lanes=lanes, reads=reads,
                off_grid=any(pg["kind"] == "lane" for pg in walk["pages"]))


# ----------------------------------------------------------------- crc32_pages_fast
WINDOW_REASONS = ("short", "room", "len_off", "page_off", "F")


def classify_windows(lens, page_addrs, P, F, live_rows):
    """page_window for one 64-row group (32 chunks: rows 2k and 2k + 1 are
    chunk k's head and tail window): pipe, and when not the reasons -- "short"
    (a chunk of at most F bytes, an empty one included: its rows are not F
    bytes), "room" (a window with less room than F in its page), "len_off" (a
    window start off the 16-B grid by the chunk's length), "page_off" (by its
    page), "F" (neither 64 nor 128).  spans: the most pages one window
    touches.  reads as classify_pages."""
    reasons, reads, spans = set(), [], 0
    rows = []
    for i in range(live_rows):
        k, tail = i >> 1, i & 1
        L = int(lens[k])
        wlen = (0 if tail else L) if L <= F else F
        start = L - F if tail and L > F else 0
        e, q = divmod(start, P)
        room = P - q
        addr = int(page_addrs[k][e]) + q if wlen else 0
        if wlen != F:
            reasons.add("short")
        else:
            if F > room:
                reasons.add("room")
            if int(page_addrs[k][e]) % 16:
                reasons.add("page_off")
            if q % 16:
                reasons.add("len_off")
        rows.append((wlen, e, room, addr, k))
    if F not in (64, 128):
        reasons.add("F")
    pipe = not reasons
    for wlen, e, room, addr, k in rows:
        if pipe:
            reads.append((addr, addr + F))
            spans = max(spans, 1)
            continue
        left, n = wlen, 0
        while left:
            piece = min(left, room)
            reads += _range_reads(addr, piece)
            left -= piece
            n += 1
            if left:
                e += 1
                addr, room = int(page_addrs[k][e]), P
        spans = max(spans, n)
    if pipe and live_rows < 64:                     # dead lanes load the group's first window again
        reads.append((rows[0][3], rows[0][3] + F))
    return dict(pipe=pipe, reasons=reasons, spans=spans, reads=reads, live=live_rows)


# ----------------------------------------------------------------- the kinds
class PKind:
    """A named group at page size P: lanes = [(length, (skew of page 0, ...))],
    and what it claims: `seq`, the kinds of its first page indexes; `has`, (page
    kind, flag) pairs that some page index of it shows under either
    arrangement; `first_has`, those that hold while the group keeps its lane
    order (mrow_nz is about which lane comes first)."""

    def __init__(self, name, P, lanes, seq=None, has=(), first_has=()):
        self.name, self.P, self.seq = name, P, None if seq is None else tuple(seq)
        self.lanes = [(int(L), tuple(int(s) for s in sk)) for L, sk in lanes]
        self.has, self.first_has = set(has), set(first_has)
        for L, sk in self.lanes:
            assert len(sk) == pages_of(L, P) and all(0 <= s < 128 for s in sk), name


_made = [0]


def _mk(name, P, shape, skews, n=64, **claims):
    """shape(l) -> (whole pages, 128-B stages past them, extra or None for the
    EXTRAS cycle); skews(l, p, np) -> the skew of lane l's page p of np."""
    rot = _made[0]
    _made[0] += 1
    lanes = []
    for l in range(n):
        full, st, extra = shape(l)
        L = full * P + 128 * st + (EXTRAS[(l + rot) % len(EXTRAS)] if extra is None else extra)
        k = pages_of(L, P)
        lanes.append((L, [skews(l, p, k) for p in range(k)]))
    return PKind(name, P, lanes, **claims)


def _on_line(l, p, k):
    return 0


def _off_line(l, p, k):
    return 16 * (1 + (l + 3 * p) % 7)


def _last_off(l, p, k):
    return OFF_SKEWS[(l + l // 8) % 8] if p == k - 1 else 0


def _stair(P):
    return lambda l: (l % 4, l % 3, None)


def _last_bytes(P, whole=lambda l: 2):
    """whole(l) whole pages and 1 .. P bytes of one more: 128 * s + extra for
    every s a page holds, the empty remainder read as a full page."""
    spp = P // 128

    def shape(l):
        s, e = l % spp, EXTRAS[(l // spp + l) % len(EXTRAS)]
        return (whole(l), s, e) if s or e else (whole(l) + 1, 0, 0)
    return shape


def _kinds():
    P, K = 256, []
    # the eleven at P = 256
    K.append(_mk("two_full_lined", P, lambda l: (2, 0, 0), _on_line, seq=("lined", "lined"), has={("lined", "plain")}))
    K.append(_mk("aligned_off_line_mixed", P, lambda l: (l % 3, (l // 3) % 2, None), _off_line,
                 has={("unlined", "clamp"), ("unlined", "standin_own"), ("unlined", "standin_ended")},
                 first_has={("unlined", "mrow_nz")}))
    K.append(_mk("staircase", P, _stair(P), _on_line,
                 has={("lined", "clamp"), ("lined", "standin_own"), ("lined", "standin_ended")},
                 first_has={("lined", "mrow_nz")}))
    K.append(_mk("page1_no_stage", P, lambda l: (1, 0, None), _on_line, seq=("lined", "skip"),
                 has={("lined", "plain")}))
    K.append(_mk("staircase_lane41_off4", P, _stair(P), lambda l, p, k: 4 if (l, p) == (41, 1) else 0,
                 seq=("lined", "lane", "lined", "lined"), has={("lane", "ring"), ("lane", "alignbit0")}))
    K.append(_mk("last_page_off", P, _last_bytes(P), _last_off, seq=("lined", "lined", "lane"),
                 has={("lined", "plain"), ("lane", "alignbit0"), ("lane", "alignbit")}))
    K.append(_mk("last_page_off_mixed", P, _last_bytes(P, lambda l: (l // 2) % 3), _last_off,
                 seq=("lane", "lane", "lane"), has={("lane", "ring"), ("lane", "alignbit0"), ("lane", "alignbit")}))
    K.append(_mk("every_page_off", P, _stair(P), lambda l, p, k: OFF_SKEWS[(l + p) % 8],
                 seq=("lane",) * 4, has={("lane", "alignbit0"), ("lane", "alignbit")}))
    K.append(PKind("empty_64", P, [(0, ())] * 64, seq=()))
    K.append(_mk("one_six_pages_lane41", P, lambda l: (5, 1, None) if l == 41 else (0, l % 2, None), _on_line,
                 seq=("lined",) * 6, has={("lined", "standin_own"), ("lined", "standin_ended"), ("lined", "mrow_nz")}))
    # beyond them
    K.append(_mk("two_full_off_line", P, lambda l: (2, 0, 0), _off_line, seq=("unlined", "unlined"),
                 has={("unlined", "plain")}))
    K.append(_mk("off_line_then_lane9_off4", P, lambda l: (2, l % 2, None),
                 lambda l, p, k: 4 if (l, p) == (9, 1) else _off_line(l, p, k), seq=("unlined", "lane", "unlined"),
                 has={("lane", "ring"), ("lane", "alignbit0")}))
    K.append(_mk("off_line_one_long_lane63", P, lambda l: (3, 1, None) if l == 63 else (l % 2, 1, None), _off_line,
                 has={("unlined", "mrow_nz"), ("unlined", "standin_ended")}))
    K.append(_mk("ragged_37", P, _stair(P), _on_line, n=37, has={("lined", "standin_dead"), ("lined", "clamp")}))
    return K


KINDS = {
    256: _kinds(),
    # one stage a page at most
    128: [_mk("one_stage_pages", 128, lambda l: (1 + l % 3, 0, None), _on_line, has={("lined", "smax1")}),
          _mk("one_stage_pages_off_line", 128, lambda l: (l % 4, 0, None), _off_line,
              has={("unlined", "smax1"), ("unlined", "standin_ended")}),
          _mk("one_stage_pages_half_off", 128, lambda l: (1 + l % 2, 0, None),
              lambda l, p, k: OFF_SKEWS[(l // 2 + p) % 8] if l % 2 else 0,
              has={("lane", "ring"), ("lane", "alignbit"), ("lane", "alignbit0")})],
    # four stages a page: rows clamped inside one page, every lane owning it
    512: [_mk("clamp_in_page", 512, lambda l: (1, 1 + l % 3, None), _on_line, seq=("lined", "lined"),
              has={("lined", "plain"), ("lined", "clamp")}),
          _mk("clamp_in_page_off_line", 512, lambda l: (l % 2, 1 + l % 3, None), _off_line,
              has={("unlined", "clamp")})],
    # a page size that is no power of two: / P and % P
    384: [_mk("p384_last_off", 384, _last_bytes(384), _last_off, seq=("lined", "lined", "lane"),
              has={("lane", "alignbit0"), ("lane", "alignbit")}),
          _mk("p384_ragged_37", 384, _stair(384), _on_line, n=37, has={("lined", "standin_dead"), ("lined", "clamp")})],
    # netcache's page: 128 stages lane by lane, then the epilogue
    16384: [_mk("p16k_one_page_off", 16384, lambda l: (1, 0, 0) if l == 0 else (0, 127, None),
                lambda l, p, k: OFF_SKEWS[l % 8], seq=("lane",), has={("lane", "alignbit0"), ("lane", "alignbit")})],
}


def ctx_combos(P=256):
    """md5_update_ctx_pages' previous-page case: lengths kP + 1 .. kP + 63, the
    previous page and the last page on and off the 16-B grid independently."""
    def shape(l):
        return (1 + (l // 4) % 3, 0, 1 + (l * 5 + l // 4) % 63)

    def skews(l, p, k):
        if p == k - 2:
            return OFF_SKEWS[(l // 4) % 8] if l % 4 in (1, 3) else 0
        if p == k - 1:
            return OFF_SKEWS[(l // 4 + 3) % 8] if l % 4 in (2, 3) else 0
        return 0
    return _mk("ctx_prev_last_combos", P, shape, skews)


def window_kinds(P, F):
    """32-chunk groups (64 window rows) for crc32_pages_fast with window F.
    For F = 64 and 128 (any P >= 256): a pipelined group and, each alone in an
    otherwise pipelined group, the reasons to leave that path; for other F,
    windows spanning pages.  The ragged pipelined group comes last."""
    def simple(l):                                  # both windows inside one page, on the 16-B grid, L > F
        k, room = l % 3, (P - F) // 16
        j = (l * 7) % (room + 1)
        if k == 0 and j == 0:
            j = 1
        return k * P + F + 16 * j

    def kind(name, lens, skews=_on_line, **claims):
        lanes = [(L, [skews(l, p, pages_of(L, P)) for p in range(pages_of(L, P))]) for l, L in enumerate(lens)]
        return PKind(name, P, lanes, **claims)
    if F in (64, 128):
        base = [simple(l) for l in range(32)]

        def one(at, L):
            return base[:at] + [L] + base[at + 1:]
        return [
            kind("win_pipe_full", base),
            kind("win_pipe_off_line", base, _off_line),
            kind("win_one_short", one(13, F - 24)),
            kind("win_one_exactly_F", one(0, F)),
            kind("win_one_empty", one(31, 0)),
            kind("win_one_tail_straddles", one(7, P + 16)),            # the tail starts F - 16 bytes before a page end
            kind("win_one_length_off", one(21, P + F + 20)),           # and here 4 bytes off the grid, inside page 1
            kind("win_one_page_off4", base, lambda l, p, k: 4 if (l, p) == (5, k - 1) else 0),
            kind("win_one_page_off1", base, lambda l, p, k: 1 if (l, p) == (30, 0) else 0),
            kind("win_pipe_ragged_19", base[:19]),
        ]
    ex = EXTRAS
    return [
        kind("win_span_long", [F + P * (l % 4) + ex[l % len(ex)] for l in range(32)]),
        kind("win_span_long_off", [F + P * (l % 3) + ex[(l + 3) % len(ex)] for l in range(32)],
             lambda l, p, k: OFF_SKEWS[(l + p) % 8] if l % 2 else 16 * (p % 8)),
        kind("win_span_short_mix", [(F - 4 * (l % 9)) if l % 3 == 0 else F + 4 * l for l in range(32)]),
        kind("win_span_ragged_19", [F + 16 * (1 + l) for l in range(19)]),
    ]


# ----------------------------------------------------------------- packing
class Batch:
    """Chunks in launch order: lens, the table (first, slot and skew per
    entry), and per chunk the kind it was built as and its lane there."""

    def __init__(self, lay, chunks):
        self.lay, self.P, self.ids = lay, lay.P, np.asarray(chunks, np.int64)
        self.lens = lay.lens[self.ids]
        need = [len(lay.slots[c]) for c in self.ids]
        self.first = np.concatenate([[0], np.cumsum(need)]).astype(np.int64)
        self.slot = np.asarray([s for c in self.ids for s in lay.slots[c]], np.int64)
        self.skew = np.asarray([s for c in self.ids for s in lay.skews[c]], np.int64)
        self.n = self.ids.size

    def at(self):
        """Byte offset of every table entry's page in the pool."""
        return self.slot * (self.P + PAD) + self.skew

    def page_addrs(self, base, i):
        """Addresses of the pages of the chunk at position i."""
        return base + self.at()[self.first[i]:self.first[i + 1]]

    def groups(self, base, order=None, cpg=64):
        """(position of the group's first chunk, lens[64 or 32], page
        addresses per lane, live) for every group of the launch; position i
        holds chunk order[i] of this batch (None: i)."""
        at = base + self.at()
        idx = np.arange(self.n) if order is None else np.asarray(order, np.int64)
        for f in range(0, self.n, cpg):
            c = idx[f:f + cpg]
            lens = np.zeros(cpg, np.int64)
            lens[:c.size] = self.lens[c]
            pa = [at[self.first[k]:self.first[k + 1]] for k in c] + [np.zeros(0, np.int64)] * (cpg - c.size)
            yield f, lens, pa, c.size

    def kind_of(self, i):
        """(kind, lane in it) of the chunk at position i of this batch."""
        return self.lay.kind_of(int(self.ids[i]))


class Layout:
    """Kinds of one page size packed back to back (cpg lanes each; only the
    last may have fewer).  Every table entry gets a slot of its own from a
    seeded permutation, so no two pages overlap; the pool is slots * (P + 128)
    + 128 bytes.  perm: whole groups shuffled (a short one stays last), lanes
    rotated inside each."""

    def __init__(self, kinds, cpg=64, seed=0x9A6E):
        assert len({k.P for k in kinds}) == 1
        assert all(len(k.lanes) == cpg for k in kinds[:-1]) and 0 < len(kinds[-1].lanes) <= cpg
        self.kinds, self.P, self.cpg = kinds, kinds[0].P, cpg
        rng = np.random.default_rng(seed)
        lanes = [(g, l, L, sk) for g, kd in enumerate(kinds) for l, (L, sk) in enumerate(kd.lanes)]
        self.lens = np.asarray([x[2] for x in lanes], np.int64)
        self.where = [(x[0], x[1]) for x in lanes]
        E = sum(len(x[3]) for x in lanes)
        free = rng.permutation(E).tolist()
        self.slots = [[free.pop() for _ in x[3]] for x in lanes]
        self.skews = [list(x[3]) for x in lanes]
        self.nslots = max(E, 1)
        self.pool_bytes = self.nslots * (self.P + PAD) + PAD
        full = len(kinds) - (len(kinds[-1].lanes) < cpg)
        perm = []
        for g in list(rng.permutation(full)) + list(range(full, len(kinds))):
            live = len(kinds[g].lanes)
            r = int(rng.integers(1, live)) if live > 1 else 0
            perm += [g * cpg + (j + r) % live for j in range(live)]
        self.perm = np.asarray(perm, np.int64)
        self.n = self.lens.size
        assert np.array_equal(np.sort(self.perm), np.arange(self.n))

    def kind_of(self, c):
        g, l = self.where[c]
        return self.kinds[g], l

    def batch(self, permuted=False):
        """The batch in built order, or built in the kind-preserving order."""
        return Batch(self, self.perm if permuted else np.arange(self.n))


def in_own_slots(reads, base, P, pool_bytes):
    """Every read range lies inside the pool and inside one slot."""
    S = P + PAD
    for lo, hi in reads:
        if not (base <= lo < hi <= base + pool_bytes and (lo - base) // S == (hi - 1 - base) // S):
            return (lo - base, hi - base)
    return None


# what tests/test_page_kinds.py launches: per page size the kinds above, the context combinations among
# those at P = 256, a ragged kind last
BATCHES = {P: list(ks) for P, ks in KINDS.items()}
BATCHES[256] = KINDS[256][:-1] + [ctx_combos(256)] + KINDS[256][-1:]
WINDOW_P = {64: 256, 128: 256, 132: 128, 1000: 128}        # the page size each window F is run at
