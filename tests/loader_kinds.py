"""Constructed 64-lane groups for the two LDS-DMA loaders of
sproxy_amd/csrc/md5_kernels.h (tests/test_loader_kinds.py).  Pure numpy: test
infrastructure, the product never imports this module.

desc_xpose_group (descriptors) and xdma_group (fixed stride) move the bytes of
almost every product kernel.  Per wave both depend on a handful of
wave-uniform quantities; a wrong clamp, stand-in row or hand-over between two
loops yields a wrong digest only for a group of exactly the right composition.
This module

  * restates those quantities in numpy (classify_desc, classify_fixed) for the
    three chunk sources of md5_kernels.h (desc_arrays, fixed_chunks,
    fast_windows),
  * names the groups that reach each path on purpose (KINDS, window_kinds,
    fixed_cases), every kind with the path and flags it claims, and
  * packs kinds back to back into one buffer (build) with two lane orders:
    the identity and a permutation that shuffles whole groups and rotates the
    lanes inside each one, so a group keeps its composition while mrow and
    the row-to-lane mapping move.

Stages are 128 B.  A lane is (length, offset of its start in its 128-B line);
lengths are 128 * stages + extra, the extras cycling over the tail residues
0, 1, 55, 56, 63 with both parities of the 64-B block count (and 100, the
extra of test_balanced_guard_free_stage_edges), one step further in every
group, so the leftover-block and finish code sees every lane position."""
import numpy as np

LINE = 128
PAD = 4096                   # bytes after the last chunk (whole-line loaders read on)
LEAD = 256                   # bytes before the first chunk (they also read back to the line)
RESIDUES = (0, 1, 55, 56, 63)
# 64 * parity + residue, all ten pairs, and 100
EXTRAS = (0, 65, 55, 120, 63, 64, 1, 119, 56, 127, 100)
LONG_BLOCKS = 4096           # kHybridLongBlocks: HYBRID's lane-direct waves

# kernel -> chunk source, LDS-DMA images per wave (NB), whole-line loads (kShift).
# (md5_update_ctx, the loader over LaneSpan, has its own harness: tests/ctx_paths.py.)
KERNELS = {
    "md5_desc_xdma": dict(src="desc", nb=1, shift=False),
    "md5_desc_lines": dict(src="desc", nb=1, shift=True),
    "md5_desc_hybrid": dict(src="desc", nb=1, shift=False, long=True),
    "md5_desc_balanced": dict(src="desc", nb=2, shift=False),
    "crc32_desc_xdma16": dict(src="desc", nb=1, shift=False),
    "md5crc32_desc_xdma16": dict(src="desc", nb=1, shift=False),
    "crc32_fast_xdma16": dict(src="windows", nb=1, shift=False),
    "md5crc32_desc_xdma16<implicit>": dict(src="fixed", nb=1, shift=False),
}
# the three loaders desc_xpose_group chooses from: run_stages, run_stages2, run_lines
STAGE_PATHS = ("run", "run2", "run_lines")


# ----------------------------------------------------------------- the chunk sources
def desc_arrays(addrs, lens):
    """DescArrays: row c is chunk c."""
    return np.asarray(addrs, np.int64), np.asarray(lens, np.int64)


def fixed_chunks(base_addr, n, stride, flen):
    """FixedChunks: row i at base + i * stride, flen bytes."""
    return base_addr + np.arange(n, dtype=np.int64) * stride, np.full(n, flen, np.int64)


def fast_windows(addrs, lens, F):
    """FastWindows: 2n rows; row 2k is chunk k's first F bytes and row 2k + 1 its
    last F; a chunk of at most F bytes is row 2k alone, row 2k + 1 empty at the
    chunk's start."""
    a, L = np.asarray(addrs, np.int64), np.asarray(lens, np.int64)
    long = L > F
    ra, rl = np.empty(2 * a.size, np.int64), np.empty(2 * a.size, np.int64)
    ra[0::2], ra[1::2] = a, np.where(long, a + L - F, a)
    rl[0::2], rl[1::2] = np.where(long, F, L), np.where(long, F, 0)
    return ra, rl


# ----------------------------------------------------------------- desc_xpose_group
def _group(a, L, live, k):
    """One wave: a, L the 64 lanes' addresses and lengths (dead lanes: the
    group's first row, length 0)."""
    lane = np.arange(64)
    lv = lane < live
    nfull = L >> 6
    nst = nfull >> 1
    smax, bmax = int(nst.max()), int(nfull.max())
    unaligned = bool((lv & ((a & 15) != 0)).any())
    g = dict(live=live, nfull=nfull, nst=nst, smax=smax, bmax=bmax, unaligned=unaligned, flags=set())
    f = g["flags"]
    if live < 64:
        f.add("ragged")
    if k.get("long") and bmax >= LONG_BLOCKS:      # (and the group among the first CUs)
        g["path"] = "lane_long"
        return g
    if unaligned:
        g["path"] = "lane_range"
        return g
    if smax == 0:
        g["path"] = "no_stage"
        return g
    mrow = int(np.flatnonzero(nst == smax)[0])
    rows = np.where(nst == 0, smax, nst)           # a row without a stage re-reads row mrow
    rlast = rows - 1
    rmin = int(rows.min()) - 1
    lined = not bool((lv & (nst != 0) & ((a & 127) != 0)).any())
    clamp = smax - 1 > rmin                        # the loaders' clamped issue branch is taken
    standin = np.flatnonzero(nst == 0)
    g.update(mrow=mrow, rlast=rlast, rmin=rmin, lined=lined, clamp=clamp, standin=standin)
    f.add("lined" if lined else "unlined")
    if clamp:
        f.add("clamp")
    if (lv & (nst == 0)).any():
        f.add("standin_live")
    if live < 64:
        f.add("standin_dead")
    if not clamp and standin.size == 0:
        f.add("uniform")
    if mrow != 0:
        f.add("mrow_nz")
    if smax == 1:
        f.add("smax1")
    f.add("smax_odd" if smax & 1 else "smax_even")
    if k["nb"] == 2:
        g["path"] = "run2"
        fmin = int(nst[lv].min())                  # stages every live lane holds
        g["fmin"] = fmin
        if fmin == 0:
            f.add("fmin0")                         # fmin - 1 wraps; the quad loop is skipped
            lim, quads = None, 0
        else:
            lim = min(rmin, fmin - 1)
            quads = lim // 4                       # for (stg = 0; stg + 4 <= lim; stg += 4)
            if lim in (3, 4, 7, 8, 9):
                f.add(f"lim{lim}")
        if rmin + 1 < fmin:
            f.add("fmin_gt")
        g.update(lim=lim, quads=quads)
        f.add(f"quads{min(quads, 2)}")
    elif k["shift"] and not lined:
        g["path"] = "run_lines"
        staged = lv & (nst != 0)
        sh = (a >> 4) & 7
        shs = set(int(x) for x in sh[staged])
        g["shs"] = shs
        if len(shs) == 8:
            f.add("sh_all8")
        if 0 in shs and len(shs) > 1:
            f.add("sh0_among_shifted")
        if (staged & (sh > 0) & (L == 128 * nst)).any():
            f.add("exact128k")                     # the last line serves its first sh pieces only
    else:
        g["path"] = "run"
    return g


def classify_desc(addrs, lens, order, n, kernel):
    """What desc_xpose_group computes for every 64-position group of a launch
    of `kernel` over n rows: row c at addrs[c] (an address, not an offset: the
    loader's alignment tests are on the pointer), lens[c] bytes, position i
    holding row order[i] (None: i).  A list of dicts: path, flags, and the
    quantities behind them."""
    k = KERNELS[kernel]
    addrs, lens = np.asarray(addrs, np.int64), np.asarray(lens, np.int64)
    idx = np.arange(n) if order is None else np.asarray(order, np.int64)[:n]
    out = []
    for first in range(0, n, 64):
        live = min(64, n - first)
        c = idx[first:first + live]
        a = np.full(64, addrs[idx[first]], np.int64)
        L = np.zeros(64, np.int64)
        a[:live], L[:live] = addrs[c], lens[c]
        out.append(_group(a, L, live, k))
    return out


# ----------------------------------------------------------------- xdma_group
def classify_fixed(base_addr, n, length, stride):
    """What xdma_group computes for every 64-chunk group of a fixed-stride
    launch: rows, nstage, the odd leftover block, tail bytes, lined, and the
    largest 32-bit buffer offset (voff + stg * 128) the group's loads carry
    (None without a stage)."""
    nfull = length >> 6
    nstage = nfull >> 1
    out = []
    for first in range(0, n, 64):
        rows = min(64, n - first)
        start = base_addr + first * stride
        lined = ((start | stride) & 127) == 0
        # row r of the image: chunk min(r, rows - 1); its 8 lanes take the
        # parts 0..7 in swizzled order, so the largest part offset is 112
        max_off = (rows - 1) * stride + 112 + (nstage - 1) * 128 if nstage else None
        out.append(dict(rows=rows, nstage=nstage, odd=bool(nfull & 1), tail=length & 63, lined=lined,
                        max_off=max_off))
    return out


# ----------------------------------------------------------------- the kinds
class Kind:
    """A named group: lanes = [(length, offset in the 128-B line)], and what it
    claims: `path` ("stage", "no_stage" or "lane_range"), `lined`, and flags
    that hold in every stage kernel / under BALANCED / under LINES' run_lines.
    `first_flags` hold while the group keeps its lane order (they are about
    which lane comes first)."""

    def __init__(self, name, lanes, path, lined=True, flags=(), balanced=(), lines=(), first_flags=()):
        self.name, self.lanes, self.path, self.lined = name, lanes, path, lined
        self.flags, self.balanced, self.lines = set(flags), set(balanced), set(lines)
        self.first_flags = set(first_flags)

    def expected_path(self, kernel):
        k = KERNELS[kernel]
        if self.path != "stage":
            return self.path
        if k["nb"] == 2:
            return "run2"
        return "run_lines" if k["shift"] and not self.lined else "run"


def _unlined(l):
    return 16 * ((3 * l + 1) % 8)           # all eight 16-B shifts, 0 among them (lane 5)


_made = [0]


def _mk(name, stages, align, path="stage", extra=None, nudge=None, **claims):
    """stages[l] 128-B stages in lane l; align: "l" (on the line), "u" (the
    _unlined cycle) or a function lane -> offset in the line."""
    where = {"l": lambda l: 0, "u": _unlined}.get(align, align)
    rot = _made[0]                          # the extras start one step further in every kind
    _made[0] += 1
    lanes = []
    for l, s in enumerate(stages):
        e = EXTRAS[(l + rot) % len(EXTRAS)] if extra is None else extra(l)
        lanes.append((128 * s + e, where(l) + (nudge(l) if nudge else 0)))
    lined = all(o % 128 == 0 for (L, o) in lanes if L >= 128)
    return Kind(name, lanes, path, lined=lined, **claims)


def _with(stages, **at):
    s = list(stages)
    for lane, v in at.items():
        s[int(lane[1:])] = v
    return s


def _parity(smax):
    return "smax_odd" if smax & 1 else "smax_even"


def _kinds():
    K = []
    for al in "lu":
        t = "@" + al
        K.append(_mk("no_stage" + t, [0] * 64, al, path="no_stage"))
        for k in (1, 2, 3, 4, 5, 8, 9, 10):
            lim = {4: "lim3", 5: "lim4", 8: "lim7", 9: "lim8", 10: "lim9"}
            K.append(_mk(f"uniform_{k}{t}", [k] * 64, al, flags={"uniform", _parity(k)} | ({"smax1"} if k == 1 else set()),
                         balanced={f"quads{min((k - 1) // 4, 2)}"} | ({lim[k]} if k in lim else set())))
        for k, lane in ((2, 11), (5, 40)):
            K.append(_mk(f"one_short_{k}{t}", _with([k] * 64, **{f"l{lane}": k - 1}), al, flags={"clamp"},
                         balanced={f"quads{(k - 2) // 4}"}))
        for k in (1, 4):
            for lane in (0, 37):
                K.append(_mk(f"one_none_{k}_lane{lane}{t}", _with([k] * 64, **{f"l{lane}": 0}), al,
                             flags={"standin_live"}, balanced={"fmin0", "quads0"},
                             first_flags={"mrow_nz"} if lane == 0 else ()))
        for k in (1, 4):
            K.append(_mk(f"one_long_{k}{t}", _with([k] * 64, l23=k + 9), al,
                         extra=lambda l: 17 if l == 23 else EXTRAS[l % len(EXTRAS)],
                         flags={"clamp", _parity(k + 9)}, balanced={f"quads{(k - 1) // 4}"},
                         first_flags={"mrow_nz"}))
        K.append(_mk("staircase" + t, [l % 9 for l in range(64)], al, flags={"clamp", "standin_live", "smax_even"},
                     balanced={"fmin0", "quads0"}, first_flags={"mrow_nz"}))
        # BALANCED's guard-free quads: rmin = lim, then a clamped guarded phase of either parity
        for lim in (3, 4, 7, 8, 9):
            for par in (1, 0):
                k = lim + 1
                smax = k + 2 if (k + 2) % 2 == par else k + 3
                K.append(_mk(f"quad_lim{lim}_{'odd' if par else 'even'}{t}", _with([k] * 64, l9=smax), al,
                             flags={"clamp", _parity(smax)}, balanced={f"lim{lim}", f"quads{lim // 4}"}))
        K.append(_mk("quad_fmin0" + t, _with([10] * 64, l44=0), al, flags={"standin_live"},
                     balanced={"fmin0", "quads0"}))
        K.append(_mk("one_off16" + t, _with([3] * 64, l50=2), al, path="lane_range",
                     nudge=lambda l: 4 if l == 21 else 0))
    base3 = _with([3] * 64, l50=2)
    K.append(_mk("lined", base3, "l", flags={"clamp"}))
    for s in range(1, 8):
        K.append(_mk(f"unlined_{s}", base3, lambda l, s=s: 16 * s, flags={"clamp"}))
    K.append(_mk("mixed_shift", base3, lambda l: 16 * (l % 8), flags={"clamp"}, lines={"sh_all8", "sh0_among_shifted"}))
    K.append(_mk("lined_and_unlined", base3, lambda l: 0 if l % 2 == 0 else 16 * ((l // 2) % 7 + 1),
                 flags={"clamp"}, lines={"sh_all8", "sh0_among_shifted"}))
    # every row that has a stage is on the line; rows without one are not: still `lined`
    K.append(_mk("stageless_unlined", _with([3] * 64, l7=0, l30=0), lambda l: 48 if l in (7, 30) else 0,
                 flags={"standin_live"}))
    # LINES
    K.append(_mk("line_smax1", [1] * 64, lambda l: 16 * (1 + l % 7), flags={"smax1", "uniform"}))
    K.append(_mk("line_exact128k", [1 + l % 3 for l in range(64)], lambda l: 16 * (1 + l % 7),
                 extra=lambda l: 0, flags={"clamp", "smax_odd"}, lines={"exact128k"}))
    for k in (3, 4):
        K.append(_mk(f"line_sh0_{'odd' if k & 1 else 'even'}", [k] * 64,
                     lambda l: 0 if l == 5 else 16 * (1 + l % 7),
                     flags={"uniform", _parity(k)}, lines={"sh0_among_shifted"}))
    return K


KINDS = _kinds()
# a batch's last group: fewer live lanes than 64
RAGGED = {
    "ragged_1": _mk("ragged_1", [3], lambda l: 16, flags={"standin_dead", "ragged"}),
    "ragged_37": _mk("ragged_37", _with([7] * 37, l20=6), "u", flags={"standin_dead", "ragged", "clamp"},
                     balanced={"quads1"}),
    "ragged_63": _mk("ragged_63", [1 + l % 4 for l in range(63)], "l", flags={"standin_dead", "ragged", "clamp"}),
    "ragged_5_no_stage": _mk("ragged_5_no_stage", [0] * 5, "u", path="no_stage", flags={"ragged"}),
}
BY_NAME = {k.name: k for k in KINDS}
# every kind is launched: the full ones and ragged_37 in one batch, the other ragged ones behind a group or alone
BATCHES = {
    "main": KINDS + [RAGGED["ragged_37"]],
    "lone_lane": [RAGGED["ragged_1"]],
    "ragged_63": [BY_NAME["staircase@u"], RAGGED["ragged_63"]],
    "ragged_no_stage": [BY_NAME["no_stage@l"], RAGGED["ragged_5_no_stage"]],
}


def window_kinds(F):
    """32-chunk groups (64 window rows) for crc32_fast_xdma16 with window F:
    a chunk longer than F whose length is F mod 16 has both windows on the
    16-B grid."""
    def k(name, lens, align, path="stage", **claims):
        where = {"l": lambda l: 0, "u": _unlined}[align]
        return Kind(name, [(int(L), where(l)) for l, L in enumerate(lens)], path, lined=False, **claims)
    ex = EXTRAS
    long_u = [F + 16 * (1 + l % 11) for l in range(32)]
    short = [128 * (l % (F // 128 + 1)) + ex[l % len(ex)] for l in range(32)]
    short = [min(s, F) for s in short]
    mix = [long_u[l] if l % 3 else short[l] for l in range(32)]
    mix[4], mix[7] = 0, F                                   # an empty chunk; one of exactly F (whole)
    return [
        k("win_uniform_lined", [F + 128 * (1 + l % 5) for l in range(32)], "l", flags={"uniform", "lined"}),
        k("win_uniform_unlined", long_u, "u", flags={"uniform", "unlined"}),
        k("win_short_mix", mix, "u", flags={"clamp", "standin_live"}),
        k("win_short_first", [100] + long_u[1:], "u", flags={"standin_live"}, first_flags={"mrow_nz"}),
        k("win_all_short", short, "l", flags={"clamp", "standin_live"}),
        k("win_tiny", [ex[l % len(ex)] for l in range(32)], "u", path="no_stage"),
        k("win_odd_tail", [F + 16 * (1 + l % 11) + (4 if l == 13 else 0) for l in range(32)], "u",
          path="lane_range"),
        k("win_ragged_19", mix[:19], "u", flags={"standin_dead", "ragged"}),
    ]


# ----------------------------------------------------------------- packing
class Packed:
    """Kinds packed back to back.  pos[c] is chunk c's place in a buffer that
    starts on a 128-B line; with align_base 16 the launch's base is 16 B into
    it (offs = pos - 16), so every address keeps its place in its line."""

    def __init__(self, kinds, pos, lens, total, perm, cpg):
        self.kinds, self.pos, self.lens, self.total, self.perm, self.cpg = kinds, pos, lens, total, perm, cpg
        self.n = lens.size

    def skew(self, align_base):
        assert align_base in (128, 16)
        return align_base % 128

    def offs(self, align_base):
        return (self.pos - self.skew(align_base)).astype(np.uint64)

    def orders(self):
        return (("identity", None), ("kind-preserving", self.perm))

    def kind_of(self, c):
        """The kind chunk c was built as."""
        return self.kinds[c // self.cpg]


def build(kinds, cpg=64, seed=0x10AD):
    """Pack `kinds` (cpg lanes each; only the last may have fewer) into one
    layout.  Every chunk starts in a fresh 128-B line at its lane's offset, at
    least 16 B after the chunk before it; the buffer (random bytes all over,
    so the gaps are live) is Packed.total bytes."""
    assert all(len(k.lanes) == cpg for k in kinds[:-1]) and 0 < len(kinds[-1].lanes) <= cpg
    pos, lens, at = [], [], LEAD
    for kd in kinds:
        for L, o in kd.lanes:
            at = (at + 16 + LINE - 1) // LINE * LINE
            pos.append(at + o)
            lens.append(L)
            at = at + o + L
    pos, lens = np.asarray(pos, np.int64), np.asarray(lens, np.int64)
    # whole groups shuffled (the short one stays last), lanes rotated inside each
    rng = np.random.default_rng(seed)
    full = len(kinds) - (len(kinds[-1].lanes) < cpg)
    perm = []
    for g in list(rng.permutation(full)) + list(range(full, len(kinds))):
        live = len(kinds[g].lanes)
        r = int(rng.integers(1, live)) if live > 1 else 0
        perm += [g * cpg + (j + r) % live for j in range(live)]
    perm = np.asarray(perm, np.uint32)
    assert np.array_equal(np.sort(perm), np.arange(lens.size))
    return Packed(kinds, pos, lens, int(at) + PAD, perm, cpg)


# ----------------------------------------------------------------- fixed-stride cases
FIXED_COUNTS = (1, 63, 64, 65, 130)


def _up(x, a):
    return (x + a - 1) // a * a


def fixed_cases():
    """(length, stride, base skew) for xdma_group: 0, 1, 2 and 5 stages with an
    odd block and without, every tail residue at both parities; per length a
    stride on the line, one off it (live gap bytes), and one on the line from
    a base 16 B off it."""
    out = []
    for i, nfull in enumerate((0, 1, 2, 3, 4, 5, 10, 11)):
        for r in (RESIDUES[i % 5], RESIDUES[(i + 2) % 5]):
            L = 64 * nfull + r
            on = max(_up(L, LINE), LINE)
            off = _up(L, 16) + 16
            if off % LINE == 0:
                off += 16
            out += [(L, on, 0), (L, off, 0), (L, on + LINE, 16)]
    return out
