"""The LDS-DMA loaders' group kinds in every kernel built on them.

desc_xpose_group and xdma_group (sproxy_amd/csrc/md5_kernels.h) decide per
wave, from a handful of wave-uniform quantities, which loop runs, which rows
are clamped, which row stands in for a row without a stage and where the
guard-free loop hands over to the guarded one.  tests/loader_kinds.py builds
64-lane groups that reach each of those on purpose and restates the loaders'
conditions in numpy.

CPU tests (-m "not gpu"): every kind classifies as it claims in every kernel,
for both lane orders and both base alignments; a coverage table (kernel x
path x flag) has a kind in every cell the kernel can reach and none in a cell
it cannot; the references agree with each other.

GPU tests: every kernel on every kind, bit-exact against hashlib.md5 and
zlib.crc32 of the host copy, a 0xAA canary record behind the last output, in
both orders, from a base on the 128-B line and from one 16 B off it; the
fixed-stride loader at 32-bit offsets just below 2^31, and the fallback just
past them."""
import hashlib
import zlib

import numpy as np
import pytest

import gen
import loader_kinds as lk
import sproxy_amd.md5 as m

BASE = 0x7F0000000000                 # a line-aligned stand-in for the device buffer's address
ALIGNS = (128, 16)
WINDOWS = (1024, 1000)                # crc32_fast_xdma16: on the 128-B stage grid and off it
DESC_KERNELS = [k for k, v in lk.KERNELS.items() if v["src"] == "desc"]
MD5_VARIANT = {"xdma": "md5_desc_xdma", "lines": "md5_desc_lines", "hybrid": "md5_desc_hybrid",
               "balanced": "md5_desc_balanced"}
SEED = 0x10ADE2
# the descriptor batches crc32_fast_xdma16 also runs, as window rows (beside lk.window_kinds)
WINDOW_BATCHES = ("main", "ragged_no_stage")

_packed = {}


def packed(name):
    """The batches the GPU tests launch, built once: lk.BATCHES, and per window
    F "win<F>" (32-chunk groups of lk.window_kinds)."""
    if name not in _packed:
        if name.startswith("win"):
            _packed[name] = lk.build(lk.window_kinds(int(name[3:])), cpg=32)
        else:
            _packed[name] = lk.build(lk.BATCHES[name])
    return _packed[name]


def _addrs(pk, ab):
    return BASE + pk.skew(ab) + pk.offs(ab).astype(np.int64)


def _window_rows(pk, ab, F, perm):
    """crc32_fast_xdma16 has no order array: a permuted launch permutes the
    descriptor arrays themselves."""
    a, L = _addrs(pk, ab), pk.lens
    if perm is not None:
        a, L = a[perm], L[perm]
    return lk.fast_windows(a, L, F)


# ----------------------------------------------------------------- CPU: the kinds are what they claim
def test_kind_names_are_unique_and_every_kind_is_launched():
    names = [k.name for k in lk.KINDS] + list(lk.RAGGED)
    assert len(set(names)) == len(names)
    for stem in ("no_stage", "uniform_1", "uniform_2", "uniform_3", "uniform_4", "uniform_5", "uniform_8",
                 "uniform_9", "one_short", "one_none", "one_long", "staircase", "lined", "unlined_1", "unlined_7",
                 "mixed_shift", "lined_and_unlined", "one_off16", "quad_lim3", "quad_lim4", "quad_lim7",
                 "quad_lim8", "quad_lim9", "quad_fmin0", "line_smax1", "line_exact128k", "line_sh0_odd",
                 "line_sh0_even", "ragged_1", "ragged_37", "ragged_63"):
        assert any(n.startswith(stem) for n in names), stem
    launched = {k.name for b in lk.BATCHES.values() for k in b}
    assert launched == set(names), "every kind is in a launched batch"


def test_lanes_cycle_residues_and_block_parity():
    """Lengths stay small; across the kinds every lane position sees every
    tail residue with an odd and with an even count of 64-B blocks."""
    pk = packed("main")
    assert 2 << 20 <= pk.total <= 8 << 20
    assert pk.lens.max() <= 3 * 1024
    full = (pk.n // 64) * 64
    L = pk.lens[:full].reshape(-1, 64)
    for lane in range(64):
        seen = {(int(x) >> 6 & 1, int(x) & 63) for x in L[:, lane]}
        assert {(p, r) for p in (0, 1) for r in lk.RESIDUES} <= seen, lane
    # one_long: k + 9 stages and 17 bytes more
    one_long = lk.BY_NAME["one_long_4@u"].lanes
    assert one_long[23][0] == 128 * 13 + 17
    # no_stage: 0 and 64..127 among the lengths
    tiny = [x for x, _ in lk.BY_NAME["no_stage@l"].lanes]
    assert max(tiny) < 128 and 0 in tiny and any(64 <= x for x in tiny)
    # staircase: lane l has l % 9 stages
    assert [x >> 7 for x, _ in lk.BY_NAME["staircase@u"].lanes] == [l % 9 for l in range(64)]


def test_layout_gaps_and_bounds():
    for name in list(lk.BATCHES) + [f"win{F}" for F in WINDOWS]:
        pk = packed(name)
        end = pk.pos + pk.lens
        assert pk.pos[0] >= lk.LEAD and np.all(pk.pos[1:] - end[:-1] >= 16), "a live gap before every chunk"
        assert int(end.max()) + lk.PAD <= pk.total
        assert np.all(pk.pos[1:] // 128 > (np.maximum(end[:-1], 1) - 1) // 128), "no two chunks share a line"
        for ab in ALIGNS:
            assert np.all(pk.offs(ab).astype(np.int64) + pk.skew(ab) == pk.pos)
        # the permutation keeps every group whole
        cpg = pk.cpg
        for first in range(0, pk.n, cpg):
            src = pk.perm[first:first + cpg].astype(np.int64) // cpg
            assert np.all(src == src[0]), "a permuted group is one built group"
        full = pk.n // cpg * cpg
        assert np.all(pk.perm[full:] >= full), "the short group stays last"
        if pk.n > cpg:
            assert not np.array_equal(pk.perm, np.arange(pk.n)), "lanes rotate"


def _position_kinds(pk, perm):
    """The kind of every 64-position group of a launch."""
    idx = np.arange(pk.n) if perm is None else perm.astype(np.int64)
    return [pk.kind_of(int(idx[first])) for first in range(0, pk.n, pk.cpg)]


def _check_claim(kd, g, kernel, identity, what):
    path = kd.expected_path(kernel)
    assert g["path"] == path, f"{what}: {kd.name} takes {g['path']}, claims {path}"
    assert g["live"] == len(kd.lanes), what
    if path in lk.STAGE_PATHS:
        want = set(kd.flags) | {"lined" if kd.lined else "unlined"}
        if path == "run2":
            want |= kd.balanced
        if path == "run_lines":
            want |= kd.lines
        if identity:
            want |= kd.first_flags
        assert want <= g["flags"], f"{what}: {kd.name} lacks {sorted(want - g['flags'])} (has {sorted(g['flags'])})"
    elif "ragged" in kd.flags:
        assert "ragged" in g["flags"], what


@pytest.mark.parametrize("kernel", DESC_KERNELS)
def test_every_kind_classifies_as_it_claims(kernel):
    """Under each kernel's conditions, both orders, both base alignments."""
    for name in lk.BATCHES:
        pk = packed(name)
        for ab in ALIGNS:
            for oname, perm in pk.orders():
                groups = lk.classify_desc(_addrs(pk, ab), pk.lens, perm, pk.n, kernel)
                kinds = _position_kinds(pk, perm)
                assert len(groups) == len(kinds)
                for kd, g in zip(kinds, groups):
                    _check_claim(kd, g, kernel, perm is None, f"{kernel}, {name}, {oname}, base {ab}")


def test_staircase_rlast_all_differ_and_one_off16_is_one_lane():
    pk = packed("ragged_63")
    g = lk.classify_desc(_addrs(pk, 128), pk.lens, None, pk.n, "md5_desc_xdma")[0]
    assert sorted(set(g["rlast"].tolist())) == list(range(8)), "rlast 0..7, the stage-less rows at smax - 1"
    assert g["mrow"] == 8 and g["standin"].tolist() == list(range(0, 64, 9))
    kd = lk.BY_NAME["one_off16@l"]
    assert [o % 16 for _, o in kd.lanes].count(4) == 1 and sum(o % 16 != 0 for _, o in kd.lanes) == 1


def test_kind_preserving_order_moves_mrow_and_rows():
    pk = packed("main")
    a = _addrs(pk, 128)
    g0 = lk.classify_desc(a, pk.lens, None, pk.n, "md5_desc_xdma")
    g1 = lk.classify_desc(a, pk.lens, pk.perm, pk.n, "md5_desc_xdma")
    by_kind0 = {kd.name: g for kd, g in zip(_position_kinds(pk, None), g0)}
    by_kind1 = {kd.name: g for kd, g in zip(_position_kinds(pk, pk.perm), g1)}
    moved = 0
    for name, g in by_kind0.items():
        h = by_kind1[name]
        assert g["path"] == h["path"] and sorted(g["nst"].tolist()) == sorted(h["nst"].tolist()), name
        if g["path"] == "run" and "uniform" not in g["flags"] and g["live"] == 64:
            moved += not np.array_equal(g["nst"], h["nst"])
    assert moved >= 20, "the rotation moves the odd lane of the non-uniform groups"
    assert by_kind0["one_none_4_lane0@u"]["mrow"] == 1 and by_kind1["one_none_4_lane0@u"]["mrow"] == 0


# ----------------------------------------------------------------- CPU: the coverage table
STAGE_FLAGS = ("uniform", "clamp", "standin_live", "standin_dead", "mrow_nz", "smax1", "smax_odd", "smax_even",
               "lined", "unlined")
RUN2_FLAGS = ("quads0", "quads1", "quads2", "fmin0", "lim3", "lim4", "lim7", "lim8", "lim9", "fmin_gt")
LINES_FLAGS = ("sh_all8", "sh0_among_shifted", "exact128k")
ONE_LENGTH = "one length per batch: every live row has smax stages, and lane 0 is live"


def coverage_cells(kernel):
    """{(path, flag): True, or why the kernel cannot reach the cell}."""
    k = lk.KERNELS[kernel]
    cells = {("lane_range", "any"): True, ("no_stage", "any"): True, ("no_stage", "ragged"): True}
    for path in lk.STAGE_PATHS:
        why = True
        if path == "run2" and k["nb"] == 1:
            why = "one LDS-DMA image per wave (NB = 1): run2 is BALANCED's"
        if path != "run2" and k["nb"] == 2:
            why = "two images per wave (NB = 2): every staged group takes run2"
        if path == "run_lines" and k["nb"] == 1 and not k["shift"]:
            why = "kShift is false: chunk-relative stages for unlined groups too"
        flags = STAGE_FLAGS + (RUN2_FLAGS if path == "run2" else LINES_FLAGS if path == "run_lines" else ())
        for f in flags:
            cells[(path, f)] = why
    if k["shift"]:
        cells[("run", "unlined")] = "LINES: an unlined group takes run_lines"
        cells[("run_lines", "lined")] = "run_lines runs only for groups with a staged row off the line"
    # rmin + 1 is the fewest stages of any row that has one (a stage-less row counts as smax), fmin
    # the fewest of any live lane: a live lane with stages bounds both, one without makes fmin 0
    if k["nb"] == 2:
        cells[("run2", "fmin_gt")] = ("fmin <= rmin + 1 always: both are minima over the lanes' stage counts, "
                                      "rmin's with 0 read as smax (dead lanes too), fmin's over the live lanes")
    if k["src"] == "fixed":
        for f in ("clamp", "standin_live", "mrow_nz"):
            cells[("run", f)] = ONE_LENGTH
    # FastWindows rows are F bytes, a whole chunk of at most F, or empty: every cell of `run` is in
    # reach (smax <= F / 128); its rows pair up, so a ragged last group still has an even live count
    return cells


# what test_fixed_chunks_source_* launch through FixedChunks: (n, length, stride, base skew)
FAR = 1 << 25                          # the first stride past xdma_group's 32-bit offsets
FIXED_SOURCE_CASES = [(3, 1000, FAR, 0)] + \
    [(65, L, FAR, skew) for L in (1000, 256, 128, 100) for skew in (0, 16)] + \
    [(n, L, L + 5, 3) for (L, _, _) in lk.fixed_cases()[::3] for n in lk.FIXED_COUNTS]


def launched_groups(kernel):
    """(kind name, group) for every group the GPU tests launch through `kernel`."""
    src = lk.KERNELS[kernel]["src"]
    out = []
    if src == "desc":
        for name in lk.BATCHES:
            pk = packed(name)
            for ab in ALIGNS:
                for _, perm in pk.orders():
                    groups = lk.classify_desc(_addrs(pk, ab), pk.lens, perm, pk.n, kernel)
                    out += [(kd.name, g) for kd, g in zip(_position_kinds(pk, perm), groups)]
    elif src == "windows":
        for F in WINDOWS:
            for name in WINDOW_BATCHES + (f"win{F}",):
                pk = packed(name)
                for ab in ALIGNS:
                    for _, perm in pk.orders():
                        ra, rl = _window_rows(pk, ab, F, perm)
                        groups = lk.classify_desc(ra, rl, None, ra.size, kernel)
                        idx = np.arange(pk.n) if perm is None else perm.astype(np.int64)
                        out += [(f"{pk.kind_of(int(idx[32 * i])).name} F={F}", g) for i, g in enumerate(groups)]
    else:
        for n, L, stride, skew in FIXED_SOURCE_CASES:
            a, rl = lk.fixed_chunks(BASE + skew, n, stride, L)
            out += [(f"{L} B at stride {stride} from base + {skew}", g)
                    for g in lk.classify_desc(a, rl, None, n, kernel)]
    return out


def coverage(kernel):
    hit = {}
    for name, g in launched_groups(kernel):
        if g["path"] in lk.STAGE_PATHS:
            flags = g["flags"] - {"ragged"}            # standin_dead says it
        else:
            flags = {"any"} | (g["flags"] & {"ragged"} if g["path"] == "no_stage" else set())
        for f in flags:
            hit.setdefault((g["path"], f), []).append(name)
    return hit


@pytest.mark.parametrize("kernel", list(lk.KERNELS))
def test_coverage_table_has_no_reachable_empty_cell(kernel):
    """Every (path, flag) cell the kernel can reach holds a launched kind; a
    cell marked unreachable holds none (or its reason is wrong)."""
    cells, hit = coverage_cells(kernel), coverage(kernel)
    lines = []
    for cell, why in sorted(cells.items()):
        kinds = sorted(set(hit.get(cell, [])))
        lines.append(f"{kernel:32s} {cell[0]:10s} {cell[1]:18s} "
                     + (f"{len(kinds)} kinds, e.g. {kinds[0]}" if kinds else f"-- {why}"))
        if why is True:
            assert kinds, f"{kernel}: no launched kind reaches {cell}"
        else:
            assert not kinds, f"{kernel}: {cell} is marked unreachable ({why}) but {kinds[:3]} reach it"
    print("\n".join(lines))
    stray = set(hit) - set(cells)
    assert not stray, f"paths or flags outside the table: {sorted(stray)}"


def test_window_rows_form_these_kinds():
    """The descriptor kinds seen as fastcrc window rows: a tail window starts
    at length - F, off the 16-B grid for most residues, so most groups take
    lane_range; groups of chunks no longer than F are whole rows beside empty
    ones (stand-in rows); lk.window_kinds(F) adds the aligned windows."""
    for F in WINDOWS:
        pk = packed("main")
        ra, rl = _window_rows(pk, 128, F, None)
        groups = lk.classify_desc(ra, rl, None, ra.size, "crc32_fast_xdma16")
        assert len(groups) == (2 * pk.n + 63) // 64
        by = {}
        for i, g in enumerate(groups):
            by.setdefault(pk.kind_of(32 * i).name, []).append(g)
        for name, gs in by.items():
            kd = lk.BY_NAME.get(name) or lk.RAGGED[name]
            lens = np.asarray([x for x, _ in kd.lanes])
            for half, g in enumerate(gs):
                part = lens[32 * half:32 * half + 32]
                starts = np.asarray([o for _, o in kd.lanes][32 * half:32 * half + 32])
                tails_off = ((part > F) & ((part - F) % 16 != 0)).any() or (starts % 16 != 0).any()
                if tails_off:
                    assert g["path"] == "lane_range", (name, F)
                elif part.max() < 128:
                    assert g["path"] == "no_stage", (name, F)
                else:
                    assert g["path"] == "run", (name, F)
                    if (part <= F).any():
                        assert "standin_live" in g["flags"], (name, F)    # the empty tail rows
        assert {g["path"] for g in by["uniform_3@l"]} == {"run"}
        assert all({"standin_live", "lined"} <= g["flags"] for g in by["uniform_3@l"])
        assert {g["path"] for g in by["quad_lim9_odd@u"]} == {"lane_range"}
        # the window kinds are what they claim, in both orders from both bases
        wk = packed(f"win{F}")
        for ab in ALIGNS:
            for oname, perm in wk.orders():
                ra, rl = _window_rows(wk, ab, F, perm)
                groups = lk.classify_desc(ra, rl, None, ra.size, "crc32_fast_xdma16")
                idx = np.arange(wk.n) if perm is None else perm.astype(np.int64)
                for i, g in enumerate(groups):
                    kd = wk.kind_of(int(idx[32 * i]))
                    assert g["path"] == kd.expected_path("crc32_fast_xdma16"), (kd.name, F, oname, ab)
                    want = kd.flags | (kd.first_flags if perm is None else set())
                    assert want <= g["flags"], (kd.name, F, oname, ab, sorted(g["flags"]))
                    if g["path"] == "run":
                        assert g["smax"] == F // 128 or kd.name == "win_all_short"


def test_balanced_quantities():
    """run2's lim, quads and the hand-over to the guarded stages, by kind."""
    pk = packed("main")
    groups = lk.classify_desc(_addrs(pk, 16), pk.lens, None, pk.n, "md5_desc_balanced")
    by = {kd.name: g for kd, g in zip(_position_kinds(pk, None), groups)}
    for lim in (3, 4, 7, 8, 9):
        for par in ("odd", "even"):
            g = by[f"quad_lim{lim}_{par}@u"]
            assert (g["lim"], g["rmin"], g["fmin"], g["quads"]) == (lim, lim, lim + 1, lim // 4)
            assert g["smax"] % 2 == (par == "odd") and g["smax"] > lim + 1
        assert by[f"uniform_{lim + 1}@l"]["lim"] == lim and by[f"uniform_{lim + 1}@l"]["smax"] == lim + 1
    g = by["quad_fmin0@l"]
    assert g["fmin"] == 0 and g["rmin"] == 9 and g["quads"] == 0, "fmin < rmin + 1: the quad loop is skipped"
    assert all(g["fmin"] <= g["rmin"] + 1 for g in groups if g["path"] == "run2")
    assert by["ragged_37"]["quads"] == 1 and by["ragged_37"]["lim"] == 5


# ----------------------------------------------------------------- CPU: the fixed-stride cases
def test_fixed_cases_reach_what_they_claim():
    cases = lk.fixed_cases()
    seen = {"nstage": set(), "odd": set(), "tail": set(), "lined": set(), "rows": set(), "parity_tail": set()}
    for L, stride, skew in cases:
        assert L <= stride and stride % 16 == 0 and skew % 16 == 0 and stride < (1 << 31) // 64, "xdma_group's launch"
        for n in lk.FIXED_COUNTS:
            for g in lk.classify_fixed(BASE + skew, n, L, stride):
                seen["nstage"].add(g["nstage"])
                seen["odd"].add(g["odd"])
                seen["tail"].add(g["tail"])
                seen["lined"].add((g["lined"], stride % 128 == 0, skew))
                seen["rows"].add(g["rows"])
                seen["parity_tail"].add((g["odd"], g["tail"]))
                assert g["max_off"] is None or g["max_off"] + 16 <= 0x7FFFFFFF
    assert seen["nstage"] == {0, 1, 2, 5} and seen["odd"] == {False, True}
    assert seen["tail"] == set(lk.RESIDUES)
    assert seen["parity_tail"] == {(p, r) for p in (False, True) for r in lk.RESIDUES}
    # on the line; stride off it; stride on it from a base 16 B off it (not lined)
    assert seen["lined"] == {(True, True, 0), (False, False, 0), (False, True, 16)}
    assert seen["rows"] == {1, 2, 63, 64}
    assert any(stride > L + 16 for L, stride, _ in cases), "live gap bytes"
    for n, L, stride, skew in FIXED_SOURCE_CASES:
        xdma = skew % 16 == 0 and stride % 16 == 0 and stride < (1 << 31) // 64
        assert not xdma, "these reach desc_xpose_group through FixedChunks"


EDGE_STRIDE, EDGE_N = (1 << 25) - 16, 65


def test_offset_edge_is_at_the_edge():
    groups = lk.classify_fixed(BASE, EDGE_N, EDGE_STRIDE, EDGE_STRIDE)
    assert [g["rows"] for g in groups] == [64, 1]
    assert EDGE_STRIDE < (1 << 31) // 64 and EDGE_STRIDE % 16 == 0, "the launchers admit it"
    top = groups[0]["max_off"]
    assert (1 << 31) - (1 << 12) <= top and top + 16 <= 0x7FFFFFFF < (1 << 31)
    assert all(top >> b & 1 for b in range(26, 31)), "bits 26..30 set"
    assert FAR >= (1 << 31) // 64 > FAR - 16, "and the next stride on the 16-B grid does not"


# ----------------------------------------------------------------- CPU: the references
def _blk_crc(b, F):
    if F == 0 or len(b) <= F:
        return zlib.crc32(b)
    return zlib.crc32(b[:F]) ^ zlib.crc32(b[-F:])


def _host(pk, seed=SEED):
    buf = gen.xorshift_array(pk.total, seed=seed)
    raw = [buf[int(p):int(p) + int(L)].tobytes() for p, L in zip(pk.pos, pk.lens)]
    return buf, raw


def _md5s(raw):
    return np.frombuffer(b"".join(hashlib.md5(b).digest() for b in raw), np.uint8).reshape(-1, 16)


@pytest.mark.parametrize("name", ["main", "win1024", "win1000"])
def test_references_agree(name):
    """hashlib and zlib over the packed buffer equal the oracle on it."""
    pk = packed(name)
    buf, raw = _host(pk)
    pos = pk.pos.astype(np.uint64)
    assert np.array_equal(_md5s(raw), gen.oracle_digests(buf, pos, pk.lens.astype(np.uint32)))
    for F in (0,) + WINDOWS:
        want = np.asarray([_blk_crc(b, F) for b in raw], dtype=np.uint32)
        assert np.array_equal(want, gen.oracle_crc32_batch(buf, pos, pk.lens.astype(np.uint32), F)), F
    big = [b for b in raw if len(b) >= 16]
    assert len(set(big)) == len(big), "no two chunks alike"


# ----------------------------------------------------------------- GPU
def _canary(n, width, cuda):
    import torch
    return torch.full((n + 1, width), 0xAA, dtype=torch.uint8, device=cuda)


def _records(out, n, what):
    import torch
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert a.shape[0] == n + 1
    assert (a[n] == 0xAA).all(), f"{what}: wrote past record n - 1"
    return a[:n]


def _same(got, want, what, namer=None):
    """Bit-exact; on a mismatch the message names the first wrong record."""
    got = np.ascontiguousarray(got).view(np.uint8).reshape(len(want), -1)
    want = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        untouched = int((got[bad] == 0xAA).all(axis=1).sum())
        where = namer(int(bad[0])) if namer else f"first wrong lane {int(bad[0]) % 64} (record {int(bad[0])})"
        pytest.fail(f"{what}: {bad.size} of {len(want)} records differ ({untouched} still 0xAA); {where}")


class DevPack:
    """A packed batch on the host and the device; references computed once."""

    def __init__(self, pk, cuda):
        import torch
        self.pk, self.cuda = pk, cuda
        self.buf, self.raw = _host(pk)
        self.md5 = _md5s(self.raw)
        self.crc = {0: np.asarray([zlib.crc32(b) for b in self.raw], dtype="<u4")}
        self.md5.setflags(write=False)
        self.d_buf = torch.from_numpy(self.buf).to(cuda)
        assert self.d_buf.data_ptr() % 128 == 0
        self.d_lens = torch.from_numpy(pk.lens.astype(np.int32)).to(cuda)
        self.d_offs = {ab: torch.from_numpy(pk.offs(ab).astype(np.int64)).to(cuda) for ab in ALIGNS}
        self.d_perm = torch.from_numpy(pk.perm.astype(np.int32)).to(cuda)
        self.inv = np.argsort(pk.perm)

    def base(self, ab):
        return self.d_buf[self.pk.skew(ab):]

    def fast(self, F):
        if F not in self.crc:
            self.crc[F] = np.asarray([_blk_crc(b, F) for b in self.raw], dtype="<u4")
        return self.crc[F]

    def launches(self):
        """(base alignment, order name, order tensor, namer of a wrong record)"""
        for ab in ALIGNS:
            for oname, perm in self.pk.orders():
                def namer(c, perm=perm):
                    p = c if perm is None else int(self.inv[c])
                    return (f"kind {self.pk.kind_of(c).name}, first wrong lane {p % 64} "
                            f"(chunk {c}, group {p // 64} of the launch)")
                yield ab, oname, (None if perm is None else self.d_perm), namer


@pytest.fixture(scope="module")
def packs(cuda):
    return {name: DevPack(packed(name), cuda) for name in lk.BATCHES}


@pytest.mark.gpu
@pytest.mark.parametrize("variant", list(MD5_VARIANT))
def test_md5_desc_kinds(packs, cuda, variant):
    """md5_desc_xdma / _lines / _hybrid / _balanced_t on every kind.  No chunk
    reaches 256 KiB, so HYBRID takes its one-image path for every group (the
    long path stays with test_hybrid_long_group_edges)."""
    for name, dp in packs.items():
        for ab, oname, od, namer in dp.launches():
            what = f"{MD5_VARIANT[variant]} ({name}), order {oname}, base alignment {ab}"
            out = _canary(dp.pk.n, 16, cuda)
            m.digest_desc(dp.base(ab), dp.d_offs[ab], dp.d_lens, od, out=out, variant=variant)
            _same(_records(out, dp.pk.n, what), dp.md5, what, namer)


@pytest.mark.gpu
def test_crc32_desc_kinds(packs, cuda):
    """crc32_desc_xdma16 (fastcrc = 0)."""
    for name, dp in packs.items():
        for ab, oname, od, namer in dp.launches():
            what = f"crc32_desc_xdma16 ({name}), order {oname}, base alignment {ab}"
            out = _canary(dp.pk.n, 4, cuda)
            m.crc32_desc(dp.base(ab), dp.d_offs[ab], dp.d_lens, od, fastcrc=0, out=out, variant="xdma16")
            _same(_records(out, dp.pk.n, what), dp.crc[0], what, namer)


@pytest.mark.gpu
def test_md5crc32_desc_kinds(packs, cuda):
    """md5crc32_desc_xdma16<false>: both digests from one read; bytes 20..31 zero."""
    for name, dp in packs.items():
        for ab, oname, od, namer in dp.launches():
            what = f"md5crc32_desc_xdma16 ({name}), order {oname}, base alignment {ab}"
            out = _canary(dp.pk.n, 32, cuda)
            m.md5crc32_desc(dp.base(ab), dp.d_offs[ab], dp.d_lens, od, out=out)
            r = _records(out, dp.pk.n, what)
            _same(r[:, :16], dp.md5, what + ", md5", namer)
            _same(r[:, 16:20], dp.crc[0], what + ", crc", namer)
            assert not r[:, 20:].any(), what


@pytest.mark.gpu
@pytest.mark.parametrize("F", WINDOWS)
def test_crc32_fast_window_kinds(packs, cuda, F):
    """crc32_fast_xdma16: the descriptor kinds as window rows, and the window
    kinds.  The kernel takes no order; the permuted launch permutes the
    descriptor arrays, so the same chunks meet in the same groups on other
    lanes."""
    import torch
    for name, dp in [(b, packs[b]) for b in WINDOW_BATCHES] + [(f"win{F}", DevPack(packed(f"win{F}"), cuda))]:
        pk, want = dp.pk, dp.fast(F)
        for ab in ALIGNS:
            for oname, perm in pk.orders():
                idx = np.arange(pk.n) if perm is None else perm.astype(np.int64)
                t = torch.from_numpy(idx).to(cuda)
                what = f"crc32_fast_xdma16 F={F} ({name}), order {oname}, base alignment {ab}"

                def namer(p, idx=idx, pk=pk):
                    return (f"kind {pk.kind_of(int(idx[p])).name}, first wrong lane {2 * (p % 32)} and the next "
                            f"(chunk {int(idx[p])}, window group {p // 32} of the launch)")
                out = _canary(pk.n, 4, cuda)
                m.crc32_desc(dp.base(ab), dp.d_offs[ab][t].contiguous(), dp.d_lens[t].contiguous(), None,
                             fastcrc=F, out=out, variant="xdma16")
                _same(_records(out, pk.n, what), want[idx], what, namer)


# ---- the fixed-stride loader
FIXED_KERNELS = ("md5_fixed_xdma1nt", "crc32_fixed_xdma16", "md5crc32_fixed_xdma16")


@pytest.fixture(scope="module")
def blob(cuda):
    import torch
    nmax = max(lk.FIXED_COUNTS)
    top = max(stride for _, stride, _ in lk.fixed_cases())
    host = gen.xorshift_array(16 + nmax * top + lk.PAD, seed=SEED + 1)
    dev = torch.from_numpy(host).to(cuda)
    assert dev.data_ptr() % 128 == 0
    return host, dev


def _fixed_want(host, n, L, stride, skew):
    raw = [host[skew + i * stride:skew + i * stride + L].tobytes() for i in range(n)]
    return _md5s(raw), np.asarray([zlib.crc32(b) for b in raw], dtype="<u4")


def _launch_fixed(kernel, dev, n, L, stride, want, what, cuda):
    md5, crc = want[0][:n], want[1][:n]
    if kernel.startswith("md5_fixed") or kernel == "md5_fixed_direct":
        out = _canary(n, 16, cuda)
        m.digest_fixed(dev, n, L, stride, out=out, variant="direct2" if kernel == "md5_fixed_direct" else "xdma1nt")
        _same(_records(out, n, what), md5, what)
    elif kernel.startswith("crc32_fixed"):
        out = _canary(n, 4, cuda)
        m.crc32_fixed(dev, n, L, stride, fastcrc=0, out=out, variant="xdma16")
        _same(_records(out, n, what), crc, what)
    else:
        out = _canary(n, 32, cuda)
        m.md5crc32_fixed(dev, n, L, stride, out=out)
        r = _records(out, n, what)
        _same(r[:, :16], md5, what + ", md5")
        _same(r[:, 16:20], crc, what + ", crc")
        assert not r[:, 20:].any(), what


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", FIXED_KERNELS)
def test_fixed_stride_kinds(blob, cuda, kernel):
    """xdma_group in its three kernels: 0, 1, 2 and 5 stages, the odd block,
    every tail, strides on and off the line, a base 16 B off it, ragged last
    waves of 1, 63, 1 (of 65) and 2 (of 130) rows."""
    host, dev = blob
    for L, stride, skew in lk.fixed_cases():
        want = _fixed_want(host, max(lk.FIXED_COUNTS), L, stride, skew)
        for n in lk.FIXED_COUNTS:
            what = f"{kernel}: kind {L} B at stride {stride} from base + {skew}, {n} chunks in chunk order"
            _launch_fixed(kernel, dev[skew:], n, L, stride, want, what, cuda)


@pytest.mark.gpu
def test_fixed_chunks_source_off_the_grid(blob, cuda):
    """md5crc32_fixed from a base 3 B off the grid with stride length + 5:
    md5crc32_desc_xdma16<true>, the FixedChunks source (every wave lane-direct)."""
    host, dev = blob
    for n, L, stride, skew in FIXED_SOURCE_CASES:
        if skew != 3:
            continue
        want = _fixed_want(host, n, L, stride, skew)
        what = f"md5crc32_desc_xdma16<implicit>: kind {L} B at stride {stride} from base + {skew}, {n} chunks"
        _launch_fixed("md5crc32", dev[skew:], n, L, stride, want, what, cuda)


def _rows(dev, n, L, stride):
    """Chunks i * stride .. + L of a device buffer, as one host array [n, L]."""
    import torch
    idx = (torch.arange(n, device=dev.device) * stride)[:, None] + torch.arange(L, device=dev.device)[None, :]
    return dev[idx].cpu().numpy()


@pytest.mark.gpu
def test_fixed_far_side_of_the_offset_limit(cuda):
    """Stride 2^25, the first past xdma_group's 32-bit group offsets: the three
    fixed entries fall back (md5_fixed_direct, crc32_desc<true>, and the
    loader through FixedChunks) and give the oracle's digests."""
    import torch
    n, L, stride = 3, 1000, FAR
    dev = torch.empty((n - 1) * stride + 1008, dtype=torch.uint8, device=cuda)
    m.fill_synthetic(dev, seed=0xFA5)
    rows = _rows(dev, n, L, stride)
    flat = np.ascontiguousarray(rows).reshape(-1)
    offs, lens = np.arange(n, dtype=np.uint64) * L, np.full(n, L, dtype=np.uint32)
    want = (gen.oracle_digests(flat, offs, lens), gen.oracle_crc32_batch(flat, offs, lens).astype("<u4"))
    assert np.array_equal(want[0], _md5s([r.tobytes() for r in rows]))
    assert want[1].tolist() == [zlib.crc32(r.tobytes()) for r in rows]
    for kernel in FIXED_KERNELS:
        _launch_fixed(kernel, dev, n, L, stride, want, f"{kernel}'s fallback at stride 2^25", cuda)
    del dev
    torch.cuda.empty_cache()


@pytest.mark.gpu
def test_fixed_offset_edge(cuda):
    """xdma_group's 32-bit buffer offsets just below 2^31: 65 chunks of
    2^25 - 16 bytes back to back, so the full group's last loads carry offsets
    with bits 26..30 set (an out-of-range buffer load would return zeros, not
    fault).  All 65 digests equal md5_fixed_direct's (64-bit addresses); six
    rows are copied back and checked against hashlib and zlib.  The same
    buffer then serves full groups of the FixedChunks source at stride 2^25."""
    import torch
    n, stride = EDGE_N, EDGE_STRIDE
    L = stride
    dev = torch.empty(n * stride, dtype=torch.uint8, device=cuda)
    assert dev.data_ptr() % 128 == 0
    m.fill_synthetic(dev, seed=0xED6E)
    try:
        ref = _canary(n, 16, cuda)
        m.digest_fixed(dev, n, L, stride, out=ref, variant="direct2")
        ref = _records(ref, n, "direct2").copy()
        probe = (0, 1, 31, 62, 63, 64)
        crc = {}
        for i in probe:
            b = dev[i * stride:i * stride + L].cpu().numpy().tobytes()
            assert hashlib.md5(b).digest() == bytes(ref[i]), f"md5_fixed_direct, row {i}"
            crc[i] = zlib.crc32(b)
        out = _canary(n, 16, cuda)
        m.digest_fixed(dev, n, L, stride, out=out, variant="xdma1nt")
        _same(_records(out, n, "xdma1nt"), ref, "md5_fixed_xdma1nt at the 32-bit offset edge")
        out = _canary(n, 4, cuda)
        m.crc32_fixed(dev, n, L, stride, fastcrc=0, out=out, variant="xdma16")
        got = _records(out, n, "crc").view("<u4").reshape(-1)
        for i in probe:
            assert int(got[i]) == crc[i], f"crc32_fixed_xdma16 at the 32-bit offset edge: first wrong lane {i % 64} (row {i})"
        out = _canary(n, 32, cuda)
        m.md5crc32_fixed(dev, n, L, stride, out=out)
        r = _records(out, n, "dual")
        _same(r[:, :16], ref, "md5crc32_fixed_xdma16 at the 32-bit offset edge, md5")
        assert np.array_equal(r[:, 16:20].copy().view("<u4").reshape(-1), got), "the two CRC kernels agree on all 65 rows"
        for i in probe:
            assert int(r[i, 16:20].copy().view("<u4")[0]) == crc[i], f"md5crc32_fixed_xdma16 crc, row {i}"
        assert not r[:, 20:].any()
        # full groups through FixedChunks (stride 2^25: uniform, lined and not, one and two stages, none)
        for k, L2, stride2, skew in FIXED_SOURCE_CASES:
            if stride2 != FAR or k != 65:
                continue
            base = dev[skew:]
            rows = _rows(base, k, L2, stride2)
            raw = [x.tobytes() for x in rows]
            want = (_md5s(raw), np.asarray([zlib.crc32(b) for b in raw], dtype="<u4"))
            _launch_fixed("md5crc32", base, k, L2, stride2, want,
                          f"md5crc32_desc_xdma16<implicit>: kind {L2} B at stride 2^25 from base + {skew}", cuda)
    finally:
        del dev
        torch.cuda.empty_cache()
