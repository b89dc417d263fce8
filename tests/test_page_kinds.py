"""The paged kernels' group kinds, off-grid tails and window groups
(sproxy_amd/csrc/md5_pages.hip), from the kernels' own branch structure.

pages_group decides per page index, wave-uniformly, whether the 64 lanes'
pages are read lane by lane, skipped, or loaded as an LDS-DMA image (lined or
not, rows clamped, rows standing in for lanes without a stage), carries each
lane's state across page indexes of different kinds, and finishes a lane from
its last page wherever that lies; md5_update_ctx_pages rebuilds in[] from the
last or the previous page; crc32_pages_fast pipelines a 64-row group or
leaves it to its lanes.  tests/page_kinds.py builds groups that reach each of
those on purpose and restates the conditions in numpy.

CPU tests (-m "not gpu"): every kind classifies as it claims under both
arrangements; the union of what is launched fills every cell of two tables
({page kind} x {flags}, {last-page alignment} x {odd block} x {tail class});
state is carried across named sequences of page kinds; the context and window
cases are present; no two pages overlap and every address the model says is
read lies in the page's own slot.

GPU tests: all of it bit-exact against hashlib.md5, zlib.crc32 and the
reference MD5Update (test_ctx.HostRef, and md5.c:169-215 restated here for
all 64 bytes of in[]), naming kind, lane and length of the first wrong
record."""
import hashlib
import zlib

import numpy as np
import pytest

import page_kinds as pk
import trips

BASE = 0x7F0000000000                 # a line-aligned stand-in for the pool's address
SEED = 0x9A6E5
WINDOWS = (64, 128, 132, 1000)
ARRANGEMENTS = ("identity", "kind-preserving")
FAST_PIPE = (16, 32)                  # crc32_pages_fast's frame: waves per CU, chunks per group (trips.py)

_lay = {}


def layout(key):
    """Layouts built once: a page size (pk.BATCHES) or "win<F>"."""
    if key not in _lay:
        if isinstance(key, str):
            F = int(key[3:])
            _lay[key] = pk.Layout(pk.window_kinds(pk.WINDOW_P[F], F), cpg=32)
        else:
            _lay[key] = pk.Layout(pk.BATCHES[key])
    return _lay[key]


def digest_launches(P):
    """(arrangement, batch, order): the digest kernels take the second
    arrangement through d_order."""
    lay = layout(P)
    return (("identity", lay.batch(), None), ("kind-preserving", lay.batch(), lay.perm))


def built_launches(key):
    """Contexts and windows have no order: the batch is built in that order."""
    lay = layout(key)
    return (("identity", lay.batch(False)), ("kind-preserving", lay.batch(True)))


def page_groups(P):
    """(arrangement, kind, classify_pages' group) of every digest group launched at P."""
    out = []
    for name, b, order in digest_launches(P):
        idx = np.arange(b.n) if order is None else order
        for f, lens, pa, live in b.groups(BASE, order):
            out.append((name, b.kind_of(int(idx[f]))[0], pk.classify_pages(lens, pa, P, live)))
    return out


def all_page_groups():
    return [x for P in pk.BATCHES for x in page_groups(P)]


# ----------------------------------------------------------------- CPU: the kinds are what they claim
def test_kind_names_are_unique_and_the_eleven_are_there():
    names = [k.name for ks in pk.BATCHES.values() for k in ks]
    assert len(set(names)) == len(names)
    # every named kind is launched: taking one out fails here, and in the tests below that name it
    assert {P: [k.name for k in ks] for P, ks in pk.BATCHES.items()} == {
        256: ["two_full_lined", "aligned_off_line_mixed", "staircase", "page1_no_stage", "staircase_lane41_off4",
              "last_page_off", "last_page_off_mixed", "every_page_off", "empty_64", "one_six_pages_lane41",
              "two_full_off_line", "off_line_then_lane9_off4", "off_line_one_long_lane63", "ctx_prev_last_combos",
              "ragged_37"],
        128: ["one_stage_pages", "one_stage_pages_off_line", "one_stage_pages_half_off"],
        512: ["clamp_in_page", "clamp_in_page_off_line"],
        384: ["p384_last_off", "p384_ragged_37"],
        16384: ["p16k_one_page_off"]}
    for P, ks in pk.BATCHES.items():
        assert max(pk.pages_of(L, P) for k in ks for L, _ in k.lanes) <= (7 if P == 256 else 4), P
    assert len(pk.BATCHES[16384]) == 1


@pytest.mark.parametrize("P", list(pk.BATCHES))
def test_every_kind_classifies_as_it_claims(P):
    for arr, kd, g in page_groups(P):
        what = f"{kd.name} at P = {P}, {arr}"
        assert g["live"] == len(kd.lanes), what
        if kd.seq is not None:
            assert pk.page_seq(g)[:len(kd.seq)] == kd.seq and (kd.seq or g["pmax"] == 0), (what, pk.page_seq(g))
        present = {(pg["kind"], f) for pg in g["pages"] for f in pg["flags"]}
        want = kd.has | (kd.first_has if arr == "identity" else set())
        assert want <= present, f"{what}: lacks {sorted(want - present)} (has {sorted(present)})"


def test_lengths_cycle_extras_one_step_further_in_every_group():
    ks = pk.BATCHES[256]
    stair = [k for k in ks if k.name in ("staircase", "staircase_lane41_off4", "every_page_off")]
    firsts = [kd.lanes[0][0] % 128 for kd in stair]
    assert len(set(firsts)) == len(firsts), "lane 0's extra differs from kind to kind"
    for kd in stair:
        assert {L % 128 for L, _ in kd.lanes} == set(pk.EXTRAS), kd.name
    for kd in ks:
        assert all(0 <= s < 128 for _, sk in kd.lanes for s in sk), "skews stay under 128"


# ----------------------------------------------------------------- CPU: the two tables
def table1_cells():
    cells = [(k, f) for k in ("lined", "unlined") for f in ("clamp", "standin_own", "standin_ended", "mrow_nz", "plain")]
    cells += [("lined", "standin_dead"), ("lined", "smax1")]
    cells += [("lane", s) for s in pk.LANE_SUBS] + [("lane", "all_three"), ("skip", "any")]
    return cells


def table2_cells():
    cells = [(a, o, t) for a in ("a16", "a4", "odd") for o in (False, True) for t in ("r0", "lt56", "ge56")]
    cells += [(a, lp) for a in ("a16", "a4", "odd") for lp in ("under64", "full", "between")]
    return cells + ["empty"]


def coverage(groups):
    """{cell: kinds that reach it} over (arrangement, kind, group) triples."""
    hit = {}
    for _, kd, g in groups:
        for pg in g["pages"]:
            flags = set(pg["flags"])
            if pg["kind"] == "skip":
                flags = {"any"}
            if pg["kind"] == "lane" and flags >= set(pk.LANE_SUBS):
                flags.add("all_three")
            for f in flags:
                hit.setdefault((pg["kind"], f), set()).add(kd.name)
        for c in g["chunks"]:
            if c["empty"]:
                hit.setdefault("empty", set()).add(kd.name)
            else:
                hit.setdefault((c["align"], c["odd_block"], c["tail"]), set()).add(kd.name)
                hit.setdefault((c["align"], c["lastpage"]), set()).add(kd.name)
    return hit


def empty_cells(groups):
    hit = coverage(groups)
    return [c for c in table1_cells() + table2_cells() if not hit.get(c)]


def test_no_cell_of_the_two_tables_is_empty():
    groups = all_page_groups()
    hit = coverage(groups)
    for c in table1_cells() + table2_cells():
        print(f"{str(c):40s} {len(hit.get(c, ()))} kinds, e.g. {sorted(hit.get(c, ['--']))[0]}")
    assert not empty_cells(groups)


def test_the_tables_need_the_kinds_that_fill_them():
    """A cell empties when the kinds built for it are taken out: the tables
    are filled by construction, not by chance."""
    groups = all_page_groups()

    def without(*names):
        assert set(names) <= {x[1].name for x in groups}
        return empty_cells([x for x in groups if x[1].name not in names])
    assert ("unlined", "plain") in without("two_full_off_line", "off_line_then_lane9_off4")
    assert ("lined", "standin_dead") in without("ragged_37", "p384_ragged_37")
    assert ("lined", "smax1") in without("one_stage_pages", "one_six_pages_lane41")
    assert ("lane", "all_three") in without("last_page_off_mixed", "ctx_prev_last_combos", "one_stage_pages_half_off")
    left = without("last_page_off", "last_page_off_mixed", "every_page_off", "ctx_prev_last_combos", "p384_last_off",
                   "p16k_one_page_off", "one_stage_pages_half_off")
    assert {c for c in table2_cells() if c[0] in ("a4", "odd")} <= set(left) and ("lane", "alignbit") in left
    # the eleven kinds and what extends them at P = 256 fill all of it but smax1, which takes P = 128
    assert empty_cells([x for x in groups if x[1].P == 256 and x[1].name != "one_six_pages_lane41"]) == [("lined", "smax1")]


def test_state_is_carried_across_sequences_of_page_kinds():
    def contains(seq, sub):
        return any(seq[i:i + len(sub)] == sub for i in range(len(seq) - len(sub) + 1))
    seqs = {(kd.name, arr): pk.page_seq(g) for arr, kd, g in page_groups(256)}
    for arr in ARRANGEMENTS:
        assert contains(seqs["staircase_lane41_off4", arr], ("lined", "lane", "lined"))
        assert contains(seqs["off_line_then_lane9_off4", arr], ("unlined", "lane"))
        assert contains(seqs["page1_no_stage", arr], ("lined", "skip"))
        assert seqs["last_page_off_mixed", arr][0] == "lane" and seqs["every_page_off", arr][0] == "lane"
        assert seqs["last_page_off", arr] == ("lined", "lined", "lane"), "two staged pages, then the off-grid one"
    # in those groups a lane with blocks on both sides of the change of kind exists
    for arr, kd, g in page_groups(256):
        if kd.name == "staircase_lane41_off4" and arr == "identity":
            L = kd.lanes[41][0]
            assert L > 2 * 256 and kd.lanes[41][1][1] == 4, "lane 41: a staged page, its page 4 bytes off, and more"
            assert sum(1 for L, _ in kd.lanes if L >= 3 * 256 - 128) > 8, "lanes staged on both sides of page 1"


# ----------------------------------------------------------------- CPU: contexts
def ctx_groups(P):
    """(arrangement, round, kind, classify_ctx's group): round 1 from MD5Init,
    round 2 the same batch over what round 1 left pending."""
    out = []
    for arr, b in built_launches(P):
        for rnd in (1, 2):
            pend = np.zeros(b.n, np.int64) if rnd == 1 else b.lens % 64
            for f, lens, pa, live in b.groups(BASE):
                t = np.zeros(64, np.int64)
                t[:live] = pend[f:f + live]
                out.append((arr, rnd, b.kind_of(f)[0], pk.classify_ctx(lens, pa, P, live, t)))
    return out


def test_context_cases_are_present():
    groups = [x for P in pk.BATCHES for x in ctx_groups(P)]
    assert all(g["route"] == "loader" for _, rnd, _, g in groups if rnd == 1), "round 1: the loader route everywhere"
    prev, last, srcs = set(), set(), set()
    for _, rnd, kd, g in groups:
        for l, c in g["lanes"].items():
            srcs.add(c["src"])
            if c["src"] == "prev":
                prev.add((c["blk_align"] != "a16", c["tail_align"] != "a16"))
                if kd.name == "ctx_prev_last_combos":
                    assert 1 <= kd.lanes[0][0] % kd.P <= 63
            if c["src"] == "last":
                last.add(c["tail_align"])
                assert c["blk_align"] == c["tail_align"]
    assert srcs == {"in", "last", "prev"}
    assert prev == {(a, b) for a in (False, True) for b in (False, True)}, "previous page x last page, on and off the grid"
    assert last == {"a16", "a4", "odd"}
    combos = [g for _, rnd, kd, g in groups if kd.name == "ctx_prev_last_combos" and rnd == 1]
    assert all(c["src"] == "prev" for g in combos for c in g["lanes"].values()) and len(combos[0]["lanes"]) == 64
    assert {(c["blk_align"] != "a16", c["tail_align"] != "a16") for c in combos[0]["lanes"].values()} == prev
    # round 2: the lane route over pages off the grid, and a group that stays on the loader
    lane_off = {kd.name for _, rnd, kd, g in groups if rnd == 2 and g["route"] == "lane" and g["off_grid"]}
    assert {"last_page_off", "last_page_off_mixed", "every_page_off", "ctx_prev_last_combos", "p384_last_off",
            "p16k_one_page_off"} <= lane_off
    assert any(g["route"] == "loader" for _, rnd, kd, g in groups if rnd == 2 and kd.name == "two_full_lined")


# ----------------------------------------------------------------- CPU: windows
def window_groups(F):
    out = []
    for arr, b in built_launches(f"win{F}"):
        for f, lens, pa, live in b.groups(BASE, cpg=32):
            out.append((arr, b.kind_of(f)[0], pk.classify_windows(lens, pa, b.P, F, 2 * live)))
    return out


@pytest.mark.parametrize("F", WINDOWS)
def test_window_cases_are_present(F):
    groups = window_groups(F)
    by = {(kd.name, arr): g for arr, kd, g in groups}
    for arr in ARRANGEMENTS:
        if F in (64, 128):
            for name in ("win_pipe_full", "win_pipe_off_line", "win_pipe_ragged_19"):
                assert by[name, arr]["pipe"], name
            assert by["win_pipe_full", arr]["live"] == 64 and by["win_pipe_ragged_19", arr]["live"] == 38
            for name, why in (("win_one_short", "short"), ("win_one_exactly_F", "short"), ("win_one_empty", "short"),
                              ("win_one_tail_straddles", "room"), ("win_one_length_off", "len_off"),
                              ("win_one_page_off4", "page_off"), ("win_one_page_off1", "page_off")):
                g = by[name, arr]
                assert not g["pipe"] and g["reasons"] == {why}, (name, F, g["reasons"])
        else:
            assert pk.WINDOW_P[F] == 128
            for (name, a), g in by.items():
                assert not g["pipe"] and "F" in g["reasons"], name
            assert by["win_span_long", arr]["spans"] >= -(-F // 128), "windows over several pages"
            assert by["win_span_long_off", arr]["spans"] >= -(-F // 128) and "page_off" in by["win_span_long_off", arr]["reasons"]
    lay = layout(f"win{F}")
    assert len(lay.kinds[-1].lanes) == 19, "the ragged kind is the launch's last group"
    if F in (64, 128):
        assert {r for _, _, g in groups for r in g["reasons"]} == set(pk.WINDOW_REASONS) - {"F"}


# ----------------------------------------------------------------- CPU: the layout
def test_no_two_pages_overlap_and_every_read_is_in_its_slot():
    for key in list(pk.BATCHES) + [f"win{F}" for F in WINDOWS]:
        lay = layout(key)
        slots = [s for c in lay.slots for s in c]
        assert len(set(slots)) == len(slots) and max(slots, default=0) < lay.nslots, "a slot per table entry"
        for b in (lay.batch(False), lay.batch(True)):
            assert np.array_equal(np.sort(b.slot), np.sort(slots)) and ((0 <= b.skew) & (b.skew < 128)).all()
            assert (b.at() + b.P <= lay.pool_bytes - pk.PAD).all()
    reads = []
    for P in pk.BATCHES:
        lay = layout(P)
        got = [r for _, _, g in page_groups(P) for r in g["reads"]] + [r for *_, g in ctx_groups(P) for r in g["reads"]]
        assert got and pk.in_own_slots(got, BASE, P, lay.pool_bytes) is None, (P, pk.in_own_slots(got, BASE, P, lay.pool_bytes))
        reads.append(len(got))
    for F in WINDOWS:
        lay = layout(f"win{F}")
        got = [r for _, _, g in window_groups(F) for r in g["reads"]]
        assert got and pk.in_own_slots(got, BASE, lay.P, lay.pool_bytes) is None, F
    # the model does reach a slot's last bytes: the 17th dword of a full page's last block, 127 bytes in
    assert pk.in_own_slots(pk._block_reads(BASE + 127 + 256 - 64, 1), BASE, 256, 384 + 128) is None
    assert pk.in_own_slots(pk._block_reads(BASE + 128 + 3 + 256 - 64, 1), BASE, 256, 384 + 128) is not None


def _signature(g):
    """A group's classification without what the lane order decides."""
    pages = [(pg["kind"], tuple(sorted(pg["flags"] - {"mrow_nz", "plain"}))) for pg in g["pages"]]
    chunks = sorted(tuple(sorted(c.items())) for c in g["chunks"])
    return pages, chunks


def test_kind_preserving_arrangement_moves_mrow_and_keeps_the_kinds():
    moved = 0
    for P in pk.BATCHES:
        by = {}
        for arr, kd, g in page_groups(P):
            by.setdefault(kd.name, {})[arr] = g
        for name, two in by.items():
            a, b = two["identity"], two["kind-preserving"]
            assert _signature(a) == _signature(b), name
            moved += any(x.get("mrow") != y.get("mrow") for x, y in zip(a["pages"], b["pages"]))
        lay = layout(P)
        for f in range(0, lay.n, 64):
            src = {lay.where[c][0] for c in lay.perm[f:f + 64]}
            assert len(src) == 1, "a permuted group is one built group"
        assert not np.array_equal(lay.perm, np.arange(lay.n)) or lay.n == 64
    assert moved >= 5, "mrow moves in the groups whose longest lane is not everywhere"


# ----------------------------------------------------------------- GPU
def _paged(b, cuda, seed=SEED):
    """test_pages.Paged over a batch: the same slots and skews, so the two
    arrangements of a layout share their pool bytes."""
    from test_pages import Paged
    p = Paged(b.lens.tolist(), b.P, seed, cuda, slot=b.slot, skew=b.skew)
    assert p.pool.data_ptr() % 128 == 0 and p.pool.numel() == b.lay.pool_bytes
    assert np.array_equal(p.first.astype(np.int64), b.first) and np.array_equal(p.at, b.at())
    return p


def _namer(b):
    def name(i):
        kd, lane = b.kind_of(i)
        return f"kind {kd.name}, lane {lane} of it, {int(b.lens[i])} bytes (chunk {i} of the batch, P = {b.P})"
    return name


def _same(got, want, what, namer):
    got = np.ascontiguousarray(got).view(np.uint8).reshape(len(want), -1)
    want = np.ascontiguousarray(want).view(np.uint8).reshape(len(want), -1)
    assert got.shape == want.shape, what
    bad = np.flatnonzero((got != want).any(axis=1))
    if bad.size:
        kinds = sorted({namer(int(i)).split(",")[0] for i in bad})
        pytest.fail(f"{what}: {bad.size} of {len(want)} records differ, in {kinds}; first: {namer(int(bad[0]))}")


_paged_cache = {}


def paged_of(key, permuted, cuda):
    """The device batches, built once and left unchanged."""
    k = (key, permuted)
    if k not in _paged_cache:
        b = layout(key).batch(permuted)
        p = _paged(b, cuda)
        md5 = np.array([np.frombuffer(hashlib.md5(c).digest(), np.uint8) for c in p.chunks]).reshape(b.n, 16)
        crc = np.array([zlib.crc32(c) for c in p.chunks], dtype="<u4")
        md5.setflags(write=False)
        crc.setflags(write=False)
        _paged_cache[k] = (b, p, md5, crc)
    return _paged_cache[k]


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
@pytest.mark.parametrize("kind", ("md5", "crc32", "md5crc32"))
def test_digest_page_kinds(kind, arrangement, cuda):
    """md5_pages_xdma and pages_xdma16<CRC-32 / MD5 + CRC-32> on every kind of
    every page size, in built order and through d_order."""
    import torch
    import sproxy_amd.md5 as m
    code = {"md5": m.Batcher.MD5, "crc32": m.Batcher.CRC32, "md5crc32": m.Batcher.MD5_CRC32}[kind]
    for P in pk.BATCHES:
        b, p, md5, crc = paged_of(P, False, cuda)
        order = None if arrangement == "identity" else layout(P).perm
        what = f"{kind} at P = {P}, {arrangement}"
        width = {"md5": 16, "crc32": 4, "md5crc32": 32}[kind]
        out = torch.full((b.n + 1, width), 0xAA, dtype=torch.uint8, device=cuda)
        o = None if order is None else torch.from_numpy(order.astype(np.int32)).to(cuda)
        m.digest_pages(code, p.d_pages, p.d_first, p.d_lens, P, order=o,
                       out=out.view(torch.int32).reshape(-1) if kind == "crc32" else out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        assert (got[b.n] == 0xAA).all(), f"{what}: wrote past record n - 1"
        got = got[:b.n]
        if kind != "crc32":
            _same(got[:, :16], md5, what + ", md5", _namer(b))
        if kind != "md5":
            _same(got[:, 16:20] if kind == "md5crc32" else got, crc, what + ", crc", _namer(b))
        if kind == "md5crc32":
            assert not got[:, 20:].any(), f"{what}: bytes 20..31 of a record are zero"


def md5_update_in(ctx, data):
    """MD5Update's effect on the 88 bytes of one context, md5.c:169-215
    restated: buf is left to the reference; bits advance; in[] holds the
    pending bytes and past them what the last compressed block left there."""
    bits = int(ctx[16:24].view("<u8")[0])
    t = (bits >> 3) & 63
    lo = (int(ctx[16:20].view("<u4")[0]) + (len(data) << 3)) & 0xFFFFFFFF
    hi = (int(ctx[20:24].view("<u4")[0]) + (lo < int(ctx[16:20].view("<u4")[0])) + (len(data) >> 29)) & 0xFFFFFFFF
    stream = bytes(ctx[24:24 + t]) + data
    keep = bytes(ctx[24:88])
    nblk = len(stream) >> 6
    if nblk:
        keep = stream[64 * (nblk - 1):64 * nblk]
    r = len(stream) - 64 * nblk
    return lo, hi, stream[64 * nblk:] + keep[r:]


def _ctx_round(c, b, p, what):
    """One paged update of every context; all 88 bytes against the reference
    and in[] and bits against md5.c restated."""
    import torch
    import sproxy_amd.md5 as m
    before = c.ctx_h.copy()
    m.update_ctx_pages(c.ctx, p.d_pages, p.d_first, p.d_lens, b.P)
    torch.cuda.synchronize()
    data = np.frombuffer(b"".join(p.chunks) + b"\0", np.uint8)
    offs = np.concatenate([[0], np.cumsum(b.lens)])[:-1]
    c.ref.update(c.ctx_h, data, offs, b.lens)
    c.sofar = [s + x for s, x in zip(c.sofar, p.chunks)]
    got = c.ctx.cpu().numpy()
    want = c.ctx_h.copy()
    for i in range(b.n):                                 # in[] in full, whichever reference HostRef has
        if b.lens[i]:
            lo, hi, inb = md5_update_in(before[i], p.chunks[i])
            want[i, 16:24] = np.array([lo, hi], "<u4").view(np.uint8)
            want[i, 24:] = np.frombuffer(inb, np.uint8)
    assert c.ref.same(want, c.ctx_h), "the restatement and the reference agree"
    if c.ref.exact:
        assert np.array_equal(want, c.ctx_h)
    _same(got, want, what, _namer(b))


@pytest.mark.gpu
@pytest.mark.parametrize("arrangement", ARRANGEMENTS)
def test_ctx_page_kinds(arrangement, cuda):
    """md5_update_ctx_pages on every kind: round 1 from MD5Init with stale
    in[] (the loader route everywhere), round 2 the same batch over what
    round 1 left pending (the lane route, over pages off the grid too)."""
    import sproxy_amd.md5 as m
    from test_ctx_pages import Contexts
    for P in pk.BATCHES:
        b, p, md5, _ = paged_of(P, arrangement != "identity", cuda)
        c = Contexts(b.n, cuda, 3 + P)
        assert not c.pending().any()
        for rnd in (1, 2):
            _ctx_round(c, b, p, f"md5_update_ctx_pages at P = {P}, {arrangement}, round {rnd}")
            if rnd == 1:
                assert np.array_equal(c.pending(), b.lens % 64)
        got = m.final_ctx(c.ctx).cpu().numpy()
        assert not c.ctx.any().item()                                  # md5.c:264
        assert np.array_equal(got, c.ref.final(c.ctx_h))
        want = np.array([np.frombuffer(hashlib.md5(x + x).digest(), np.uint8) for x in p.chunks])
        _same(got, want, f"final_ctx at P = {P}, {arrangement}", _namer(b))


@pytest.mark.gpu
@pytest.mark.parametrize("F", WINDOWS)
def test_window_kinds(F, cuda):
    """crc32_pages_fast on the window kinds, built in both orders (the kernel
    takes no order); the ragged pipelined kind is the launch's last group."""
    import torch
    import sproxy_amd.md5 as m
    from test_pages_verify import window_crc
    for permuted in (False, True):
        b, p, _, _ = paged_of(f"win{F}", permuted, cuda)
        what = f"crc32_pages_fast F = {F} at P = {b.P}, {ARRANGEMENTS[permuted]}"
        out = torch.full((b.n + 1,), -0x55555556, dtype=torch.int32, device=cuda)
        m.crc32_pages(p.d_pages, p.d_first, p.d_lens, b.P, F, out=out[:b.n])
        torch.cuda.synchronize()
        got = out.cpu().numpy().view("<u4")
        assert got[b.n] == 0xAAAAAAAA, f"{what}: wrote past value n - 1"
        want = np.array([window_crc(c, F) for c in p.chunks], dtype="<u4")
        _same(got[:b.n], want, what, _namer(b))


# ---- crc32_pages_fast past its first grid trip
TRIP_P, SHORT_LEN = 256, 40
PIPE, LANE = 0, 1


def trip_shapes(G, cus):
    """PIPE or LANE per group, so that a wave's successive trips show all four
    transitions: the waves take (PIPE, PIPE), (PIPE, LANE), (LANE, PIPE) and
    (LANE, LANE) on trips 0 and 1 by their index mod 4, and the other shape
    on trip 2."""
    step = cus * FAST_PIPE[0]
    g = np.arange(G)
    w, t = g % step, g // step
    pat = np.array([[PIPE, PIPE, LANE], [PIPE, LANE, PIPE], [LANE, PIPE, LANE], [LANE, LANE, PIPE]])
    gs = pat[w % 4, np.minimum(t, 2)]
    gs[G - 1] = PIPE                                  # the ragged last group, pipelined
    return gs


def trip_batch(cus):
    """(lens, first, slot per entry, nslots, shapes): about 2.25 trips of
    32-chunk groups.  Chunks have one or two pages; lengths are 128 + 16 j
    bytes past a page start, so both windows of 64 and of 128 bytes lie
    inside one page on the 16-B grid -- except in the LANE groups, which
    alternate between every length 4 bytes longer (tail windows off the grid)
    and one chunk of SHORT_LEN bytes.  Pages are drawn from a small pool:
    one page serves many chunks."""
    wpc, cpg = FAST_PIPE
    G = trips.ngroups_for(cus, wpc, 2.25)
    gs = trip_shapes(G, cus)
    n = (G - 1) * cpg + trips.RAGGED[cpg]
    rng = np.random.default_rng(SEED)
    k = rng.integers(0, 2, (G, cpg))
    j = rng.integers(0, 9, (G, cpg))
    j[(k == 0) & (j == 0)] = 1                        # longer than 128 bytes
    lens = k * TRIP_P + 128 + 16 * j
    lane = np.flatnonzero(gs == LANE)
    lens[lane[0::2]] += 4
    lens[lane[1::2], rng.integers(0, trips.RAGGED[cpg], lane[1::2].size)] = SHORT_LEN
    lens = lens.reshape(-1)[:n]
    need = (lens + TRIP_P - 1) // TRIP_P
    first = np.concatenate([[0], np.cumsum(need)])
    nslots = 4096
    slot = rng.integers(0, nslots, int(first[-1]))
    return lens, first, slot, nslots, gs


def test_trip_shapes_show_all_four_transitions():
    for cus in (8, 256, 304):
        wpc, cpg = FAST_PIPE
        lens, first, slot, nslots, gs = trip_batch(cus)
        G = gs.size
        assert trips.trip_of(G - 1, cus, wpc) == 2 and lens.size == (G - 1) * cpg + trips.RAGGED[cpg]
        assert trips.shape_pairs(gs, cus, wpc) == {(a, b) for a in (PIPE, LANE) for b in (PIPE, LANE)}
        if cus != 8:
            continue
        # the marks are what the kernel will see, for both windows
        at = BASE + slot * (TRIP_P + pk.PAD)
        for F in (64, 128):
            for g in range(G):
                c = np.arange(g * cpg, min((g + 1) * cpg, lens.size))
                l32 = np.zeros(cpg, np.int64)
                l32[:c.size] = lens[c]
                w = pk.classify_windows(l32, [at[first[i]:first[i + 1]] for i in c], TRIP_P, F, 2 * c.size)
                assert w["pipe"] == (gs[g] == PIPE), (F, g)
                if gs[g] == LANE:
                    # 4 bytes longer: the tail window is off the grid (and may then straddle a page end)
                    assert w["reasons"] in ({"len_off"}, {"len_off", "room"}, {"short"}), (F, g, w["reasons"])
        lanes = np.flatnonzero(gs == LANE)
        assert (lens.reshape(-1)[lanes[0] * cpg:(lanes[0] + 1) * cpg] % 16 == 4).all()
        assert (lens[lanes[1] * cpg:(lanes[1] + 1) * cpg] == SHORT_LEN).sum() == 1


@pytest.fixture(scope="module")
def trip_pool(cuda):
    """One pool and one table for both windows."""
    import torch
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    lens, first, slot, nslots, gs = trip_batch(cus)
    S = TRIP_P + pk.PAD
    host = np.random.default_rng(SEED + 1).integers(0, 256, nslots * S + pk.PAD, dtype=np.uint8)
    pool = torch.from_numpy(host).to(cuda)
    assert pool.data_ptr() % 128 == 0
    dev = dict(pages=torch.from_numpy(pool.data_ptr() + slot * S).to(cuda),
               first=torch.from_numpy(first[:-1].copy()).to(cuda),
               lens=torch.from_numpy(lens.astype(np.int32)).to(cuda))
    host.setflags(write=False)
    return cus, lens, first, slot, gs, host, pool, dev


@pytest.mark.gpu
@pytest.mark.parametrize("F", (64, 128))
def test_window_trips(F, trip_pool, cuda):
    """About 2.25 trips of crc32_pages_fast's (16 waves, 32 chunks) frame: a
    wave hashes a group while the next one's windows are in flight (F = 128:
    both halves of the ring), and goes from pipelined groups to lane groups
    and back in every order."""
    import torch
    import sproxy_amd.md5 as m
    cus, lens, first, slot, gs, host, pool, dev = trip_pool
    wpc, cpg = FAST_PIPE
    assert trips.shape_pairs(gs, cus, wpc) == {(a, b) for a in (PIPE, LANE) for b in (PIPE, LANE)}
    assert lens.size % cpg == trips.RAGGED[cpg], "the last group is ragged"
    n, S = lens.size, TRIP_P + pk.PAD
    out = torch.full((n + 1,), -0x55555556, dtype=torch.int32, device=cuda)
    m.crc32_pages(dev["pages"], dev["first"], dev["lens"], TRIP_P, F, out=out[:n])
    torch.cuda.synchronize()
    got = out.cpu().numpy().view("<u4")
    assert got[n] == 0xAAAAAAAA
    from test_pages_verify import window_crc
    at = slot * S
    want = np.empty(n, "<u4")
    for i in range(n):
        L = int(lens[i])
        c = b"".join(host[a:a + min(TRIP_P, L - k * TRIP_P)].tobytes() for k, a in enumerate(at[first[i]:first[i + 1]]))
        want[i] = window_crc(c, F)
    bad = np.flatnonzero(got[:n] != want)
    if bad.size:
        g = int(bad[0]) // cpg
        pytest.fail(f"F = {F}: {bad.size} of {n} differ; first: chunk {int(bad[0])}, lane {2 * (int(bad[0]) % cpg)} of "
                    f"{'lane' if gs[g] else 'pipelined'} group {g} (trip {trips.trip_of(g, cus, wpc)}), "
                    f"{int(lens[bad[0]])} bytes; groups {sorted(set((bad // cpg).tolist()))[:8]}")
