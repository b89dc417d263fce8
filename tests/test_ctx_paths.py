"""md5hip_update_ctx on its fast paths with pending bytes in the contexts.

The entry keeps callers fast when each context's data is 16-B aligned past its
pending bytes (t != 0, (ptr + 64 - t) % 16 == 0): such groups run as fed pairs
in md5_update_ctx_fed and through the LDS-DMA loader in md5_update_ctx, with
the chain starting from a state the pending block has already changed and the
span starting 64 - t bytes into the update.  tests/test_ctx.py reaches that
combination in one shape of the fed kernel and never in the loader kernel
(test_existing_shapes_leave_the_gap states it); the plans here (tests/
ctx_paths.py) hold it in every group kind, in both kernels, and compare all 88
bytes of every context with md5.c after every update.

CPU tests (-m "not gpu") keep the coverage claim honest: every group of every
plan takes the path its kind claims for 64, 256 and 304 CUs, the numpy model of
bits[] and in[] equals the reference, and the reference sequence's digests are
hashlib's."""
import contextlib
import ctypes
import functools
import hashlib

import numpy as np
import pytest

import ctx_paths as cp
import gen
import sproxy_amd.md5 as m
from test_ctx import HostRef

POOL_SEED = 0xC7C7
FED_GROUPS = len(cp.KINDS)               # P: one full group of every kind, then a ragged one
CANARY_KINDS = ("residues", "mixed_odd", "lined", "mixed")
MD5_INIT = bytes.fromhex("0123456789abcdeffedcba9876543210")


def n_fed():
    return 64 * FED_GROUPS + cp.RAGGED


def n_loader(cus):
    return 64 * (cus + 2) + cp.RAGGED


@functools.lru_cache(maxsize=None)
def pool():
    p = gen.xorshift_array(cp.POOL, seed=POOL_SEED)
    p.setflags(write=False)
    return p


def _frozen(a):
    a.setflags(write=False)
    return a


class Case:
    """A plan and, computed once on the host: the contexts after MD5Init and
    after each of the three rounds from md5.c (HostRef) and from the model
    (bits[] and in[] only), the digests from md5.c and from hashlib."""

    def __init__(self, plan):
        self.plan, self.n = plan, plan.n
        self.ref = ref = HostRef()
        data = pool()
        rng = np.random.default_rng(88)      # a plan's head starts from the same bytes
        self.start = _frozen(rng.integers(0, 256, (plan.n, 88), dtype=np.uint8))   # before MD5Init
        ctx = self.start.copy()
        ctx[:, :16] = np.frombuffer(MD5_INIT, np.uint8)
        ctx[:, 16:24] = 0                                        # in[] keeps its stale bytes
        model = ctx.copy()
        self.after, self.model = [_frozen(ctx.copy())], [_frozen(model)]
        for offs, lens, _ in plan.rounds:
            ref.update(ctx, data, offs, lens)
            model = cp.model_update(model, data, offs, lens)
            self.after.append(_frozen(ctx.copy()))
            self.model.append(_frozen(model))
        self.digests = _frozen(ref.final(ctx))
        assert not ctx.any()
        self.hashlib = _frozen(np.array([np.frombuffer(hashlib.md5(b"".join(
            data[int(o[i]):int(o[i]) + int(L[i])].tobytes() for o, L, _ in plan.rounds)).digest(), np.uint8)
            for i in range(plan.n)]))

    def bad_rows(self, got, k):
        """Contexts that differ from md5.c's after step k (what HostRef.same compares)."""
        want = self.after[k]
        if self.ref.exact:
            return np.flatnonzero((got != want).any(axis=1))
        return np.array([i for i in range(self.n) if not self.ref.same(got[i:i + 1], want[i:i + 1])], np.int64)


@functools.lru_cache(maxsize=None)
def case_for(n, kinds=None):
    return Case(cp.build(n, kinds=kinds))


# ----------------------------------------------------------------- CPU: the plans
@pytest.mark.parametrize("cus", [64, 256, 304])
def test_every_group_takes_the_path_its_kind_claims(cus):
    for kernel, n in (("fed", n_fed()), ("loader", n_loader(cus))):
        plan = cp.build(n)
        g = (n + 63) // 64
        assert n % 64 == cp.RAGGED, "a ragged last group"
        assert g <= cus if kernel == "fed" else g >= cus + 2
        assert set(plan.kinds) == set(cp.KINDS) and plan.kinds.count("long_lane") == 1
        for rnd in (1, 2):
            offs, lens, t = plan.rounds[rnd]
            assert offs.min() >= 0 and int((offs + lens).max()) <= cp.POOL
            got_kernel, paths = cp.classify(t, offs, lens, n, cus)
            assert got_kernel == kernel
            want = [cp.claim(k, kernel, rnd) for k in plan.kinds]
            wrong = [(i, plan.kinds[i], paths[i], want[i]) for i in range(g) if paths[i] != want[i]]
            assert not wrong, (kernel, rnd, wrong[:8])
        assert {"fed", "lane", "nostage"} <= set(paths) if kernel == "fed" else \
            {"dma_lined", "dma_offline", "lane", "nostage"} <= set(paths)


def test_plan_shapes_are_what_they_claim():
    """Per kind: the pending bytes, block counts, roles and alignments of the
    issue's table, in both measured rounds; the asymmetry between the two
    kernels' alignment tests; one_off next to groups that keep their path."""
    n = n_loader(64)
    plan = cp.build(n)
    full = n // 64
    for rnd in (1, 2):
        offs, lens, t = plan.rounds[rnd]
        append, pos, nblk = cp.spans(t, lens)
        role = plan.roles[rnd]
        for k in range(full):
            s = slice(64 * k, 64 * k + 64)
            kind, T, A, B, L = plan.kinds[k], t[s], (offs + pos)[s], nblk[s], lens[s]
            if kind == "t0":
                assert not T.any() and not (L % 64).any() and not (A % 128).any()
                continue
            if not kind.startswith("mixed"):
                assert sorted(T) == list(range(64)), (kind, rnd)           # every residue in one group
                assert sorted((T + L) % 64) == list(range(64)), (kind, rnd)    # tails 0..63
            if kind in ("residues", "lined", "offline", "one_off"):
                assert B.min() >= 2 and B.max() <= 9
            if kind == "lined":
                assert not (A % 128).any()
            if kind == "offline":
                assert not (A % 16).any() and (A % 128 != 0).all() and len(set(A % 128)) == 7
            if kind == "residues":
                assert not (A % 16).any() and (A % 128 != 0).any()
            if kind == "one_off":
                off = np.flatnonzero(A % 16)
                assert off.size == 1 and A[off[0]] % 16 == 4 and off[0] < cp.RAGGED
                assert plan.kinds[k - 1] == "residues" and plan.kinds[k + 1] == "lined"
            if kind.startswith("small_bmax"):
                b = int(kind[10:])
                assert B.max() == b and (B == b).sum() == 1 and int(np.argmax(B)) < cp.RAGGED
                assert not (A % 16).any()
            if kind == "long_lane":
                assert sorted(B)[-3:] == list(cp.LONG_BLOCKS) and sorted(B)[-4] == 2
                assert max(cp.LONG_LANES) < cp.RAGGED
            if kind.startswith("mixed"):
                R = role[s]
                z, ap, ex = R == cp.ZERO, R == cp.APPEND, R == cp.EXACT
                assert min(z.sum(), ap.sum(), ex.sum()) >= 6, (kind, rnd)
                assert min(z[:cp.RAGGED].sum(), ap[:cp.RAGGED].sum(), ex[:cp.RAGGED].sum()) >= 3
                assert not L[z].any()
                assert (T[ap] != 0).all() and (L[ap] >= 1).all() and ((T + L)[ap] < 64).all()
                assert append[s][ap].all() and not append[s][~ap & ~z].any()
                assert (T[ex] != 0).all() and ((T + L)[ex] == 64).all() and not B[ex].any()
                assert B[cp.MIXED_TOP] == cp.MIXED_BMAX == B.max() and (B == B.max()).sum() == 1
                assert ((B == 0) & (R == cp.BULK)).any(), "a bulk lane without a whole block"
                none = B == 0
                assert not (A[~none] % 16).any()
                if kind == "mixed":
                    assert not (A[none] % 16).any()          # aligned to its pos: the loader takes DMA
                else:
                    assert (A[none] % 2 == 1).all()          # odd: fed ignores them, the loader does not
    # a zero-length lane has a valid pointer (a pool offset), and there are many
    offs, lens, _ = plan.rounds[1]
    assert (lens == 0).sum() >= 6 * plan.kinds.count("mixed") and offs[lens == 0].max() < cp.POOL
    # round 0 only leaves the pending bytes
    offs, lens, t = plan.rounds[0]
    assert not t.any() and np.array_equal(lens, plan.rounds[1][2]) and lens.max() == 63
    # the same groups whatever the batch size
    small = cp.build(n_fed())
    for a, b in zip(small.rounds[1:], plan.head(n_fed()).rounds[1:]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _existing_shapes(golden):
    """(name, n, data alignment known?, [(t, offs, lens)]) of tests/test_ctx.py's
    update calls, drawn as that file draws them."""
    out = []
    g = golden["random_lengths"]
    lens, splits = np.array(g["lengths"]), np.array(g["splits"])
    out.append(("golden", lens.size, [(np.zeros(lens.size, np.int64), np.zeros(lens.size, np.int64), splits),
                                      (splits % 64, splits, lens - splits)]))
    rng = np.random.default_rng(1321)
    n, size = 512, 4 << 20
    rng.integers(0, 256, (n, 64), dtype=np.uint8)
    t, calls = np.zeros(n, np.int64), []
    for r in range(7):
        kind = rng.integers(0, 5, n)
        lens = np.where(kind == 0, 0,
               np.where(kind == 1, rng.integers(1, 64, n),
               np.where(kind == 2, rng.integers(64, 200, n),
               np.where(kind == 3, rng.integers(1000, 70000, n), rng.integers(0, 300000, n)))))
        offs = rng.integers(0, size - 300000, n)
        calls.append((t, offs, lens))
        t = (t + lens) % 64
    out.append(("random sequences", n, calls))
    rng = np.random.default_rng(29)
    n = 64
    rng.integers(0, 256, (n, 88), dtype=np.uint8)
    rng.integers(0, 1 << 31, n)
    lens = rng.integers(0, 9000, n)
    lens[0] = (1 << 29) + 5
    offs = rng.integers(0, 4000, n)
    offs[0] = 3
    out.append(("bit count", n, [(np.arange(n) % 64, offs, lens)]))
    for groups in (24, 300):
        rng = np.random.default_rng(4242 + groups)
        n, size = 64 * groups, 12 << 20
        wave = np.arange(n) // 64
        t, calls = np.zeros(n, np.int64), []
        for r in range(3):
            lens = rng.integers(1, 200, n) * 64 + np.where(wave % 3 == 0, 0, rng.integers(0, 64, n))
            offs = rng.integers(0, (size - 20000) // 128, n) * 128
            offs = np.where(wave % 4 == 1, offs + 16 * rng.integers(1, 8, n), offs)
            offs = np.where(wave % 4 == 2, offs + rng.integers(1, 16, n), offs)
            calls.append((t, offs, lens))
            t = (t + lens) % 64
        out.append((f"lds dma {groups}", n, calls))
    return out


@pytest.mark.parametrize("cus", [64, 256, 304])
def test_existing_shapes_leave_the_gap(golden, cus):
    """tests/test_ctx.py's shapes (device buffers are 128-B aligned, so an offset
    is an address here): no group with pending bytes on an LDS-DMA path in
    either kernel, and pending bytes on the fed path only in the golden test."""
    seen = set()
    for name, n, calls in _existing_shapes(golden):
        for t, offs, lens in calls:
            kernel, paths = cp.classify(t, offs, lens, n, cus)
            for k, path in enumerate(paths):
                pending = bool(np.asarray(t)[64 * k:64 * k + 64].any())
                seen.add((kernel, path, pending))
                if pending and path.startswith("dma"):
                    pytest.fail(f"{name}: group {k} has pending bytes on {path} in the {kernel} kernel")
                if pending and path == "fed":
                    assert name == "golden", name
    assert ("fed", "fed", True) in seen                        # the one exception
    assert {p for k, p, pend in seen if k == "loader"} == ({"dma_lined", "dma_offline", "lane"} if cus < 300 else set())


# ----------------------------------------------------------------- CPU: the model and the reference
def _same_bits_and_in(ref, model, want):
    """bits[] and in[] of the model against md5.c's (all 64 bytes of in[] with
    the reference build, in[0 .. count) with the restatement)."""
    if ref.exact:
        return np.array_equal(model[:, 16:], want[:, 16:])
    patched = want.copy()
    patched[:, :16] = model[:, :16]
    return ref.same(model, patched)


@pytest.mark.parametrize("which", ["fed", "loader"])
def test_model_equals_md5c_on_the_plans(which):
    c = case_for(n_fed() if which == "fed" else n_loader(64))
    for k, (model, want) in enumerate(zip(c.model, c.after)):
        assert _same_bits_and_in(c.ref, model, want), k


def test_model_equals_md5c_on_random_triples():
    """2,000 random (t, len, alignment): zero, appending, exactly completing,
    straddling and multi-block lengths; stale in[] bytes; any bit count."""
    ref = HostRef()
    rng = np.random.default_rng(2000)
    n, data = 2000, pool()
    ctx = rng.integers(0, 256, (n, 88), dtype=np.uint8)
    t = rng.integers(0, 64, n)
    bits = ctx[:, 16:24].view("<u4")
    bits[:, 0] = (bits[:, 0] & ~np.uint32(63 << 3)) | (t << 3).astype(np.uint32)
    bits[:n // 8, 0] |= np.uint32(0xFFFF0000)                  # near the carry into bits[1]
    kind = rng.integers(0, 6, n)
    lens = np.where(kind == 0, 0,
           np.where(kind == 1, rng.integers(0, 64, n) % np.maximum(64 - t, 1),
           np.where(kind == 2, 64 - t,
           np.where(kind == 3, 64 - t + rng.integers(0, 64, n),
           np.where(kind == 4, rng.integers(64, 700, n), rng.integers(0, 70000, n))))))
    offs = rng.integers(0, 4096, n) * 128 + rng.integers(0, 128, n)
    want = ctx.copy()
    model = cp.model_update(ctx, data, offs, lens)
    ref.update(want, data, offs, lens)
    assert _same_bits_and_in(ref, model, want)
    append, pos, nblk = cp.spans(t, lens)
    assert append.sum() > 100 and ((pos > 0) & (nblk == 0)).sum() > 100 and ((pos > 0) & (nblk > 0)).sum() > 100


@pytest.mark.parametrize("which", ["fed", "loader"])
def test_reference_digests_are_hashlibs(which):
    c = case_for(n_fed() if which == "fed" else n_loader(64))
    assert np.array_equal(c.digests, c.hashlib)


# ----------------------------------------------------------------- GPU
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def d_pool(cuda):
    import torch
    d = torch.from_numpy(np.array(pool())).to(cuda)
    assert d.data_ptr() % 128 == 0                             # a pool offset's alignment is its address's
    return d


def _kinds_of(case, rows):
    return sorted({case.plan.kinds[g] for g in np.unique(np.asarray(rows) // 64)})


class Run:
    """One plan on the device.  The contexts are rows 0 .. n - 1 of an
    [n + 1, 88] view that starts `shift` bytes into a flat tensor, the digests
    rows 0 .. n - 1 of [n + 1, 16]; everything around them is 0xAA and is
    asserted untouched by every snapshot."""

    def __init__(self, case, d_pool, cuda, shift=0, stream=None):
        import torch
        self.case, self.n, self.stream, self.shift = case, case.n, stream, shift
        n = case.n
        self.flat = torch.full((16 + (n + 1) * 88,), 0xAA, dtype=torch.uint8, device=cuda)
        self.rows = self.flat[shift:shift + (n + 1) * 88].view(n + 1, 88)
        self.ctx = self.rows[:n]
        self.ctx.copy_(torch.from_numpy(np.array(case.start)))
        assert self.ctx.data_ptr() % 16 == shift
        self.dig = torch.full((n + 1, 16), 0xAA, dtype=torch.uint8, device=cuda)
        self.h_ptrs = [(offs + d_pool.data_ptr()).astype(np.int64) for offs, _, _ in case.plan.rounds]
        self.h_lens = [lens.astype(np.int32) for _, lens, _ in case.plan.rounds]
        self.ptrs = [torch.from_numpy(p).to(cuda) for p in self.h_ptrs]
        self.lens = [torch.from_numpy(L).to(cuda) for L in self.h_lens]
        if stream is not None:
            stream.wait_stream(torch.cuda.current_stream())

    def snapshot(self, what):
        """The n contexts, once the bytes around them are seen untouched."""
        if self.stream is not None:
            self.stream.synchronize()
        flat = self.flat.cpu().numpy()
        lo, hi = self.shift + self.n * 88, self.shift + (self.n + 1) * 88
        assert (flat[:self.shift] == 0xAA).all(), f"{what}: wrote in front of context 0"
        assert (flat[lo:hi] == 0xAA).all(), f"{what}: wrote context n"
        assert (flat[hi:] == 0xAA).all(), f"{what}: wrote past context n"
        return flat[self.shift:lo].reshape(self.n, 88)

    def check(self, k, what):
        """Every context byte after step k (0 = init, 1..3 = the rounds)."""
        c = self.case
        got = self.snapshot(what)
        if not c.ref.same(got, c.after[k]):
            bad = c.bad_rows(got, k)
            pytest.fail(f"{what}: {bad.size} of {self.n} contexts differ from md5.c, first {int(bad[0])}; "
                        f"groups {np.unique(bad // 64)[:12].tolist()} of kinds {_kinds_of(c, bad)}")
        bad = np.flatnonzero((got[:, 16:] != c.model[k][:, 16:]).any(axis=1))
        if bad.size:
            pytest.fail(f"{what}: bits[] / in[] of {bad.size} contexts differ from the model, first "
                        f"{int(bad[0])}; kinds {_kinds_of(c, bad)}")
        return got

    def go(self, each_round=True):
        """init, the three rounds, final; -> the snapshots taken."""
        snaps = []
        m.init_ctx(self.ctx, stream=self.stream)
        if each_round:
            snaps.append(self.check(0, "init"))
        for r in range(3):
            m.update_ctx(self.ctx, self.ptrs[r], self.lens[r], stream=self.stream)
            if each_round:
                snaps.append(self.check(r + 1, f"round {r}"))
        m.final_ctx(self.ctx, out=self.dig[:self.n], stream=self.stream)
        left = self.snapshot("final")
        dig = self.dig.cpu().numpy()
        assert (dig[self.n] == 0xAA).all(), "final: wrote digest n"
        c = self.case
        bad = np.flatnonzero((dig[:self.n] != c.digests).any(axis=1))
        assert not bad.size, f"{bad.size} digests differ from md5.c, first {int(bad[0])}; kinds {_kinds_of(c, bad)}"
        assert np.array_equal(dig[:self.n], c.hashlib)
        assert not left.any(), "contexts not zeroed (md5.c:264)"
        for r in range(3):
            assert np.array_equal(self.ptrs[r].cpu().numpy(), self.h_ptrs[r]), f"ptrs of round {r} changed"
            assert np.array_equal(self.lens[r].cpu().numpy(), self.h_lens[r]), f"lens of round {r} changed"
        return snaps


def _assert_paths(case, d_pool, kernel):
    """On this device's CU count and the pool's real address, every group
    takes the path its kind claims."""
    for rnd in (1, 2):
        offs, lens, t = case.plan.rounds[rnd]
        got_kernel, paths = cp.classify(t, offs + d_pool.data_ptr(), lens, case.n, _cus())
        assert got_kernel == kernel
        assert paths == [cp.claim(k, kernel, rnd) for k in case.plan.kinds]


@pytest.mark.gpu
def test_fed_kernel_paths(cuda, d_pool):
    """md5_update_ctx_fed: 16 full groups, one of every kind, and a ragged
    `mixed` one; every context byte after init and after every round."""
    assert (n_fed() + 63) // 64 <= _cus()
    c = case_for(n_fed())
    _assert_paths(c, d_pool, "fed")
    Run(c, d_pool, cuda).go()


@pytest.mark.gpu
def test_loader_kernel_paths(cuda, d_pool):
    """md5_update_ctx: the same groups cycled over two groups more than the
    device has CUs, a ragged `residues` group last."""
    c = case_for(n_loader(_cus()))
    _assert_paths(c, d_pool, "loader")
    Run(c, d_pool, cuda).go()


@pytest.mark.gpu
def test_kernel_boundary(cuda, d_pool):
    """Exactly one group per CU (the fed kernel) and the same plan with one
    group more (the loader kernel): both equal md5.c, and the contexts they
    share are byte-identical after every step."""
    cus = _cus()
    big = cp.build(64 * cus + cp.RAGGED)
    runs = []
    for plan, kernel in ((big.head(64 * cus), "fed"), (big, "loader")):
        c = Case(plan)
        offs, lens, t = plan.rounds[1]
        assert cp.classify(t, offs, lens, plan.n, cus)[0] == kernel
        runs.append(Run(c, d_pool, cuda).go())
    assert len(runs[0]) == len(runs[1]) == 4
    for k, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a, b[:64 * cus]), f"step {k}: the two kernels disagree"


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 200])
def test_canaries_and_alignment(cuda, d_pool, n):
    """The context array 0, 4, 8 and 12 bytes past a 16-B boundary (struct
    MD5Context needs 4); nothing written around the contexts and digests, and
    the pointer and length arrays unchanged."""
    c = case_for(n, CANARY_KINDS[:(n + 63) // 64])
    for shift in (0, 4, 8, 12):
        Run(c, d_pool, cuda, shift=shift).go()


@contextlib.contextmanager
def _side_stream(cuda):
    """A non-blocking stream of this test's own as a torch stream, destroyed on
    the way out.  torch.cuda.Stream() hands out pooled streams that keep their
    hardware queue for the life of the process, and the runtime places every
    later stream on the queue with the fewest users: with two more pooled
    streams in use, the two launches of test_queue.py's overlap test
    (test_queue_tickets_complete_out_of_order) no longer overlapped."""
    import torch
    torch.cuda.current_stream().synchronize()                  # the runtime is up and mapped
    with open("/proc/self/maps") as f:                         # the HIP runtime torch has loaded
        hip = ctypes.CDLL(next(line.split()[-1] for line in f if "libamdhip64.so" in line))
    hip.hipStreamCreateWithFlags.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint]
    hip.hipStreamDestroy.argtypes = [ctypes.c_void_p]
    handle = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(handle), 1) == 0      # hipStreamNonBlocking
    try:
        s = torch.cuda.ExternalStream(handle.value, device=cuda)
        yield s
        s.synchronize()
    finally:
        assert hip.hipStreamDestroy(handle) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["fed", "loader"])
def test_back_to_back_on_a_side_stream(cuda, d_pool, which):
    """init, three updates and final enqueued on a side stream with no host
    synchronisation between them; one comparison at the end."""
    c = case_for(n_fed() if which == "fed" else n_loader(_cus()))
    with _side_stream(cuda) as s:
        Run(c, d_pool, cuda, stream=s).go(each_round=False)
