"""The multi-GPU pool's routes as a table: what sproxy_amd/csrc/md5_pool.c does
with a submission -- whether it is split, where it is cut, which devices take
the parts, what happens when a device refuses or fails, what its ticket says,
which digest kind it runs with and where its digests land -- at every switch
point, from both sides.

A case is a short script of public calls (md5hip_pool_* only) on one pool of
four devices with slices of 1 MiB.  A submission names its chunks by length
alone: chunk i lies in one shared arena after chunks [0, i).
tests/test_pool_routes.py runs the table on the CPU against a scripted fake
batcher (tests/c/pool_routes.c) and holds every expectation against the
fake's records; tests/test_pool_routes_gpu.py runs it through
md5hip_pool_create(devices = (0, 0, 0, 0)) on the device and compares every
digest with hashlib and zlib.

The expectations are written from include/md5hip.h, never taken from a run:
the return code of every call, how many parts (min(ceil(weight / split),
healthy devices, n), weight = sum(len + 64)), the cuts (`plan` below is the
header's rule in exact fractions, and the cut cases carry theirs as
literals), per part the fake's answers to every attempt (T taken, N / F
refused healthy / failed, e / E launch failed healthy / with its device, D
failed before the launch, B -E2BIG), the digest kind, window, urgency and
digest offset (lo x record size) of every attempt, the counters, health and
every ticket's wait and poll results.  What the header leaves open is not pinned: which of several equally
loaded devices goes first, which part lands on which device (a case whose
fault is injected on a device, not aimed at a part, compares the parts'
answers as a multiset: `anyorder`), where an exact tie is cut (`tie`), and
what `parts` and `failovers` count when a move found no device.

Steps: Sub (below) and tuples --
  ("split", bytes)  ("digest", kind, fastcrc, rc)  ("fault", g, after)
  ("kill", g): the fault and 8 synchronous whole submissions, all 0 and exact
  ("wait" | "poll" | "waitnext", k, rc[, blocked parts])  ("twait" | "tpoll", ticket, rc)
  ("stats", {...})  ("spread", n, "even" | "healthy")
and, on the CPU only, the fake's controls --
  ("load", g, weight)  ("ans", g, codes)  ("seq", codes)  ("failat", g, nth query)
  ("manual", 0 | 1)  ("finish", k).
"""
from fractions import Fraction

MD5, CRC32, MD5_CRC32 = 0, 1, 2
DSZ = {MD5: 16, CRC32: 4, MD5_CRC32: 32}
ENODEV, EIO, E2BIG, EINVAL = -19, -5, -7, -22
NDEV = 4
SLICE = 1 << 20
ARENA = 8 << 20
S = 65536                                  # the split threshold of most cases
MT = 1 << 63


def arena():
    """the bytes every chunk is cut from: byte k = (k * 2654435761 mod 2^32) >> 24"""
    import numpy as np
    k = np.arange(ARENA, dtype=np.uint64)
    return (((k * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)).astype(np.uint8)


def weight(lens):
    """md5hip.h: weight(chunk) = len + 64"""
    return sum(ln + 64 for ln in lens)


def nparts(lens, split, healthy=NDEV):
    """md5hip.h: only a submission heavier than the threshold is cut, into
    min(ceil(weight / split), healthy devices, n) parts; one device cuts nothing"""
    w = weight(lens)
    if w <= split or healthy <= 1:
        return 1
    return min(-(-w // split), healthy, len(lens))


def plan(lens, k, tie=False):
    """md5hip_pool_plan by the header's words, in exact fractions: part g starts
    at the first chunk whose prefix weight reaches g * total / k, and a chunk
    that straddles the target goes to the side that holds more of it.  A chunk
    with exactly half on each side may go to either (tie=True: both answers);
    a table case keeps clear of a tie by more than integer rounding."""
    w = [ln + 64 for ln in lens]
    total, first, i, acc = sum(w), [0], 0, 0
    ties = []
    for g in range(1, k):
        target = Fraction(total * g, k)
        while i < len(w):
            before = 2 * (target - acc) - w[i]           # > 0: more than half lies before the target
            if abs(before) <= 2:
                assert tie and before == 0, (lens, k, g, i)
                ties.append(len(first))
                break
            if before < 0:
                break
            acc += w[i]
            i += 1
        first.append(i)
    first.append(len(w))
    if not tie:
        return first
    assert len(ties) == 1
    other = list(first)
    other[ties[0]] += 1
    return [first, other]


def fixed_plan(n, k):
    """md5hip.h: lens == NULL: equal counts, first[g] = g * n / nparts"""
    return [g * n // k for g in range(k + 1)]


class Sub:
    """One submission.  entry: ptrs (chunks = [length]), iov / verify /
    upgrade (chunks = [[segment length, ...]]), fixed (chunks = (n, length,
    stride)).  k: the parts it is planned in; cuts: first[0..k] (tie: the two
    allowed answers); calls: per non-empty part the fake's answers to its
    attempts in order ("" = never placed), default all "T"; anyorder: compare
    them as a multiset; devs: the devices of the parts' first attempts (of a
    whole submission: the devices it may go to); distinct: those differ;
    blocked: the parts the call itself waits for while they run (manual
    mode); bad: the chunk whose expected digest verify / upgrade corrupts;
    kind: the (kind, fastcrc) its device submissions carry."""

    def __init__(self, entry, chunks, sync=True, k=1, cuts=None, tie=False, rc=0, calls=None, anyorder=False,
                 devs=None, distinct=True, blocked=(), bad=-1, kind=(MD5, 0)):
        self.entry, self.chunks, self.sync, self.k, self.rc = entry, chunks, sync, k, rc
        self.tie, self.anyorder, self.devs, self.distinct = tie, anyorder, devs, distinct
        self.blocked, self.bad, self.kind = blocked, bad, kind
        if entry == "fixed":
            self.n, self.lens = chunks[0], [chunks[1]] * chunks[0]
            ref = fixed_plan(self.n, k)
        else:
            self.lens = list(chunks) if entry == "ptrs" else [sum(c) for c in chunks]
            self.n = len(self.lens)
            ref = plan(self.lens, k, tie)
        self.cuts = cuts if cuts is not None else ref
        assert self.cuts == ref, (self.cuts, ref)             # a literal is the header's rule worked out by hand
        first = self.cuts[0] if tie else self.cuts
        self.parts = [(first[g], first[g + 1]) for g in range(k)]
        full = [p for p in self.parts if p[0] != p[1]]
        self.calls = list(calls) if calls is not None else (["T"] * len(full) if rc != ENODEV or k > 1 else [])
        assert tie or len(self.calls) == len(full) or not self.calls, (self.calls, full)

    def ranges(self, first):
        return [(first[g], first[g + 1]) for g in range(self.k) if first[g] != first[g + 1]]

    def ticket(self):
        """the class of *ticket after the call: 0, w (whole: the device in its low 6 bits), s (split: bit 63)"""
        if self.sync or self.rc or self.entry in ("verify", "upgrade"):
            return "0"
        return "s" if self.k > 1 else "w"

    def all_taken(self):
        return all(c == "T" for c in self.calls)

    def segments(self, i):
        """chunk i as [(arena offset, length)]"""
        if self.entry == "fixed":
            return [(i * self.chunks[2], self.chunks[1])]
        if self.entry == "ptrs":
            return [(sum(self.lens[:i]), self.lens[i])]
        at, out = sum(self.lens[:i]), []
        for ln in self.chunks[i]:
            out.append((at, ln))
            at += ln
        return out

    def words(self):
        w = ["sub", self.entry, int(self.sync), self.k, self.n]
        if self.entry == "fixed":
            return w + [self.chunks[1], self.chunks[2]]
        if self.entry == "ptrs":
            return w + self.lens
        for c in self.chunks:
            w += [len(c), *c]
        return w + ([self.bad] if self.entry in ("verify", "upgrade") else [])


def stats(submissions, whole, split, parts, nfailed=0, mask=0, failovers=0):
    """md5hip_pool_stats and md5hip_pool_health; None = left open"""
    return ("stats", dict(submissions=submissions, routed_whole=whole, split=split, parts=parts,
                          nfailed=nfailed, mask=mask, failovers=failovers))


CPU_STEPS = ("load", "ans", "seq", "failat", "manual", "finish")


class Case:
    def __init__(self, id, steps, only=None):
        self.id, self.steps, self.only = id, steps, only
        assert only == "cpu" or not any(isinstance(s, tuple) and s[0] in CPU_STEPS for s in steps), id

    def subs(self):
        return [s for s in self.steps if isinstance(s, Sub)]

    def script(self):
        """the case for tests/c/pool_routes.c"""
        w = ["case", self.id, NDEV, SLICE]
        for s in self.steps:
            if isinstance(s, Sub):
                w += s.words()
            elif s[0] == "kill":
                w += ["fault", s[1], 1, "spread", 8]
            elif s[0] in ("twait", "tpoll"):
                w += [s[0], hex(s[1])]
            elif s[0] == "stats":
                w += ["stats"]
            elif s[0] in ("wait", "poll", "waitnext", "spread"):
                w += [s[0], s[1]]
            elif s[0] == "digest":
                w += ["digest", s[1], s[2]]
            else:
                w += list(s)                                  # split, fault and the fake's controls
        return " ".join(str(x) for x in w + ["end"])

    def expect(self):
        """what tests/c/pool_routes.c prints for the case, its src and dev lines apart"""
        out, k = [], 0
        for s in self.steps:
            if isinstance(s, Sub):
                if s.k > 1:
                    firsts = s.cuts if s.tie else [s.cuts]
                    out.append([f"plan|{k}|0|{','.join(map(str, f))}" for f in firsts])
                out += [f"blocked|{k}|{lo}|{hi}" for lo, hi in s.blocked]
                if s.entry in ("verify", "upgrade"):
                    ok = "".join("0" if i == s.bad else "1" for i in range(s.n))
                    out.append(f"{s.entry}|{k}|{s.rc}|{ok}" + ("|md5=ok" if s.entry == "upgrade" else ""))
                else:
                    out.append(f"rc|{k}|{s.rc}|{s.ticket()}")
                    if s.sync and s.rc == 0:
                        out.append(f"digests|{k}|ok")
                k += 1
            elif s[0] == "split":
                out.append("split|0")
            elif s[0] == "digest":
                out.append(f"digest|{s[3]}")
            elif s[0] == "fault":
                out.append("fault|0")
            elif s[0] == "kill":
                out += ["fault|0", "spread|0|0|*"]
            elif s[0] in ("wait", "poll", "waitnext"):
                out += [f"blocked|{s[1]}|{lo}|{hi}" for lo, hi in (s[3] if len(s) > 3 else ())]
                out.append(f"{s[0]}|{s[1]}|{s[2]}")
                if s[0] == "wait" and s[2] == 0:
                    out.append(f"digests|{s[1]}|ok")
            elif s[0] in ("twait", "tpoll"):
                out.append(f"{s[0]}|{s[1]:x}|{s[2]}")
            elif s[0] == "stats":
                d = s[1]
                out.append("stats|" + "|".join(f"{f}={'*' if d[f] is None else d[f]}"
                                               for f in ("submissions", "routed_whole", "split", "parts")))
                out.append(f"health|ndev={NDEV}|nfailed={d['nfailed']}|mask={'*' if d['mask'] is None else format(d['mask'], 'x')}|"
                           f"failovers={'*' if d['failovers'] is None else d['failovers']}")
            elif s[0] == "spread":
                out.append(f"spread|0|0|{s[2]}")
        return out + ["guard|ok"]


# ------------------------------------------------------------------ the cases
def ptrs(lens, **kw):
    return Sub("ptrs", lens, **kw)


EIGHT = [32704] * 8                        # weight 4 S: four parts of two chunks
assert weight(EIGHT) == 4 * S and nparts(EIGHT, S) == 4
TWO = [32704, 32705]                       # weight S + 1: two parts
SMALL = [1000, 0, 2000, 777]


def _threshold():
    c = []
    at, past = [32704, 32704], TWO
    assert weight(at) == S and weight(past) == S + 1 and nparts(at, S) == 1 and nparts(past, S) == 2
    c.append(Case("weight_at_split_goes_whole", [("split", S), ptrs(at), stats(1, 1, 0, 1)]))
    c.append(Case("weight_past_split_two_parts", [("split", S), ptrs(past, k=2, cuts=[0, 1, 2]), stats(1, 0, 1, 2)]))
    # a non-zero threshold is honoured below the slice; 0 is one slice again
    slice_at, slice_past = [65472] * 16, [65472] * 15 + [65473]
    assert weight(slice_at) == SLICE and nparts(slice_past, SLICE) == 2
    c.append(Case("split_zero_is_one_slice",
                  [("split", S), ptrs(past, k=2, cuts=[0, 1, 2]), ("split", 0), ptrs(past), ptrs(slice_at),
                   ptrs(slice_past, k=2, cuts=[0, 8, 16]), stats(4, 2, 2, 6)]))
    # parts = min(ceil(weight / split), healthy, n): each of the three the least
    heavy2 = [65536, 65536]
    assert -(-weight(heavy2) // S) == 3 and nparts(heavy2, S) == 2
    c.append(Case("two_heavy_chunks_make_two_parts", [("split", S), ptrs(heavy2, k=2, cuts=[0, 1, 2]), stats(1, 0, 1, 2)]))
    ten = [16320] * 10
    assert 2 * weight(ten) == 5 * S and nparts(ten, S) == 3
    c.append(Case("two_and_a_half_thresholds_make_three_parts",
                  [("split", S), ptrs(ten, k=3, cuts=[0, 3, 7, 10]), stats(1, 0, 1, 3)]))
    # n the least, where it matters: with four parts the first target would fall nearer the first chunk's end
    three = [186, 106, 716]
    assert weight(three) == 1200 and nparts(three, 100) == 3 and plan(three, 4) == [0, 1, 2, 3, 3]
    c.append(Case("more_thresholds_and_devices_than_chunks",
                  [("split", 100), ptrs(three, k=3, cuts=[0, 2, 2, 3]), stats(1, 0, 1, 2)], only="cpu"))
    twenty = [65536] * 20
    assert -(-weight(twenty) // S) > NDEV
    c.append(Case("many_thresholds_make_one_part_per_device",
                  [("split", S), ptrs(twenty, k=4, cuts=[0, 5, 10, 15, 20]), stats(1, 0, 1, 4)]))
    # three, two and one healthy device: one splits nothing, however heavy
    c.append(Case("healthy_devices_bound_the_parts",
                  [("split", S), ("kill", 2), stats(8, 8, 0, None, 1, 4, 1),
                   ptrs(twenty, k=3), ("kill", 1), stats(17, 16, 1, None, 2, 6, 2),
                   ptrs(twenty, k=2, cuts=[0, 10, 20]), ("kill", 3), stats(26, 24, 2, None, 3, 14, 3),
                   ptrs(twenty), ptrs(twenty, sync=False), ("wait", 3, 0), ("wait", 3, 0),
                   stats(28, 26, 2, None, 3, 14, 3), ("spread", 8, "8,0,0,0")]))
    return c


def _cuts():
    c = []
    # a chunk across the target: more of it after, more of it before, exactly half
    for id, lens, cuts in (("straddling_chunk_mostly_after_the_target", [31936, 39936, 27936], [0, 1, 3]),
                           ("straddling_chunk_mostly_before_the_target", [27936, 39936, 31936], [0, 2, 3])):
        assert weight(lens) == 100000 and nparts(lens, S) == 2
        c.append(Case(id, [("split", S), ptrs(lens, k=2, cuts=cuts), stats(1, 0, 1, 2)]))
    half = [29936, 39936, 29936]
    c.append(Case("straddling_chunk_half_and_half",
                  [("split", S), ptrs(half, k=2, tie=True, cuts=[[0, 1, 3], [0, 2, 3]]), stats(1, 0, 1, 2)]))
    # empty chunks weigh 64 each and spread
    c.append(Case("empty_chunks_spread",
                  [("split", S), ptrs([0] * 4096, k=4, cuts=[0, 1024, 2048, 3072, 4096]),
                   ptrs([0] * 3072 + [65472], k=4, cuts=[0, 1024, 2048, 3072, 3073], sync=False), ("wait", 1, 0),
                   stats(2, 0, 2, 8)]))
    # both targets inside one chunk: the planned part between them is empty and is not submitted
    lens = [65536, 65536, 136]
    assert nparts(lens, S) == 3
    c.append(Case("a_planned_part_is_empty",
                  [("split", S), ptrs(lens, k=3, cuts=[0, 1, 1, 3]), ptrs(lens, k=3, cuts=[0, 1, 1, 3], sync=False),
                   ("wait", 1, 0), ("poll", 1, 1), stats(2, 0, 2, 4), ("spread", 40, "even")]))
    # the source kinds
    iov = [[], [20000], [10000, 5000, 7000]] * 4
    c.append(Case("iov_chunks_of_0_1_and_3_segments",
                  [("split", S), Sub("iov", iov, k=3, cuts=[0, 5, 8, 12]),
                   Sub("iov", iov, k=3, cuts=[0, 5, 8, 12], sync=False), ("wait", 1, 0), stats(2, 0, 2, 6)]))
    c.append(Case("host_fixed_equal_counts",
                  [("split", S), Sub("fixed", (10, 30000, 30016), k=4, cuts=[0, 2, 5, 7, 10]),
                   Sub("fixed", (3, 100, 128)), stats(2, 1, 1, 5)]))
    # 4-, 16- and 32-byte records: every part's digests start at lo x the record size
    for id, kind, f in (("crc32_records_of_a_split", CRC32, 0), ("crc32_window_records_of_a_split", CRC32, 64),
                        ("md5_crc32_records_of_a_split", MD5_CRC32, 0)):
        lens = [32704, 100, 32604, 1, 32703, 30000, 0, 32704, 16000, 21000]
        c.append(Case(id, [("split", S), ("digest", kind, f, 0),
                           ptrs(lens, k=4, kind=(kind, f)), ptrs(lens, k=4, kind=(kind, f), sync=False), ("wait", 1, 0),
                           ptrs(SMALL, kind=(kind, f)), stats(3, 1, 2, 9)]))
    return c


def _devices():
    c = []
    # the least loaded devices get the parts
    c.append(Case("least_loaded_devices_get_the_parts",
                  [("split", S), ("load", 0, 500000), ("load", 2, 300000),
                   ptrs(TWO, k=2, devs={1, 3}), ptrs([16320] * 10, k=3, devs={1, 2, 3}), ptrs(SMALL, devs={1, 3}),
                   ptrs(SMALL, sync=False, devs={1, 3}), ("wait", 3, 0),
                   ("load", 0, 0), ("load", 1, 9), ("load", 2, 9), ("load", 3, 9), ptrs(SMALL, devs={0}),
                   stats(5, 3, 2, 8),
                   # and when the least loaded one refuses and fails, the submission moves on
                   ("ans", 0, "F"), ptrs(SMALL, devs={0}, calls=["FT"]), stats(6, 4, 2, None, 1, 1, 1)], only="cpu"))
    # a failed device is never picked, by a whole submission or a part
    c.append(Case("failed_device_is_never_picked",
                  [("split", S), ("kill", 2), ("spread", 40, "healthy"), ptrs(EIGHT, k=3), ("spread", 40, "healthy"),
                   stats(89, 88, 1, None, 1, 4, 1)]))
    # a device fails between the count of healthy devices and their choice: four parts on three devices
    c.append(Case("fewer_healthy_devices_than_parts",
                  [("split", S), ("failat", 2, 2), ptrs(EIGHT, k=4, devs={0, 1, 3}, distinct=False), stats(1, 0, 1, 4, 1, 4, 0),
                   ("spread", 39, "healthy")], only="cpu"))
    return c


def _failover():
    c = []
    # the launch fails and the device with it: a synchronous caller is moved, an asynchronous ticket keeps -EIO
    c.append(Case("sync_split_part_moves_off_a_failed_launch",
                  [("split", S), ("fault", 2, 1), ptrs(EIGHT, k=4, calls=["ET", "T", "T", "T"], anyorder=True),
                   stats(1, 0, 1, None, 1, 4, 1), ptrs(EIGHT, k=3), ("spread", 8, "healthy")]))
    c.append(Case("async_split_ticket_keeps_eio",
                  [("split", S), ("fault", 1, 1),
                   ptrs(EIGHT, k=4, sync=False, calls=["E", "T", "T", "T"], anyorder=True),
                   ("wait", 0, EIO), ("wait", 0, EIO), ("poll", 0, EIO), ("poll", 0, EIO),
                   stats(1, 0, 1, 4, 1, 2, 0), ptrs(EIGHT, k=3, sync=False), ("wait", 1, 0), ("poll", 1, 1)]))
    c.append(Case("last_device_fails",
                  [("split", S), ("kill", 1), ("kill", 2), ("kill", 3), ("fault", 0, 1),
                   ptrs(SMALL, sync=False, calls=["E"]), ("wait", 0, EIO), ("poll", 0, EIO), ("wait", 0, EIO),
                   ("poll", 0, EIO), stats(25, 25, 0, None, 4, 15, 3),
                   ptrs(SMALL, rc=ENODEV), ptrs(SMALL, rc=ENODEV, sync=False), ptrs(EIGHT, rc=ENODEV, sync=False),
                   Sub("fixed", (3, 100, 128), rc=ENODEV), Sub("iov", [[10], [20, 30]], rc=ENODEV),
                   stats(30, 25, 0, None, 4, 15, 3)]))
    c.append(Case("last_device_fails_under_a_sync_caller",
                  [("split", S), ("kill", 1), ("kill", 2), ("kill", 3), ("fault", 0, 1),
                   ptrs(SMALL, rc=ENODEV, calls=["E"]), stats(25, 25, 0, None, 4, 15, None)]))
    # the fake's answers, aimed at a part
    for sync in (True, False):
        tag = "sync" if sync else "async"
        tail = [] if sync else [("wait", 0, 0), ("poll", 0, 1)]
        # refused before the device took the chunks, by a device that failed: moved, one failover each
        c.append(Case(f"refused_whole_moves_{tag}",
                      [("seq", "FF"), ptrs(SMALL, sync=sync, calls=["FFT"]), *tail, stats(1, 1, 0, None, 2, None, 2)],
                      only="cpu"))
        c.append(Case(f"refused_part_moves_{tag}",
                      [("split", S), ("seq", "TF"), ptrs(EIGHT, k=4, sync=sync, calls=["T", "FT", "T", "T"]), *tail,
                       stats(1, 0, 1, None, 1, None, 1)], only="cpu"))
        # -ENODEV from a device that still reads healthy: returned, not moved
        c.append(Case(f"enodev_from_a_healthy_device_is_returned_{tag}",
                      [("split", S), ("manual", 1), ("seq", "N"), ptrs(SMALL, sync=sync, rc=ENODEV, calls=["N"]),
                       ("seq", "TN"), ptrs(EIGHT, k=4, sync=sync, rc=ENODEV, calls=["T", "N", "", ""], blocked=[(0, 2)]),
                       stats(2, None, None, None, 0, 0, 0), ("manual", 0), ("spread", 40, "even")], only="cpu"))
        # another errno: no later part is placed, the placed ones are waited for, nothing stays claimed
        c.append(Case(f"e2big_part_ends_the_split_{tag}",
                      [("split", S), ("manual", 1), ("seq", "TTB"),
                       ptrs(EIGHT, k=4, sync=sync, rc=E2BIG, calls=["T", "T", "B", ""], blocked=[(0, 2), (2, 4)]),
                       ("seq", "B"), ptrs(SMALL, sync=sync, rc=E2BIG, calls=["B"]),
                       stats(2, None, None, None, 0, 0, 0), ("manual", 0), ("spread", 40, "even")], only="cpu"))
    # the launch fails, the device stays healthy: -EIO is returned, nothing moves
    c.append(Case("eio_from_a_healthy_device_is_returned",
                  [("split", S), ("seq", "e"), ptrs(SMALL, rc=EIO, calls=["e"]),
                   ("seq", "Te"), ptrs(EIGHT, k=4, rc=EIO, calls=["T", "e", "T", "T"]),
                   ("seq", "e"), ptrs(SMALL, sync=False, calls=["e"]), ("wait", 2, EIO), ("wait", 2, EIO),
                   ("poll", 2, EIO), stats(3, 2, 1, 6, 0, 0, 0), ("spread", 40, "even")], only="cpu"))
    # a synchronous whole submission whose launch fails with its device is placed again
    c.append(Case("sync_whole_moves_off_a_failed_launch",
                  [("seq", "E"), ptrs(SMALL, calls=["ET"]), stats(1, 1, 0, None, 1, None, 1),
                   ("seq", "E"), ptrs(SMALL, sync=False, calls=["E"]), ("wait", 1, EIO), ("wait", 1, EIO),
                   stats(2, 2, 0, None, 2, None, 1),
                   # the device fails before the launch: the ticket completes -ENODEV, and the same holds
                   ("seq", "D"), ptrs(SMALL, calls=["DT"]), stats(3, 3, 0, None, 3, None, 2),
                   ("seq", "D"), ptrs(SMALL, sync=False, calls=["D"]), ("wait", 3, ENODEV),
                   ("poll", 3, ENODEV), ("wait", 3, ENODEV), stats(4, 4, 0, None, 4, 15, 2)], only="cpu"))
    # a split ticket's error is its first failing part's, while it is live and after it was dropped
    c.append(Case("first_failing_part_names_the_error",
                  [("split", S), ("manual", 1), ("seq", "TeDT"), ptrs(EIGHT, k=4, sync=False, calls=["T", "e", "D", "T"]),
                   ("finish", 0), ("poll", 0, EIO), ("wait", 0, EIO), ("wait", 0, EIO), ("poll", 0, EIO),
                   ("seq", "TeDT"), ptrs(EIGHT, k=3, sync=False, calls=["T", "e", "D"]), ("finish", 1),
                   ptrs(TWO, k=2, sync=False, calls=["T", "T"], distinct=False), ("wait", 1, EIO), ("poll", 1, EIO)],
                  only="cpu"))
    # once a part has failed for good the others are only waited for: a launch that fails with its device stays failed
    c.append(Case("no_move_after_a_part_failed_for_good",
                  [("split", S), ("seq", "TeET"), ptrs(EIGHT, k=4, rc=EIO, calls=["T", "e", "E", "T"]),
                   stats(1, 0, 1, 4, 1, None, 0)], only="cpu"))
    # every device refuses and fails: -ENODEV, no ticket
    c.append(Case("every_device_refuses_and_fails",
                  [("split", S), ("seq", "FFFF"), ptrs(SMALL, rc=ENODEV, sync=False, calls=["FFFF"]),
                   stats(1, None, None, None, 4, 15, None), ptrs(EIGHT, rc=ENODEV)], only="cpu"))
    return c


def _tickets():
    c = []
    c.append(Case("whole_and_split_tickets",
                  [("split", S), ptrs(SMALL, sync=False), ptrs(EIGHT, k=4, sync=False), ("waitnext", 1, EINVAL),
                   ("wait", 1, 0), ("wait", 0, 0), ("wait", 1, 0), ("wait", 0, 0), ("poll", 0, 1), ("poll", 1, 1),
                   ("poll", 0, 1), ("poll", 1, 1), ("waitnext", 1, EINVAL), stats(2, 1, 1, 5)]))
    unknown = [(99999 << 6) | 1, (5 << 6) | 9, (1 << 6) | NDEV, MT | 999, MT, MT | 1]
    c.append(Case("ticket_0_and_tickets_never_issued",
                  [("twait", 0, 0), ("tpoll", 0, 1), ("twait", 0, 0), ("tpoll", 0, 1)] +
                  [(op, t, EINVAL) for t in unknown for op in ("twait", "tpoll")] + [stats(0, 0, 0, 0)]))
    # tickets completed on command.  78 split tickets, 10 of them done and dropped before the other 68
    # are alive at once; every seventh holds a failed part; waited in reverse
    tiny = [0, 0]
    steps = [("manual", 1), ("split", 100)]
    for k in range(10):
        steps += [ptrs(tiny, k=2, sync=False), ("finish", k), ("wait", k, 0)]
    fails = [k for k in range(10, 78) if k % 7 == 0]
    for k in range(10, 78):
        if k in fails:
            steps.append(("seq", "Te"))
        steps.append(ptrs(tiny, k=2, sync=False, calls=["T", "e"] if k in fails else None))
    for k in reversed(range(78)):
        rc = EIO if k in fails else 0
        steps += [("wait", k, rc, [(0, 1), (1, 2)] if k >= 10 else []), ("poll", k, rc or 1), ("wait", k, rc)]
    c.append(Case("split_tickets_past_one_ring_waited_in_reverse", steps + [stats(78, 0, 78, 156)], only="cpu"))
    # a finished entry behind a running one: each ticket reports its own result, and no wait returns early
    c.append(Case("finished_ticket_behind_a_running_one",
                  [("manual", 1), ("split", 100), ptrs(tiny, k=2, sync=False), ("seq", "Te"),
                   ptrs(tiny, k=2, sync=False, calls=["T", "e"]), ("finish", 1), ptrs(tiny, k=2, sync=False),
                   ("poll", 1, EIO), ("wait", 1, EIO), ("poll", 0, 0), ("poll", 2, 0),
                   ("wait", 0, 0, [(0, 1), (1, 2)]), ("poll", 1, EIO), ("wait", 1, EIO), ("wait", 0, 0),
                   ("poll", 2, 0), ("wait", 2, 0, [(0, 1), (1, 2)]), ("wait", 1, EIO), ("wait", 2, 0), ("poll", 0, 1),
                   ("waitnext", 2, EINVAL)], only="cpu"))
    return c


def _kind():
    c = []
    iov = [[4000, 96], [30000], [], [32000, 1000], [100], [31000]]
    assert nparts([sum(x) for x in iov], S) == 2
    c.append(Case("verify_and_upgrade_submit_with_their_own_kind",
                  [("split", S), ("digest", CRC32, 64, 0),
                   Sub("verify", iov, k=2, rc=1, bad=4, kind=(CRC32, 64)),
                   Sub("upgrade", iov, k=2, rc=1, bad=1, kind=(MD5_CRC32, 0)),
                   Sub("upgrade", iov[:3], rc=0, kind=(MD5_CRC32, 0)),
                   Sub("iov", iov, k=2, kind=(CRC32, 64)), ("digest", MD5, 0, 0),
                   Sub("verify", iov, k=2, rc=0, kind=(MD5, 0)), stats(5, 1, 4, 9)]))
    c.append(Case("set_digest_leaves_earlier_submissions_their_kind",
                  [("split", S), ("digest", MD5, 4, EINVAL), ("digest", CRC32, 6, EINVAL), ("digest", 3, 0, EINVAL),
                   ptrs(EIGHT, k=4, sync=False), ("digest", MD5_CRC32, 0, 0),
                   ptrs(EIGHT, k=4, sync=False, kind=(MD5_CRC32, 0)), ("digest", CRC32, 128, 0),
                   ptrs(SMALL, sync=False, kind=(CRC32, 128)), ("wait", 2, 0), ("wait", 1, 0), ("wait", 0, 0),
                   stats(3, 1, 2, 9)]))
    return c


# One half only.  CPU: loads, refusals aimed at a part, a device that fails
# between two health queries and tickets completed on command are the fake's
# controls; the device half fails devices with the library's own
# md5hip_pool_inject_fault.  GPU: nothing -- every case that needs no such
# control runs on both.
CPU_ONLY = ["least_loaded_devices_get_the_parts", "fewer_healthy_devices_than_parts",
            "refused_whole_moves_sync", "refused_whole_moves_async", "refused_part_moves_sync",
            "refused_part_moves_async", "enodev_from_a_healthy_device_is_returned_sync",
            "enodev_from_a_healthy_device_is_returned_async", "e2big_part_ends_the_split_sync",
            "e2big_part_ends_the_split_async", "eio_from_a_healthy_device_is_returned",
            "sync_whole_moves_off_a_failed_launch", "no_move_after_a_part_failed_for_good",
            "first_failing_part_names_the_error", "more_thresholds_and_devices_than_chunks",
            "every_device_refuses_and_fails", "split_tickets_past_one_ring_waited_in_reverse",
            "finished_ticket_behind_a_running_one"]
GPU_ONLY = []


def cases():
    c = _threshold() + _cuts() + _devices() + _failover() + _tickets() + _kind()
    assert len({x.id for x in c}) == len(c)
    return c
