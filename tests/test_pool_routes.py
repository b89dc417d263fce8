"""Which route a submission takes through the multi-GPU pool
(sproxy_amd/csrc/md5_pool.c) with no device.  tests/c/pool_routes.c links
md5_pool.c, md5_stream.c and nc_digest.c against a scripted fake batcher of
its own into a plain executable under ASan + UBSan -- nothing is preloaded,
nothing is loaded into Python -- and runs every case of tests/pool_cases.py:
the return code of every call, the parts cut where md5hip_pool_plan cuts and
where the header says it cuts, every device submission with its range, digest
kind, window, urgency and digest offset, the devices chosen, every attempt's
answer (taken, refused, failed) and what the pool did next, every ticket's
wait and poll results, the digests against the host MD5 / CRC-32, the 0xAA
guards around every digest array, and the pool's and the devices' counters.
The expectations are the table's, written from md5hip.h;
tests/test_pool_routes_gpu.py runs the same table on the device.

Skipped only where gcc or the HIP headers are absent."""
import os
import re
import shutil
import subprocess
from collections import Counter

import pytest

import gen
import pool_cases as pc

CSRC = os.path.join(gen.REPO, "sproxy_amd", "csrc")
INC = os.path.join(gen.REPO, "include")
SRCS = [os.path.join(gen.REPO, "tests", "c", "pool_routes.c")] + \
       [os.path.join(CSRC, s) for s in ("md5_pool.c", "md5_stream.c", "nc_digest.c")]


@pytest.fixture(scope="module")
def harness():
    if not shutil.which("gcc") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers absent")
    exe = os.path.join(gen.REPO, "build", "pool_routes_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-ffunction-sections", "-fdata-sections", "-Wl,--gc-sections",
           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", INC, *SRCS, "-lpthread", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def cpu_cases():
    return [c for c in pc.cases() if c.only != "gpu"]


@pytest.fixture(scope="module")
def observed(harness):
    """{id: [lines]} of one harness process"""
    text = f"arena {pc.ARENA}\n" + "\n".join(c.script() for c in cpu_cases()) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([harness], input=text, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("routes done")
    got, cur = {}, None
    for line in out.stdout.splitlines():
        m = re.fullmatch(r"case (\S+)", line)
        if m:
            cur = got[m.group(1)] = []
        elif line not in ("end", "routes done"):
            cur.append(line)
    return got


class Rec:
    """one md5hip_submit_src call as the fake saw it"""

    def __init__(self, line):
        f = line.split("|")
        self.sub, self.dev, self.lo, self.hi, self.kind, self.fastcrc, self.urgent, self.off = map(int, f[1:9])
        self.ans = f[9]


def records(lines):
    return [Rec(ln) for ln in lines if ln.startswith("src|")]


def spread_ok(got, mode):
    """a spread line against what the table says of it"""
    _, rcs, bad, counts, healthy = got.split("|")
    counts, healthy = [int(x) for x in counts.split(",")], [c == "1" for c in healthy[len("healthy="):]]
    if (rcs, bad) != ("0", "0"):
        return False
    if mode == "*":
        return True
    if mode in ("even", "healthy"):
        live = [c for c, h in zip(counts, healthy) if h]
        return all(c == 0 for c, h in zip(counts, healthy) if not h) and \
            (mode == "healthy" or len(set(live)) == 1)
    return counts == [int(x) for x in mode.split(",")]


def line_ok(got, want):
    if isinstance(want, list):                      # any of these
        return got in want
    if want.startswith("spread|"):
        return got.startswith("spread|") and spread_ok(got, want.split("|")[3])
    g, w = got.split("|"), want.split("|")
    if g[0] == "rc" and re.fullmatch(r"w\d+", g[3]):       # the device in a whole ticket: held against its record
        g[3] = "w"
    return len(g) == len(w) and all(a == b or b.endswith("=*") and a.startswith(b[:-1]) for a, b in zip(g, w))


def test_the_table_names_its_one_sided_cases():
    ids = [c.id for c in pc.cases()]
    assert sorted(c.id for c in pc.cases() if c.only == "cpu") == sorted(pc.CPU_ONLY)
    assert sorted(c.id for c in pc.cases() if c.only == "gpu") == sorted(pc.GPU_ONLY)
    assert set(pc.CPU_ONLY + pc.GPU_ONLY) <= set(ids) and len(pc.CPU_ONLY) == 18 and len(pc.GPU_ONLY) == 0


def test_every_call_returns_what_the_header_says(observed):
    """every line but the device submissions: return codes, tickets, plans, waits and polls (and what
    they blocked on), digests, counters, health, spreading, guards"""
    cases = cpu_cases()
    assert sorted(observed) == sorted(c.id for c in cases)
    bad = []
    for c in cases:
        got = [ln for ln in observed[c.id] if not ln.startswith(("src|", "dev|"))]
        want = c.expect()
        k = next((k for k, (a, b) in enumerate(zip(got, want)) if not line_ok(a, b)), None)
        if k is None and len(got) != len(want):
            k = min(len(got), len(want))
        if k is not None:
            bad.append(f"{c.id}: {len(got)} lines, {len(want)} expected; first difference at {k}\n"
                       f"  want: " + "\n        ".join(map(str, want[max(k - 2, 0):k + 3] or ["(nothing)"])) + "\n"
                       f"  got:  " + "\n        ".join(got[max(k - 2, 0):k + 3] or ["(nothing)"]))
    assert not bad, f"{len(bad)} of {len(cases)} cases:\n" + "\n".join(bad)


def test_every_part_goes_where_the_header_says(observed):
    """the device submissions of each pool submission: ranges, attempts and their answers, kind, window,
    urgency, digest offset, devices"""
    for c in cpu_cases():
        lines = observed[c.id]
        recs = records(lines)
        subs = c.subs()
        assert {r.sub for r in recs} <= set(range(len(subs))), c.id
        for k, s in enumerate(subs):
            what = f"{c.id}: submission {k}"
            mine = [r for r in recs if r.sub == k]
            first = [0, s.n]
            if s.k > 1:                                     # cut where md5hip_pool_plan cuts (held against the table above)
                plan = next(ln for ln in lines if ln.startswith(f"plan|{k}|"))
                first = [int(x) for x in plan.split("|")[3].split(",")]
            ranges = s.ranges(first) if s.k > 1 else [(0, s.n)]
            by_part = {rg: [r for r in mine if (r.lo, r.hi) == rg] for rg in ranges}
            assert sum(map(len, by_part.values())) == len(mine), f"{what}: a device submission of no planned part"
            answers = ["".join(r.ans for r in by_part[rg]) for rg in ranges]
            if s.anyorder:
                assert Counter(answers) == Counter(s.calls), what
            else:
                assert answers == (s.calls or [""] * len(ranges)), what
            dsz = pc.DSZ[s.kind[0]]
            for r in mine:
                assert (r.kind, r.fastcrc) == s.kind, f"{what}: [{r.lo}, {r.hi}) ran as kind {r.kind} window {r.fastcrc}"
                assert r.urgent == int(s.sync), f"{what}: urgent {r.urgent}"
                assert r.off == dsz * r.lo, f"{what}: digests of [{r.lo}, {r.hi}) at byte {r.off}"
            firsts = [by_part[rg][0].dev for rg in ranges if by_part[rg]]
            if s.k > 1 and s.distinct:
                assert len(set(firsts)) == len(firsts), f"{what}: parts share a device: {firsts}"
            if s.devs is not None:
                assert set(firsts) == s.devs if s.k > 1 else set(firsts) <= s.devs, f"{what}: devices {firsts}"
            for rg in ranges:                               # a part moves to another device, never back to one that failed
                devs = [r.dev for r in by_part[rg]]
                assert len(set(devs)) == len(devs), f"{what}: [{rg[0]}, {rg[1]}) tried {devs}"
            # a whole ticket names the device that took it
            rc = next((ln for ln in lines if ln.startswith(f"rc|{k}|")), None)
            if rc and rc.split("|")[3].startswith("w"):
                assert int(rc.split("|")[3][1:]) == mine[-1].dev, what


def test_device_counters_are_the_devices_own(observed):
    """md5hip_pool_device_stats and _device_health of device g are those of the batcher that took the
    submissions recorded for g"""
    seen = 0
    for c in cpu_cases():
        taken, chunks, failed = Counter(), Counter(), set()
        for ln in observed[c.id]:
            f = ln.split("|")
            if f[0] == "src" and f[9] in "TeED":
                taken[int(f[2])] += 1
                chunks[int(f[2])] += int(f[4]) - int(f[3])
            elif f[0] == "spread":
                for g, n in enumerate(f[3].split(",")):
                    taken[g] += int(n)
                    chunks[g] += 4 * int(n)
                failed = {g for g, h in enumerate(f[4][len("healthy="):]) if h == "0"}
            elif f[0] == "health":
                failed = {g for g in range(pc.NDEV) if int(f[3][len("mask="):], 16) >> g & 1}
            elif f[0] == "dev":
                g = int(f[1])
                assert f[2:] == [str(pc.ENODEV if g in failed else 0), f"submissions={taken[g]}", f"chunks={chunks[g]}"], \
                    f"{c.id}: {ln}"
                seen += 1
    assert seen > 100


def test_the_table_reaches_every_branch(observed):
    """Each switch of the table's sections is taken by some case, from both sides: read off the records."""
    lines = [ln for got in observed.values() for ln in got]
    recs = records(lines)
    subs = {(c.id, k): s for c in cpu_cases() for k, s in enumerate(c.subs())}

    def seen(pattern):
        return any(re.search(pattern, ln) for ln in lines)

    # every answer of the fake, and none it gives only to a pool that asks what it must not
    assert {r.ans for r in recs} == set("TNFeEBD")
    # whole and split, synchronous and asynchronous, each kind and window, each record width at a part boundary
    assert {(s.k > 1, s.sync) for s in subs.values()} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {r.urgent for r in recs} == {0, 1}
    assert {(r.kind, r.fastcrc) for r in recs} >= {(pc.MD5, 0), (pc.CRC32, 0), (pc.CRC32, 64), (pc.MD5_CRC32, 0)}
    for kind, dsz in pc.DSZ.items():
        assert any(r.kind == kind and r.lo and r.off == dsz * r.lo and r.ans == "T" for r in recs), kind
    # the three source kinds, an iov chunk of no segment, the closed form of a fixed source
    assert {s.entry for s in subs.values()} == {"ptrs", "iov", "fixed", "verify", "upgrade"}
    assert seen(r"^plan\|\d+\|0\|0,2,5,7,10$")
    # the threshold from both sides, each of the three bounds on the parts, one healthy device
    assert {s.k for s in subs.values()} == {1, 2, 3, 4}
    # cuts: both sides of the target and the tie, empty chunks, an empty part
    assert seen(r"^plan\|\d+\|0\|0,1,3$") and seen(r"^plan\|\d+\|0\|0,2,3$") and seen(r"^plan\|\d+\|0\|0,1,1,3$")
    assert seen(r"^plan\|\d+\|0\|0,1024,2048,3072,4096$")
    # failover: a part moved after a refusal and after a failed launch, and each error that is returned
    answers = Counter()
    for (sub, lo, hi), rs in _by_part(observed).items():
        answers["".join(r.ans for r in rs)] += 1
    assert {"T", "FT", "FFT", "ET", "DT", "N", "e", "E", "D", "B", "FFFF"} <= set(answers), answers
    assert {int(ln.split("|")[2]) for ln in lines if ln.startswith("rc|")} == {0, pc.ENODEV, pc.EIO, pc.E2BIG}
    # tickets: each class, each wait and poll result, waits that blocked, a ring of more than 64
    assert {ln.split("|")[3][0] for ln in lines if ln.startswith("rc|")} == {"0", "w", "s"}
    assert {int(ln.split("|")[2]) for ln in lines if ln.startswith("wait|")} == {0, pc.EIO, pc.ENODEV}
    assert {int(ln.split("|")[2]) for ln in lines if ln.startswith("poll|")} == {0, 1, pc.EIO, pc.ENODEV}
    assert seen(r"^blocked\|") and seen(r"^waitnext\|\d+\|-22$") and seen(r"^twait\|8000000000000001\|-22$")
    assert max(len([s for s in c.subs() if s.ticket() == "s"]) for c in cpu_cases()) > 64 + 10
    # health: failed devices and failovers counted
    assert seen(r"^health\|ndev=4\|nfailed=4\|mask=f\|") and seen(r"\|failovers=3$")


def _by_part(observed):
    parts = {}
    for id, got in observed.items():
        for r in records(got):
            parts.setdefault(((id, r.sub), r.lo, r.hi), []).append(r)
    return parts
