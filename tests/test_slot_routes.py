"""Which route a slot takes: the batcher of sproxy_amd/csrc/md5_submit.c with
no device.  tests/c/slot_check.c links md5_submit.c, md5_stream.c and
nc_digest.c against the fake runtime (tests/c/fake_hip.c, its record log on)
into a plain executable under ASan + UBSan -- nothing is preloaded, nothing is
loaded into Python -- and runs every case of tests/slot_cases.py: the return
code of each submission, every copy (direction, bytes, whose memory), every
gather table entry, every order build, every planner choice and the hash
launch with the arrays, order and output it was given, then the digests
against the host MD5 / CRC-32 of the source bytes, the 0xAA guard around the
device outputs and the batcher's counters.  The expectations are the table's,
written from md5hip.h; tests/test_slot_routes_gpu.py runs the same table on
the device.

Skipped only where gcc or the HIP headers are absent."""
import os
import re
import shutil
import subprocess

import pytest

import gen
import slot_cases as sc

CSRC = os.path.join(gen.REPO, "sproxy_amd", "csrc")
INC = os.path.join(gen.REPO, "include")
SRCS = [os.path.join(gen.REPO, "tests", "c", s) for s in ("slot_check.c", "fake_hip.c", "fake_dual.c")] + \
       [os.path.join(CSRC, s) for s in ("md5_submit.c", "md5_stream.c", "nc_digest.c")]


@pytest.fixture(scope="module")
def harness():
    if not shutil.which("gcc") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers absent")
    exe = os.path.join(gen.REPO, "build", "slot_check_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", INC,
           *SRCS, "-lpthread", "-o", exe]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]
    return exe


def cpu_cases():
    return [c for c in sc.cases() if c.only != "gpu"]


@pytest.fixture(scope="module")
def observed(harness):
    """{id: [lines]} of one harness process"""
    text = f"arenas {sc.H_BYTES} {sc.D_BYTES} {sc.O_BYTES}\n" + "\n".join(c.script() for c in cpu_cases()) + "\n"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([harness], input=text, capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    got, cur = {}, None
    for line in out.stdout.splitlines():
        m = re.fullmatch(r"case (\S+)", line)
        if m:
            cur = got[m.group(1)] = []
        elif line != "end":
            cur.append(line)
    return got


def _plan_record(nm, r):
    """made by slot_prepare, and made again when the progress thread planned ahead"""
    return r.startswith(("order|", "plan_desc|", "choice|lines|")) or \
        (r.startswith("copy|H2D|") and (f"|{nm.DBKT}+0|" in r or r.endswith(f"|{nm.DORD}+0|{nm.HORD}+0")))


def _desc_copy(nm, r):
    return r.startswith("copy|H2D|") and (f"|{nm.MOFF}+" in r or f"|{nm.MLEN}+" in r)


def route(case, lines):
    """the records of the case's own launches, as the table states them"""
    nm = sc.Names(case.create)
    rec = [ln for ln in lines if not ln.startswith(("rc|", "wait|", "digests|", "guard|", "stats|"))]
    if case.coalesced:
        assert rec.count("mark") == 1
        rec = rec[rec.index("mark") + 1:]
        h = next(k for k, r in enumerate(rec) if r.startswith("hash|"))
        last = max(k for k in range(h) if rec[k].startswith("choice|lines|"))
        start = last
        while start and _plan_record(nm, rec[start - 1]):
            start -= 1
        rec = [r for k, r in enumerate(rec) if k >= start or not _plan_record(nm, r)]
    return sum_desc(nm, rec) if case.sum_desc else rec


def sum_desc(nm, rec):
    """the descriptor copies as one record of their total"""
    total = sum(int(r.split("|")[2]) for r in rec if _desc_copy(nm, r))
    out, done = [], False
    for r in rec:
        if not _desc_copy(nm, r):
            out.append(r)
        elif not done:
            out.append(f"desc|{total}")
            done = True
    return out


def test_the_table_names_its_one_sided_cases():
    ids = [c.id for c in sc.cases()]
    assert sorted(c.id for c in sc.cases() if c.only == "cpu") == sorted(sc.CPU_ONLY)
    assert sorted(c.id for c in sc.cases() if c.only == "gpu") == sorted(sc.GPU_ONLY)
    assert set(sc.CPU_ONLY + sc.GPU_ONLY) <= set(ids) and len(sc.CPU_ONLY) == 3 and len(sc.GPU_ONLY) == 1


def test_every_case_takes_the_route_the_header_says(observed):
    cases = cpu_cases()
    assert sorted(observed) == sorted(c.id for c in cases)
    bad = []
    for c in cases:
        lines = observed[c.id]
        nm = sc.Names(c.create)
        got = route(c, lines)
        want = sum_desc(nm, c.expect) if c.sum_desc else c.expect
        if got != want:
            k = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
            bad.append(f"{c.id}: {len(got)} records, {len(want)} expected; first difference at {k}\n"
                       f"  want: " + "\n        ".join(want[max(k - 2, 0):k + 3] or ["(nothing)"]) + "\n"
                       f"  got:  " + "\n        ".join(got[max(k - 2, 0):k + 3] or ["(nothing)"]))
    assert not bad, f"{len(bad)} of {len(cases)} cases:\n" + "\n".join(bad)


def test_every_submission_returns_0_with_its_digests(observed):
    for c in cpu_cases():
        lines = observed[c.id]
        nsub = len(c.subs) + c.coalesced
        assert [ln for ln in lines if ln.startswith("rc|")] == [f"rc|{k}|0" for k in range(nsub)], c.id
        assert not [ln for ln in lines if ln.startswith("wait|")], c.id
        assert [ln for ln in lines if ln.startswith("digests|")] == [f"digests|{k}|ok" for k in range(nsub)], c.id
        assert "guard|ok" in lines, c.id


def test_counters(observed):
    for c in cpu_cases():
        line = next(ln for ln in observed[c.id] if ln.startswith("stats|"))
        st = {k: int(v) for k, v in (f.split("=") for f in line.split("|")[1:])}
        want = dict(c.stats, submissions=len(c.subs) + c.coalesced,
                    chunks=sum(s.n for s in c.subs) + c.coalesced)
        assert {k: st[k] for k in want} == want, c.id


def test_the_table_reaches_every_branch(observed):
    """Each route named in the table's sections is taken by some case: read off the records."""
    nm = sc.Names(sc.B1)
    rec = [r for lines in observed.values() for r in lines]
    hashes = [r.split("|") for r in rec if r.startswith("hash|") and "_desc|" in r]

    def seen(pattern):
        return any(re.search(pattern, r) for r in rec)

    D, HD, O = re.escape(nm.DATA), re.escape(nm.HDATA), r"O\+\d+"
    # bytes in: staged, gathered by the kernel, DMA per run, fixed from pinned and from pageable, none
    assert seen(rf"^copy\|H2D\|\d+\|{D}\+0\|{HD}\+0$")
    assert seen(rf"^gather\|\d+\|\S+\|{D}\+0$") and seen(rf"^seg\|H\+\d+\|{D}\+\d+\|65536$")
    assert seen(rf"^copy\|H2D\|\d+\|{D}\+\d+\|H\+\d+$")
    assert seen(r"^hash\|md5_fixed\|.*\|D\+\d+\|") and seen(rf"^hash\|md5_fixed\|.*\|{D}\+0\|")
    # every fixed entry and every descriptor entry
    for what in ("md5_fixed", "crc_fixed", "dual_fixed", "md5_desc", "crc_desc", "dual_desc"):
        assert seen(rf"^hash\|{what}\|"), what
    # descriptors: the mapped host arrays, and the device copies
    assert {(h[6], h[7]) for h in hashes} >= {(nm.MOFF + "+0", nm.MLEN + "+0"), (nm.DOFF + "+0", nm.DLEN + "+0")}
    assert seen(rf"^copy\|H2D\|65536\|{re.escape(nm.DOFF)}\+0\|") and seen(rf"^copy\|H2D\|80\|{re.escape(nm.DOFF)}\+65536\|")
    # order: none, order_device on mapped and on copied lengths, stable done and refused, the host plan
    assert {h[8] for h in hashes} == {"NULL", nm.DORD + "+0"}
    assert seen(rf"^order\|device\|{re.escape(nm.MLEN)}\+0\|") and seen(rf"^order\|device\|{re.escape(nm.DLEN)}\+0\|")
    assert seen(r"^order\|stable\|.*\|done$") and seen(r"^order\|stable\|.*\|refused$")
    assert seen(r"^plan_desc\|") and seen(rf"^copy\|H2D\|8\|{re.escape(nm.DORD)}\+0\|{re.escape(nm.HORD)}\+0$")
    # kernel: both answers of each choice
    assert {h[2] for h in hashes if h[1] == "md5_desc"} == {str(sc.XDMA), str(sc.LINES)}
    assert {h[2] for h in hashes if h[1] == "crc_desc"} == {str(sc.CRC_XDMA16), str(sc.CRC_SPLIT)}
    assert {h[2] for h in hashes if h[1] == "dual_desc"} == {str(sc.DUAL_XDMA16), str(sc.DUAL_FEDSPLIT)}
    assert seen(r"^choice\|crc\|6\|128$") and seen(r"^choice\|crc\|3073\|2047$") and seen(r"^choice\|dual\|2\|1023$")
    # digests out: in place and scattered for each record width, D2H alone and beside a scatter
    for what, dsz in (("md5_desc", 16), ("crc_desc", 4), ("dual_desc", 32)):
        outs = {h[9] for h in hashes if h[1] == what}
        assert "O+0" in outs and nm.DIG + "+0" in outs, what
        assert seen(rf"^seg\|{re.escape(nm.DIG)}\+0\|O\+4\|{3 * dsz}$"), what
    assert seen(rf"^seg\|\S+\|{O}\|32784$") and seen(rf"^seg\|\S+\|{O}\|65552$") and seen(rf"^seg\|\S+\|O\+20\|20$")
    assert seen(rf"^copy\|D2H\|\d+\|{re.escape(nm.HDIG)}\+0\|{re.escape(nm.DIG)}\+0$")
