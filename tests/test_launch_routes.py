"""Which kernel a call runs, and with what geometry: the launchers of
sproxy_amd/csrc/md5_kernels.hip and md5_pages.hip with no device.
tests/c/launch_check.cc links the product's own build/obj/md5_kernels.o,
md5_pages.o and md5_plan.o with a recording
stand-in for the HIP runtime (tests/c/fake_hip_rt.cc) into a plain executable
under ASan + UBSan -- nothing is preloaded, nothing is loaded into Python --
and prints, for each case of tests/launch_cases.py, the return code and every
launch: kernel, grid, block, dynamic LDS, stream and argument bytes, with
BALANCED's attribute call and memsets in order.  The table is run at 8, 256
and 304 compute units, and its expectations are written from md5hip.h, never
taken from the library.

The same test reads the two gfx950 code objects' metadata notes (no disassembly)
and holds the launches against them: no scratch and no VGPR spill in any
kernel, every block within the kernel's limit and exactly the size its
indexing is written for, LDS within a CU's 160 KiB, and the workgroups per CU
and waves per SIMD that the kernels' comments claim.  Register and SGPR-spill
counts are compared with tests/golden/kernel_resources.json only under the
compiler that wrote it.

Skipped only where hipcc or g++ is absent."""
import os
import re
import shutil
import subprocess

import pytest

import gen
import kernel_resources
import launch_cases as lc

CUS = [8, 256, 304]
EXE = os.path.join(gen.REPO, "build", "c", "launch_check")
HIPCC = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(HIPCC) or not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("hipcc, g++ or make absent")
    # remakes build/obj/md5_kernels.o through the product Makefile when it is missing or stale
    out = subprocess.run(["make", "-C", os.path.join(gen.REPO, "tests", "c"), "launch_check"],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return EXE


def run_cases(exe, cases, cus):
    """{id: (rc, [records])} of one harness process.  A case without a device
    name gets a number of its own, so nothing cached reaches it."""
    named, lines = {}, []
    for k, c in enumerate(cases):
        dev = named.setdefault(c.device, k) if c.device else k
        lines.append(c.line(dev, cus))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-1000:] + out.stderr[-3000:]
    got, cur = {}, None
    for line in out.stdout.splitlines():
        m = re.fullmatch(r"case (\S+) rc (-?\d+)", line)
        if m:
            cur = got[m.group(1)] = (int(m.group(2)), [])
        elif line != "end":
            # BALANCED's counter is whatever the stand-in's hipMalloc returned
            cur[1].append(re.sub(r"0x7f00[0-9a-f]{8}\b", lc.CTR, line))
    return got


@pytest.fixture(scope="module")
def observed(harness):
    return {cus: run_cases(harness, lc.cases(cus), cus) for cus in CUS}


@pytest.mark.parametrize("cus", CUS)
def test_every_case_launches_what_the_header_says(observed, cus):
    cases, got = lc.cases(cus), observed[cus]
    assert sorted(got) == sorted(c.id for c in cases)
    bad = []
    for c in cases:
        rc, records = got[c.id]
        if rc != c.rc or records != c.records:
            bad.append(f"{c.id} at {cus} CUs: {c.entry}({', '.join(hex(a) for a in c.args)})\n"
                       f"  want rc {c.rc}: " + "\n             ".join(c.records or ["(nothing)"]) + "\n"
                       f"  got  rc {rc}: " + "\n             ".join(records or ["(nothing)"]))
    assert not bad, f"{len(bad)} of {len(cases)} cases:\n" + "\n".join(bad)


def _launches(observed):
    """(kernel, block, dynamic LDS) of every launch any case made"""
    out = set()
    for got in observed.values():
        for rc, records in got.values():
            for r in records:
                f = r.split("|")
                if f[0] == "launch":
                    gx, gy, gz = (int(x) for x in f[2].split(","))
                    bx, by, bz = (int(x) for x in f[3].split(","))
                    assert gx >= 1 and (gy, gz, by, bz) == (1, 1, 1, 1), r
                    out.add((f[1], bx, int(f[4])))
    return out


@pytest.fixture(scope="module")
def resources(harness):
    table = kernel_resources.read(kernel_resources.kernel_names(harness))
    return {k: v for k, v in table.items() if kernel_resources.ours(k)}


def test_the_table_reaches_every_kernel(observed, resources):
    launched = {k for k, _, _ in _launches(observed)}
    assert launched == set(resources), (sorted(set(resources) - launched), sorted(launched - set(resources)))


def test_no_kernel_uses_scratch(resources):
    assert len(resources) >= 34
    for k, r in resources.items():
        assert r["private_segment_fixed_size"] == 0, f"{k}: {r['private_segment_fixed_size']} B of scratch per lane"
        assert r["vgpr_spill_count"] == 0, f"{k}: {r['vgpr_spill_count']} VGPRs spilled"


def test_blocks_and_lds_fit_the_kernels(observed, resources):
    seen = set()
    for k, block, dyn in _launches(observed):
        r = resources[k]
        assert block <= r["max_flat_workgroup_size"], f"{k}: block {block} past its launch bound"
        assert r["group_segment_fixed_size"] + dyn <= lc.LDS_PER_CU, f"{k}: {r['group_segment_fixed_size']} + {dyn} B of LDS"
        if k in lc.EXACT_BLOCK:
            assert block == lc.EXACT_BLOCK[k], f"{k}: block {block}, written for {lc.EXACT_BLOCK[k]}"
            seen.add(k)
    assert seen == set(lc.EXACT_BLOCK), sorted(set(lc.EXACT_BLOCK) - seen)


@pytest.mark.parametrize("kernel,want,comment", lc.WORKGROUPS_PER_CU, ids=[r[0].removeprefix("md5hip::") for r in lc.WORKGROUPS_PER_CU])
def test_workgroups_per_cu_by_lds(observed, resources, kernel, want, comment):
    dyns = {dyn for k, _, dyn in _launches(observed) if k == kernel}
    assert dyns, f"{kernel} never launched"
    for dyn in dyns:
        lds = resources[kernel]["group_segment_fixed_size"] + dyn
        assert lc.LDS_PER_CU // lds == want, f"{kernel}: {lds} B of LDS are {lc.LDS_PER_CU // lds} per CU; {comment}"


@pytest.mark.parametrize("kernel,how,want,comment", lc.WAVES_PER_SIMD, ids=[r[0].removeprefix("md5hip::") for r in lc.WAVES_PER_SIMD])
def test_waves_per_simd_by_registers(resources, kernel, how, want, comment):
    r = resources[kernel]
    got = lc.waves_per_simd(r["vgpr_count"], r["agpr_count"])
    ok = got == want if how == "eq" else got >= want
    assert ok, f"{kernel}: {r['vgpr_count']} VGPRs + {r['agpr_count']} AGPRs are {got} waves per SIMD; {comment}"


def test_fedsplit_has_no_agprs(resources):
    """md5crc32_fedsplit's comment: '163 VGPRs ... and no AGPRs'"""
    for k in ("md5hip::md5crc32_fedsplit<true>", "md5hip::md5crc32_fedsplit<false>"):
        assert resources[k]["agpr_count"] == 0 and resources[k]["vgpr_count"] <= 168, resources[k]


def test_registers_no_higher_than_recorded(resources, capsys):
    gold = kernel_resources.golden()
    assert set(gold["kernels"]) == set(resources), "tests/golden/kernel_resources.json: python tests/kernel_resources.py --write"
    here = kernel_resources.compiler_version()
    if here != gold["compiler"]:
        with capsys.disabled():
            print(f"\nregister counts not compared: compiled by {here!r}, recorded under {gold['compiler']!r}")
        return
    for k, g in gold["kernels"].items():
        for f in ("vgpr_count", "sgpr_spill_count"):
            assert resources[k][f] <= g[f], f"{k}: {f} {resources[k][f]}, recorded {g[f]}"
