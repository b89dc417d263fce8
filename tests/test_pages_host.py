"""Device-resident page lists (md5hip_digest_pages,
md5_batch_submit_device_pages) with no device.  First the argument rules of
both entries through libmd5hip.so: every refusal comes back before any device
work, and *ticket is zeroed by every refused call.  Then tests/c/pages_check.c,
a stand-alone program that links md5_submit.c, md5_pool.c, md5_stream.c and
nc_digest.c against the fake runtime (tests/c/fake_hip.c), the MD5_CRC32
stand-ins (tests/c/fake_dual.c) and a CPU stand-in for the paged launcher that
counts its launches (tests/c/fake_pages.c), under ASan+UBSan: the three kinds,
the caller's arrays overwritten after the call, slices cut at the chunk bound
and at the page-table bound, the page tables allocated by the first paged call
only (the program wraps hipMalloc and hipHostMalloc to count them and to fail
one), -E2BIG, -ENOMEM and the failure policy.  A second build without
fake_pages.c has no launcher: the entry is -ENOSYS with nothing enqueued.  A
third runs 8 threads of paged, device and host submissions on one batcher
under ThreadSanitizer.  Nothing is preloaded and nothing sanitized is loaded
into Python."""
import ctypes
import errno
import os
import shutil
import subprocess

import numpy as np
import pytest

import gen
from sproxy_amd import _lib

CSRC = os.path.join(gen.REPO, "sproxy_amd", "csrc")
INC = os.path.join(gen.REPO, "include")
EINVAL = -errno.EINVAL
WRAP = ("-Wl,--wrap=hipMalloc", "-Wl,--wrap=hipHostMalloc")


def test_digest_pages_argument_errors_before_device_work():
    L = _lib.lib()
    p = ctypes.c_void_p
    dp = L.md5hip_digest_pages
    assert dp(0, None, None, None, None, 0, 0, None, None) == 0                    # empty: a no-op
    assert dp(2, None, None, None, None, 0, 100, None, None) == 0
    good = (0, p(64), p(64), p(64), None, 5, 16384, p(64), None)

    def with_(**kw):
        names = ("kind", "pages", "first", "lens", "order", "n", "page_bytes", "out", "stream")
        return dp(*[kw.get(k, v) for k, v in zip(names, good)])

    for kind in (-1, 3, 99):
        assert with_(kind=kind) == EINVAL, kind
    for name in ("pages", "first", "lens", "out"):
        assert with_(**{name: None}) == EINVAL, name
    for pb in (0, 64, 100, 16384 + 64, (1 << 30) + 128, 0xFFFFFF80):
        assert with_(page_bytes=pb) == EINVAL, pb
    assert with_(out=p(72)) == EINVAL and with_(kind=2, out=p(72)) == EINVAL        # 16-B records
    assert with_(kind=1, out=p(66)) == EINVAL                                       # 4-B records
    # what is left is the device's to refuse: this machine has none, or the launch is made
    assert with_(kind=1, out=p(68), n=0) == 0


def test_queue_entry_argument_errors_and_ticket_zeroed():
    L = _lib.lib()
    p = ctypes.c_void_p
    h, a = p(16), p(64)                    # never dereferenced: every call below is refused before that
    t = ctypes.c_uint64()
    tp = ctypes.byref(t)
    fn = L.md5_batch_submit_device_pages

    def refused(*args):
        t.value = 77
        rc = fn(*args)
        assert t.value == 0, "ticket left"
        return rc

    pages = np.full(8, 4096, dtype=np.uint64)
    first = np.array([0, 2, 4], dtype=np.uint64)
    lens = np.array([256, 129], dtype=np.uint32)
    P, F, Ln = pages.ctypes.data, first.ctypes.data, lens.ctypes.data
    assert refused(None, P, F, Ln, 2, 128, a, 0, None, 0, tp) == EINVAL            # NULL handle
    assert refused(h, None, None, None, 0, 0, None, 0, None, 0, tp) == 0           # empty: no handle is touched
    assert refused(h, None, F, Ln, 2, 128, a, 0, None, 0, tp) == EINVAL
    assert refused(h, P, None, Ln, 2, 128, a, 0, None, 0, tp) == EINVAL
    assert refused(h, P, F, None, 2, 128, a, 0, None, 0, tp) == EINVAL
    assert refused(h, P, F, Ln, 2, 128, None, 0, None, 0, tp) == EINVAL            # no digests
    for pb in (0, 64, 192, (1 << 30) + 128):
        assert refused(h, P, F, Ln, 2, pb, a, 0, None, 0, tp) == EINVAL, pb
    down = np.array([0, 4, 2], dtype=np.uint64)
    assert refused(h, P, down.ctypes.data, Ln, 2, 128, a, 0, None, 0, tp) == EINVAL   # page_first decreases
    short = np.array([0, 1, 3], dtype=np.uint64)
    assert refused(h, P, short.ctypes.data, Ln, 2, 128, a, 0, None, 0, tp) == EINVAL  # 256 B in one 128-B entry
    pages[2] = 0
    assert refused(h, pages.ctypes.data, F, Ln, 2, 128, a, 0, None, 0, tp) == EINVAL  # a NULL page that is read
    assert fn(h, P, F, Ln, 2, 0, a, 0, None, 0, None) == EINVAL                     # synchronous form


def _build(name, san, extra_srcs, defines):
    if not shutil.which("gcc") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers absent")
    srcs = [os.path.join(gen.REPO, "tests", "c", s) for s in ("pages_check.c", "fake_hip.c", "fake_dual.c", *extra_srcs)] + \
           [os.path.join(CSRC, s) for s in ("md5_submit.c", "md5_pool.c", "md5_stream.c", "nc_digest.c")]
    exe = os.path.join(gen.REPO, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", f"-fsanitize={san}",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", INC,
           *defines, *srcs, "-lpthread", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    return exe


def _run(exe, args, env_extra):
    out = subprocess.run([exe, *args], capture_output=True, text=True, env=dict(os.environ, **env_extra), timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("pages ok")
    return out.stdout


ASAN = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1"}


def test_pages_through_the_queue_under_asan():
    out = _run(_build("pages_check_asan", "address,undefined", ("fake_pages.c",), WRAP), (), ASAN)
    assert "kinds: MD5, CRC-32, MD5_CRC32; synchronous, by ticket, device digests; the caller's arrays overwritten" in out
    assert "slices: 200 chunks of 64 per slot in 4 launches, 90,000 entries of 65,536 per slot in 2; order only when needed; -E2BIG" in out
    assert "buffers: two allocations by the first paged call, none otherwise; refusals: -EINVAL, -ENOMEM before anything is enqueued" in out
    assert "failures: failed launch -EIO, injected fault -EIO then -ENODEV, nothing delivered" in out


def test_refused_without_the_launcher_under_asan():
    out = _run(_build("pages_check_nosys_asan", "address,undefined", (), ("-DNO_PAGES", *WRAP)), (), ASAN)
    assert "refusals: without the paged launcher the entry is -ENOSYS, nothing enqueued, the old entries work" in out


def test_threads_under_tsan():
    out = _run(_build("pages_check_tsan", "thread", ("fake_pages.c",), WRAP), ("threads",),
               {"TSAN_OPTIONS": "halt_on_error=1"})
    assert "threads: 8 threads x 60 rounds of paged / device / host submissions on one batcher" in out
