"""fastcrc windows over page lists (crc32hip_pages) and verify / upgrade of
paged blocks (md5_batch_verify_device_pages, md5_batch_upgrade_device_pages)
with no device.  First the argument rules of the three entries through
libmd5hip.so: every refusal comes back before any device work, and *ticket is
zeroed by every refused call.  Then tests/c/pages_verify_check.c, a
stand-alone program that links md5_submit.c, md5_pool.c, md5_stream.c and
nc_digest.c against the fake runtime (tests/c/fake_hip.c), the MD5_CRC32
stand-ins (fake_dual.c) and CPU stand-ins for the paged launcher
(fake_pages.c), the compare launcher (fake_compare.c) and the window launcher,
which counts its launches (fake_pages_fast.c), under ASan+UBSan: every kind
with its mismatch counts, slices at the chunk bound and at the table bound,
the buffers allocated once (the program wraps hipMalloc and hipHostMalloc to
count them and to fail one), the refusal order, -ENOMEM and the failure
policy.  A second build without fake_pages_fast.c has no window launcher:
-ENOSYS under a window while the other kinds verify.  A third runs 8 threads
of paged verifies, paged submissions and device verifies on one batcher under
ThreadSanitizer.  Nothing is preloaded and nothing sanitized is loaded into
Python."""
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


def test_crc32_pages_argument_errors_before_device_work():
    L = _lib.lib()
    p = ctypes.c_void_p
    cp = L.crc32hip_pages
    assert cp(None, None, None, None, 0, 0, 0, None, None) == 0                     # empty: a no-op
    assert cp(None, None, None, None, 0, 100, 130, None, None) == 0
    good = (p(64), p(64), p(64), None, 5, 16384, 128, p(64), None)
    names = ("pages", "first", "lens", "order", "n", "page_bytes", "fastcrc", "crcs", "stream")

    def with_(**kw):
        return cp(*[kw.get(k, v) for k, v in zip(names, good)])

    for F in (0, 128):                                                              # both routes refuse alike
        for name in ("pages", "first", "lens", "crcs"):
            assert with_(fastcrc=F, **{name: None}) == EINVAL, (F, name)
        for pb in (0, 64, 100, 16384 + 64, (1 << 30) + 128, 0xFFFFFF80):
            assert with_(fastcrc=F, page_bytes=pb) == EINVAL, (F, pb)
        assert with_(fastcrc=F, crcs=p(66)) == EINVAL                               # 4-B values
    for F in (1, 2, 3, 6, 127, 130, 0xFFFFFFFF):                                    # a multiple of 4, as crc32hip_fixed rules
        assert with_(fastcrc=F) == EINVAL, F


def _refusing(fn, t):
    def refused(*args):
        t.value = 77
        rc = fn(*args)
        assert t.value == 0, "ticket left"
        return rc
    return refused


def test_queue_entries_argument_errors_and_ticket_zeroed():
    L = _lib.lib()
    p = ctypes.c_void_p
    h, a = p(16), p(64)                    # never dereferenced: every call below is refused before that
    t = ctypes.c_uint64()
    tp = ctypes.byref(t)
    nbad = ctypes.c_uint64(5)
    nb = ctypes.byref(nbad)
    pages = np.full(8, 4096, dtype=np.uint64)
    first = np.array([0, 2, 4], dtype=np.uint64)
    lens = np.array([256, 129], dtype=np.uint32)
    P, F, Ln = pages.ctypes.data, first.ctypes.data, lens.ctypes.data
    down = np.array([0, 4, 2], dtype=np.uint64)                                     # page_first decreases
    short = np.array([0, 1, 3], dtype=np.uint64)                                    # 256 B in one 128-B entry
    holed = pages.copy()
    holed[2] = 0                                                                    # a NULL page that is read

    verify = _refusing(L.md5_batch_verify_device_pages, t)

    def v(b=h, pg=P, fi=F, ln=Ln, n=2, pb=128, exp=a, ok=a):
        return verify(b, pg, fi, ln, n, pb, exp, ok, 0, None, 0, nb, tp)

    upgrade = _refusing(L.md5_batch_upgrade_device_pages, t)

    def u(b=h, pg=P, fi=F, ln=Ln, n=2, pb=128, want=a, ok=a, md5=a):
        return upgrade(b, pg, fi, ln, n, pb, want, ok, md5, None, 0, nb, tp)

    for f in (v, u):
        assert f(b=None) == EINVAL                                                  # NULL handle
        nbad.value = 5
        assert f(n=0, pg=None, fi=None, ln=None, pb=0, ok=None) == 0 and nbad.value == 0   # empty: no handle is touched
        for name in ("pg", "fi", "ln", "ok"):
            assert f(**{name: None}) == EINVAL, name
        for pb in (0, 64, 192, (1 << 30) + 128):
            assert f(pb=pb) == EINVAL, pb
        assert f(fi=down.ctypes.data) == EINVAL
        assert f(fi=short.ctypes.data) == EINVAL
        assert f(pg=holed.ctypes.data) == EINVAL
    assert v(exp=None) == EINVAL
    assert u(want=None) == EINVAL and u(md5=None) == EINVAL
    # the synchronous forms
    assert L.md5_batch_verify_device_pages(h, P, F, Ln, 2, 0, a, a, 0, None, 0, None, None) == EINVAL
    assert L.md5_batch_upgrade_device_pages(h, P, F, Ln, 2, 0, a, a, a, None, 0, None, None) == EINVAL


def _build(name, san, extra_srcs, defines):
    if not shutil.which("gcc") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers absent")
    srcs = [os.path.join(gen.REPO, "tests", "c", s)
            for s in ("pages_verify_check.c", "fake_hip.c", "fake_dual.c", "fake_pages.c", "fake_compare.c", *extra_srcs)] + \
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
    assert out.stdout.strip().endswith("pages verify ok")
    return out.stdout


ASAN = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1"}


def test_paged_verify_through_the_queue_under_asan():
    out = _run(_build("pages_verify_check_asan", "address,undefined", ("fake_pages_fast.c",), WRAP), (), ASAN)
    assert "kinds: MD5, CRC-32, CRC-32 window, MD5_CRC32 with 4 mismatches; synchronous, by ticket, host and device forms; upgrade with 2" in out
    assert "slices: 200 blocks of 64 per slot in 4 launches and 4 compares, nbad summed, ok in order; 90,000 entries of 65,536 per slot in 2" in out
    assert "buffers: page tables and verify buffers each allocated once; refusals in order: -EINVAL, -E2BIG, -ENOMEM, nothing enqueued, ticket zeroed" in out
    assert "failures: failed hash launch and failed compare -EIO, injected fault -EIO then -ENODEV, nothing delivered" in out


def test_window_refused_without_its_launcher_under_asan():
    out = _run(_build("pages_verify_check_nosys_asan", "address,undefined", (), ("-DNO_FAST", *WRAP)), (), ASAN)
    assert "refusals: without the window launcher a paged verify under a window is -ENOSYS, after -EINVAL and before -E2BIG; the other kinds verify" in out


def test_threads_under_tsan():
    out = _run(_build("pages_verify_check_tsan", "thread", ("fake_pages_fast.c",), WRAP), ("threads",),
               {"TSAN_OPTIONS": "halt_on_error=1"})
    assert "threads: 8 threads x 60 rounds of paged verifies, paged submissions and device verifies on one batcher" in out
