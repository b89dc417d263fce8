"""Asynchronous verify and upgrade (digests compared on the device) with no
device.  First the argument rules of the new entries through libmd5hip.so:
errors come back before any device work, and *ticket is zeroed by every
refused call.  Then tests/c/verify_check.c, a stand-alone program that links
md5_submit.c, md5_pool.c, md5_stream.c and nc_digest.c against the fake
runtime (tests/c/fake_hip.c), the MD5_CRC32 stand-ins (tests/c/fake_dual.c) and
a CPU stand-in for the compare launcher that counts its launches
(tests/c/fake_compare.c), under ASan+UBSan: every kind, expected values
overwritten after the call, coalescing into one compare launch, no digest
copy-back for verify-only slots, several slots, the pool whole and split,
failed launches.  A second build without fake_compare.c has no launcher: every
new entry is -ENOSYS with nothing enqueued.  A third runs 8 threads of mixed
work on one batcher and one pool under ThreadSanitizer.  Nothing is preloaded
and nothing sanitized is loaded into Python."""
import ctypes
import errno
import os
import shutil
import subprocess

import pytest

import gen
from sproxy_amd import _lib

CSRC = os.path.join(gen.REPO, "sproxy_amd", "csrc")
INC = os.path.join(gen.REPO, "include")
EINVAL = -errno.EINVAL


def test_digest_compare_argument_errors_before_device_work():
    L = _lib.lib()
    p = ctypes.c_void_p
    cmp_ = L.md5hip_digest_compare
    assert cmp_(None, 16, 0, 16, None, 0, None, None, None) == 0                   # empty: a no-op
    assert cmp_(None, 7, 1, 99, None, 0, None, None, None) == 0
    good = (p(64), 16, 0, 16, p(64), 5, p(64), p(64), None)

    def with_(**kw):
        names = ("got", "gsz", "goff", "wsz", "want", "n", "ok", "nbad", "stream")
        return cmp_(*[kw.get(k, v) for k, v in zip(names, good)])

    assert with_(got=None) == EINVAL and with_(want=None) == EINVAL and with_(ok=None) == EINVAL
    for gsz in (0, 8, 12, 20, 64):
        assert with_(gsz=gsz, wsz=4) == EINVAL, gsz
    assert with_(wsz=0) == EINVAL and with_(wsz=6) == EINVAL and with_(wsz=20) == EINVAL
    assert with_(goff=2, wsz=4) == EINVAL                       # goff off the word
    assert with_(goff=16, wsz=4) == EINVAL                      # past a 16-byte record
    assert with_(gsz=32, goff=16, wsz=20) == EINVAL             # goff + wsz > gsz
    assert with_(gsz=4, wsz=4, got=p(66)) == EINVAL             # records aligned to min(gsz, 16)
    assert with_(got=p(72)) == EINVAL and with_(gsz=32, wsz=32, got=p(72)) == EINVAL
    assert with_(nbad=p(12)) == EINVAL                          # the counter is a uint64


def test_entry_argument_errors_and_ticket_zeroed():
    L = _lib.lib()
    p = ctypes.c_void_p
    h, a = p(16), p(64)                    # never dereferenced: every call below is refused before that
    t = ctypes.c_uint64()
    tp = ctypes.byref(t)
    nb = ctypes.c_uint64()
    nbp = ctypes.byref(nb)

    def refused(fn, *args):
        t.value = 77
        rc = fn(*args)
        assert t.value == 0, (fn.__name__, "ticket left")
        return rc

    for fn in (L.md5hip_batch_verify_iov_async, L.md5hip_pool_verify_iov_async):
        assert refused(fn, None, a, a, 1, a, a, nbp, tp) == EINVAL            # NULL handle
        assert refused(fn, h, a, a, 1, None, a, nbp, tp) == EINVAL            # no expected
        assert refused(fn, h, a, a, 1, a, None, nbp, tp) == EINVAL            # no ok
        assert fn(h, a, a, 1, a, a, nbp, None) == EINVAL                      # async form without a ticket
    for fn in (L.md5hip_batch_upgrade_iov_async, L.md5hip_pool_upgrade_iov_async):
        assert refused(fn, None, a, a, 1, a, a, a, nbp, tp) == EINVAL
        assert refused(fn, h, a, a, 1, None, a, a, nbp, tp) == EINVAL         # no want_crc
        assert refused(fn, h, a, a, 1, a, None, a, nbp, tp) == EINVAL         # no ok
        assert refused(fn, h, a, a, 1, a, a, None, nbp, tp) == EINVAL         # no md5_out
        assert fn(h, a, a, 1, a, a, a, nbp, None) == EINVAL
    dv = L.md5_batch_verify_device
    assert refused(dv, None, a, a, 1, a, a, 0, None, 0, nbp, tp) == EINVAL
    assert refused(dv, h, a, a, 1, None, a, 0, None, 0, nbp, tp) == EINVAL
    assert refused(dv, h, a, a, 1, a, None, 1, None, 0, nbp, tp) == EINVAL
    # an empty submission: 0, ticket 0, *nbad zeroed -- no handle is touched
    nb.value = 99
    assert refused(L.md5hip_batch_verify_iov_async, h, None, None, 0, None, None, nbp, tp) == 0 and nb.value == 0
    nb.value = 99
    assert refused(L.md5hip_batch_upgrade_iov_async, h, None, None, 0, None, None, None, nbp, tp) == 0 and nb.value == 0
    nb.value = 99
    assert refused(dv, h, None, None, 0, None, None, 0, None, 0, nbp, tp) == 0 and nb.value == 0
    assert dv(h, None, None, 0, None, None, 0, None, 0, None, None) == 0      # synchronous, no counter


def _build(name, san, extra_srcs, defines):
    if not shutil.which("gcc") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers absent")
    srcs = [os.path.join(gen.REPO, "tests", "c", s) for s in ("verify_check.c", "fake_hip.c", "fake_dual.c", *extra_srcs)] + \
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
    assert out.stdout.strip().endswith("verify ok")
    return out.stdout


ASAN = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1"}


def test_verify_through_batcher_and_pool_under_asan():
    out = _run(_build("verify_check_asan", "address,undefined", ("fake_compare.c",), ()), (), ASAN)
    assert "kinds: MD5, CRC-32 (fastcrc 0, 64), MD5_CRC32, upgrade, device-resident; expected copied; several slots summed" in out
    assert "coalesced: 5 verify + 2 digest tickets in one launch, 1 compare launch; no digest copy for verify-only slots" in out
    assert "pool: whole and split verify and upgrade, mismatches in every part, one nbad" in out
    assert "failures: failed compare launch -EIO, device lost after launch 2 -EIO / -ENODEV, nothing delivered" in out


def test_refused_without_the_launcher_under_asan():
    out = _run(_build("verify_check_nosys_asan", "address,undefined", (), ("-DNO_COMPARE",)), (), ASAN)
    assert "refusals: without the compare launcher every new entry is -ENOSYS, nothing enqueued, the old entries work" in out


def test_threads_under_tsan():
    out = _run(_build("verify_check_tsan", "thread", ("fake_compare.c",), ()), ("threads",),
               {"TSAN_OPTIONS": "halt_on_error=1"})
    assert "threads: 8 threads x 60 rounds of verify / upgrade / submit on one batcher and one pool" in out
