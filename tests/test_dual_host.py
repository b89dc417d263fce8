"""The MD5_CRC32 digest kind with no device.  First the argument rules of the
new entries through libmd5hip.so (errors come back before any device work).
Then tests/c/dual_check.c, a stand-alone program that links md5_submit.c,
md5_pool.c, md5_stream.c and nc_digest.c against the fake runtime
(tests/c/fake_hip.c) and CPU stand-ins for the two launchers
(tests/c/fake_dual.c), under ASan+UBSan: every submit path of a batcher and a
pool under the kind, kind switches, interleaved kinds, verify_iov, upgrade_iov,
a failed launch and a device lost after launch K.  A second build without
fake_dual.c has no launchers: the kind must be refused with -ENOSYS before
anything is enqueued."""
import ctypes
import errno
import os
import shutil
import subprocess

import pytest

import gen
from sproxy_amd import _lib
from sproxy_amd import md5 as m

CSRC = os.path.join(gen.REPO, "sproxy_amd", "csrc")
INC = os.path.join(gen.REPO, "include")
EINVAL, ENOSYS = -errno.EINVAL, -errno.ENOSYS


def test_entry_argument_errors_before_device_work():
    L = _lib.lib()
    p = ctypes.c_void_p
    assert L.md5crc32hip_fixed(None, 0, 16, 16, None, None) == 0                   # empty batch: no-op
    assert L.md5crc32hip_fixed(None, 5, 16, 16, p(32), None) == EINVAL
    assert L.md5crc32hip_fixed(p(16), 5, 16, 16, None, None) == EINVAL
    assert L.md5crc32hip_fixed(p(16), 5, 32, 16, p(32), None) == EINVAL             # len > stride
    assert L.md5crc32hip_fixed(p(16), 5, 16, 16, p(8), None) == EINVAL              # output off the 16-B grid
    assert L.md5crc32hip_desc(None, None, None, None, 0, None, None) == 0
    assert L.md5crc32hip_desc(None, p(16), p(16), None, 3, p(32), None) == EINVAL
    assert L.md5crc32hip_desc(p(16), None, p(16), None, 3, p(32), None) == EINVAL
    assert L.md5crc32hip_desc(p(16), p(16), None, None, 3, p(32), None) == EINVAL
    assert L.md5crc32hip_desc(p(16), p(16), p(16), None, 3, None, None) == EINVAL
    assert L.md5crc32hip_desc(p(16), p(16), p(16), None, 3, p(40), None) == EINVAL
    # the kind: no fastcrc window, no kind 3; NULL handles
    assert L.md5hip_batcher_set_digest(p(16), 2, 4) == EINVAL
    assert L.md5hip_batcher_set_digest(p(16), 3, 0) == EINVAL
    assert L.md5hip_batcher_set_digest(None, 2, 0) == EINVAL
    assert L.md5hip_pool_set_digest(p(16), 2, 4) == EINVAL
    assert L.md5hip_pool_set_digest(p(16), 3, 0) == EINVAL
    assert L.md5hip_pool_set_digest(None, 2, 0) == EINVAL
    assert L.md5hip_batch_upgrade_iov(None, None, None, 1, None, None, None) == EINVAL
    assert L.md5hip_pool_upgrade_iov(None, None, None, 1, None, None, None) == EINVAL


def test_record_layout_and_split_records():
    import numpy as np
    src = r'''
    #include <stddef.h>
    #include "md5hip.h"
    _Static_assert(sizeof(struct md5hip_md5crc32) == 32, "size");
    _Static_assert(offsetof(struct md5hip_md5crc32, crc) == 16, "crc");
    _Static_assert(offsetof(struct md5hip_md5crc32, zero) == 20, "zero");
    _Static_assert(MD5HIP_DIGEST_MD5_CRC32 == 2, "kind");
    int main(void) { return 0; }
    '''
    exe = os.path.join(gen.REPO, "build", "dual_hdrcheck")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-x", "c", "-", "-o", exe],
                   input=src, text=True, check=True)
    assert subprocess.run([exe]).returncode == 0
    rec = np.zeros((3, 32), dtype=np.uint8)
    rec[:, :16] = np.arange(48, dtype=np.uint8).reshape(3, 16)
    rec[1, 16:20] = [0x78, 0x56, 0x34, 0x12]
    md5, crc = m.split_records(rec)
    assert md5.shape == (3, 16) and md5.dtype == np.uint8 and np.array_equal(md5, rec[:, :16])
    assert crc.dtype == np.uint32 and crc.tolist() == [0, 0x12345678, 0]
    assert m.Batcher.MD5_CRC32 == 2


def _build_and_run(name, extra_srcs, defines):
    if not shutil.which("gcc") or not os.path.exists("/opt/rocm/include/hip/hip_runtime_api.h"):
        pytest.skip("gcc or the HIP headers absent")
    srcs = [os.path.join(gen.REPO, "tests", "c", s) for s in ("dual_check.c", "fake_hip.c", *extra_srcs)] + \
           [os.path.join(CSRC, s) for s in ("md5_submit.c", "md5_pool.c", "md5_stream.c", "nc_digest.c")]
    exe = os.path.join(gen.REPO, "build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", INC,
           *defines, *srcs, "-lpthread", "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.strip().endswith("dual ok")
    return out.stdout


def test_kind_through_batcher_and_pool_under_asan():
    out = _build_and_run("dual_check_asan", ("fake_dual.c",), ())
    assert "batcher: every submit path, kind switches, interleaved kinds, verify and upgrade ok" in out
    assert "staging: host_fixed stages the same bytes under the kind as under MD5" in out
    assert "pool: whole and split submissions, verify and upgrade ok" in out
    assert "failures: failed launch -EIO, device lost after launch 2 -EIO / -ENODEV, no record written" in out


def test_kind_refused_without_launchers_under_asan():
    out = _build_and_run("dual_check_nosys_asan", (), ("-DNO_DUAL",))
    assert "refusals: MD5_CRC32 without its launchers is -ENOSYS, nothing enqueued" in out
