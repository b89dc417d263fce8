"""The small-batch path of the MD5 + CRC-32 kind with no device: where
md5crc32hip_plan draws the line (256 CUs when no device is visible), the
argument rules of the two entries that name the kernel (errors come back
before any device work), and the batcher against a stand-in that has the
plain launchers only (tests/c/fake_dual.c): its weak references to the new
entries are then null and it calls the plain ones, so tests/c/dual_check.c
passes as it is."""
import ctypes
import errno
import os
import re
import subprocess

import gen
import test_dual_host as host
from sproxy_amd import _lib
from sproxy_amd import md5 as m

EINVAL = -errno.EINVAL


def test_plan_boundary():
    MIN = m.MD5CRC32_FEDSPLIT_MIN_LEN
    assert m.md5crc32_plan(64, 16384) == "fedsplit"
    assert m.md5crc32_plan(16384, 16384) == "fedsplit"        # one 64-chunk group per CU
    assert m.md5crc32_plan(16385, 16384) == "xdma16"
    assert m.md5crc32_plan(1000, MIN) == "fedsplit"
    assert m.md5crc32_plan(1000, MIN - 1) == "xdma16"
    assert m.md5crc32_plan(0, 16384) == "xdma16"
    assert m.md5crc32_plan(1, MIN) == "fedsplit"
    # many short chunks are bound by the CRC role: at most CUs x len / 256 chunks
    assert m.md5crc32_plan(2048, 2048) == "fedsplit" and m.md5crc32_plan(2049, 2048) == "xdma16"
    assert m.md5crc32_plan(8192, 8192) == "fedsplit" and m.md5crc32_plan(8193, 8192) == "xdma16"
    assert m.md5crc32_plan(MIN, MIN) == "fedsplit" and m.md5crc32_plan(MIN + 1, MIN) == "xdma16"
    assert m.MD5CRC32_VARIANTS == {"auto": 0, "xdma16": 1, "fedsplit": 2}


def test_python_constants_mirror_the_header():
    text = open(host.INC + "/md5hip.h").read()
    assert int(re.search(r"#define MD5CRC32HIP_FEDSPLIT_MIN_LEN (\d+)u", text).group(1)) == \
        m.MD5CRC32_FEDSPLIT_MIN_LEN
    for name, v in m.MD5CRC32_VARIANTS.items():
        assert re.search(rf"MD5CRC32HIP_{name.upper()} = {v}\b", text), name
    assert re.search(r"MD5CRC32HIP_NUM_VARIANTS = 3\b", text)
    assert _lib.lib().md5hip_abi_version() == 5


def test_variant_entries_argument_errors_before_device_work():
    L = _lib.lib()
    p = ctypes.c_void_p
    for v in (0, 1, 2):
        assert L.md5crc32hip_fixed_variant(None, 0, 16, 16, None, None, v) == 0            # empty batch: no-op
        assert L.md5crc32hip_fixed_variant(None, 5, 16, 16, p(32), None, v) == EINVAL
        assert L.md5crc32hip_fixed_variant(p(16), 5, 16, 16, None, None, v) == EINVAL
        assert L.md5crc32hip_fixed_variant(p(16), 5, 32, 16, p(32), None, v) == EINVAL      # len > stride
        assert L.md5crc32hip_fixed_variant(p(16), 5, 16, 16, p(8), None, v) == EINVAL       # output off the 16-B grid
        assert L.md5crc32hip_desc_variant(None, None, None, None, 0, None, None, v) == 0
        assert L.md5crc32hip_desc_variant(None, p(16), p(16), None, 3, p(32), None, v) == EINVAL
        assert L.md5crc32hip_desc_variant(p(16), None, p(16), None, 3, p(32), None, v) == EINVAL
        assert L.md5crc32hip_desc_variant(p(16), p(16), None, None, 3, p(32), None, v) == EINVAL
        assert L.md5crc32hip_desc_variant(p(16), p(16), p(16), None, 3, None, None, v) == EINVAL
        assert L.md5crc32hip_desc_variant(p(16), p(16), p(16), None, 3, p(40), None, v) == EINVAL
    for v in (3, -1, 99):                                                                  # 3 = MD5CRC32HIP_NUM_VARIANTS
        assert L.md5crc32hip_fixed_variant(p(16), 5, 16, 16, p(32), None, v) == EINVAL
        assert L.md5crc32hip_desc_variant(p(16), p(16), p(16), None, 3, p(32), None, v) == EINVAL


def test_batcher_without_the_new_launchers():
    """dual_check.c against fake_hip.c + fake_dual.c, which define neither
    md5crc32hip_*_variant nor md5crc32hip_plan: the link succeeds on weak
    references and every MD5_CRC32 launch goes to a plain entry (the program
    counts them through fake_dual_launches)."""
    out = host._build_and_run("dual_small_check_asan", ("fake_dual.c",), ())
    assert "batcher: every submit path, kind switches, interleaved kinds, verify and upgrade ok" in out
    assert "pool: whole and split submissions, verify and upgrade ok" in out
    exe = os.path.join(gen.REPO, "build", "dual_small_check_asan")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True, check=True).stdout.splitlines()
    weak = {ln.split()[-1] for ln in syms if ln.split()[:1] == ["w"]}
    defined = {ln.split()[-1] for ln in syms if len(ln.split()) == 3}
    new = {"md5crc32hip_fixed_variant", "md5crc32hip_desc_variant", "md5crc32hip_plan"}
    assert new <= weak and not new & defined, "the batcher refers to the new entries weakly; the stand-in has none"
    assert {"md5crc32hip_fixed", "md5crc32hip_desc"} <= defined
