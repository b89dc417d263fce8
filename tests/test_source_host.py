"""The batcher's host chunk sources (sproxy_amd/csrc/md5_source.h, included by
md5_submit.c) on the host under AddressSanitizer + UBSan: PTRS and IOV sources
with 1-byte, empty and unevenly cut segments, empty chunks and first != 0
against a flat copy -- whole chunks, every byte range of a 300-byte chunk, the
staged head || tail form around the fastcrc window, and the threaded gather
cut into 1, 2, 5 and 32 parts (tests/c/source_check.c)."""
import os
import shutil
import subprocess

import pytest

import gen


def test_chunk_sources_under_asan():
    if not shutil.which("gcc"):
        pytest.skip("gcc absent")
    exe = os.path.join(gen.REPO, "build", "source_check_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["gcc", "-O1", "-g", "-std=gnu11", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(gen.REPO, "tests", "c", "source_check.c"), "-o", exe, "-lpthread"],
                   check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0")
    env.pop("MD5HIP_GATHER_THREADS", None)
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr[-2000:]
    assert out.stdout.strip().endswith("source ok")
