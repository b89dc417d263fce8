"""The batch planner with no device: tests/c/plan_check.cc links
sproxy_amd/csrc/md5_plan.cc alone and supplies the planner's one device
entry, md5hip_cu_count(), from a variable, so every case runs at 256 compute
units and the planner cases also at 8 and 304 (the thresholds scale with it).
md5hip_plan_order against a naive stable sort on (len >> 6) + 1 descending:
n = 0, 1, 63, 64, 65, all-equal lengths, lengths that differ only below
bit 6 (ties, in index order), 2^18 - 1, 2^18 and 2^18 + 1 chunks (the first
sizes that split over helper threads) and keys past 2^20 (the comparison
sort).  md5hip_plan_hist against md5hip_plan_desc on the same lengths: the
same variant, bucket starts where each key begins in the order; uniform
batches one chunk under, at and over two groups per CU (LANE / XDMA) and one
group per CU with a longest chunk of one and of two whole blocks (LANE /
FED), HYBRID's 256 KiB edge, a few 8 MiB - 64 B chunks among 48,000 of
16 KiB (once and three times), C3's length classes once (HYBRID at 256 CUs)
and three times (BALANCED), and what kmax = 0, kmax > MD5HIP_HIST_KMAX, an
empty histogram and hist == NULL return.  md5hip_lines_choice at exactly
half and one byte past; md5hip_crc_desc_choice and md5hip_crc_split_fits at
12, 16 and 128 chunks per CU, one under and one over, on both sides of
2,048 bytes and with no length.  A plain executable under ASan + UBSan:
nothing is preloaded and nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

import gen

SRCS = [os.path.join(gen.REPO, "tests", "c", "plan_check.cc"),
        os.path.join(gen.REPO, "sproxy_amd", "csrc", "md5_plan.cc")]


def test_planner_under_asan():
    if not shutil.which("g++"):
        pytest.skip("g++ absent")
    exe = os.path.join(gen.REPO, "build", "plan_check_asan")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-I", os.path.join(gen.REPO, "include"), *SRCS, "-lpthread",
           "-o", exe]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1:verify_asan_link_order=0")
    out = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert out.stdout.strip().startswith("plan ok:")
    assert out.stdout.strip().endswith("checks at 256, 8 and 304 CUs")
