"""bench.py --dump-outputs and --full.

On CPU: dump_outputs' file format (float32 / float64, exact), its seeded row
sample of a large array, and a dry run that writes the same digests twice.
On the GPU: one small plain C2 run -- the line carries the headline alone,
--steps is the number of timed steps, and the dumped digests are the MD5 of
the very batch the run hashed (re-generated here, digested by the oracle)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import gen

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _run(args, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, BENCH, *args], capture_output=True, text=True,
                       timeout=timeout, env=env, cwd=REPO)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_dump_small_arrays_whole_and_exact(tmp_path):
    a = argparse.Namespace(dump_outputs=str(tmp_path / "d"))
    dig = np.arange(5 * 16, dtype=np.uint8).reshape(5, 16)
    crc = np.array([0, 1, -1, -(1 << 31)], dtype=np.int32)        # CRC-32 bits in an int32 array
    bench.dump_outputs(a, 0, 1, {"digests": dig, "crc32": crc})
    assert sorted(os.listdir(a.dump_outputs)) == ["crc32.npy", "digests.npy"]
    d = np.load(os.path.join(a.dump_outputs, "digests.npy"))
    assert d.dtype == np.float32 and np.array_equal(d, dig)
    c = np.load(os.path.join(a.dump_outputs, "crc32.npy"))
    assert c.dtype == np.float64 and c.tolist() == [0.0, 1.0, 4294967295.0, 2147483648.0]


def test_dump_samples_large_arrays_the_same_way_every_time(tmp_path):
    n = bench.DUMP_BYTES // 64 + 1000                             # one row over the budget and more
    dig = (np.arange(n * 16, dtype=np.int64) * 2654435761 >> 7).astype(np.uint8).reshape(n, 16)
    got = []
    for k in (0, 1):
        a = argparse.Namespace(dump_outputs=str(tmp_path / f"d{k}"))
        bench.dump_outputs(a, 1, 2, {"digests": dig})
        rows = np.load(os.path.join(a.dump_outputs, "digests_rows_rank1.npy"))
        d = np.load(os.path.join(a.dump_outputs, "digests_rank1.npy"))
        got.append((rows, d))
        files = [os.path.join(a.dump_outputs, f) for f in os.listdir(a.dump_outputs)]
        assert sum(os.path.getsize(f) for f in files) <= 64 * 1000 * 1000
    rows, d = got[0]
    assert np.array_equal(rows, got[1][0]) and np.array_equal(d, got[1][1])
    idx = rows.astype(np.int64)
    assert idx[0] == 0 and idx[-1] == n - 1 and np.all(np.diff(idx) > 0)
    assert idx.size == bench.DUMP_BYTES // 64
    assert d.dtype == np.float32 and np.array_equal(d, dig[idx])


def test_dump_is_off_without_the_option(tmp_path):
    bench.dump_outputs(argparse.Namespace(dump_outputs=None), 0, 1, {"digests": np.zeros((2, 16), np.uint8)})
    assert os.listdir(tmp_path) == []


def test_dry_run_dumps_identical_digests_twice(tmp_path):
    outs = []
    for k in (0, 1):
        d = str(tmp_path / f"run{k}")
        line = _run(["--dry-run", "--steps", "2", "--warmup", "0", "--chunks", "9", "--len", "1000",
                     "--dump-outputs", d])
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        outs.append(np.load(os.path.join(d, "digests.npy")))
    assert outs[0].dtype == np.float32 and outs[0].shape == (9, 16)
    assert np.array_equal(outs[0], outs[1])
    buf = np.random.default_rng(0x5EED0000).integers(0, 256, 9 * 1000, dtype=np.uint8)
    assert np.array_equal(outs[0], gen.oracle_digests_fixed(buf, 9, 1000))


def test_full_is_an_option_and_off_by_default():
    assert bench.parse_args([]).full is False and bench.parse_args([]).dump_outputs is None
    assert bench.parse_args(["--full"]).full is True


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_it_hashed(cuda, tmp_path):
    import torch
    from sproxy_amd import md5 as m
    n, L = 4099, 16384                       # odd count, more than one block
    d = str(tmp_path / "out")
    line = _run(["--gpus", "1", "--steps", "3", "--warmup", "1", "--chunks", str(n), "--dump-outputs", d])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["unit"] == "GiB/s" and line["higher_is_better"] is True and line["dtype"] == "u32"
    # value = bytes of the 3 timed steps / their wall time; ms_per_step the same wall time per step
    gib = n * L / float(1 << 30)
    assert line["value"] == pytest.approx(gib / (line["ms_per_step"] * 1e-3), rel=1e-2)
    # the headline alone: nothing that --full measures or checks
    for key in ("parity", "board", "c3q", "c5", "cpu_baseline", "cpu_baseline_all_cores"):
        assert key not in line, key
    assert line["roofline"]["traffic"] is None and line["full"] is False
    got = np.load(os.path.join(d, "digests.npy"))
    assert got.dtype == np.float32 and got.shape == (n, 16)
    data = torch.empty(n * L, dtype=torch.uint8, device=cuda)
    m.fill_synthetic(data, seed=0x5EED0000)                       # bench.py's rank-0 batch
    torch.cuda.synchronize()
    assert np.array_equal(got, gen.oracle_digests_fixed(data.cpu().numpy(), n, L))
