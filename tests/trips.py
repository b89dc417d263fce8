"""Descriptor batches that take the persistent per-CU kernels past their first
grid trip (tests/test_grid_trips.py).  Pure numpy: test infrastructure, the
product never imports this module.

A persistent kernel launches one workgroup per CU; wave `w` of workgroup `b`
starts at group `w * cus + b` and steps `cus * waves_per_cu` groups, so group
`g` is hashed on trip `g // (cus * waves_per_cu)` by the wave that hashed
`g - cus * waves_per_cu` the trip before.  A frame is (waves_per_cu,
chunks_per_group): (12, 64) the XDMA16 kernels, (12, 32) crc32_fast_xdma16's
window rows, (16, 32) crc32_fast_pipe, (4, 64) BALANCED (whose waves take
groups from a counter: the same groups, in arrival order).

build() draws one shape per group from a seeded generator, so a wave's
successive groups differ in shape; the last group is ragged."""
import math

import numpy as np

LINE = 128
PAD = 4096                   # bytes after the last chunk (whole-line loaders read on)
LONG_CHUNK = 16384 + 77      # shape A6's one long chunk: 257 blocks, the raised priority
RAGGED = {64: 37, 32: 19}    # chunks in the last group
RESIDUES = (0, 1, 55, 56, 63)

# name -> weight.  Batch A: 64-chunk groups for the MD5, CRC and dual descriptor
# kernels (weights keep a 2.25-trip batch of the 12-wave frame near 160 MB at
# 256 CUs: the ragged and the off-line shapes are the heavy ones).
SHAPES_A = {
    "lined256": 0.22,      # 256 B on 128-B lines: nt loads, two stages
    "offline": 0.14,       # 384-640 B, 16-B-aligned off the line: default cache policy
    "tiny": 0.22,          # every chunk < 128 B, some empty: no stage (smax == 0)
    "skew4": 0.14,         # offline with one start 4 B off the 16-B grid: lane-direct
    "ragged": 0.10,        # 0..1,536 B: rows without a stage, clamped rows, tail residues
    "long1": 0.18,         # short chunks and one of 16 KiB + 77: the priority is raised
}
# Batch B: 32-chunk groups of 144-400 B chunks for the fastcrc windows, F = 64 / 128
SHAPES_B = {
    "simple": 0.60,        # > F, 16-B-aligned, length = 0 mod 16: the pipelined path
    "short": 0.14,         # simple with one chunk <= F and one empty
    "oddlen": 0.13,        # lengths != 0 mod 16: unaligned tail windows, the group falls back
    "pack4": 0.13,         # simple lengths packed on the 4-B grid
}
B_SHORT_MAX = 64           # "short"'s chunk is <= every pipelined window (F = 64, 128)


def ngroups_for(cus, waves_per_cu, trips):
    return math.ceil(trips * waves_per_cu * cus) + 1


def group_shapes(ngroups, shapes, seed):
    """Shape index (into list(shapes)) of every group."""
    w = np.asarray(list(shapes.values()), dtype=np.float64)
    return np.random.default_rng(seed).choice(len(w), size=ngroups, p=w / w.sum())


def _up(x, a):
    return (x + a - 1) // a * a


def build(cus, waves_per_cu, chunks_per_group, trips, shapes, seed):
    """(lens uint32 [n], offs uint64 [n], total): a descriptor batch in chunk
    order (order=None); group g is chunks [g * cpg, (g + 1) * cpg).  `total`
    bytes hold every chunk and PAD bytes more."""
    cpg = chunks_per_group
    G = ngroups_for(cus, waves_per_cu, trips)
    names = list(shapes)
    gs = group_shapes(G, shapes, seed)
    rng = np.random.default_rng([seed, 1])
    shp = (G, cpg)
    lens = np.zeros(shp, dtype=np.int64)
    adv = np.zeros(shp, dtype=np.int64)            # bytes from a chunk's start to the next one's
    nudge = np.zeros(shp, dtype=np.int64)          # added to a chunk's start alone
    skew = np.zeros(G, dtype=np.int64)             # group start past its 128-B line
    special = rng.integers(0, RAGGED[cpg], G)      # a column the ragged last group keeps
    rows = np.arange(G)

    def of(name):
        return gs == names.index(name) if name in names else np.zeros(G, dtype=bool)

    def put(sel, L, a=None):
        lens[sel] = L[sel]
        adv[sel] = _up(L, 16)[sel] if a is None else a[sel]

    # ---- batch A
    put(of("lined256"), np.full(shp, 256))
    off_l = rng.integers(384, 641, shp)
    for name in ("offline", "skew4"):
        put(of(name), off_l)
        skew[of(name)] = 16
    s = of("skew4")
    nudge[rows[s], special[s]] = 4
    tiny = rng.integers(0, 128, shp) * (rng.random(shp) >= 0.15)
    put(of("tiny"), tiny)
    rag = rng.integers(0, 1537, shp)
    rag[:, :5] = 64 * rng.integers(0, 24, (G, 5)) + np.asarray(RESIDUES)
    rag[:, 5] = rng.integers(0, 128, G)            # a row without any stage
    put(of("ragged"), rag)
    lng = rng.integers(0, 256, shp)
    lng[rows, special] = LONG_CHUNK
    put(of("long1"), lng)
    # ---- batch B
    simple = 16 * rng.integers(9, 26, shp)         # 144..400, = 0 mod 16
    put(of("simple"), simple)
    sh = simple.copy()
    sh[rows, special] = rng.integers(1, B_SHORT_MAX + 1, G)
    sh[rows, (special + 1) % RAGGED[cpg]] = 0
    put(of("short"), sh)
    put(of("oddlen"), simple + rng.integers(1, 16, shp))
    p4 = of("pack4")
    put(p4, simple, simple + 4 * rng.integers(1, 4, shp))
    skew[p4] = 4

    inside = np.cumsum(adv, axis=1) - adv
    gsize = _up(adv.sum(axis=1) + skew, LINE) + LINE
    gstart = np.cumsum(gsize) - gsize
    offs = gstart[:, None] + skew[:, None] + inside + nudge
    n = (G - 1) * cpg + RAGGED[cpg]
    total = int(gstart[-1] + gsize[-1]) + PAD
    return (lens.reshape(-1)[:n].astype(np.uint32), offs.reshape(-1)[:n].astype(np.uint64), total)


def trip_of(g, cus, waves_per_cu):
    """Trip index on which a wave of a full grid hashes group g."""
    return g // (cus * waves_per_cu)


def shape_pairs(gs, cus, waves_per_cu):
    """The set of (shape, next shape) over consecutive trips of every wave."""
    step = cus * waves_per_cu
    return set(zip(gs[:-step].tolist(), gs[step:].tolist()))
