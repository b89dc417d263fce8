"""Update plans that take md5hip_update_ctx down each of its wave-level paths
with pending bytes in the contexts (tests/test_ctx_paths.py).  Pure numpy: test
infrastructure, the product never imports this module.

The entry is two kernels (sproxy_amd/csrc/md5_kernels.h).  md5_update_ctx_fed
runs when ceil(n / 64) <= CUs, the 64-thread md5_update_ctx otherwise.  With
t the context's pending bytes, pos = 64 - t when the update completes the
pending block (else 0) and nblk the whole blocks after it:

  fed kernel   a group runs as a fed pair iff its most blocks bmax >= 2 and no
               lane with nblk > 0 has (ptr + pos) % 16 != 0; otherwise wave 0
               runs the loader body.
  loader body  (desc_xpose_group over LaneSpan{ptr + pos, nblk * 64})
               "lane"         some live lane has (ptr + pos) % 16 != 0 -- lanes
                              with nblk == 0 count here, not in the fed test;
               "nostage"      no lane has two whole blocks;
               "dma_lined"    every lane with a 128-B stage starts on a line;
               "dma_offline"  otherwise.

classify() restates those conditions, model_update() restates what
md5.c:169-214 leaves in bits[] and in[], and build() lays out three rounds of
updates -- one that leaves t pending bytes, two measured ones aligned to the
pending bytes the round before left -- in groups of the kinds below over one
read-only pool."""
import numpy as np

POOL = 1 << 20               # bytes of shared data; contexts' spans may overlap
RAGGED = 37                  # contexts in the last group
LONG_BLOCKS = (257, 1025, 4100)      # past the loader's priority steps at 256, 1,024 and 4,096
LONG_LANES = (3, 17, 30)
MIXED_TOP, MIXED_BMAX = 21, 6
BULK, ZERO, APPEND, EXACT = 0, 1, 2, 3   # a lane's role in one round

# one group of each, in this order, then again ("long_lane" once: `offline` after that)
KINDS = ("mixed", "t0", "residues", "one_off", "lined", "offline", "mixed_odd",
         "small_bmax1", "small_bmax2", "small_bmax3", "small_bmax4", "small_bmax5",
         "small_bmax6", "small_bmax7", "small_bmax8", "long_lane")


def kinds_for(ngroups):
    k = [KINDS[g % len(KINDS)] for g in range(ngroups)]
    return [("offline" if x == "long_lane" and g >= len(KINDS) else x) for g, x in enumerate(k)]


def claim(kind, kernel, rnd):
    """The path a group of `kind` must take in `kernel` in measured round 1 / 2."""
    if kind == "small_bmax1":
        return "nostage"                       # bmax < 2: the fed kernel falls back too
    if kind == "one_off":
        return "lane"
    if kernel == "fed":
        return "fed"
    if kind == "mixed_odd":
        return "lane"
    if kind.startswith("small_bmax"):
        return "dma_lined" if int(kind[10:]) % 2 == 0 else "dma_offline"
    if kind == "long_lane":
        return "dma_lined" if rnd == 1 else "dma_offline"
    return "dma_lined" if kind in ("lined", "t0") else "dma_offline"


# ----------------------------------------------------------------- the kernels' conditions
def spans(t, lens):
    """(append_only, pos, nblk) of every context: md5.c:188-210."""
    t, lens = np.asarray(t, np.int64), np.asarray(lens, np.int64)
    append = (t != 0) & (lens < 64 - t)
    pos = np.where((t != 0) & ~append, 64 - t, 0)
    nblk = np.where(append, 0, (lens - pos) >> 6)
    return append, pos, nblk


def classify(t, ptr, lens, n, cus):
    """(kernel, [path of every 64-context group]) for one md5hip_update_ctx
    call: t = pending bytes, ptr = data addresses, lens = update lengths."""
    g = (n + 63) // 64
    full = g * 64

    def pad(a):                              # dead lanes: length 0, pointer 0
        out = np.zeros(full, np.int64)
        out[:n] = np.asarray(a, np.int64)[:n]
        return out.reshape(g, 64)

    live = (np.arange(full) < n).reshape(g, 64)
    t, ptr, lens = pad(t), pad(ptr), pad(lens)
    _, pos, nblk = spans(t, lens)
    off16 = ((ptr + pos) & 15) != 0
    off128 = ((ptr + pos) & 127) != 0
    nst = nblk >> 1
    kernel = "fed" if g <= cus else "loader"
    paths = []
    for k in range(g):
        if (live[k] & off16[k]).any():
            body = "lane"
        elif nst[k].max() == 0:
            body = "nostage"
        elif (live[k] & (nst[k] != 0) & off128[k]).any():
            body = "dma_offline"
        else:
            body = "dma_lined"
        pair = nblk[k].max() >= 2 and not ((nblk[k] > 0) & off16[k]).any()
        paths.append("fed" if kernel == "fed" and pair else body)
    return kernel, paths


# ----------------------------------------------------------------- md5.c:169-214 on bits[] and in[]
def model_update(ctx, data, offs, lens):
    """A copy of the [n, 88] contexts with bits[] (bytes 16..23) and in[]
    (24..87) as MD5Update(ctx[i], data + offs[i], lens[i]) leaves them; buf[]
    (0..15) is copied through, not modelled.  in[] ends as: the tail bytes in
    front; behind them bytes [r, 64) of the last block compressed -- the
    completed pending block when no whole block followed it, else the last
    whole block of the data; the old bytes where nothing was compressed, and
    past the appended bytes where the update only appended."""
    out = np.array(ctx, dtype=np.uint8, copy=True)
    n = out.shape[0]
    offs = np.asarray(offs, np.int64).reshape(n, 1)
    lens = np.asarray(lens, np.int64).reshape(n, 1)
    bits = out[:, 16:24].copy().view("<u4").astype(np.uint64)
    lo = (bits[:, :1] + ((lens.astype(np.uint64) << np.uint64(3)) & np.uint64(0xFFFFFFFF))) & np.uint64(0xFFFFFFFF)
    hi = (bits[:, 1:] + (lo < bits[:, :1]) + (lens.astype(np.uint64) >> np.uint64(29))) & np.uint64(0xFFFFFFFF)
    out[:, 16:24] = np.concatenate([lo, hi], axis=1).astype("<u4").view(np.uint8)
    t = ((bits[:, :1] >> np.uint64(3)) & np.uint64(63)).astype(np.int64)
    append, pos, nblk = spans(t, lens)
    r = np.where(append, 0, lens - pos - 64 * nblk)
    j = np.arange(64).reshape(1, 64)
    data = np.asarray(data, np.uint8)

    def at(idx):                             # data[idx] where the caller selects it, else anything
        return data[np.clip(idx, 0, data.size - 1)]

    old = out[:, 24:].copy()
    appended = np.where((j >= t) & (j < t + lens), at(offs + j - t), old)
    pending = np.where(j < t, old, at(offs + j - t))            # the completed pending block
    block = at(offs + pos + 64 * (nblk - 1) + j)                # the last whole block
    last = np.where(nblk > 0, block, np.where(pos > 0, pending, old))
    done = np.where(j < r, at(offs + pos + 64 * nblk + j), last)
    out[:, 24:] = np.where(append, appended, done)
    return out


# ----------------------------------------------------------------- the plan
class Plan:
    """n contexts in 64-context groups of `kinds`; rounds[0] leaves t0 pending
    bytes, rounds[1] and [2] are the measured ones.  A round is (offs, lens,
    t_in): int64 [n] pool offsets and lengths, and the pending bytes it meets."""

    def __init__(self, n, kinds, rounds, roles):
        self.n, self.kinds, self.rounds, self.roles = n, kinds, rounds, roles

    def head(self, n):
        """The plan of the first n contexts alone."""
        g = (n + 63) // 64
        return Plan(n, self.kinds[:g], [tuple(a[:n] for a in r) for r in self.rounds],
                    [a[:n] for a in self.roles])


def _group(kind, g, rnd, t_in, rng):
    """(offs, lens, t_out, role) of one group's 64 lanes in measured round `rnd`."""
    lane = np.arange(64)
    role = np.full(64, BULK)
    nblk = rng.integers(2, 10, 64)
    tail = (37 * lane + 11 + 5 * rnd + g) % 64           # every residue in every group
    a = 16 * (lane % 8)                                  # (ptr + pos) % 128: on the 16-B grid
    lined, offline = np.zeros(64, np.int64), 16 * (1 + lane % 7)
    if kind == "t0":
        tail[:] = 0
        a = lined
    elif kind == "lined":
        a = lined
    elif kind == "offline":
        a = offline
    elif kind == "one_off":
        a = a.copy()
        a[(7 + 11 * rnd) % RAGGED] += 4
    elif kind == "long_lane":
        nblk[:] = 2
        nblk[list(LONG_LANES)] = LONG_BLOCKS
        a = lined if rnd == 1 else offline
    elif kind.startswith("small_bmax"):
        b = int(kind[10:])
        nblk = rng.integers(0, b, 64)
        nblk[(5 * b) % RAGGED] = b
        a = lined if b % 2 == 0 else offline
    elif kind in ("mixed", "mixed_odd"):
        nblk = rng.integers(0, MIXED_BMAX, 64)
        nblk[MIXED_TOP] = MIXED_BMAX
        r8 = (lane + rnd) % 8
        role[r8 == 0], role[r8 == 1], role[r8 == 2] = ZERO, APPEND, EXACT
        role[MIXED_TOP] = BULK
        role[(role == APPEND) & ((t_in == 0) | (t_in == 63))] = BULK     # nothing to append to / no room
        role[(role == EXACT) & (t_in == 0)] = BULK                       # 64 bytes would be a whole block
    elif kind != "residues":
        raise ValueError(kind)
    pos = np.where(t_in != 0, 64 - t_in, 0)
    lens = pos + 64 * nblk + tail
    t_out = tail.copy()
    z, ap, ex = role == ZERO, role == APPEND, role == EXACT
    lens[z], t_out[z] = 0, t_in[z]
    lens[ap] = 1 + (rng.random(64) * (63 - t_in)).astype(np.int64)[ap]   # 1 .. 63 - t
    t_out[ap] = (t_in + lens)[ap]
    lens[ex], t_out[ex] = (64 - t_in)[ex], 0
    pos[z | ap] = 0
    if kind == "mixed_odd":                              # lanes without a whole block: off the grid
        a = a + np.where((lens - pos) < 64, 1 + 2 * (lane % 8), 0)
    slot = (rng.random(64) * ((POOL - lens - 256) // 128)).astype(np.int64)
    offs = 128 * slot + (a - pos) % 128
    return offs, lens, t_out, role


def build(n, seed=0xC7C7, kinds=None):
    g = (n + 63) // 64
    kinds = list(kinds_for(g) if kinds is None else kinds)
    assert len(kinds) == g
    lane = np.tile(np.arange(64), g)
    t0 = np.where(np.repeat([k == "t0" for k in kinds], 64), 0, lane)
    rng0 = np.random.default_rng([seed, 0])
    rounds = [(rng0.integers(0, POOL - 256, 64 * g), t0.copy(), np.zeros(64 * g, np.int64))]
    roles = [np.full(64 * g, APPEND)]
    t = t0
    for rnd in (1, 2):
        parts = [_group(kinds[k], k, rnd, t[64 * k:64 * k + 64], np.random.default_rng([seed, rnd, k]))
                 for k in range(g)]
        offs, lens, t_out, role = (np.concatenate(x) for x in zip(*parts))
        rounds.append((offs, lens, t))
        roles.append(role)
        t = t_out
    return Plan(n, kinds, [tuple(a[:n].astype(np.int64) for a in r) for r in rounds], [a[:n] for a in roles])
