"""Batched MD5Update over page-list blocks (md5hip_update_ctx_pages) against
the reference md5.c driven call by call on host copies of the same 88-byte
contexts (test_ctx.py's HostRef: oracle/_ref/libmd5_ref.so when present,
byte-exact on all 88 bytes; else the restatement with its narrower
comparison), each chunk's bytes concatenated on the host.  Final digests are
also compared against hashlib.md5 of everything an object was fed.

The batches are test_pages.py's Paged: slots of page_bytes + 128, a slot and a
skew per table entry.  A 64-context group takes the loader route when none of
its contexts that get bytes has a pending partial block, the lane route
otherwise; a page off the 16-B grid is read lane by lane on either."""
import hashlib

import numpy as np
import pytest
import torch

import sproxy_amd.md5 as m
from test_ctx import HostRef
from test_pages import Paged, pages_of

pytestmark = pytest.mark.gpu


class Contexts:
    """n contexts on the device, their host copies under the reference, and
    (for contexts that start at MD5Init) every object's bytes so far."""

    def __init__(self, n, cuda, seed, ctx_h=None):
        self.ref, self.n = HostRef(), n
        if ctx_h is None:
            ctx_h = np.zeros((n, 88), np.uint8)
            ctx_h[:, 24:] = np.random.default_rng(seed).integers(0, 256, (n, 64), dtype=np.uint8)   # stale in[]
            self.ctx = torch.from_numpy(ctx_h).to(cuda)
            m.init_ctx(self.ctx)
            self.ctx_h = self.ctx.cpu().numpy()
            assert np.array_equal(self.ctx_h[:, 24:], ctx_h[:, 24:])          # MD5Init leaves in[] alone
            self.sofar = [b""] * n
        else:
            self.ctx_h, self.ctx, self.sofar = ctx_h.copy(), torch.from_numpy(ctx_h).to(cuda), None

    def pending(self):
        return (self.ctx_h[:, 16:20].copy().view("<u4")[:, 0] >> 3) & 63

    def update(self, b, what=""):
        """One paged update of every context with batch b, every context byte
        against the reference afterwards."""
        assert len(b.chunks) == self.n
        m.update_ctx_pages(self.ctx, b.d_pages, b.d_first, b.d_lens, b.P)
        torch.cuda.synchronize()
        data = np.frombuffer(b"".join(b.chunks) + b"\0", np.uint8)
        offs = np.concatenate([[0], np.cumsum(b.lens.astype(np.int64))])[:-1]
        self.ref.update(self.ctx_h, data, offs, b.lens)
        if self.sofar is not None:
            self.sofar = [s + c for s, c in zip(self.sofar, b.chunks)]
        got = self.ctx.cpu().numpy()
        if not self.ref.same(got, self.ctx_h):
            bad = np.flatnonzero((got != self.ctx_h).any(axis=1))[:8]
            cols = [np.flatnonzero(got[i] != self.ctx_h[i])[:6].tolist() for i in bad]
            pytest.fail(f"{what}: contexts {bad.tolist()} (lens {b.lens[bad].tolist()}) differ at bytes {cols}")

    def final(self):
        got = m.final_ctx(self.ctx).cpu().numpy()
        assert np.array_equal(got, self.ref.final(self.ctx_h))
        if self.sofar is not None:
            want = np.array([np.frombuffer(hashlib.md5(s).digest(), np.uint8) for s in self.sofar])
            assert np.array_equal(got, want)
        assert not self.ctx.any().item()                                      # md5.c:264
        return got


def edge_lengths(P):
    return [0, 1, 55, 56, 63, 64, 65, 127, 128, 129, P - 1, P, P + 1, P + 63, P + 64, P + 65,
            2 * P - 1, 2 * P, 2 * P + 64, 2 * P + 127, 3 * P + 191]


@pytest.mark.parametrize("P", (128, 256, 16384))
def test_edge_lengths_no_pending_bytes(P, cuda):
    """One context per length from MD5Init with random stale in[]: 0 and 1..63
    leave stale bytes in place, P + 1 .. P + 63 take the bytes past the tail
    from the end of the previous page, P and 2P end on a page end."""
    c = Contexts(len(edge_lengths(P)), cuda, 3)
    c.update(Paged(edge_lengths(P), P, 7, cuda))
    c.final()


def residue_lengths(t, cat, P):
    """A length for a context with t pending bytes: 0 append-only, 1 exact
    completion, 2-4 completion and blocks whose stream crosses one, two and
    three page ends, 5 a stream that ends exactly on a page end."""
    t = int(t)
    # the block that straddles the k-th page end starts at k * P - t and ends 64 bytes on
    return [(63 - t) // 2 if t else 31, 64 - t, P - t + 64 + 5 if t else P + 69,
            2 * P - t + 64 + 5 if t else 2 * P + 69, 3 * P - t + 64 + 7 if t else 3 * P + 71, 3 * P][cat]


def test_every_pending_residue(cuda):
    """64 contexts left with t = 0..63 pending bytes by a first update of t
    bytes, then three rounds at P = 128 in which context i takes kind
    (i + round) % 6 of residue_lengths: with t pending, the blocks after the
    completion sit 64 - t bytes into the stream and every second one
    straddles two 128-byte pages."""
    P, n = 128, 64
    c = Contexts(n, cuda, 5)
    c.update(Paged(list(range(n)), P, 11, cuda), "first update")
    assert np.array_equal(c.pending(), np.arange(n))
    seen = set()
    for r in range(3):
        t = c.pending()
        cats = (np.arange(n) + r) % 6
        seen |= {(int(x) != 0, int(k)) for x, k in zip(t, cats)}
        lens = [residue_lengths(t[i], cats[i], P) for i in range(n)]
        c.update(Paged(lens, P, 13 + r, cuda), f"round {r}")
    assert {(True, k) for k in range(6)} <= seen
    c.final()


def test_mixed_routes_in_one_launch(cuda):
    """Group 0: no pending bytes, pages on the line; group 1: the same, pages
    16-B aligned off the line; group 2: one context pending; group 3: no
    pending bytes, one page 4 bytes and one page 1 byte off the 16-B grid;
    group 4 ragged (37 contexts), again on the line.  The first launch leaves
    5 pending bytes in one context of group 2 and writes no other context."""
    P, n = 256, 4 * 64 + 37
    rng = np.random.default_rng(17)
    c = Contexts(n, cuda, 19)
    one = np.zeros(n, dtype=np.int64)
    one[2 * 64 + 9] = 5
    c.update(Paged(one.tolist(), P, 23, cuda), "one context")
    lens = rng.integers(0, 3 * P + 1, n)
    lens[2 * 64 + 9], lens[3 * 64 + 30], lens[3 * 64 + 41] = 2 * P + 70, 3 * P, 2 * P + 33
    first = np.concatenate([[0], np.cumsum([pages_of(int(x), P) for x in lens])])
    skew = np.zeros(int(first[-1]), dtype=np.int64)
    skew[first[64]:first[128]] = rng.choice([16, 48, 80, 112], int(first[128] - first[64]))
    skew[first[3 * 64 + 30] + 2] = 4
    skew[first[3 * 64 + 41] + 1] = 1
    c.update(Paged(lens.tolist(), P, 29, cuda, skew=skew), "mixed groups")
    c.final()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
def test_ragged_last_group(n, cuda):
    """Two rounds of random lengths at P = 128: the first from MD5Init (the
    loader route), the second over what it left pending (the lane route),
    with canaries around the contexts."""
    P, guard = 128, 176
    rng = np.random.default_rng(n)
    c = Contexts(n, cuda, 31 + n)
    buf = torch.full((guard + n * 88 + guard,), 0xA5, dtype=torch.uint8, device=cuda)
    buf[guard:guard + n * 88] = c.ctx.reshape(-1)
    c.ctx = buf[guard:guard + n * 88].view(n, 88)
    for r in range(2):
        c.update(Paged(rng.integers(0, 3 * P + 2, n).tolist(), P, 37 + n + r, cuda), f"round {r}")
    h = buf.cpu().numpy()
    assert (h[:guard] == 0xA5).all() and (h[guard + n * 88:] == 0xA5).all()
    c.final()


def test_scattered_and_shared_pages(cuda):
    """test_pages.py's scattered layout: chunk 0's pages descend and interleave
    with chunk 1's, one page is in chunks 0 and 2, chunk 3 owns spare entries
    that name another chunk's page.  Twice: the second update finds pending
    bytes."""
    P = 256
    lens = [3 * P + 77, 3 * P, P + 5, P + 1, 2 * P]
    owned = [4, 3, 2, 5, 2]
    slot = [9, 7, 5, 3,     8, 6, 4,   5, 10,    12, 11, 0, 0, 0,  2, 1]
    c = Contexts(len(lens), cuda, 41)
    for r in range(2):
        c.update(Paged(lens, P, 43 + r, cuda, owned=owned, slot=slot), f"round {r}")
    c.final()


def test_streaming_objects_against_contiguous_updates(cuda):
    """130 objects arriving in four rounds of one block each, 16 KiB pages,
    four pages a block, the last round ragged: every context byte after every
    round, the digests against hashlib.md5 of each object's bytes and against
    the same rounds through the contiguous update_ctx, the contexts zeroed."""
    P, n = 16384, 130
    ragged = [0, 1, 16383, 16384 + 77, 4 * P, 3 * P + 63, 64, 2 * P, 4 * P - 1, P + 64]
    c = Contexts(n, cuda, 47)
    flat = torch.zeros((n, 88), dtype=torch.uint8, device=cuda)
    m.init_ctx(flat)
    for r in range(4):
        lens = [4 * P] * n if r < 3 else [ragged[i % len(ragged)] for i in range(n)]
        b = Paged(lens, P, 53 + r, cuda)
        c.update(b, f"round {r}")
        data = torch.from_numpy(np.frombuffer(b"".join(b.chunks) + b"\0", np.uint8).copy()).to(cuda)
        offs = np.concatenate([[0], np.cumsum(b.lens.astype(np.int64))])[:-1]
        m.update_ctx(flat, torch.from_numpy(offs + data.data_ptr()).to(cuda), b.d_lens)
        torch.cuda.synchronize()
        assert torch.equal(flat, c.ctx), r
    want = m.final_ctx(flat).cpu().numpy()
    assert np.array_equal(c.final(), want)


def test_bit_count_carry(cuda):
    """Contexts whose bits[0] sits just below 2^32, as test_ctx.py sets them
    up: group 0 with every residue pending (the lane route), group 1 with
    none (the loader route); one update of up to a few KiB each carries into
    bits[1]."""
    P, n = 256, 128
    rng = np.random.default_rng(59)
    ctx_h = rng.integers(0, 256, (n, 88), dtype=np.uint8)
    bits = ctx_h[:, 16:24].view("<u4")
    t = np.where(np.arange(n) < 64, np.arange(n) % 64, 0).astype(np.uint64)
    bits[:, 0] = (np.uint64(0xFFFFFE00) + t * np.uint64(8)).astype(np.uint32)
    bits[:, 1] = rng.integers(0, 1 << 31, n).astype(np.uint32)
    c = Contexts(n, cuda, 0, ctx_h=ctx_h)
    hi = bits[:, 1].copy()
    lens = rng.integers(64, 5000, n)
    c.update(Paged(lens.tolist(), P, 61, cuda))
    assert np.array_equal(c.ctx_h[:, 20:24].copy().view("<u4")[:, 0], hi + 1)  # every context carried
    c.final()


def test_many_workgroups(cuda):
    """64 x 300 contexts at P = 128, lengths below 3P, two rounds (loader, then
    lane route): a lane that took a context of another group would show."""
    P, n = 128, 64 * 300
    rng = np.random.default_rng(67)
    c = Contexts(n, cuda, 71)
    for r in range(2):
        c.update(Paged(rng.integers(0, 3 * P, n).tolist(), P, 73 + r, cuda), f"round {r}")
    c.final()
