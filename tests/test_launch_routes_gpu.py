"""Every route of the launchers, run: each case of tests/launch_cases.py that
launches a hash kernel is called on the device with the same count, length,
stride, skew, window and variant, at the device's own CU count, and its
results are compared bit for bit with hashlib.md5 and zlib.crc32 of the host
copy.  tests/test_launch_routes.py proves on the CPU that the case reaches
the kernel and geometry the table names; this proves the route right at its
edge.  Cases whose grid is 2^31 - 1 workgroups are the table's only hash
launches left out: no device holds their chunks.

One xorshift buffer serves every case; a reference is computed once per
(skew, length, stride) and grown as a case needs more chunks.  Every output
is a 0xAA canary with a guard record behind the last one.  Descriptor cases
pack lengths from 0 to the case's length at 16 B, so a wave holds chunks
with and without whole blocks and, with a window, chunks on both sides of
it."""
import ctypes
import hashlib
import zlib

import numpy as np
import pytest
import torch

import gen
import launch_cases as lc
from sproxy_amd import _lib

pytestmark = pytest.mark.gpu

IDS = [c.id for c in lc.cases(256) if c.shape]     # the same ids at every CU count
SEED = 0x10A7E5


def _desc_lens(n, top):
    """n lengths in [0, top]: every fourth `top`, chunk 1 empty, the rest spread"""
    i = np.arange(n, dtype=np.uint64)
    lens = (i * np.uint64(2654435761) >> np.uint64(7)) % np.uint64(top + 1)
    lens[::4] = top
    if n > 1:
        lens[1] = 0
    return lens.astype(np.uint32)


def _desc_layout(shape):
    lens = _desc_lens(shape["n"], shape["len"])
    offs = np.zeros(len(lens), dtype=np.uint64)
    np.cumsum((lens[:-1].astype(np.uint64) + np.uint64(15)) // np.uint64(16) * np.uint64(16), out=offs[1:])
    return offs, lens


def _bytes_needed(shape):
    if "stride" in shape:
        return shape["skew"] + (shape["n"] - 1) * shape["stride"] + shape["len"]
    if shape["kind"] == "update_ctx":
        return shape["n"] * ((shape["len"] + 15) // 16 * 16)
    offs, lens = _desc_layout(shape)
    return int(offs[-1]) + int(lens[-1])


class World:
    """The device's table, the shared buffer and the references."""

    def __init__(self, cuda):
        self.cuda = cuda
        self.cus = torch.cuda.get_device_properties(0).multi_processor_count
        self.cases = {c.id: c for c in lc.cases(self.cus)}
        assert sorted(c.id for c in self.cases.values() if c.shape) == sorted(IDS)
        nbytes = max(_bytes_needed(c.shape) for c in self.cases.values() if c.shape) + 4096
        self.host = gen.xorshift_array(nbytes, seed=SEED)
        self.dev = torch.from_numpy(self.host).to(cuda)
        self.lib = _lib.lib()
        self.stream = torch.cuda.current_stream().cuda_stream
        self._md5, self._crc = {}, {}

    def _grow(self, memo, key, offs, lens, one, dtype, width):
        have = memo.get(key)
        k = 0 if have is None else len(have)
        if k < len(offs):
            more = np.empty((len(offs) - k,) + width, dtype=dtype)
            for j in range(k, len(offs)):
                o, L = int(offs[j]), int(lens[j])
                more[j - k] = one(self.host[o:o + L])
            have = memo[key] = more if have is None else np.concatenate([have, more])
        return have[:len(offs)]

    def md5(self, key, offs, lens):
        return self._grow(self._md5, key, offs, lens,
                          lambda b: np.frombuffer(hashlib.md5(b).digest(), dtype=np.uint8), np.uint8, (16,))

    def crc(self, key, offs, lens, fastcrc=0):
        def one(b):
            if fastcrc == 0 or len(b) <= fastcrc:           # md5hip.h: 'fastcrc == 0 || len_i <= fastcrc'
                return zlib.crc32(b)
            return zlib.crc32(b[:fastcrc]) ^ zlib.crc32(b[len(b) - fastcrc:])
        return self._grow(self._crc, key + (fastcrc,), offs, lens, one, np.uint32, ())

    def canary(self, n, width):
        return torch.full((n + 1, width), 0xAA, dtype=torch.uint8, device=self.cuda)

    def arrays(self, offs, lens, with_order):
        o = torch.from_numpy(offs.astype(np.int64)).to(self.cuda)
        ln = torch.from_numpy(lens.astype(np.int32)).to(self.cuda)
        od = None
        if with_order:
            order = np.empty(len(lens), dtype=np.uint32)
            assert self.lib.md5hip_plan_order(lens.ctypes.data, len(lens), order.ctypes.data) == 0
            od = torch.from_numpy(order.astype(np.int32)).to(self.cuda)
        return o, ln, od


@pytest.fixture(scope="module")
def world(cuda):
    return World(cuda)


def _check_md5(got, want, what):
    bad = np.flatnonzero((got != want).any(axis=1))
    assert bad.size == 0, f"{what}: md5 of chunks {bad[:8].tolist()} ({bad.size} of {len(want)})"


def _check_crc(got_bytes, want, what):
    got = np.ascontiguousarray(got_bytes).view("<u4").reshape(-1)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: crc of chunks {bad[:8].tolist()} ({bad.size} of {len(want)})"


def _finish(out, n, what):
    torch.cuda.synchronize()
    a = out.cpu().numpy()
    assert (a[n] == 0xAA).all(), f"{what}: wrote past record n - 1"
    return a[:n]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


@pytest.mark.parametrize("id", IDS)
def test_route(world, id):
    w, c = world, world.cases[id]
    s, n = c.shape, c.shape["n"]
    what = f"{id} ({c.kernel}, {w.cus} CUs)"
    variant = [] if s.get("variant") is None else [s["variant"]]
    fn = getattr(w.lib, c.entry)
    if "stride" in s:                                        # fixed length: chunk i at skew + i * stride
        offs = s["skew"] + np.arange(n, dtype=np.uint64) * np.uint64(s["stride"])
        lens = np.full(n, s["len"], dtype=np.uint32)
        key = (s["skew"], s["len"], s["stride"])
        base = ctypes.c_void_p(w.dev.data_ptr() + s["skew"])
        head = [base, n, s["len"], s["stride"]]
    elif s["kind"] != "update_ctx":                          # descriptors
        offs, lens = _desc_layout(s)
        key = ("desc", s["len"])           # the layout of n chunks is a prefix of a longer one
        o, ln, od = w.arrays(offs, lens, s["order"])
        head = [_ptr(w.dev), _ptr(o), _ptr(ln), _ptr(od), n]

    if s["kind"] in ("md5_fixed", "md5_desc"):
        out = w.canary(n, 16)
        assert fn(*head, _ptr(out), w.stream, *variant) == 0, what
        _check_md5(_finish(out, n, what), w.md5(key, offs, lens), what)
    elif s["kind"] in ("crc_fixed", "crc_desc"):
        out = w.canary(n, 4)
        assert fn(*head, s["fastcrc"], _ptr(out), w.stream, *variant) == 0, what
        _check_crc(_finish(out, n, what), w.crc(key, offs, lens, s["fastcrc"]), what)
    elif s["kind"] in ("dual_fixed", "dual_desc"):
        out = w.canary(n, 32)
        assert fn(*head, _ptr(out), w.stream, *variant) == 0, what
        r = _finish(out, n, what)
        _check_md5(r[:, :16], w.md5(key, offs, lens), what)
        _check_crc(r[:, 16:20], w.crc(key, offs, lens), what)
        assert not r[:, 20:].any(), f"{what}: bytes 20..31 of a record not zero"
    else:                                                    # MD5Init, one MD5Update, MD5Final on n contexts
        stride = (s["len"] + 15) // 16 * 16
        offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        lens = np.full(n, s["len"], dtype=np.uint32)
        ctxs = w.canary(n, 88)
        ptrs = torch.from_numpy((offs + np.uint64(w.dev.data_ptr())).astype(np.int64)).to(w.cuda)
        ln = torch.from_numpy(lens.astype(np.int32)).to(w.cuda)
        out = w.canary(n, 16)
        assert w.lib.md5hip_init_ctx(_ptr(ctxs), n, w.stream) == 0, what
        assert fn(_ptr(ctxs), _ptr(ptrs), _ptr(ln), n, w.stream) == 0, what
        assert w.lib.md5hip_final_ctx(_ptr(ctxs), n, _ptr(out), w.stream) == 0, what
        _check_md5(_finish(out, n, what), w.md5((0, s["len"], stride), offs, lens), what)
        assert (ctxs.cpu().numpy()[n] == 0xAA).all(), f"{what}: wrote past context n - 1"
