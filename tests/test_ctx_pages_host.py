"""MD5Update on caller-owned contexts over page lists
(md5hip_update_ctx_pages) with no device: the argument rules through
libmd5hip.so.  Every refusal comes back before any device work, so the
pointers here are sentinels that are never dereferenced."""
import ctypes
import errno

from sproxy_amd import _lib

EINVAL = -errno.EINVAL


def test_update_ctx_pages_argument_errors_before_device_work():
    L = _lib.lib()
    p = ctypes.c_void_p
    up = L.md5hip_update_ctx_pages
    assert up(None, None, None, None, 0, 0, None) == 0                      # empty: a no-op
    assert up(p(65), None, p(64), None, 0, 100, p(8)) == 0                  # whatever else is passed
    good = (p(64), p(64), p(64), p(64), 5, 16384, None)
    names = ("ctxs", "pages", "first", "lens", "n", "page_bytes", "stream")

    def with_(**kw):
        return up(*[kw.get(k, v) for k, v in zip(names, good)])

    for name in ("ctxs", "pages", "first", "lens"):
        assert with_(**{name: None}) == EINVAL, name
    for addr in (65, 66, 67, 0x1001):
        assert with_(ctxs=p(addr)) == EINVAL, addr                          # struct MD5Context is 4-byte aligned
    for pb in (0, 64, 100, 16384 + 64, (1 << 30) + 128, 0xFFFFFF80):
        assert with_(page_bytes=pb) == EINVAL, pb
    assert with_(n=64 * (1 << 31)) == EINVAL                                # 2^31 groups of 64 contexts
    # a context array off the 16-B grid is fine (88-byte structs): what is
    # left is the device's to refuse, so only the empty call is made here
    assert with_(ctxs=p(68), n=0) == 0
