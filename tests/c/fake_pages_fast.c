/*
 * fake_pages_fast.c -- TEST INFRASTRUCTURE: a CPU stand-in for the fastcrc
 * windows over page lists (crc32hip_pages, md5_pages.hip), linked beside
 * fake_hip.c and fake_pages.c: the batcher's weak reference then resolves and
 * a paged verify under a CRC-32 window works (tests/c/pages_verify_check.c).
 * "Device" memory is host memory; a window's bytes are gathered from the pages
 * that hold them and summed with the library's host CRC-32 (nc_digest.c) when
 * the launch is enqueued.  fastcrc == 0 is fake_pages.c's launch, as the real
 * entry is md5hip_digest_pages'.
 *   fake_pages_fast_launches    window launches made (fastcrc > 0)
 *   fake_pages_fast_last_n      chunks of the last one
 *   fake_pages_fast_fail_next   the next one fails with -EIO and writes nothing
 * Nothing here is part of the product.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "md5hip.h"
#include "nc_digest.h"

unsigned long fake_pages_fast_launches;
uint64_t fake_pages_fast_last_n;
int fake_pages_fast_fail_next;

/* bytes [at, at + len) of a chunk whose pages start at table entry `first` */
static uint32_t window(const uint64_t *pages, uint64_t first, uint32_t page_bytes, uint32_t at, uint32_t len,
                       unsigned char *buf)
{
    for (uint32_t k = 0; k < len;) {
        const uint32_t in = (at + k) % page_bytes;
        const uint32_t take = len - k < page_bytes - in ? len - k : page_bytes - in;
        memcpy(buf + k, (const unsigned char *)(uintptr_t)pages[first + (at + k) / page_bytes] + in, take);
        k += take;
    }
    return nc_crc32(buf, len);
}

int crc32hip_pages(const uint64_t *d_pages, const uint64_t *d_first, const uint32_t *d_lens, const uint32_t *d_order,
                   uint64_t n, uint32_t page_bytes, uint32_t fastcrc, uint32_t *d_crcs, void *stream)
{
    if (fastcrc == 0)
        return md5hip_digest_pages(MD5HIP_DIGEST_CRC32, d_pages, d_first, d_lens, d_order, n, page_bytes, d_crcs, stream);
    if (n == 0) return 0;
    if (!d_pages || !d_first || !d_lens || !d_crcs || ((uintptr_t)d_crcs & 3u) || (fastcrc & 3u) || page_bytes == 0 ||
        (page_bytes & 127u) || page_bytes > MD5HIP_PAGE_BYTES_MAX)
        return -EINVAL;
    __atomic_fetch_add(&fake_pages_fast_launches, 1, __ATOMIC_RELAXED);
    if (__atomic_exchange_n(&fake_pages_fast_fail_next, 0, __ATOMIC_RELAXED)) return -EIO;
    unsigned char *buf = malloc(fastcrc);
    if (!buf) return -ENOMEM;
    for (uint64_t c = 0; c < n; c++) {
        const uint32_t L = d_lens[c];
        d_crcs[c] = L <= fastcrc ? window(d_pages, d_first[c], page_bytes, 0, L, buf)
                                 : window(d_pages, d_first[c], page_bytes, 0, fastcrc, buf) ^
                                       window(d_pages, d_first[c], page_bytes, L - fastcrc, fastcrc, buf);
    }
    free(buf);
    __atomic_store_n(&fake_pages_fast_last_n, n, __ATOMIC_RELAXED);
    return 0;
}
