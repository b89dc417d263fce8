/*
 * fake_pages.c -- TEST INFRASTRUCTURE: a CPU stand-in for the paged launcher
 * (md5hip_digest_pages, md5_pages.hip), linked beside fake_hip.c, which has
 * none: the batcher's weak reference then resolves and
 * md5_batch_submit_device_pages works (tests/c/pages_check.c).  "Device"
 * memory is host memory; a chunk's bytes are gathered from its pages and
 * hashed with the library's host MD5 (md5_stream.c) and CRC-32 (nc_digest.c)
 * when the launch is enqueued.
 *   fake_pages_launches    launches made
 *   fake_pages_last_n      chunks of the last launch
 *   fake_pages_last_ents   table entries the last launch read (the highest + 1)
 *   fake_pages_ordered     launches that came with an order
 *   fake_pages_fail_next   the next launch fails with -EIO and writes nothing
 * Nothing here is part of the product.
 */
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "md5.h"
#include "md5hip.h"
#include "nc_digest.h"

unsigned long fake_pages_launches, fake_pages_ordered;
uint64_t fake_pages_last_n, fake_pages_last_ents;
int fake_pages_fail_next;

int md5hip_digest_pages(int kind, const uint64_t *d_pages, const uint64_t *d_first, const uint32_t *d_lens,
                        const uint32_t *d_order, uint64_t n, uint32_t page_bytes, void *d_out, void *stream)
{
    (void)stream;
    if (n == 0) return 0;
    if (kind != MD5HIP_DIGEST_MD5 && kind != MD5HIP_DIGEST_CRC32 && kind != MD5HIP_DIGEST_MD5_CRC32) return -EINVAL;
    if (!d_pages || !d_first || !d_lens || !d_out || page_bytes == 0 || (page_bytes & 127u) ||
        page_bytes > MD5HIP_PAGE_BYTES_MAX || ((uintptr_t)d_out & (kind == MD5HIP_DIGEST_CRC32 ? 3u : 15u)))
        return -EINVAL;
    __atomic_fetch_add(&fake_pages_launches, 1, __ATOMIC_RELAXED);
    if (d_order) __atomic_fetch_add(&fake_pages_ordered, 1, __ATOMIC_RELAXED);
    if (__atomic_exchange_n(&fake_pages_fail_next, 0, __ATOMIC_RELAXED)) return -EIO;
    uint64_t ents = 0;
    for (uint64_t k = 0; k < n; k++) {               /* lanes in `order`, records by chunk */
        const uint64_t c = d_order ? d_order[k] : k;
        if (c >= n) return -EINVAL;
        const uint32_t len = d_lens[c];
        unsigned char *buf = malloc(len ? len : 1);
        if (!buf) return -ENOMEM;
        for (uint32_t at = 0, p = 0; at < len; at += page_bytes, p++) {
            const uint32_t take = len - at < page_bytes ? len - at : page_bytes;
            memcpy(buf + at, (const void *)(uintptr_t)d_pages[d_first[c] + p], take);
            if (d_first[c] + p + 1 > ents) ents = d_first[c] + p + 1;
        }
        unsigned char md5[16];
        struct MD5Context ctx;
        MD5Init(&ctx);
        MD5Update(&ctx, buf, len);
        MD5Final(md5, &ctx);
        const uint32_t crc = nc_crc32(buf, len);
        const unsigned char le[4] = {(unsigned char)crc, (unsigned char)(crc >> 8), (unsigned char)(crc >> 16),
                                     (unsigned char)(crc >> 24)};
        free(buf);
        if (kind == MD5HIP_DIGEST_MD5) {
            memcpy((unsigned char *)d_out + 16 * c, md5, 16);
        } else if (kind == MD5HIP_DIGEST_CRC32) {
            memcpy((unsigned char *)d_out + 4 * c, le, 4);
        } else {
            unsigned char *r = (unsigned char *)d_out + 32 * c;
            memset(r, 0, 32);
            memcpy(r, md5, 16);
            memcpy(r + 16, le, 4);
        }
    }
    __atomic_store_n(&fake_pages_last_n, n, __ATOMIC_RELAXED);
    __atomic_store_n(&fake_pages_last_ents, ents, __ATOMIC_RELAXED);
    return 0;
}
