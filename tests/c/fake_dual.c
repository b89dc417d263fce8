/*
 * fake_dual.c -- TEST INFRASTRUCTURE: CPU stand-ins for the two MD5_CRC32
 * launchers (md5crc32hip_fixed / md5crc32hip_desc, md5_kernels.hip), linked
 * beside fake_hip.c, which has none: the batcher's weak references then
 * resolve and the kind is usable (tests/c/dual_check.c).  Records come from
 * the library's host MD5 (md5_stream.c) and CRC-32 (nc_digest.c).
 *   fake_dual_launches   launches made (either entry)
 *   fake_dual_fail_next  the next launch fails with -EIO and writes nothing
 * Nothing here is part of the product.
 */
#include <errno.h>
#include <stdint.h>
#include <string.h>

#include "md5.h"
#include "md5hip.h"
#include "nc_digest.h"

unsigned long fake_dual_launches;
int fake_dual_fail_next;

static int begin(const void *out)
{
    __atomic_fetch_add(&fake_dual_launches, 1, __ATOMIC_RELAXED);
    if (__atomic_exchange_n(&fake_dual_fail_next, 0, __ATOMIC_RELAXED)) return -EIO;
    return ((uintptr_t)out & 15u) ? -EINVAL : 0;
}

static void record_of(const unsigned char *p, uint32_t len, struct md5hip_md5crc32 *r)
{
    struct MD5Context c;
    MD5Init(&c);
    MD5Update(&c, p, len);
    MD5Final(r->md5, &c);
    const uint32_t crc = nc_crc32(p, len);
    unsigned char *b = (unsigned char *)&r->crc;          /* little-endian, as the kernel stores it */
    b[0] = (unsigned char)crc; b[1] = (unsigned char)(crc >> 8);
    b[2] = (unsigned char)(crc >> 16); b[3] = (unsigned char)(crc >> 24);
    memset(r->zero, 0, sizeof r->zero);
}

int md5crc32hip_fixed(const void *d_base, uint64_t n, uint32_t len, uint64_t stride,
                      struct md5hip_md5crc32 *d_out, void *stream)
{
    (void)stream;
    if (n == 0) return 0;
    if (!d_base || !d_out || len > stride) return -EINVAL;
    const int rc = begin(d_out);
    if (rc) return rc;
    for (uint64_t i = 0; i < n; i++) record_of((const unsigned char *)d_base + i * stride, len, d_out + i);
    return 0;
}

int md5crc32hip_desc(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
                     const uint32_t *d_order, uint64_t n, struct md5hip_md5crc32 *d_out, void *stream)
{
    (void)stream;
    if (n == 0) return 0;
    if (!d_base || !d_offsets || !d_lens || !d_out) return -EINVAL;
    const int rc = begin(d_out);
    if (rc) return rc;
    for (uint64_t k = 0; k < n; k++) {               /* lanes in `order`, records by chunk */
        const uint64_t c = d_order ? d_order[k] : k;
        if (c >= n) return -EINVAL;
        record_of((const unsigned char *)((uintptr_t)d_base + d_offsets[c]), d_lens[c], d_out + c);
    }
    return 0;
}
