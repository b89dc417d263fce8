/*
 * fake_compare.c -- TEST INFRASTRUCTURE: a CPU stand-in for the digest-compare
 * table launcher (md5hip_compare_launch, md5_verify.hip), linked beside
 * fake_hip.c, which has none: the batcher's weak reference then resolves and
 * the asynchronous verify entries work (tests/c/verify_check.c).  "Device"
 * memory is host memory, and the compare runs when it is enqueued.
 *   fake_compare_launches   launches made
 *   fake_compare_entries    table entries of all launches
 *   fake_compare_fail_next  the next launch fails with -EIO and writes nothing
 * Nothing here is part of the product.
 */
#include <errno.h>
#include <stdint.h>
#include <string.h>

#include "md5hip.h"
#include "../../sproxy_amd/csrc/md5_internal.h"

unsigned long fake_compare_launches, fake_compare_entries;
int fake_compare_fail_next;

int md5hip_compare_launch(const void *d_got, uint32_t gsz, const struct md5hip_cmp *d_tab, uint64_t nent,
                          void *stream)
{
    (void)stream;
    if (nent == 0) return 0;
    if (!d_got || !d_tab || !(gsz == 4 || gsz == 16 || gsz == 32)) return -EINVAL;
    __atomic_fetch_add(&fake_compare_launches, 1, __ATOMIC_RELAXED);
    __atomic_fetch_add(&fake_compare_entries, nent, __ATOMIC_RELAXED);
    if (__atomic_exchange_n(&fake_compare_fail_next, 0, __ATOMIC_RELAXED)) return -EIO;
    for (uint64_t k = 0; k < nent; k++) {
        const struct md5hip_cmp *e = &d_tab[k];
        if (e->count > MD5HIP_CMP_PIECE || (e->goff & 3u) || (e->wsz & 3u) || e->goff + e->wsz > gsz) return -EINVAL;
        const unsigned char *want = (const unsigned char *)(uintptr_t)e->want;
        unsigned char *ok = (unsigned char *)(uintptr_t)e->ok;
        uint64_t bad = 0;
        for (uint64_t i = 0; i < e->count; i++) {
            ok[i] = memcmp((const unsigned char *)d_got + (size_t)gsz * (e->first + i) + e->goff,
                           want + (size_t)e->wsz * i, e->wsz) == 0;
            bad += !ok[i];
        }
        memcpy((void *)(uintptr_t)e->cnt, &bad, 8);
    }
    return 0;
}
