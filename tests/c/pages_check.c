/*
 * pages_check.c -- TEST: md5_batch_submit_device_pages (device-resident chunks
 * laid out as page lists) through the batcher with no device.  Links
 * md5_submit.c, md5_pool.c, md5_stream.c and nc_digest.c against the fake
 * runtime (fake_hip.c), the MD5_CRC32 stand-ins (fake_dual.c) and the CPU
 * stand-in for the paged launcher (fake_pages.c); hipMalloc and hipHostMalloc
 * are wrapped (-Wl,--wrap) so that allocations are counted and one can fail:
 *   - the three kinds against the library's host MD5 / nc_crc32, synchronous
 *     and by ticket, digests to the host and to "device" memory, the caller's
 *     three arrays overwritten as soon as the call returns;
 *   - a submission cut at the chunk bound (200 chunks, 64 per slot: 4
 *     launches) and at the page-table bound (3 chunks of 30,000 entries in a
 *     table of 65,536: 2 launches), one launch per slice; an order only for
 *     slices whose keys are not already non-increasing;
 *   - the page tables allocated by the first paged call alone, two
 *     allocations for all slots; host and device submissions allocate nothing;
 *   - every refusal before anything is enqueued, the ticket zeroed: -EINVAL,
 *     -E2BIG, -ENOMEM (then the next call allocates and works);
 *   - a failed launch (-EIO, the batcher stays healthy), an injected device
 *     fault (-EIO, the host array untouched, then -ENODEV).
 * `pages_check threads`: 8 threads mix paged, device and host submissions on
 * one batcher (ThreadSanitizer).
 * Built with -DNO_PAGES and without fake_pages.c the launcher is absent: the
 * entry returns -ENOSYS with nothing enqueued, the old ones work.
 */
#define _GNU_SOURCE
#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <hip/hip_runtime_api.h>

#include "md5.h"
#include "md5hip.h"
#include "nc_digest.h"

#define NCH 200
#define PB 256u                  /* page_bytes of the common batch */
#define MAXPG 5                  /* pages per chunk there, at most */
#define CHECK(c, ...)                                        \
    do {                                                     \
        if (!(c)) {                                          \
            printf("FAIL %s:%d: ", __func__, __LINE__);      \
            printf(__VA_ARGS__);                             \
            printf("\n");                                    \
            return 1;                                        \
        }                                                    \
    } while (0)

/* ---- the wrapped allocators: counted; the next pinned one may fail */
hipError_t __real_hipMalloc(void **ptr, size_t size);
hipError_t __real_hipHostMalloc(void **ptr, size_t size, unsigned int flags);
static unsigned long g_dev_allocs, g_host_allocs;
static int g_fail_host_alloc;

hipError_t __wrap_hipMalloc(void **ptr, size_t size)
{
    __atomic_fetch_add(&g_dev_allocs, 1, __ATOMIC_RELAXED);
    return __real_hipMalloc(ptr, size);
}

hipError_t __wrap_hipHostMalloc(void **ptr, size_t size, unsigned int flags)
{
    __atomic_fetch_add(&g_host_allocs, 1, __ATOMIC_RELAXED);
    if (__atomic_exchange_n(&g_fail_host_alloc, 0, __ATOMIC_RELAXED)) {
        *ptr = NULL;
        return hipErrorOutOfMemory;
    }
    return __real_hipHostMalloc(ptr, size, flags);
}

#ifndef NO_PAGES
extern unsigned long fake_pages_launches, fake_pages_ordered;
extern uint64_t fake_pages_last_n, fake_pages_last_ents;
extern int fake_pages_fail_next;
#endif

/* The common batch: NCH chunks of 0 .. MAXPG pages of PB bytes; the pages of
 * the heap are handed out in a scrambled order, chunk i owning i % 3 entries
 * more than its length needs. */
static unsigned char *g_heap;
static uint64_t g_pages[NCH * (MAXPG + 2)], g_first[NCH + 1], g_dptr[NCH];
static uint32_t g_lens[NCH];
static unsigned char g_md5[NCH][16], g_rec[NCH][32];
static uint32_t g_crc[NCH];
static unsigned char *g_flat[NCH];               /* each chunk's bytes, contiguous */

static uint64_t rnd(uint64_t *s)
{
    *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17;
    return *s;
}

static void digests_of(const unsigned char *p, uint32_t len, unsigned char md5[16], uint32_t *crc, unsigned char rec[32])
{
    struct MD5Context c;
    MD5Init(&c);
    MD5Update(&c, p, len);
    MD5Final(md5, &c);
    *crc = nc_crc32(p, len);
    memset(rec, 0, 32);
    memcpy(rec, md5, 16);
    for (int q = 0; q < 4; q++) rec[16 + q] = (unsigned char)(*crc >> (8 * q));
}

static int setup(void)
{
    uint64_t s = 0x9E3779B97F4A7C15ull;
    const uint64_t npages = (uint64_t)NCH * MAXPG;
    g_heap = malloc(npages * PB);
    if (!g_heap) return 1;
    for (uint64_t k = 0; k < npages * PB; k++) g_heap[k] = (unsigned char)(rnd(&s) >> 24);
    uint64_t e = 0, used = 0;
    for (int i = 0; i < NCH; i++) {
        g_lens[i] = i == 7 ? 0u : i == 8 ? PB : i == 9 ? PB + 1 : (uint32_t)(rnd(&s) % (MAXPG * PB + 1));
        const uint64_t need = (g_lens[i] + PB - 1) / PB;
        g_first[i] = e;
        g_flat[i] = malloc(g_lens[i] ? g_lens[i] : 1);
        if (!g_flat[i]) return 1;
        for (uint64_t p = 0; p < need; p++, used++) {
            const uint64_t page = (used * 7919u) % npages;            /* 7919 is prime to npages = 1000 */
            const uint32_t take = g_lens[i] - p * PB < PB ? (uint32_t)(g_lens[i] - p * PB) : PB;
            g_pages[e++] = (uint64_t)(uintptr_t)(g_heap + page * PB);
            memcpy(g_flat[i] + p * PB, g_heap + page * PB, take);
        }
        for (int spare = 0; spare < i % 3; spare++) g_pages[e++] = (uint64_t)(uintptr_t)g_heap;   /* owned, not read */
        digests_of(g_flat[i], g_lens[i], g_md5[i], &g_crc[i], g_rec[i]);
        g_dptr[i] = (uint64_t)(uintptr_t)g_flat[i];
    }
    g_first[NCH] = e;
    return 0;
}

static int all_are(const void *p, size_t n, unsigned char v)
{
    for (size_t i = 0; i < n; i++)
        if (((const unsigned char *)p)[i] != v) return 0;
    return 1;
}

#ifndef NO_PAGES
static const void *right(int kind)
{
    return kind == MD5HIP_DIGEST_MD5 ? (const void *)g_md5 : kind == MD5HIP_DIGEST_CRC32 ? (const void *)g_crc : (const void *)g_rec;
}
static uint32_t dsz_of(int kind) { return kind == MD5HIP_DIGEST_MD5 ? 16 : kind == MD5HIP_DIGEST_CRC32 ? 4 : 32; }

static int kinds(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(1, 0, 3, &b) == 0, "create");
    const int ks[3] = {MD5HIP_DIGEST_MD5, MD5HIP_DIGEST_CRC32, MD5HIP_DIGEST_MD5_CRC32};
    static uint64_t pages[sizeof g_pages / 8], first[NCH + 1];
    static uint32_t lens[NCH];
    for (int k = 0; k < 3; k++) {
        const uint32_t dsz = dsz_of(ks[k]);
        unsigned char out[32 * NCH];
        unsigned char *dev = NULL;
        uint64_t t = 0;
        int rc;
        CHECK(md5hip_batcher_set_digest(b, ks[k], 0) == 0, "set_digest");
        CHECK(hipMalloc((void **)&dev, 32 * NCH) == hipSuccess, "hipMalloc");
        memset(out, 0xAA, sizeof out);
        CHECK((rc = md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, NULL)) == 0, "sync %d", rc);
        CHECK(!memcmp(out, right(ks[k]), (size_t)dsz * NCH) && all_are(out + dsz * NCH, sizeof out - dsz * NCH, 0xAA), "kind %d sync", ks[k]);
        /* by ticket, the caller's arrays gone as soon as the call is back */
        memcpy(pages, g_pages, sizeof g_pages);
        memcpy(first, g_first, sizeof g_first);
        memcpy(lens, g_lens, sizeof g_lens);
        memset(out, 0xAA, sizeof out);
        CHECK((rc = md5_batch_submit_device_pages(b, pages, first, lens, NCH, PB, out, 0, NULL, 1, &t)) == 0 && t != 0, "async %d", rc);
        memset(pages, 0xEE, sizeof pages);
        memset(first, 0xEE, sizeof first);
        memset(lens, 0xEE, sizeof lens);
        CHECK(md5_batch_wait(b, t) == 0 && !memcmp(out, right(ks[k]), (size_t)dsz * NCH), "kind %d async", ks[k]);
        /* digests left on the "device" */
        memset(dev, 0xAA, 32 * NCH);
        CHECK(md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, dev, 1, NULL, 0, &t) == 0 && md5_batch_wait(b, t) == 0 &&
                  !memcmp(dev, right(ks[k]), (size_t)dsz * NCH), "kind %d device digests", ks[k]);
        hipFree(dev);
    }
    struct md5hip_batcher_stats st;
    md5hip_batcher_get_stats(b, &st);
    CHECK(st.launches == 9 && st.chunks == 9 * NCH && st.bytes_staged == 0, "stats: %llu launches, %llu chunks, %llu staged",
          (unsigned long long)st.launches, (unsigned long long)st.chunks, (unsigned long long)st.bytes_staged);
    md5hip_batcher_destroy(b);
    printf("kinds: MD5, CRC-32, MD5_CRC32; synchronous, by ticket, device digests; the caller's arrays overwritten\n");
    return 0;
}

static int slices(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(0, 64, 3, &b) == 0, "create");
    unsigned char out[16 * NCH];
    unsigned long l0 = fake_pages_launches, o0 = fake_pages_ordered;
    /* the chunk bound: 64 + 64 + 64 + 8 */
    CHECK(md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, NULL) == 0 && !memcmp(out, g_md5, sizeof out),
          "chunk-bound slices");
    CHECK(fake_pages_launches - l0 == 4 && fake_pages_last_n == 8 && fake_pages_ordered - o0 == 4, "%lu launches, last of %llu chunks, %lu ordered",
          fake_pages_launches - l0, (unsigned long long)fake_pages_last_n, fake_pages_ordered - o0);
    struct md5hip_batcher_stats st;
    md5hip_batcher_get_stats(b, &st);
    CHECK(st.launches == 4 && st.chunks == NCH && st.max_chunks_per_launch == 64 && st.submissions == 1, "stats");
    /* keys already non-increasing: no order is built */
    static const uint32_t down[4] = {3 * PB, 2 * PB + 70, 2 * PB + 65, 0};
    static const uint64_t dfirst[5] = {0, 3, 6, 9, 9};
    unsigned char d4[4][16], want[16];
    uint32_t crc;
    unsigned char rec[32];
    o0 = fake_pages_ordered;
    CHECK(md5_batch_submit_device_pages(b, g_pages, dfirst, down, 4, PB, &d4[0][0], 0, NULL, 0, NULL) == 0 && fake_pages_ordered == o0,
          "a sorted slice got an order");
    /* the page-table bound: MD5HIP_PAGES_PER_SLOT(64) = 65,536 entries; three
     * chunks of 30,000 entries (all naming the heap's first pages) */
    enum { BIG = 30000 };
    CHECK(MD5HIP_PAGES_PER_SLOT(64) == 65536, "capacity");
    uint64_t *pg = malloc(8 * 3 * BIG);
    unsigned char *flat = malloc((size_t)BIG * 128);
    CHECK(pg && flat, "malloc");
    for (int e = 0; e < 3 * BIG; e++) pg[e] = (uint64_t)(uintptr_t)(g_heap + 128 * (e % 1000));
    const uint64_t bfirst[4] = {0, BIG, 2 * BIG, 3 * BIG};
    const uint32_t blens[3] = {BIG * 128u, BIG * 128u - 127u, BIG * 128u - 64u};
    unsigned char got[3][16];
    l0 = fake_pages_launches;
    CHECK(md5_batch_submit_device_pages(b, pg, bfirst, blens, 3, 128, &got[0][0], 0, NULL, 0, NULL) == 0, "table-bound slices");
    CHECK(fake_pages_launches - l0 == 2 && fake_pages_last_n == 1 && fake_pages_last_ents == BIG, "%lu launches, last of %llu chunks / %llu entries",
          fake_pages_launches - l0, (unsigned long long)fake_pages_last_n, (unsigned long long)fake_pages_last_ents);
    for (int c = 0; c < 3; c++) {
        for (int e = 0; e < BIG; e++) memcpy(flat + 128 * (size_t)e, (const void *)(uintptr_t)pg[c * BIG + e], 128);
        digests_of(flat, blens[c], want, &crc, rec);
        CHECK(!memcmp(got[c], want, 16), "big chunk %d", c);
    }
    /* one chunk reading more entries than a slot's table */
    const uint64_t hfirst[2] = {0, 3 * BIG};
    const uint32_t hlen = 65537u * 128u;
    uint64_t t = 9;
    l0 = fake_pages_launches;
    md5hip_batcher_get_stats(b, &st);
    const uint64_t subs = st.submissions;
    CHECK(md5_batch_submit_device_pages(b, pg, hfirst, &hlen, 1, 128, &got[0][0], 0, NULL, 0, &t) == -E2BIG && t == 0, "E2BIG");
    md5hip_batcher_get_stats(b, &st);
    CHECK(fake_pages_launches == l0 && st.submissions == subs, "a refused chunk was enqueued");
    free(pg);
    free(flat);
    md5hip_batcher_destroy(b);
    printf("slices: 200 chunks of 64 per slot in 4 launches, 90,000 entries of 65,536 per slot in 2; order only when needed; -E2BIG\n");
    return 0;
}

static int buffers_and_refusals(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(2, 256, 3, &b) == 0, "create");
    unsigned char out[32 * NCH];
    uint64_t t = 9;
    int rc;
    /* a batcher that never pages: host and device submissions allocate nothing */
    unsigned long d0 = g_dev_allocs, h0 = g_host_allocs;
    const void *ptrs[NCH];
    for (int i = 0; i < NCH; i++) ptrs[i] = g_flat[i];
    CHECK(md5_batch_submit(b, ptrs, g_lens, NCH, out) == 0 && !memcmp(out, g_md5, 16 * NCH), "host submit");
    CHECK(md5_batch_submit_device(b, g_dptr, g_lens, NCH, out, 0) == 0 && !memcmp(out, g_md5, 16 * NCH), "device submit");
    CHECK(g_dev_allocs == d0 && g_host_allocs == h0, "allocations without a paged call");
    /* refusals: nothing allocated, nothing enqueued, the ticket zeroed */
    struct md5hip_batcher_stats s0, s1;
    md5hip_batcher_get_stats(b, &s0);
    const unsigned long l0 = fake_pages_launches;
#define REFUSED(want, ...)                                                                         \
    do {                                                                                           \
        t = 9;                                                                                     \
        CHECK((rc = md5_batch_submit_device_pages(__VA_ARGS__)) == (want) && t == 0, "%s: %d, ticket %llu", #__VA_ARGS__, rc, \
              (unsigned long long)t);                                                              \
    } while (0)
    REFUSED(-EINVAL, NULL, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t);
    REFUSED(-EINVAL, b, NULL, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t);
    REFUSED(-EINVAL, b, g_pages, NULL, g_lens, NCH, PB, out, 0, NULL, 0, &t);
    REFUSED(-EINVAL, b, g_pages, g_first, NULL, NCH, PB, out, 0, NULL, 0, &t);
    REFUSED(-EINVAL, b, g_pages, g_first, g_lens, NCH, PB, NULL, 0, NULL, 0, &t);
    REFUSED(-EINVAL, b, g_pages, g_first, g_lens, NCH, 0, out, 0, NULL, 0, &t);
    REFUSED(-EINVAL, b, g_pages, g_first, g_lens, NCH, 192, out, 0, NULL, 0, &t);
    REFUSED(-EINVAL, b, g_pages, g_first, g_lens, NCH, (1u << 30) + 128, out, 0, NULL, 0, &t);
    REFUSED(0, b, NULL, NULL, NULL, 0, 0, NULL, 0, NULL, 0, &t);                 /* empty: complete at once */
    uint64_t first[NCH + 1];
    memcpy(first, g_first, sizeof first);
    first[50] = first[49] - 1;                                                  /* decreasing */
    REFUSED(-EINVAL, b, g_pages, first, g_lens, NCH, PB, out, 0, NULL, 0, &t);
    memcpy(first, g_first, sizeof first);
    CHECK(g_lens[10] > 0 && 10 % 3 == 1, "chunk 10 reads pages and owns one spare entry");
    for (int i = 11; i <= NCH; i++) first[i] -= 2;                              /* chunk 10 one entry short */
    REFUSED(-EINVAL, b, g_pages, first, g_lens, NCH, PB, out, 0, NULL, 0, &t);
    uint64_t pages[sizeof g_pages / 8];
    memcpy(pages, g_pages, sizeof pages);
    pages[g_first[20]] = 0;                                                     /* a NULL page that is read */
    CHECK(g_lens[20] > 0, "chunk 20 reads a page");
    REFUSED(-EINVAL, b, pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t);
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, 64) == 0, "fastcrc 64");
    REFUSED(-EINVAL, b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t);
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5, 0) == 0, "MD5 again");
    CHECK(g_dev_allocs == d0 && g_host_allocs == h0, "a refused call allocated");
    /* the tables cannot be had: -ENOMEM, nothing kept; the next call allocates them */
    __atomic_store_n(&g_fail_host_alloc, 1, __ATOMIC_RELAXED);
    REFUSED(-ENOMEM, b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t);
    md5hip_batcher_get_stats(b, &s1);
    CHECK(fake_pages_launches == l0 && s1.launches == s0.launches && s1.submissions == s0.submissions, "a refused call was enqueued");
    h0 = g_host_allocs;
    memset(out, 0xAA, sizeof out);
    CHECK(md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, NULL) == 0 && !memcmp(out, g_md5, 16 * NCH), "first paged call");
    CHECK(g_host_allocs - h0 == 1 && g_dev_allocs - d0 == 1, "%lu pinned and %lu device allocations by the first paged call", g_host_allocs - h0,
          g_dev_allocs - d0);
    for (int k = 0; k < 5; k++)
        CHECK(md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, NULL) == 0, "paged call %d", k);
    CHECK(g_host_allocs - h0 == 1 && g_dev_allocs - d0 == 1, "later paged calls allocated");
    md5hip_batcher_destroy(b);
    printf("buffers: two allocations by the first paged call, none otherwise; refusals: -EINVAL, -ENOMEM before anything is enqueued, ticket zeroed\n");
    return 0;
}

static int failures(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(3, 0, 3, &b) == 0, "create");
    unsigned char out[16 * NCH];
    uint64_t t = 0;
    int rc;
    /* a launch that fails on a healthy device */
    memset(out, 0x5A, sizeof out);
    __atomic_store_n(&fake_pages_fail_next, 1, __ATOMIC_RELAXED);
    CHECK((rc = md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t)) == 0, "submit %d", rc);
    CHECK((rc = md5_batch_wait(b, t)) == -EIO && all_are(out, sizeof out, 0x5A), "failed launch %d", rc);
    CHECK(md5hip_batcher_health(b) == 0, "healthy after a failed launch");
    CHECK(md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, NULL) == 0 && !memcmp(out, g_md5, sizeof out), "after it");
    /* the injected device fault: -EIO, nothing delivered, then -ENODEV at once */
    CHECK(md5hip_batcher_inject_fault(b, 1) == 0, "inject");
    memset(out, 0x5A, sizeof out);
    CHECK((rc = md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t)) == 0, "submit %d", rc);
    CHECK((rc = md5_batch_wait(b, t)) == -EIO && all_are(out, sizeof out, 0x5A), "the faulted launch's ticket %d", rc);
    CHECK(md5hip_batcher_health(b) == -ENODEV, "failed");
    const unsigned long l0 = fake_pages_launches;
    t = 9;
    CHECK((rc = md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t)) == -ENODEV && t == 0, "later %d", rc);
    CHECK(fake_pages_launches == l0 && all_are(out, sizeof out, 0x5A), "a failed device was used");
    md5hip_batcher_destroy(b);
    printf("failures: failed launch -EIO, injected fault -EIO then -ENODEV, nothing delivered\n");
    return 0;
}

/* ---- `threads`: 8 threads on one batcher */
static md5hip_batcher *g_b;
static int g_thread_fail;

static void *worker(void *arg)
{
    uint64_t s = 0x1234567ull + (uint64_t)(uintptr_t)arg * 977u;
    for (int round = 0; round < 60 && !__atomic_load_n(&g_thread_fail, __ATOMIC_RELAXED); round++) {
        const int lo = (int)(rnd(&s) % (NCH - 40)), n = 1 + (int)(rnd(&s) % 40);
        unsigned char dig[16 * 40];
        uint64_t first[41], t = 0;
        const void *ptrs[40];
        int rc;
        const int what = (int)(rnd(&s) % 4);
        memset(dig, 0, sizeof dig);
        switch (what) {
        case 0:
        case 1:
            memcpy(first, g_first + lo, 8 * ((size_t)n + 1));
            rc = md5_batch_submit_device_pages(g_b, g_pages, first, g_lens + lo, (uint64_t)n, PB, dig, 0, NULL, 0, what ? &t : NULL);
            memset(first, 0xEE, sizeof first);
            if (!rc && what) rc = md5_batch_wait(g_b, t);
            break;
        case 2:
            rc = md5_batch_submit_device_async(g_b, g_dptr + lo, g_lens + lo, (uint64_t)n, dig, 0, &t);
            if (!rc) rc = md5_batch_wait(g_b, t);
            break;
        default:
            for (int i = 0; i < n; i++) ptrs[i] = g_flat[lo + i];
            rc = md5_batch_submit(g_b, ptrs, g_lens + lo, (uint64_t)n, dig);
            break;
        }
        if (rc || memcmp(dig, g_md5[lo], 16 * (size_t)n)) {
            printf("FAIL worker: what %d lo %d n %d rc %d\n", what, lo, n, rc);
            __atomic_store_n(&g_thread_fail, 1, __ATOMIC_RELAXED);
        }
    }
    return NULL;
}

static int threads(void)
{
    CHECK(md5hip_queue_create(0, 16, 3, &g_b) == 0, "create");       /* 16 per slot: paged submissions cut into slices */
    pthread_t th[8];
    for (uintptr_t k = 0; k < 8; k++) CHECK(pthread_create(&th[k], NULL, worker, (void *)k) == 0, "thread");
    for (int k = 0; k < 8; k++) pthread_join(th[k], NULL);
    md5hip_batcher_destroy(g_b);
    CHECK(!g_thread_fail, "a worker failed");
    printf("threads: 8 threads x 60 rounds of paged / device / host submissions on one batcher\n");
    return 0;
}
#else  /* NO_PAGES: the launcher is absent */
static int refusals(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(0, 0, 3, &b) == 0, "create");
    struct md5hip_batcher_stats s0, s1;
    md5hip_batcher_get_stats(b, &s0);
    const unsigned long d0 = g_dev_allocs, h0 = g_host_allocs;
    unsigned char out[16 * NCH];
    uint64_t t = 9;
    int rc;
    memset(out, 0xAA, sizeof out);
    CHECK((rc = md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, &t)) == -ENOSYS && t == 0, "by ticket %d", rc);
    CHECK((rc = md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, NULL)) == -ENOSYS, "synchronous %d", rc);
    md5hip_batcher_get_stats(b, &s1);
    CHECK(all_are(out, sizeof out, 0xAA) && s1.launches == s0.launches && s1.submissions == s0.submissions && g_dev_allocs == d0 &&
              g_host_allocs == h0, "something was enqueued or allocated");
    /* the old entries as before */
    const void *ptrs[NCH];
    for (int i = 0; i < NCH; i++) ptrs[i] = g_flat[i];
    CHECK(md5_batch_submit(b, ptrs, g_lens, NCH, out) == 0 && !memcmp(out, g_md5, sizeof out), "host submit");
    memset(out, 0xAA, sizeof out);
    CHECK(md5_batch_submit_device_async(b, g_dptr, g_lens, NCH, out, 0, &t) == 0 && md5_batch_wait(b, t) == 0 && !memcmp(out, g_md5, sizeof out),
          "device submit");
    md5hip_batcher_destroy(b);
    printf("refusals: without the paged launcher the entry is -ENOSYS, nothing enqueued, the old entries work\n");
    return 0;
}
#endif

int main(int argc, char **argv)
{
    setvbuf(stdout, NULL, _IOLBF, 0);
    if (setup()) return 2;
#ifndef NO_PAGES
    if (argc > 1 && !strcmp(argv[1], "threads")) {
        if (threads()) return 1;
    } else if (kinds() || slices() || buffers_and_refusals() || failures()) {
        return 1;
    }
#else
    (void)argc;
    (void)argv;
    if (refusals()) return 1;
#endif
    for (int i = 0; i < NCH; i++) free(g_flat[i]);
    free(g_heap);
    printf("pages ok\n");
    return 0;
}
