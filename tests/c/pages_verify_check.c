/*
 * pages_verify_check.c -- TEST: md5_batch_verify_device_pages and
 * md5_batch_upgrade_device_pages (verify and upgrade of blocks laid out as
 * page lists, compared on the device) through the batcher with no device.
 * Links md5_submit.c, md5_pool.c, md5_stream.c and nc_digest.c against the
 * fake runtime (fake_hip.c), the MD5_CRC32 stand-ins (fake_dual.c), the CPU
 * stand-ins for the paged launcher (fake_pages.c), the compare launcher
 * (fake_compare.c) and the window launcher (fake_pages_fast.c); hipMalloc and
 * hipHostMalloc are wrapped (-Wl,--wrap) so that allocations are counted and
 * one can fail:
 *   - every kind -- MD5, CRC-32 of the whole block, CRC-32 under a 128-byte
 *     window, MD5_CRC32 records -- with four wrong expected values, each
 *     wrong at another byte: synchronous and by ticket, expected / ok on the
 *     host (the caller's arrays overwritten as soon as the call returns) and
 *     on the "device"; the upgrade with two wrong CRCs and every MD5;
 *   - a call cut at the chunk bound (200 blocks, 64 per slot: 4 launches, 4
 *     compares, nbad summed, ok in submission order) and at the page-table
 *     bound (2 launches);
 *   - the page tables and the verify buffers each allocated once, by the first
 *     call that needs them;
 *   - the refusals in their order -- -EINVAL, -E2BIG, -ENOMEM -- before
 *     anything is enqueued, the ticket zeroed;
 *   - a failed hash launch, a failed compare launch, an injected device
 *     fault: nothing delivered to ok, md5_out or nbad.
 * `pages_verify_check threads`: 8 threads mix paged verifies, paged
 * submissions and device verifies on one batcher (ThreadSanitizer).
 * Built with -DNO_FAST and without fake_pages_fast.c the window launcher is
 * absent: a paged verify under a window is -ENOSYS -- after -EINVAL, before
 * -E2BIG -- with nothing enqueued, and the other kinds verify as before.
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
#define MAXPG 4                  /* pages per block there, at most */
#define FW 128u                  /* the fastcrc window */
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

extern unsigned long fake_pages_launches, fake_compare_launches;
extern uint64_t fake_pages_last_n;
extern int fake_pages_fail_next, fake_compare_fail_next;
#ifndef NO_FAST
extern unsigned long fake_pages_fast_launches;
extern uint64_t fake_pages_fast_last_n;
#endif

/* The common batch: NCH blocks of 0 .. MAXPG pages of PB bytes, the heap's
 * pages handed out in a scrambled order. */
static unsigned char *g_heap;
static uint64_t g_pages[NCH * MAXPG], g_first[NCH + 1], g_dptr[NCH];
static uint32_t g_lens[NCH];
static unsigned char g_md5[NCH][16], g_rec[NCH][32];
static uint32_t g_crc[NCH], g_win[NCH];          /* whole-block CRCs, and blk_make_crc's under FW */
static unsigned char *g_flat[NCH];               /* each block's bytes, contiguous */
static const int g_bad[4] = {0, 63, 64, 199};

static uint64_t rnd(uint64_t *s)
{
    *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17;
    return *s;
}

static int setup(void)
{
    uint64_t s = 0x9E3779B97F4A7C15ull;
    const uint64_t npages = (uint64_t)NCH * MAXPG;
    g_heap = malloc(npages * PB);
    if (!g_heap) return 1;
    for (uint64_t k = 0; k < npages * PB; k++) g_heap[k] = (unsigned char)(rnd(&s) >> 24);
    uint64_t e = 0;
    for (int i = 0; i < NCH; i++) {
        /* an empty block, one of exactly the window, one a byte longer, a tail straddling two pages */
        g_lens[i] = i == 7 ? 0u : i == 8 ? FW : i == 9 ? FW + 1 : i == 10 ? 2 * PB + 1 : (uint32_t)(rnd(&s) % (MAXPG * PB + 1));
        const uint32_t L = g_lens[i];
        g_first[i] = e;
        g_flat[i] = malloc(L ? L : 1);
        if (!g_flat[i]) return 1;
        for (uint64_t p = 0; p * PB < L; p++, e++) {
            const uint64_t page = (e * 7919u) % npages;               /* 7919 is prime to npages = 800 */
            g_pages[e] = (uint64_t)(uintptr_t)(g_heap + page * PB);
            memcpy(g_flat[i] + p * PB, g_heap + page * PB, L - p * PB < PB ? L - p * PB : PB);
        }
        struct MD5Context c;
        MD5Init(&c);
        MD5Update(&c, g_flat[i], L);
        MD5Final(g_md5[i], &c);
        g_crc[i] = nc_crc32(g_flat[i], L);
        g_win[i] = L <= FW ? g_crc[i] : nc_crc32(g_flat[i], FW) ^ nc_crc32(g_flat[i] + L - FW, FW);
        memset(g_rec[i], 0, 32);
        memcpy(g_rec[i], g_md5[i], 16);
        for (int q = 0; q < 4; q++) g_rec[i][16 + q] = (unsigned char)(g_crc[i] >> (8 * q));
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

/* a digest kind with its window, the right values and the record size */
struct kindw {
    int kind;
    uint32_t fastcrc, dsz;
    const void *right;
    const char *name;
};
static const struct kindw g_kinds[4] = {{MD5HIP_DIGEST_MD5, 0, 16, g_md5, "MD5"},
                                        {MD5HIP_DIGEST_CRC32, 0, 4, g_crc, "CRC-32"},
                                        {MD5HIP_DIGEST_CRC32, FW, 4, g_win, "CRC-32 window"},
                                        {MD5HIP_DIGEST_MD5_CRC32, 0, 32, g_rec, "MD5_CRC32"}};

/* the right values with one bit flipped in the blocks g_bad, each at another
 * byte of the record; want_ok: what ok must then be */
static void spoil(const struct kindw *k, unsigned char *exp, unsigned char *want_ok)
{
    const uint32_t at[4] = {0, 1, k->dsz - 2, k->dsz - 1};
    memcpy(exp, k->right, (size_t)k->dsz * NCH);
    memset(want_ok, 1, NCH);
    for (int j = 0; j < 4; j++) {
        exp[(size_t)k->dsz * g_bad[j] + at[j]] ^= (unsigned char)(1u << j);
        want_ok[g_bad[j]] = 0;
    }
}

static int verify_kind(md5hip_batcher *b, const struct kindw *k)
{
    unsigned char exp[32 * NCH], scratch[32 * NCH], want_ok[NCH], ok[NCH + 8];
    static uint64_t pages[NCH * MAXPG], first[NCH + 1];
    static uint32_t lens[NCH];
    uint64_t nbad = 99, t = 0;
    int rc;
    spoil(k, exp, want_ok);
    CHECK(md5hip_batcher_set_digest(b, k->kind, k->fastcrc) == 0, "set_digest");
    /* synchronous, host */
    memset(ok, 0xAA, sizeof ok);
    CHECK((rc = md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, exp, ok, 0, NULL, 0, &nbad, NULL)) == 0, "%s sync %d", k->name, rc);
    CHECK(nbad == 4 && !memcmp(ok, want_ok, NCH) && all_are(ok + NCH, 8, 0xAA), "%s sync: nbad %llu", k->name, (unsigned long long)nbad);
    /* by ticket, every array of the caller's gone as soon as the call is back */
    memcpy(pages, g_pages, sizeof g_pages);
    memcpy(first, g_first, sizeof g_first);
    memcpy(lens, g_lens, sizeof g_lens);
    memcpy(scratch, exp, sizeof exp);
    memset(ok, 0xAA, sizeof ok);
    nbad = 99;
    CHECK((rc = md5_batch_verify_device_pages(b, pages, first, lens, NCH, PB, scratch, ok, 0, NULL, 1, &nbad, &t)) == 0 && t != 0, "%s async %d", k->name, rc);
    memset(pages, 0xEE, sizeof pages);
    memset(first, 0xEE, sizeof first);
    memset(lens, 0xEE, sizeof lens);
    memset(scratch, 0xEE, sizeof scratch);
    CHECK(md5_batch_wait(b, t) == 0 && nbad == 4 && !memcmp(ok, want_ok, NCH), "%s by ticket: nbad %llu", k->name, (unsigned long long)nbad);
    /* expected and ok on the "device", expected off every grid */
    unsigned char *dev = NULL;
    CHECK(hipMalloc((void **)&dev, 32 * NCH + 1 + NCH) == hipSuccess, "hipMalloc");
    memcpy(dev + 1, exp, (size_t)k->dsz * NCH);
    unsigned char *dok = dev + 1 + 32 * NCH;
    memset(dok, 0xAA, NCH);
    nbad = 99;
    CHECK((rc = md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, dev + 1, dok, 1, NULL, 0, &nbad, &t)) == 0 &&
              md5_batch_wait(b, t) == 0 && nbad == 4 && !memcmp(dok, want_ok, NCH), "%s device form %d", k->name, rc);
    nbad = 99;
    CHECK(md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, dev + 1, dok, 1, NULL, 0, &nbad, NULL) == 0 && nbad == 4,
          "%s device form, synchronous", k->name);
    hipFree(dev);
    return 0;
}

static int upgrade(md5hip_batcher *b)
{
    uint32_t want[NCH];
    unsigned char want_ok[NCH], ok[NCH], md5[NCH][16];
    uint64_t nbad = 99, t = 0;
    int rc;
    memcpy(want, g_crc, sizeof want);
    memset(want_ok, 1, NCH);
    want[1] ^= 0x100u;
    want[65] ^= 0x80000000u;
    want_ok[1] = want_ok[65] = 0;
    memset(md5, 0xAA, sizeof md5);
    CHECK((rc = md5_batch_upgrade_device_pages(b, g_pages, g_first, g_lens, NCH, PB, want, ok, &md5[0][0], NULL, 0, &nbad, NULL)) == 0, "sync %d", rc);
    CHECK(nbad == 2 && !memcmp(ok, want_ok, NCH) && !memcmp(md5, g_md5, sizeof md5), "upgrade: nbad %llu", (unsigned long long)nbad);
    memset(md5, 0xAA, sizeof md5);
    memset(ok, 0xAA, sizeof ok);
    CHECK(md5_batch_upgrade_device_pages(b, g_pages, g_first, g_lens, NCH, PB, want, ok, &md5[0][0], NULL, 0, &nbad, &t) == 0 && t != 0, "async");
    memset(want, 0xEE, sizeof want);
    CHECK(md5_batch_wait(b, t) == 0 && nbad == 2 && !memcmp(ok, want_ok, NCH) && !memcmp(md5, g_md5, sizeof md5), "upgrade by ticket");
    return 0;
}

#ifndef NO_FAST
static int kinds(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(1, 0, 3, &b) == 0, "create");
    const unsigned long f0 = fake_pages_fast_launches, p0 = fake_pages_launches, c0 = fake_compare_launches;
    for (int k = 0; k < 4; k++)
        if (verify_kind(b, &g_kinds[k])) return 1;
    CHECK(fake_pages_fast_launches - f0 == 4 && fake_pages_launches - p0 == 12 && fake_compare_launches - c0 == 16,
          "%lu window, %lu paged, %lu compare launches", fake_pages_fast_launches - f0, fake_pages_launches - p0, fake_compare_launches - c0);
    /* the upgrade is MD5_CRC32 whatever the batcher is set to: here, a window */
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, FW) == 0, "set_digest");
    if (upgrade(b)) return 1;
    CHECK(fake_pages_fast_launches - f0 == 4 && fake_pages_launches - p0 == 14, "the upgrade's launches");
    struct md5hip_batcher_stats st;
    md5hip_batcher_get_stats(b, &st);
    CHECK(st.launches == 18 && st.chunks == 18 * NCH && st.bytes_staged == 0, "stats: %llu launches, %llu chunks, %llu staged",
          (unsigned long long)st.launches, (unsigned long long)st.chunks, (unsigned long long)st.bytes_staged);
    md5hip_batcher_destroy(b);
    printf("kinds: MD5, CRC-32, CRC-32 window, MD5_CRC32 with 4 mismatches; synchronous, by ticket, host and device forms; upgrade with 2\n");
    return 0;
}

static int slices(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(0, 64, 3, &b) == 0, "create");
    unsigned char exp[32 * NCH], want_ok[NCH], ok[NCH];
    uint64_t nbad = 99, t = 0;
    /* the chunk bound: 64 + 64 + 64 + 8, under the window and under MD5 */
    for (int k = 2; k >= 0; k -= 2) {
        spoil(&g_kinds[k], exp, want_ok);
        CHECK(md5hip_batcher_set_digest(b, g_kinds[k].kind, g_kinds[k].fastcrc) == 0, "set_digest");
        const unsigned long l0 = k ? fake_pages_fast_launches : fake_pages_launches, c0 = fake_compare_launches;
        memset(ok, 0xAA, sizeof ok);
        CHECK(md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, exp, ok, 0, NULL, 0, &nbad, &t) == 0 && md5_batch_wait(b, t) == 0,
              "chunk-bound slices");
        CHECK(nbad == 4 && !memcmp(ok, want_ok, NCH), "%s: nbad %llu over the slices", g_kinds[k].name, (unsigned long long)nbad);
        const unsigned long l1 = k ? fake_pages_fast_launches : fake_pages_launches;
        CHECK(l1 - l0 == 4 && (k ? fake_pages_fast_last_n : fake_pages_last_n) == 8 && fake_compare_launches - c0 == 4, "%lu launches, %lu compares",
              l1 - l0, fake_compare_launches - c0);
    }
    struct md5hip_batcher_stats st;
    md5hip_batcher_get_stats(b, &st);
    CHECK(st.launches == 8 && st.chunks == 2 * NCH && st.max_chunks_per_launch == 64 && st.submissions == 2, "stats");
    /* the page-table bound: MD5HIP_PAGES_PER_SLOT(64) = 65,536 entries; three
     * blocks of 30,000 entries (all naming the heap's first pages), the
     * second one's MD5 wrong */
    enum { BIG = 30000 };
    uint64_t *pg = malloc(8 * 3 * BIG);
    unsigned char *flat = malloc((size_t)BIG * 128);
    CHECK(pg && flat, "malloc");
    for (int e = 0; e < 3 * BIG; e++) pg[e] = (uint64_t)(uintptr_t)(g_heap + 128 * (e % 1000));
    const uint64_t bfirst[4] = {0, BIG, 2 * BIG, 3 * BIG};
    const uint32_t blens[3] = {BIG * 128u, BIG * 128u - 127u, BIG * 128u - 64u};
    unsigned char want[3][16];
    for (int c = 0; c < 3; c++) {
        struct MD5Context x;
        for (int e = 0; e < BIG; e++) memcpy(flat + 128 * (size_t)e, (const void *)(uintptr_t)pg[c * BIG + e], 128);
        MD5Init(&x);
        MD5Update(&x, flat, blens[c]);
        MD5Final(want[c], &x);
    }
    want[1][15] ^= 1;
    const unsigned long l0 = fake_pages_launches;
    CHECK(md5_batch_verify_device_pages(b, pg, bfirst, blens, 3, 128, want, ok, 0, NULL, 0, &nbad, NULL) == 0, "table-bound slices");
    CHECK(fake_pages_launches - l0 == 2 && fake_pages_last_n == 1 && nbad == 1 && ok[0] == 1 && ok[1] == 0 && ok[2] == 1, "%lu launches, nbad %llu",
          fake_pages_launches - l0, (unsigned long long)nbad);
    free(pg);
    free(flat);
    md5hip_batcher_destroy(b);
    printf("slices: 200 blocks of 64 per slot in 4 launches and 4 compares, nbad summed, ok in order; 90,000 entries of 65,536 per slot in 2\n");
    return 0;
}

static int buffers_and_refusals(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(2, 256, 3, &b) == 0, "create");
    unsigned char ok[NCH], md5[NCH][16];
    uint64_t t = 9, nbad = 9;
    int rc;
    const unsigned long d0 = g_dev_allocs, h0 = g_host_allocs;
    struct md5hip_batcher_stats s0, s1;
    md5hip_batcher_get_stats(b, &s0);
    const unsigned long l0 = fake_pages_launches + fake_pages_fast_launches, c0 = fake_compare_launches;
    memset(ok, 0x5A, sizeof ok);
#define REFUSED(fn, want, ...)                                                                                     \
    do {                                                                                                           \
        t = 9;                                                                                                     \
        CHECK((rc = fn(__VA_ARGS__)) == (want) && t == 0, "%s(%s): %d, ticket %llu", #fn, #__VA_ARGS__, rc, (unsigned long long)t); \
    } while (0)
#define V md5_batch_verify_device_pages
#define U md5_batch_upgrade_device_pages
    REFUSED(V, -EINVAL, NULL, g_pages, g_first, g_lens, NCH, PB, g_md5, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(V, -EINVAL, b, NULL, g_first, g_lens, NCH, PB, g_md5, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(V, -EINVAL, b, g_pages, NULL, g_lens, NCH, PB, g_md5, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(V, -EINVAL, b, g_pages, g_first, NULL, NCH, PB, g_md5, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(V, -EINVAL, b, g_pages, g_first, g_lens, NCH, PB, NULL, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(V, -EINVAL, b, g_pages, g_first, g_lens, NCH, PB, g_md5, NULL, 0, NULL, 0, &nbad, &t);
    REFUSED(V, -EINVAL, b, g_pages, g_first, g_lens, NCH, 0, g_md5, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(V, -EINVAL, b, g_pages, g_first, g_lens, NCH, 192, g_md5, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(V, -EINVAL, b, g_pages, g_first, g_lens, NCH, (1u << 30) + 128, g_md5, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(V, 0, b, NULL, NULL, NULL, 0, 0, NULL, NULL, 0, NULL, 0, &nbad, &t);         /* empty: complete at once */
    CHECK(nbad == 0, "nbad of an empty call");
    REFUSED(U, -EINVAL, NULL, g_pages, g_first, g_lens, NCH, PB, g_crc, ok, &md5[0][0], NULL, 0, &nbad, &t);
    REFUSED(U, -EINVAL, b, g_pages, g_first, g_lens, NCH, PB, NULL, ok, &md5[0][0], NULL, 0, &nbad, &t);
    REFUSED(U, -EINVAL, b, g_pages, g_first, g_lens, NCH, PB, g_crc, NULL, &md5[0][0], NULL, 0, &nbad, &t);
    REFUSED(U, -EINVAL, b, g_pages, g_first, g_lens, NCH, PB, g_crc, ok, NULL, NULL, 0, &nbad, &t);
    REFUSED(U, -EINVAL, b, g_pages, g_first, g_lens, NCH, 64, g_crc, ok, &md5[0][0], NULL, 0, &nbad, &t);
    REFUSED(U, 0, b, NULL, NULL, NULL, 0, 0, NULL, NULL, NULL, NULL, 0, &nbad, &t);
    uint64_t first[NCH + 1];
    memcpy(first, g_first, sizeof first);
    first[50] = first[49] - 1;                                                          /* decreasing */
    REFUSED(V, -EINVAL, b, g_pages, first, g_lens, NCH, PB, g_md5, ok, 0, NULL, 0, &nbad, &t);
    static uint64_t pages[NCH * MAXPG];
    memcpy(pages, g_pages, sizeof pages);
    pages[g_first[20]] = 0;                                                             /* a NULL page that is read */
    CHECK(g_lens[20] > 0, "block 20 reads a page");
    REFUSED(V, -EINVAL, b, pages, g_first, g_lens, NCH, PB, g_md5, ok, 0, NULL, 0, &nbad, &t);
    /* -EINVAL wins over -E2BIG, -E2BIG over -ENOMEM: one block of more
     * entries than a slot's table (MD5HIP_PAGES_PER_SLOT(256) = 65,536) */
    enum { HUGE_ENTS = 65537 };
    uint64_t *pg = malloc(8 * HUGE_ENTS);
    CHECK(pg != NULL, "malloc");
    for (int e = 0; e < HUGE_ENTS; e++) pg[e] = (uint64_t)(uintptr_t)g_heap;
    const uint64_t hfirst[2] = {0, HUGE_ENTS};
    const uint32_t hlen = HUGE_ENTS * 128u;
    REFUSED(V, -EINVAL, b, pg, hfirst, &hlen, 1, 128, NULL, ok, 0, NULL, 0, &nbad, &t);
    __atomic_store_n(&g_fail_host_alloc, 1, __ATOMIC_RELAXED);
    REFUSED(V, -E2BIG, b, pg, hfirst, &hlen, 1, 128, g_md5, ok, 0, NULL, 0, &nbad, &t);
    REFUSED(U, -E2BIG, b, pg, hfirst, &hlen, 1, 128, g_crc, ok, &md5[0][0], NULL, 0, &nbad, &t);
    CHECK(__atomic_load_n(&g_fail_host_alloc, __ATOMIC_RELAXED) == 1 && g_dev_allocs == d0 && g_host_allocs == h0, "a refused call allocated");
    free(pg);
    /* the buffers cannot be had: -ENOMEM, nothing enqueued; the next call allocates them */
    REFUSED(V, -ENOMEM, b, g_pages, g_first, g_lens, NCH, PB, g_md5, ok, 0, NULL, 0, &nbad, &t);
    md5hip_batcher_get_stats(b, &s1);
    CHECK(fake_pages_launches + fake_pages_fast_launches == l0 && fake_compare_launches == c0 && s1.launches == s0.launches &&
              s1.submissions == s0.submissions && all_are(ok, sizeof ok, 0x5A) && nbad == 0,
          "a refused call was enqueued or delivered");
    /* the page tables (one pinned, one device allocation) and the verify
     * buffers (two and two), each by the first call that needs them */
    unsigned long h1 = g_host_allocs, d1 = g_dev_allocs;
    unsigned char out[16 * NCH];
    CHECK(md5_batch_submit_device_pages(b, g_pages, g_first, g_lens, NCH, PB, out, 0, NULL, 0, NULL) == 0 && !memcmp(out, g_md5, sizeof out), "paged submit");
    CHECK(g_host_allocs - h1 == 1 && g_dev_allocs - d1 == 1, "%lu pinned and %lu device allocations by the first paged call", g_host_allocs - h1, g_dev_allocs - d1);
    CHECK(md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_md5, ok, 0, NULL, 0, &nbad, NULL) == 0 && nbad == 0 && all_are(ok, NCH, 1),
          "first paged verify");
    CHECK(g_host_allocs - h1 == 3 && g_dev_allocs - d1 == 3, "%lu pinned and %lu device allocations after the first verify", g_host_allocs - h1, g_dev_allocs - d1);
    for (int k = 0; k < 4; k++) {
        CHECK(md5hip_batcher_set_digest(b, g_kinds[k].kind, g_kinds[k].fastcrc) == 0, "set_digest");
        CHECK(md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_kinds[k].right, ok, 0, NULL, 0, &nbad, NULL) == 0 && nbad == 0, "verify %d", k);
        CHECK(md5_batch_upgrade_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_crc, ok, &md5[0][0], NULL, 0, &nbad, NULL) == 0 && nbad == 0, "upgrade %d", k);
        CHECK(md5_batch_verify_device(b, g_dptr, g_lens, NCH, g_kinds[k].right, ok, 0, NULL, 0, &nbad, NULL) == 0 && nbad == 0, "device verify %d", k);
    }
    CHECK(g_host_allocs - h1 == 3 && g_dev_allocs - d1 == 3, "later calls allocated");
    md5hip_batcher_destroy(b);
    /* a batcher whose first paged call is a verify: all six at once */
    CHECK(md5hip_queue_create(2, 256, 3, &b) == 0, "create");
    h1 = g_host_allocs, d1 = g_dev_allocs;
    CHECK(md5_batch_upgrade_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_crc, ok, &md5[0][0], NULL, 0, &nbad, NULL) == 0 && nbad == 0, "upgrade first");
    CHECK(g_host_allocs - h1 == 3 && g_dev_allocs - d1 == 3, "allocations of a first call that verifies");
    md5hip_batcher_destroy(b);
    printf("buffers: page tables and verify buffers each allocated once; refusals in order: -EINVAL, -E2BIG, -ENOMEM, nothing enqueued, ticket zeroed\n");
    return 0;
}

static int failures(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(3, 0, 3, &b) == 0, "create");
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, FW) == 0, "set_digest");
    unsigned char ok[NCH], md5[NCH][16];
    uint64_t t = 0, nbad = 9;
    int rc;
    extern int fake_pages_fast_fail_next;
    /* a hash launch, then a compare launch, that fails on a healthy device */
    for (int which = 0; which < 2; which++) {
        memset(ok, 0x5A, sizeof ok);
        __atomic_store_n(which ? &fake_compare_fail_next : &fake_pages_fast_fail_next, 1, __ATOMIC_RELAXED);
        CHECK((rc = md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_win, ok, 0, NULL, 0, &nbad, &t)) == 0, "submit %d", rc);
        CHECK((rc = md5_batch_wait(b, t)) == -EIO && all_are(ok, sizeof ok, 0x5A) && nbad == 0, "failed launch %d: %d, nbad %llu", which, rc, (unsigned long long)nbad);
        CHECK(md5hip_batcher_health(b) == 0, "healthy after a failed launch");
        CHECK(md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_win, ok, 0, NULL, 0, &nbad, NULL) == 0 && nbad == 0 && all_are(ok, NCH, 1), "after it");
    }
    memset(ok, 0x5A, sizeof ok);
    memset(md5, 0x5A, sizeof md5);
    __atomic_store_n(&fake_pages_fail_next, 1, __ATOMIC_RELAXED);
    CHECK(md5_batch_upgrade_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_crc, ok, &md5[0][0], NULL, 0, &nbad, NULL) == -EIO, "failed upgrade");
    CHECK(all_are(ok, sizeof ok, 0x5A) && all_are(md5, sizeof md5, 0x5A) && nbad == 0, "a failed upgrade delivered");
    /* the injected device fault: -EIO, nothing delivered, then -ENODEV at once */
    CHECK(md5hip_batcher_inject_fault(b, 1) == 0, "inject");
    CHECK((rc = md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_win, ok, 0, NULL, 0, &nbad, &t)) == 0, "submit %d", rc);
    CHECK((rc = md5_batch_wait(b, t)) == -EIO && all_are(ok, sizeof ok, 0x5A) && nbad == 0, "the faulted launch's ticket %d", rc);
    CHECK(md5hip_batcher_health(b) == -ENODEV, "failed");
    const unsigned long l0 = fake_pages_fast_launches + fake_pages_launches;
    t = 9;
    CHECK((rc = md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_win, ok, 0, NULL, 0, &nbad, &t)) == -ENODEV && t == 0, "later %d", rc);
    CHECK((rc = md5_batch_upgrade_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_crc, ok, &md5[0][0], NULL, 0, &nbad, &t)) == -ENODEV && t == 0, "later upgrade %d", rc);
    CHECK(fake_pages_fast_launches + fake_pages_launches == l0 && all_are(ok, sizeof ok, 0x5A) && nbad == 0, "a failed device was used");
    md5hip_batcher_destroy(b);
    printf("failures: failed hash launch and failed compare -EIO, injected fault -EIO then -ENODEV, nothing delivered\n");
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
        unsigned char dig[16 * 40], exp[16 * 40], ok[40];
        uint64_t first[41], t = 0, nbad = 9, want_bad = 0;
        int rc, good = 1;
        const int what = (int)(rnd(&s) % 4), flip = (int)(rnd(&s) % (unsigned)n);
        memcpy(exp, g_md5[lo], 16 * (size_t)n);
        memcpy(first, g_first + lo, 8 * ((size_t)n + 1));
        memset(ok, 0xAA, sizeof ok);
        switch (what) {
        case 0:
        case 1:                                     /* a paged verify with one wrong value, synchronous or by ticket */
            exp[16 * flip + 3] ^= 0x40;
            want_bad = 1;
            rc = md5_batch_verify_device_pages(g_b, g_pages, first, g_lens + lo, (uint64_t)n, PB, exp, ok, 0, NULL, 0, &nbad, what ? &t : NULL);
            memset(first, 0xEE, sizeof first);
            memset(exp, 0xEE, sizeof exp);
            if (!rc && what) rc = md5_batch_wait(g_b, t);
            for (int i = 0; i < n; i++) good &= ok[i] == (i != flip);
            break;
        case 2:                                     /* a paged submission */
            rc = md5_batch_submit_device_pages(g_b, g_pages, first, g_lens + lo, (uint64_t)n, PB, dig, 0, NULL, 0, &t);
            if (!rc) rc = md5_batch_wait(g_b, t);
            good = !memcmp(dig, g_md5[lo], 16 * (size_t)n);
            nbad = 0;
            break;
        default:                                    /* a device verify, all right */
            rc = md5_batch_verify_device(g_b, g_dptr + lo, g_lens + lo, (uint64_t)n, exp, ok, 0, NULL, 0, &nbad, &t);
            if (!rc) rc = md5_batch_wait(g_b, t);
            good = all_are(ok, (size_t)n, 1);
            break;
        }
        if (rc || !good || nbad != want_bad) {
            printf("FAIL worker: what %d lo %d n %d rc %d nbad %llu\n", what, lo, n, rc, (unsigned long long)nbad);
            __atomic_store_n(&g_thread_fail, 1, __ATOMIC_RELAXED);
        }
    }
    return NULL;
}

static int threads(void)
{
    CHECK(md5hip_queue_create(0, 16, 3, &g_b) == 0, "create");       /* 16 per slot: paged calls cut into slices */
    pthread_t th[8];
    for (uintptr_t k = 0; k < 8; k++) CHECK(pthread_create(&th[k], NULL, worker, (void *)k) == 0, "thread");
    for (int k = 0; k < 8; k++) pthread_join(th[k], NULL);
    md5hip_batcher_destroy(g_b);
    CHECK(!g_thread_fail, "a worker failed");
    printf("threads: 8 threads x 60 rounds of paged verifies, paged submissions and device verifies on one batcher\n");
    return 0;
}
#else  /* NO_FAST: the window launcher is absent */
static int refusals(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_queue_create(0, 0, 3, &b) == 0, "create");
    /* the other kinds verify, and the upgrade works */
    for (int k = 0; k < 4; k++)
        if (k != 2 && verify_kind(b, &g_kinds[k])) return 1;
    if (upgrade(b)) return 1;
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, FW) == 0, "set_digest");
    struct md5hip_batcher_stats s0, s1;
    md5hip_batcher_get_stats(b, &s0);
    const unsigned long d0 = g_dev_allocs, h0 = g_host_allocs, l0 = fake_pages_launches, c0 = fake_compare_launches;
    unsigned char ok[NCH];
    uint64_t t = 9, nbad = 9;
    int rc;
    memset(ok, 0xAA, sizeof ok);
    CHECK((rc = md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_win, ok, 0, NULL, 0, &nbad, &t)) == -ENOSYS && t == 0 && nbad == 0, "by ticket %d", rc);
    CHECK((rc = md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_win, ok, 0, NULL, 0, &nbad, NULL)) == -ENOSYS, "synchronous %d", rc);
    /* -EINVAL first, -ENOSYS before -E2BIG */
    t = 9;
    CHECK((rc = md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, 192, g_win, ok, 0, NULL, 0, &nbad, &t)) == -EINVAL && t == 0, "page rule %d", rc);
    enum { HUGE_ENTS = 65537 };
    uint64_t *pg = malloc(8 * HUGE_ENTS);
    CHECK(pg != NULL, "malloc");
    for (int e = 0; e < HUGE_ENTS; e++) pg[e] = (uint64_t)(uintptr_t)g_heap;
    const uint64_t hfirst[2] = {0, HUGE_ENTS};
    const uint32_t hlen = HUGE_ENTS * 128u;
    t = 9;
    CHECK((rc = md5_batch_verify_device_pages(b, pg, hfirst, &hlen, 1, 128, g_win, ok, 0, NULL, 0, &nbad, &t)) == -ENOSYS && t == 0, "too big, no launcher %d", rc);
    free(pg);
    md5hip_batcher_get_stats(b, &s1);
    CHECK(all_are(ok, sizeof ok, 0xAA) && s1.launches == s0.launches && s1.submissions == s0.submissions && g_dev_allocs == d0 &&
              g_host_allocs == h0 && fake_pages_launches == l0 && fake_compare_launches == c0, "something was enqueued or allocated");
    /* whole-block CRC-32 still verifies on the same batcher */
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, 0) == 0, "set_digest");
    CHECK(md5_batch_verify_device_pages(b, g_pages, g_first, g_lens, NCH, PB, g_crc, ok, 0, NULL, 0, &nbad, NULL) == 0 && nbad == 0 && all_are(ok, NCH, 1), "CRC-32 after");
    md5hip_batcher_destroy(b);
    printf("refusals: without the window launcher a paged verify under a window is -ENOSYS, after -EINVAL and before -E2BIG; the other kinds verify\n");
    return 0;
}
#endif

int main(int argc, char **argv)
{
    setvbuf(stdout, NULL, _IOLBF, 0);
    if (setup()) return 2;
#ifndef NO_FAST
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
    printf("pages verify ok\n");
    return 0;
}
