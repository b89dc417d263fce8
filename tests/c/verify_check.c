/*
 * verify_check.c -- TEST: the asynchronous verify / upgrade entries (digests
 * compared on the device) through the batcher and the pool with no device.
 * Links md5_submit.c, md5_pool.c, md5_stream.c and nc_digest.c against the
 * fake runtime (fake_hip.c), the MD5_CRC32 stand-ins (fake_dual.c) and the
 * CPU stand-in for the compare launcher (fake_compare.c):
 *   - every kind (MD5, CRC-32 with fastcrc 0 and 64, MD5_CRC32 whole records,
 *     upgrade), page lists and device-resident chunks with host and "device"
 *     expected / ok, results against the library's host MD5 / nc_crc32; the
 *     caller's expected array is overwritten as soon as the call returns;
 *   - five verify tickets and two digest tickets coalesced behind a held
 *     launch: ONE compare launch, every ticket its own results; a slot
 *     without verify segments: none;
 *   - a slot whose host segments are all verify copies no digests back (the
 *     fake runtime's copy log);
 *   - a submission over three slots and more: nbad summed;
 *   - a pool, whole and split, mismatches in every part;
 *   - a failed compare launch and a device lost after launch 2: -EIO /
 *     -ENODEV, ok and md5_out untouched, nothing added to nbad.
 * `verify_check threads`: 8 threads mix async verifies, upgrades and plain
 * submissions on one batcher and one pool (ThreadSanitizer).
 * Built with -DNO_COMPARE and without fake_compare.c the launcher is absent:
 * every new entry returns -ENOSYS with nothing enqueued, the old ones work.
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
#include "../../sproxy_amd/csrc/md5_internal.h"

#define NCH 300
#define CHECK(c, ...)                                        \
    do {                                                     \
        if (!(c)) {                                          \
            printf("FAIL %s:%d: ", __func__, __LINE__);      \
            printf(__VA_ARGS__);                             \
            printf("\n");                                    \
            return 1;                                        \
        }                                                    \
    } while (0)

extern int fake_hip_hold;
extern FILE *fake_hip_log;
#ifndef NO_COMPARE
extern unsigned long fake_compare_launches, fake_compare_entries;
extern int fake_compare_fail_next;
#endif

static unsigned char *g_heap;
static uint64_t g_offs[NCH];
static uint32_t g_lens[NCH];
static unsigned char g_rec[NCH][32], g_md5[NCH][16];
static uint32_t g_crc[NCH], g_crc64[NCH];
static struct md5hip_iov g_segs[3 * NCH];
static uint64_t g_first[NCH + 1];
static uint64_t g_dptr[NCH];

static uint64_t rnd(uint64_t *s)
{
    *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17;
    return *s;
}

static uint32_t blk_crc(const unsigned char *p, uint32_t len, uint32_t F)
{
    if (F == 0 || len <= F) return nc_crc32(p, len);
    return nc_crc32(p, F) ^ nc_crc32(p + (len - F), F);
}

static int setup(void)
{
    uint64_t s = 0x9E3779B97F4A7C15ull, total = 0;
    for (int i = 0; i < NCH; i++) {
        g_lens[i] = i == 7 ? 0u : i == 8 ? 64u : 1u + (uint32_t)(rnd(&s) % 40000u);
        g_offs[i] = total;
        total += g_lens[i];
    }
    g_heap = malloc(total + 16);
    if (!g_heap) return 1;
    for (uint64_t k = 0; k < total; k++) g_heap[k] = (unsigned char)(rnd(&s) >> 24);
    uint64_t k = 0;
    for (int i = 0; i < NCH; i++) {
        const unsigned char *p = g_heap + g_offs[i];
        struct MD5Context c;
        MD5Init(&c);
        MD5Update(&c, p, g_lens[i]);
        MD5Final(g_md5[i], &c);
        g_crc[i] = nc_crc32(p, g_lens[i]);
        g_crc64[i] = blk_crc(p, g_lens[i], 64);
        memset(g_rec[i], 0, 32);
        memcpy(g_rec[i], g_md5[i], 16);
        for (int q = 0; q < 4; q++) g_rec[i][16 + q] = (unsigned char)(g_crc[i] >> (8 * q));
        g_dptr[i] = (uint64_t)(uintptr_t)p;
        g_first[i] = k;                                  /* chunk i in 1 + i % 3 segments */
        const uint32_t parts = 1u + (uint32_t)i % 3u, L = g_lens[i];
        uint32_t at = 0;
        for (uint32_t q = 0; q < parts; q++) {
            const uint32_t l = q + 1 == parts ? L - at : L / parts;
            g_segs[k++] = (struct md5hip_iov){g_heap + g_offs[i] + at, l};
            at += l;
        }
    }
    g_first[NCH] = k;
    return 0;
}

static int is_bad(int i) { return i == 0 || i == 63 || i == 64 || i == NCH - 1 || i % 37 == 5; }
static int nbad_in(int lo, int hi)
{
    int c = 0;
    for (int i = lo; i < hi; i++) c += is_bad(i);
    return c;
}

/* `dsz` bytes per chunk of the right values of chunks [lo, hi), chunk i's last byte flipped where is_bad(i) */
static void make_expected(unsigned char *e, const void *right, uint32_t dsz, int lo, int hi)
{
    memcpy(e, (const unsigned char *)right + (size_t)dsz * lo, (size_t)dsz * (hi - lo));
    for (int i = lo; i < hi; i++)
        if (is_bad(i)) e[(size_t)dsz * (i - lo) + dsz - 1] ^= 0x40;
}

static int ok_right(const unsigned char *ok, int lo, int hi)
{
    for (int i = lo; i < hi; i++)
        if (ok[i - lo] != !is_bad(i)) return 0;
    return 1;
}

static int all_are(const unsigned char *p, size_t bytes, unsigned char v)
{
    for (size_t k = 0; k < bytes; k++)
        if (p[k] != v) return 0;
    return 1;
}

#ifndef NO_COMPARE
#define SENTINEL 0xAAAAAAAAAAAAAAAAull

/* one async verify of chunks [0, NCH) under the batcher's kind, expected overwritten after the call */
static int verify_once(md5hip_batcher *b, const void *right, uint32_t dsz, const char *what)
{
    unsigned char *e = malloc((size_t)dsz * NCH), ok[NCH + 2];
    CHECK(e, "alloc");
    make_expected(e, right, dsz, 0, NCH);
    memset(ok, 0xAA, sizeof ok);
    uint64_t nbad = SENTINEL, t = 0;
    int rc = md5hip_batch_verify_iov_async(b, g_segs, g_first, NCH, e, ok + 1, &nbad, &t);
    memset(e, 0xEE, (size_t)dsz * NCH);              /* the call copied it */
    CHECK(rc == 0 && t, "%s: submit %d", what, rc);
    CHECK((rc = md5_batch_wait(b, t)) == 0, "%s: wait %d", what, rc);
    CHECK(ok_right(ok + 1, 0, NCH) && ok[0] == 0xAA && ok[NCH + 1] == 0xAA, "%s: ok", what);
    CHECK(nbad == (uint64_t)nbad_in(0, NCH), "%s: nbad %llu", what, (unsigned long long)nbad);
    free(e);
    return 0;
}

static int kinds(void)
{
    md5hip_batcher *b;
    int rc;
    CHECK(md5hip_batcher_create(0, 1u << 20, 3, &b) == 0, "create");
    struct md5hip_batcher_stats s0, s1;
    md5hip_batcher_get_stats(b, &s0);
    if (verify_once(b, g_md5, 16, "MD5")) return 1;
    md5hip_batcher_get_stats(b, &s1);
    CHECK(s1.launches - s0.launches >= 3, "the submission spans %llu slots", (unsigned long long)(s1.launches - s0.launches));
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, 0) == 0, "CRC-32");
    if (verify_once(b, g_crc, 4, "CRC-32")) return 1;
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, 64) == 0, "fastcrc 64");
    if (verify_once(b, g_crc64, 4, "CRC-32 fastcrc 64")) return 1;
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 0) == 0, "MD5_CRC32");
    if (verify_once(b, g_rec, 32, "MD5_CRC32 records")) return 1;

    /* upgrade, whatever the batcher is set to (here CRC-32 with a window) */
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, 64) == 0, "window");
    uint32_t want[NCH];
    unsigned char ok[NCH], md5s[NCH][16];
    make_expected((unsigned char *)want, g_crc, 4, 0, NCH);
    memset(ok, 0xAA, sizeof ok);
    memset(md5s, 0xAA, sizeof md5s);
    uint64_t nbad = SENTINEL, t = 0;
    rc = md5hip_batch_upgrade_iov_async(b, g_segs, g_first, NCH, want, ok, &md5s[0][0], &nbad, &t);
    memset(want, 0xEE, sizeof want);
    CHECK(rc == 0 && t && md5_batch_wait(b, t) == 0, "upgrade %d", rc);
    CHECK(ok_right(ok, 0, NCH) && nbad == (uint64_t)nbad_in(0, NCH), "upgrade ok / nbad %llu", (unsigned long long)nbad);
    CHECK(memcmp(md5s, g_md5, sizeof g_md5) == 0, "upgrade: the MD5 of every block");
    int kind;
    uint32_t fc;
    CHECK(md5hip_batcher_get_digest(b, &kind, &fc) == 0 && kind == MD5HIP_DIGEST_CRC32 && fc == 64, "kind kept");

    /* device-resident chunks: expected / ok on the host, then both "on the device" (ok off any alignment),
     * asynchronous and synchronous (ticket NULL) */
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5, 0) == 0, "MD5");
    for (int on_dev = 0; on_dev < 2; on_dev++)
        for (int sync = 0; sync < 2; sync++) {
            unsigned char *e = malloc(16 * NCH + 1), okd[NCH + 3];
            CHECK(e, "alloc");
            make_expected(e + 1, g_md5, 16, 0, NCH);
            memset(okd, 0xAA, sizeof okd);
            nbad = SENTINEL;
            rc = md5_batch_verify_device(b, g_dptr, g_lens, NCH, e + 1, okd + 1, on_dev, NULL, sync, &nbad, sync ? NULL : &t);
            if (!on_dev) memset(e, 0xEE, 16 * NCH + 1);
            CHECK(rc == 0 && (sync || md5_batch_wait(b, t) == 0), "verify_device %d/%d: %d", on_dev, sync, rc);
            CHECK(ok_right(okd + 1, 0, NCH) && okd[0] == 0xAA && okd[NCH + 1] == 0xAA && nbad == (uint64_t)nbad_in(0, NCH),
                  "verify_device %d/%d: ok / nbad %llu", on_dev, sync, (unsigned long long)nbad);
            free(e);
        }

    /* arguments, *ticket zeroed and nothing enqueued */
    md5hip_batcher_get_stats(b, &s0);
    unsigned char e16[16 * NCH];
    t = 9;
    CHECK(md5hip_batch_verify_iov_async(NULL, g_segs, g_first, 1, e16, ok, &nbad, &t) == -EINVAL && t == 0, "NULL handle");
    t = 9;
    CHECK(md5hip_batch_verify_iov_async(b, g_segs, g_first, 1, NULL, ok, &nbad, &t) == -EINVAL && t == 0, "NULL expected");
    t = 9;
    CHECK(md5hip_batch_verify_iov_async(b, g_segs, g_first, 1, e16, NULL, &nbad, &t) == -EINVAL && t == 0, "NULL ok");
    CHECK(md5hip_batch_verify_iov_async(b, g_segs, g_first, 1, e16, ok, &nbad, NULL) == -EINVAL, "no ticket");
    t = 9;
    CHECK(md5hip_batch_verify_iov_async(b, NULL, g_first, 1, e16, ok, &nbad, &t) == -EINVAL && t == 0, "NULL segs");
    t = 9;
    CHECK(md5hip_batch_upgrade_iov_async(b, g_segs, g_first, 1, NULL, ok, &md5s[0][0], &nbad, &t) == -EINVAL && t == 0, "NULL want_crc");
    t = 9;
    CHECK(md5hip_batch_upgrade_iov_async(b, g_segs, g_first, 1, want, ok, NULL, &nbad, &t) == -EINVAL && t == 0, "NULL md5_out");
    CHECK(md5hip_batch_upgrade_iov_async(b, g_segs, g_first, 1, want, ok, &md5s[0][0], &nbad, NULL) == -EINVAL, "upgrade: no ticket");
    t = 9;
    CHECK(md5_batch_verify_device(b, NULL, g_lens, 1, e16, ok, 0, NULL, 0, &nbad, &t) == -EINVAL && t == 0, "NULL d_ptrs");
    t = 9;
    nbad = SENTINEL;
    CHECK(md5hip_batch_verify_iov_async(b, g_segs, g_first, 0, NULL, NULL, &nbad, &t) == 0 && t == 0 && nbad == 0, "empty");
    CHECK(md5_batch_wait(b, t) == 0, "ticket 0");
    md5hip_batcher_get_stats(b, &s1);
    CHECK(s1.submissions == s0.submissions && s1.launches == s0.launches, "a refused call enqueued something");
    md5hip_batcher_destroy(b);
    printf("kinds: MD5, CRC-32 (fastcrc 0, 64), MD5_CRC32, upgrade, device-resident; expected copied; several slots summed\n");
    return 0;
}

/* D2H copies in the fake runtime's log: how many, and the bytes of the last */
static void d2h_of(const char *log, unsigned *count, size_t *last)
{
    *count = 0;
    *last = 0;
    for (const char *p = log; (p = strstr(p, "copy|D2H|")); p += 9) {
        (*count)++;
        *last = (size_t)strtoull(p + 9, NULL, 10);
    }
}

static int coalesced(void)
{
    enum { NT = 7, PER = 8 };                        /* tickets 0-4 verify, 5-6 digests; PER chunks each */
    md5hip_batcher *b;
    int rc;
    CHECK(md5hip_batcher_create(0, 4u << 20, 3, &b) == 0, "create");
    CHECK(md5hip_batcher_set_inflight(b, 1) == 0 && md5hip_batcher_set_chain(b, 0) == 0, "knobs");
    unsigned char blk[16], e[NT][16 * PER], ok[NT][PER], dig[NT][16 * PER];
    uint64_t nbad[NT], t[NT], tb = 0;
    struct md5hip_batcher_stats s0, s1;
    md5hip_batcher_get_stats(b, &s0);
    const unsigned long c0 = fake_compare_launches, e0 = fake_compare_entries;
    __atomic_store_n(&fake_hip_hold, 1, __ATOMIC_RELAXED);
    CHECK(md5_batch_submit_iov_async(b, g_segs, g_first, 1, blk, &tb) == 0, "blocker");
    for (int r = 0; r < NT; r++) {
        const int lo = 60 + r * PER;                 /* chunks 63 and 64 are corrupted */
        make_expected(e[r], g_md5, 16, lo, lo + PER);
        memset(ok[r], 0xAA, PER);
        memset(dig[r], 0xAA, 16 * PER);
        nbad[r] = SENTINEL;
        /* a page list of its own for the range: seg_first re-based to 0 */
        uint64_t first[PER + 1];
        for (int i = 0; i <= PER; i++) first[i] = g_first[lo + i] - g_first[lo];
        rc = r < 5 ? md5hip_batch_verify_iov_async(b, g_segs + g_first[lo], first, PER, e[r], ok[r], &nbad[r], &t[r])
                   : md5_batch_submit_iov_async(b, g_segs + g_first[lo], first, PER, dig[r], &t[r]);
        CHECK(rc == 0 && t[r], "ticket %d: %d", r, rc);
        memset(e[r], 0xEE, sizeof e[r]);
    }
    CHECK(fake_compare_launches == c0, "a compare launch before the held launch ended");
    __atomic_store_n(&fake_hip_hold, 0, __ATOMIC_RELAXED);
    for (int r = NT - 1; r >= 0; r--) CHECK((rc = md5_batch_wait(b, t[r])) == 0, "wait %d: %d", r, rc);
    CHECK(md5_batch_wait(b, tb) == 0 && memcmp(blk, g_md5[0], 16) == 0, "blocker's digest");
    md5hip_batcher_get_stats(b, &s1);
    CHECK(s1.launches - s0.launches == 2, "launches %llu", (unsigned long long)(s1.launches - s0.launches));
    CHECK(fake_compare_launches - c0 == 1 && fake_compare_entries - e0 == 5, "%lu compare launches, %lu entries",
          fake_compare_launches - c0, fake_compare_entries - e0);
    for (int r = 0; r < NT; r++) {
        const int lo = 60 + r * PER;
        if (r < 5) {
            CHECK(ok_right(ok[r], lo, lo + PER) && nbad[r] == (uint64_t)nbad_in(lo, lo + PER), "ticket %d: ok / nbad %llu", r,
                  (unsigned long long)nbad[r]);
            CHECK(all_are(dig[r], 16 * PER, 0xAA), "ticket %d got digests", r);
        } else {
            CHECK(memcmp(dig[r], g_md5[lo], 16 * PER) == 0 && all_are(ok[r], PER, 0xAA) && nbad[r] == SENTINEL,
                  "digest ticket %d", r);
        }
    }
    /* a slot without verify segments: no compare launch */
    const unsigned long c1 = fake_compare_launches;
    CHECK(md5_batch_submit_iov(b, g_segs, g_first, 20, &dig[0][0]) == 0, "plain");
    CHECK(fake_compare_launches == c1, "a compare launch for a slot without verify segments");

    /* all host segments verify: ONE copy back, of the counts and ok bytes -- no digests */
    char *log = NULL;
    size_t logsz = 0;
    FILE *f = open_memstream(&log, &logsz);
    CHECK(f, "memstream");
    make_expected(e[0], g_md5, 16, 60, 60 + PER);
    uint64_t first[PER + 1];
    for (int i = 0; i <= PER; i++) first[i] = g_first[60 + i] - g_first[60];
    fake_hip_log = f;
    rc = md5hip_batch_verify_iov_async(b, g_segs + g_first[60], first, PER, e[0], ok[0], &nbad[0], &t[0]);
    CHECK(rc == 0 && md5_batch_wait(b, t[0]) == 0, "verify %d", rc);
    unsigned n1, n2;
    size_t last;
    fflush(f);
    d2h_of(log, &n1, &last);
    CHECK(n1 == 1 && last == 8 + PER, "%u copies back, the last of %zu bytes", n1, last);
    /* an upgrade needs its MD5s: the record copy as today, beside the ok copy */
    uint32_t want[PER];
    unsigned char md5s[PER][16];
    memcpy(want, g_crc + 60, sizeof want);
    rc = md5hip_batch_upgrade_iov_async(b, g_segs + g_first[60], first, PER, want, ok[0], &md5s[0][0], &nbad[0], &t[0]);
    CHECK(rc == 0 && md5_batch_wait(b, t[0]) == 0 && nbad[0] == 0 && memcmp(md5s, g_md5[60], sizeof md5s) == 0, "upgrade %d", rc);
    fflush(f);
    d2h_of(log, &n2, &last);
    CHECK(n2 - n1 == 2 && last == 32 * PER, "upgrade: %u copies back, the last of %zu bytes", n2 - n1, last);
    fake_hip_log = NULL;
    md5hip_batcher_destroy(b);
    fclose(f);
    free(log);
    printf("coalesced: 5 verify + 2 digest tickets in one launch, 1 compare launch; no digest copy for verify-only slots\n");
    return 0;
}

static int pool_paths(void)
{
    const int devs[2] = {0, 1};
    md5hip_pool *p;
    int rc;
    CHECK(md5hip_pool_create(devs, 2, 1u << 20, 3, &p) == 0, "pool create");
    for (int split = 0; split < 2; split++) {
        CHECK(md5hip_pool_set_split(p, split ? 64u << 10 : 1ull << 40) == 0, "set_split");
        CHECK(md5hip_pool_set_digest(p, MD5HIP_DIGEST_MD5, 0) == 0, "MD5");
        unsigned char e[16 * NCH], ok[NCH], md5s[NCH][16];
        uint32_t want[NCH];
        uint64_t nbad = SENTINEL, t = 0;
        make_expected(e, g_md5, 16, 0, NCH);
        memset(ok, 0xAA, sizeof ok);
        rc = md5hip_pool_verify_iov_async(p, g_segs, g_first, NCH, e, ok, &nbad, &t);
        memset(e, 0xEE, sizeof e);
        CHECK(rc == 0 && t && (rc = md5hip_pool_wait(p, t)) == 0, "pool verify %d", rc);
        CHECK(ok_right(ok, 0, NCH) && nbad == (uint64_t)nbad_in(0, NCH), "pool verify ok / nbad %llu", (unsigned long long)nbad);
        make_expected((unsigned char *)want, g_crc, 4, 0, NCH);
        memset(ok, 0xAA, sizeof ok);
        memset(md5s, 0xAA, sizeof md5s);
        nbad = SENTINEL;
        rc = md5hip_pool_upgrade_iov_async(p, g_segs, g_first, NCH, want, ok, &md5s[0][0], &nbad, &t);
        memset(want, 0xEE, sizeof want);
        CHECK(rc == 0 && t, "pool upgrade %d", rc);
        while ((rc = md5hip_pool_poll(p, t)) == 0) ;
        CHECK(rc == 1, "pool upgrade poll %d", rc);
        CHECK(ok_right(ok, 0, NCH) && nbad == (uint64_t)nbad_in(0, NCH) && memcmp(md5s, g_md5, sizeof g_md5) == 0,
              "pool upgrade ok / nbad %llu / md5", (unsigned long long)nbad);
        struct md5hip_pool_stats ps;
        md5hip_pool_get_stats(p, &ps);
        CHECK(split ? ps.split >= 2 : ps.split == 0, "split submissions: %llu", (unsigned long long)ps.split);
        t = 9;
        CHECK(md5hip_pool_verify_iov_async(p, g_segs, g_first, 1, NULL, ok, &nbad, &t) == -EINVAL && t == 0, "NULL expected");
        t = 9;
        CHECK(md5hip_pool_upgrade_iov_async(p, g_segs, g_first, 1, want, ok, NULL, &nbad, &t) == -EINVAL && t == 0, "NULL md5_out");
        CHECK(md5hip_pool_verify_iov_async(p, g_segs, g_first, 1, e, ok, &nbad, NULL) == -EINVAL, "no ticket");
        CHECK(md5hip_pool_verify_iov_async(NULL, g_segs, g_first, 1, e, ok, &nbad, &t) == -EINVAL, "NULL pool");
        nbad = SENTINEL;
        CHECK(md5hip_pool_verify_iov_async(p, g_segs, g_first, 0, NULL, NULL, &nbad, &t) == 0 && t == 0 && nbad == 0, "empty");
    }
    md5hip_pool_destroy(p);
    printf("pool: whole and split verify and upgrade, mismatches in every part, one nbad\n");
    return 0;
}

static int failures(void)
{
    enum { NS = 20 };
    md5hip_batcher *b;
    int rc;
    CHECK(md5hip_batcher_create(2, 1u << 20, 3, &b) == 0, "create");
    unsigned char e[16 * NS], ok[NS], md5s[NS][16];
    uint32_t want[NS];
    uint64_t nbad, t = 0;
    make_expected(e, g_md5, 16, 0, NS);
    make_expected((unsigned char *)want, g_crc, 4, 0, NS);
#define FRESH() (memset(ok, 0xAA, sizeof ok), memset(md5s, 0xAA, sizeof md5s), nbad = SENTINEL)
#define CLEAN() (all_are(ok, sizeof ok, 0xAA) && all_are(&md5s[0][0], sizeof md5s, 0xAA) && nbad == 0)
    /* a compare launch that fails on a healthy device: the ticket -EIO, nothing delivered, the batcher usable */
    FRESH();
    __atomic_store_n(&fake_compare_fail_next, 1, __ATOMIC_RELAXED);
    CHECK((rc = md5hip_batch_upgrade_iov_async(b, g_segs, g_first, NS, want, ok, &md5s[0][0], &nbad, &t)) == 0, "submit %d", rc);
    CHECK((rc = md5_batch_wait(b, t)) == -EIO, "failed compare launch %d", rc);
    CHECK(CLEAN(), "a failed launch delivered something (nbad %llu)", (unsigned long long)nbad);
    CHECK(md5hip_batcher_health(b) == 0, "healthy after a failed launch");
    FRESH();
    CHECK(md5hip_batch_verify_iov_async(b, g_segs, g_first, NS, e, ok, &nbad, &t) == 0 && md5_batch_wait(b, t) == 0 &&
              ok_right(ok, 0, NS) && nbad == (uint64_t)nbad_in(0, NS), "after it");
    /* the device lost after launch 2: launch 1 right, launch 2 -EIO, then -ENODEV at once */
    CHECK(md5hip_batcher_inject_fault(b, 2) == 0, "inject");
    FRESH();
    CHECK(md5hip_batch_verify_iov_async(b, g_segs, g_first, NS, e, ok, &nbad, &t) == 0 && md5_batch_wait(b, t) == 0 &&
              ok_right(ok, 0, NS) && nbad == (uint64_t)nbad_in(0, NS), "launch 1");
    FRESH();
    CHECK((rc = md5hip_batch_upgrade_iov_async(b, g_segs, g_first, NS, want, ok, &md5s[0][0], &nbad, &t)) == 0, "launch 2 submit %d", rc);
    CHECK((rc = md5_batch_wait(b, t)) == -EIO, "launch 2's ticket %d", rc);
    CHECK(CLEAN(), "the lost launch delivered something");
    CHECK(md5hip_batcher_health(b) == -ENODEV, "failed");
    const unsigned long c0 = fake_compare_launches;
    t = 9;
    CHECK((rc = md5hip_batch_verify_iov_async(b, g_segs, g_first, NS, e, ok, &nbad, &t)) == -ENODEV && t == 0, "later verify %d", rc);
    t = 9;
    CHECK((rc = md5hip_batch_upgrade_iov_async(b, g_segs, g_first, NS, want, ok, &md5s[0][0], &nbad, &t)) == -ENODEV && t == 0,
          "later upgrade %d", rc);
    CHECK((rc = md5_batch_verify_device(b, g_dptr, g_lens, NS, e, ok, 0, NULL, 0, &nbad, NULL)) == -ENODEV, "later device %d", rc);
    CHECK(CLEAN() && fake_compare_launches == c0, "a failed device was used");
    md5hip_batcher_destroy(b);

    /* a pool of one device losing it */
    const int dev = 3;
    md5hip_pool *p;
    CHECK(md5hip_pool_create(&dev, 1, 1u << 20, 3, &p) == 0, "pool create");
    FRESH();
    CHECK(md5hip_pool_verify_iov_async(p, g_segs, g_first, NS, e, ok, &nbad, &t) == 0 && md5hip_pool_wait(p, t) == 0 &&
              ok_right(ok, 0, NS), "pool healthy");
    CHECK(md5hip_pool_inject_fault(p, 0, 1) == 0, "pool inject");
    FRESH();
    CHECK((rc = md5hip_pool_upgrade_iov_async(p, g_segs, g_first, NS, want, ok, &md5s[0][0], &nbad, &t)) == 0, "pool submit %d", rc);
    CHECK((rc = md5hip_pool_wait(p, t)) == -EIO, "pool: the lost launch's ticket %d", rc);
    CHECK(CLEAN(), "pool: the lost launch delivered something");
    CHECK((rc = md5hip_pool_verify_iov_async(p, g_segs, g_first, NS, e, ok, &nbad, &t)) == -ENODEV && t == 0 && CLEAN(),
          "pool later %d", rc);
    md5hip_pool_destroy(p);
    printf("failures: failed compare launch -EIO, device lost after launch 2 -EIO / -ENODEV, nothing delivered\n");
    return 0;
}

/* ---- `threads`: 8 threads on one batcher and one pool */
static md5hip_batcher *g_b;
static md5hip_pool *g_p;
static int g_thread_fail;

static void *worker(void *arg)
{
    uint64_t s = 0x1234567ull + (uint64_t)(uintptr_t)arg * 977u;
    for (int round = 0; round < 60 && !__atomic_load_n(&g_thread_fail, __ATOMIC_RELAXED); round++) {
        const int lo = (int)(rnd(&s) % (NCH - 40)), n = 1 + (int)(rnd(&s) % 40);
        uint64_t first[41];
        for (int i = 0; i <= n; i++) first[i] = g_first[lo + i] - g_first[lo];
        const struct md5hip_iov *segs = g_segs + g_first[lo];
        unsigned char e[16 * 40], ok[40], md5s[40][16], dig[16 * 40];
        uint32_t want[40];
        uint64_t nbad = SENTINEL, t = 0;
        int rc, good = 1;
        const int what = (int)(rnd(&s) % 5);
        make_expected(e, g_md5, 16, lo, lo + n);
        make_expected((unsigned char *)want, g_crc, 4, lo, lo + n);
        switch (what) {
        case 0:
            rc = md5hip_batch_verify_iov_async(g_b, segs, first, (uint64_t)n, e, ok, &nbad, &t);
            memset(e, 0xEE, sizeof e);
            if (!rc) rc = md5_batch_wait(g_b, t);
            good = ok_right(ok, lo, lo + n) && nbad == (uint64_t)nbad_in(lo, lo + n);
            break;
        case 1:
            rc = md5hip_batch_upgrade_iov_async(g_b, segs, first, (uint64_t)n, want, ok, &md5s[0][0], &nbad, &t);
            if (!rc) rc = md5_batch_wait(g_b, t);
            good = ok_right(ok, lo, lo + n) && nbad == (uint64_t)nbad_in(lo, lo + n) && !memcmp(md5s, g_md5[lo], 16 * (size_t)n);
            break;
        case 2:
            rc = md5_batch_submit_iov_async(g_b, segs, first, (uint64_t)n, dig, &t);
            if (!rc) rc = md5_batch_wait(g_b, t);
            good = !memcmp(dig, g_md5[lo], 16 * (size_t)n);
            break;
        case 3:
            rc = md5hip_pool_verify_iov_async(g_p, segs, first, (uint64_t)n, e, ok, &nbad, &t);
            if (!rc) rc = md5hip_pool_wait(g_p, t);
            good = ok_right(ok, lo, lo + n) && nbad == (uint64_t)nbad_in(lo, lo + n);
            break;
        default:
            rc = md5hip_pool_upgrade_iov_async(g_p, segs, first, (uint64_t)n, want, ok, &md5s[0][0], &nbad, &t);
            if (!rc) rc = md5hip_pool_wait(g_p, t);
            good = ok_right(ok, lo, lo + n) && nbad == (uint64_t)nbad_in(lo, lo + n) && !memcmp(md5s, g_md5[lo], 16 * (size_t)n);
            break;
        }
        if (rc || !good) {
            printf("FAIL worker: what %d lo %d n %d rc %d good %d\n", what, lo, n, rc, good);
            __atomic_store_n(&g_thread_fail, 1, __ATOMIC_RELAXED);
        }
    }
    return NULL;
}

static int threads(void)
{
    const int devs[2] = {0, 1};
    CHECK(md5hip_batcher_create(0, 1u << 20, 3, &g_b) == 0, "create");
    CHECK(md5hip_pool_create(devs, 2, 1u << 20, 3, &g_p) == 0 && md5hip_pool_set_split(g_p, 128u << 10) == 0, "pool");
    pthread_t th[8];
    for (uintptr_t k = 0; k < 8; k++) CHECK(pthread_create(&th[k], NULL, worker, (void *)k) == 0, "thread");
    for (int k = 0; k < 8; k++) pthread_join(th[k], NULL);
    md5hip_batcher_destroy(g_b);
    md5hip_pool_destroy(g_p);
    CHECK(!g_thread_fail, "a worker failed");
    printf("threads: 8 threads x 60 rounds of verify / upgrade / submit on one batcher and one pool\n");
    return 0;
}
#else  /* NO_COMPARE: the launcher is absent */
static int refusals(void)
{
    md5hip_batcher *b;
    const int devs[2] = {0, 1};
    md5hip_pool *p;
    int rc;
    CHECK(md5hip_batcher_create(0, 1u << 20, 3, &b) == 0 && md5hip_pool_create(devs, 2, 1u << 20, 3, &p) == 0, "create");
    struct md5hip_batcher_stats s0, s1;
    struct md5hip_pool_stats ps;
    md5hip_batcher_get_stats(b, &s0);
    unsigned char e[16 * NCH], ok[NCH], md5s[NCH][16];
    uint64_t nbad = 7, t = 9;
    make_expected(e, g_md5, 16, 0, NCH);
    memset(ok, 0xAA, sizeof ok);
    memset(md5s, 0xAA, sizeof md5s);
    CHECK((rc = md5hip_batch_verify_iov_async(b, g_segs, g_first, NCH, e, ok, &nbad, &t)) == -ENOSYS && t == 0, "verify %d", rc);
    t = 9;
    CHECK((rc = md5hip_batch_upgrade_iov_async(b, g_segs, g_first, NCH, g_crc, ok, &md5s[0][0], &nbad, &t)) == -ENOSYS && t == 0,
          "upgrade %d", rc);
    t = 9;
    CHECK((rc = md5_batch_verify_device(b, g_dptr, g_lens, NCH, e, ok, 0, NULL, 0, &nbad, &t)) == -ENOSYS && t == 0, "device %d", rc);
    CHECK((rc = md5_batch_verify_device(b, g_dptr, g_lens, NCH, e, ok, 0, NULL, 0, &nbad, NULL)) == -ENOSYS, "device sync %d", rc);
    t = 9;
    CHECK((rc = md5hip_pool_verify_iov_async(p, g_segs, g_first, NCH, e, ok, &nbad, &t)) == -ENOSYS && t == 0, "pool verify %d", rc);
    t = 9;
    CHECK((rc = md5hip_pool_upgrade_iov_async(p, g_segs, g_first, NCH, g_crc, ok, &md5s[0][0], &nbad, &t)) == -ENOSYS && t == 0,
          "pool upgrade %d", rc);
    CHECK(all_are(ok, sizeof ok, 0xAA) && all_are(&md5s[0][0], sizeof md5s, 0xAA), "a refused call wrote results");
    md5hip_batcher_get_stats(b, &s1);
    md5hip_pool_get_stats(p, &ps);
    CHECK(s1.launches == s0.launches && s1.submissions == s0.submissions && ps.submissions == 0, "something was enqueued");
    /* the old entries as before */
    CHECK((rc = md5hip_batch_verify_iov(b, g_segs, g_first, NCH, e, ok)) == nbad_in(0, NCH) && ok_right(ok, 0, NCH), "verify_iov %d", rc);
    CHECK((rc = md5hip_pool_verify_iov(p, g_segs, g_first, NCH, e, ok)) == nbad_in(0, NCH) && ok_right(ok, 0, NCH), "pool verify_iov %d", rc);
    CHECK((rc = md5hip_batch_upgrade_iov(b, g_segs, g_first, NCH, g_crc, ok, &md5s[0][0])) == 0 && !memcmp(md5s, g_md5, sizeof g_md5),
          "upgrade_iov %d", rc);
    uint64_t tk = 0;
    CHECK(md5_batch_submit_iov_async(b, g_segs, g_first, NCH, &md5s[0][0], &tk) == 0 && md5_batch_wait(b, tk) == 0 &&
              !memcmp(md5s, g_md5, sizeof g_md5), "submit_iov_async");
    md5hip_batcher_destroy(b);
    md5hip_pool_destroy(p);
    printf("refusals: without the compare launcher every new entry is -ENOSYS, nothing enqueued, the old entries work\n");
    return 0;
}
#endif

int main(int argc, char **argv)
{
    setvbuf(stdout, NULL, _IOLBF, 0);
    if (setup()) return 2;
#ifndef NO_COMPARE
    if (argc > 1 && !strcmp(argv[1], "threads")) {
        if (threads()) return 1;
    } else if (kinds() || coalesced() || pool_paths() || failures()) {
        return 1;
    }
#else
    (void)argc;
    (void)argv;
    if (refusals()) return 1;
#endif
    free(g_heap);
    printf("verify ok\n");
    return 0;
}
