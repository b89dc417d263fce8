/*
 * dual_check.c -- TEST: the MD5_CRC32 digest kind (one pass, 32-byte records)
 * through the batcher and the pool with no device.  Links md5_submit.c,
 * md5_pool.c, md5_stream.c and nc_digest.c against the fake runtime
 * (fake_hip.c) and the CPU stand-ins for the two launchers (fake_dual.c):
 *   - every submit path under the kind, on a batcher and on a pool (host
 *     pointers, page lists, async, device-resident with host and device
 *     records, device_on / device_after, device_fixed, host_fixed pinned and
 *     pageable, a pool submission split over two devices);
 *   - kind switches MD5 -> both -> CRC-32 -> both on one handle, and async
 *     submissions of different kinds interleaved on one batcher;
 *   - verify_iov over whole records, upgrade_iov (stored CRC checked, MD5 of
 *     every block returned) whatever kind the handle is set to;
 *   - a failed launch and a device lost after launch K: -EIO / -ENODEV and no
 *     record written from a failed launch.
 * Built with -DNO_DUAL and without fake_dual.c, the launchers are absent and
 * set_digest / upgrade_iov must refuse the kind with -ENOSYS before anything
 * is enqueued, MD5 and CRC-32 working as before.
 */
#define _GNU_SOURCE
#include <errno.h>
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

extern unsigned long fake_dual_launches;
extern int fake_dual_fail_next;

static unsigned char *g_heap;
static uint64_t g_offs[NCH];
static uint32_t g_lens[NCH];
static unsigned char g_rec[NCH][32], g_md5[NCH][16];
static uint32_t g_crc[NCH];

static uint64_t rnd(uint64_t *s)
{
    *s ^= *s << 13; *s ^= *s >> 7; *s ^= *s << 17;
    return *s;
}

static void record_of(const unsigned char *p, uint32_t len, unsigned char *rec)
{
    struct MD5Context c;
    MD5Init(&c);
    MD5Update(&c, p, len);
    MD5Final(rec, &c);
    const uint32_t crc = nc_crc32(p, len);
    rec[16] = (unsigned char)crc; rec[17] = (unsigned char)(crc >> 8);
    rec[18] = (unsigned char)(crc >> 16); rec[19] = (unsigned char)(crc >> 24);
    memset(rec + 20, 0, 12);
}

static int setup(void)
{
    uint64_t s = 0x9E3779B97F4A7C15ull, total = 0;
    for (int i = 0; i < NCH; i++) {
        g_lens[i] = i == 7 ? 0u : 1u + (uint32_t)(rnd(&s) % 40000u);     /* one empty chunk */
        g_offs[i] = total;
        total += g_lens[i];
    }
    g_heap = malloc(total + 16);
    if (!g_heap) return 1;
    for (uint64_t k = 0; k < total; k++) g_heap[k] = (unsigned char)(rnd(&s) >> 24);
    for (int i = 0; i < NCH; i++) {
        record_of(g_heap + g_offs[i], g_lens[i], g_rec[i]);
        memcpy(g_md5[i], g_rec[i], 16);
        g_crc[i] = nc_crc32(g_heap + g_offs[i], g_lens[i]);
    }
    return 0;
}

/* the page list of chunks [0, NCH): chunk i in 1 + i % 3 segments */
static struct md5hip_iov g_segs[3 * NCH];
static uint64_t g_first[NCH + 1];
static void make_iov(void)
{
    uint64_t k = 0;
    for (int i = 0; i < NCH; i++) {
        g_first[i] = k;
        const uint32_t parts = 1u + (uint32_t)i % 3u, L = g_lens[i];
        uint32_t at = 0;
        for (uint32_t p = 0; p < parts; p++) {
            const uint32_t l = p + 1 == parts ? L - at : L / parts;
            g_segs[k++] = (struct md5hip_iov){g_heap + g_offs[i] + at, l};
            at += l;
        }
    }
    g_first[NCH] = k;
}

static int same(const void *got, const void *want, size_t bytes) { return memcmp(got, want, bytes) == 0; }
static int untouched(const unsigned char *p, size_t bytes)
{
    for (size_t k = 0; k < bytes; k++)
        if (p[k] != 0x5a) return 0;
    return 1;
}

#ifndef NO_DUAL
/* fixed-length chunks: NF of FL bytes every FS, records in g_frec */
enum { NF = 3000, FL = 1000, FS = 1003 };
static unsigned char g_frec[NF][32];

static int batcher_paths(void)
{
    md5hip_batcher *b;
    int rc = md5hip_batcher_create(0, 1u << 20, 3, &b);
    CHECK(rc == 0, "create %d", rc);
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 4) == -EINVAL, "kind 2 takes no fastcrc window");
    CHECK(md5hip_batcher_set_digest(b, 3, 0) == -EINVAL, "kind 3");
    CHECK((rc = md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 0)) == 0, "set_digest %d", rc);
    int kind = -1;
    uint32_t fc = 9;
    CHECK(md5hip_batcher_get_digest(b, &kind, &fc) == 0 && kind == MD5HIP_DIGEST_MD5_CRC32 && fc == 0, "get_digest");

    const void *ptrs[NCH];
    uint64_t dptrs[NCH];
    for (int i = 0; i < NCH; i++) {
        ptrs[i] = g_heap + g_offs[i];
        dptrs[i] = (uint64_t)(uintptr_t)ptrs[i];
    }
    unsigned char(*rec)[32] = aligned_alloc(16, sizeof g_rec);
    CHECK(rec, "alloc");
#define FRESH() memset(rec, 0x5a, sizeof g_rec)
    uint64_t t = 0;
    FRESH();
    CHECK((rc = md5_batch_submit(b, ptrs, g_lens, NCH, &rec[0][0])) == 0 && same(rec, g_rec, sizeof g_rec), "ptrs %d", rc);
    FRESH();
    CHECK((rc = md5_batch_submit_iov(b, g_segs, g_first, NCH, &rec[0][0])) == 0 && same(rec, g_rec, sizeof g_rec), "iov %d", rc);
    FRESH();
    CHECK((rc = md5_batch_submit_async(b, ptrs, g_lens, NCH, &rec[0][0], &t)) == 0 && t, "async %d", rc);
    CHECK((rc = md5_batch_wait(b, t)) == 0 && same(rec, g_rec, sizeof g_rec), "async wait %d", rc);
    FRESH();
    CHECK((rc = md5_batch_submit_iov_async(b, g_segs, g_first, NCH, &rec[0][0], &t)) == 0 && t, "iov async %d", rc);
    CHECK((rc = md5_batch_wait(b, t)) == 0 && same(rec, g_rec, sizeof g_rec), "iov async wait %d", rc);
    for (int on_dev = 0; on_dev < 2; on_dev++) {         /* records to the host, then left "on the device" */
        FRESH();
        CHECK((rc = md5_batch_submit_device(b, dptrs, g_lens, NCH, &rec[0][0], on_dev)) == 0 &&
                  same(rec, g_rec, sizeof g_rec), "device (records on device %d) %d", on_dev, rc);
        FRESH();
        CHECK((rc = md5_batch_submit_device_async(b, dptrs, g_lens, NCH, &rec[0][0], on_dev, &t)) == 0, "device async %d", rc);
        CHECK((rc = md5_batch_wait(b, t)) == 0 && same(rec, g_rec, sizeof g_rec), "device async wait %d", rc);
        FRESH();
        CHECK((rc = md5_batch_submit_device_on(b, dptrs, g_lens, NCH, &rec[0][0], on_dev, NULL, &t)) == 0, "device_on %d", rc);
        CHECK((rc = md5_batch_wait(b, t)) == 0 && same(rec, g_rec, sizeof g_rec), "device_on wait %d", rc);
        FRESH();
        CHECK((rc = md5_batch_submit_device_after(b, dptrs, g_lens, NCH, &rec[0][0], on_dev, NULL, 1, &t)) == 0,
              "device_after %d", rc);
        CHECK((rc = md5_batch_wait(b, t)) == 0 && same(rec, g_rec, sizeof g_rec), "device_after wait %d", rc);
        /* two device submissions in one slot: records on the device are scattered, not written in place */
        FRESH();
        uint64_t t2 = 0;
        CHECK((rc = md5_batch_submit_device_async(b, dptrs, g_lens, 100, &rec[0][0], on_dev, &t)) == 0, "part 1 %d", rc);
        CHECK((rc = md5_batch_submit_device_async(b, dptrs + 100, g_lens + 100, NCH - 100, &rec[100][0], on_dev, &t2)) == 0,
              "part 2 %d", rc);
        CHECK(md5_batch_wait(b, t2) == 0 && md5_batch_wait(b, t) == 0 && same(rec, g_rec, sizeof g_rec), "two parts");
    }
    free(rec);

    /* fixed-length: device-resident (records on the device and on the host), host pinned and pageable */
    unsigned char *fx = malloc((size_t)NF * FS), *pin = NULL;
    unsigned char(*frec)[32] = aligned_alloc(16, sizeof g_frec);
    CHECK(fx && frec && hipHostMalloc((void **)&pin, (size_t)NF * FS, 0) == hipSuccess, "alloc");
    uint64_t s = 5;
    for (size_t k = 0; k < (size_t)NF * FS; k++) fx[k] = (unsigned char)(rnd(&s) >> 32);
    memcpy(pin, fx, (size_t)NF * FS);
    for (int i = 0; i < NF; i++) record_of(fx + (size_t)i * FS, FL, g_frec[i]);
    for (int on_dev = 0; on_dev < 2; on_dev++) {
        memset(frec, 0x5a, sizeof g_frec);
        CHECK((rc = md5_batch_submit_device_fixed(b, fx, NF, FL, FS, &frec[0][0], on_dev, NULL, 0, &t)) == 0,
              "device_fixed %d", rc);
        CHECK((rc = md5_batch_wait(b, t)) == 0 && same(frec, g_frec, sizeof g_frec), "device_fixed wait %d", rc);
    }
    memset(frec, 0x5a, sizeof g_frec);
    CHECK((rc = md5hip_batch_host_fixed(b, pin, NF, FL, FS, &frec[0][0])) == 0 && same(frec, g_frec, sizeof g_frec),
          "host_fixed pinned %d", rc);
    memset(frec, 0x5a, sizeof g_frec);
    CHECK((rc = md5hip_batch_host_fixed(b, fx, NF, FL, FS, &frec[0][0])) == 0 && same(frec, g_frec, sizeof g_frec),
          "host_fixed pageable %d", rc);
    free(frec);
    free(fx);
    hipHostFree(pin);

    /* kind switches on one handle: MD5 -> both -> CRC-32 -> both */
    unsigned char(*out)[32] = malloc(sizeof g_rec);
    CHECK(out, "alloc");
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5, 0) == 0, "MD5");
    CHECK(md5_batch_submit(b, ptrs, g_lens, NCH, &out[0][0]) == 0 && same(out, g_md5, sizeof g_md5), "MD5 digests");
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 0) == 0, "both");
    CHECK(md5_batch_submit(b, ptrs, g_lens, NCH, &out[0][0]) == 0 && same(out, g_rec, sizeof g_rec), "records");
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, 0) == 0, "CRC-32");
    CHECK(md5_batch_submit(b, ptrs, g_lens, NCH, &out[0][0]) == 0 && same(out, g_crc, sizeof g_crc), "CRCs");
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 0) == 0, "both again");
    CHECK(md5_batch_submit_iov(b, g_segs, g_first, NCH, &out[0][0]) == 0 && same(out, g_rec, sizeof g_rec), "records again");

    /* async submissions of different kinds interleaved: each ticket of its own kind */
    {
        enum { R = 12, PER = NCH / R };
        static const int kinds[3] = {MD5HIP_DIGEST_MD5, MD5HIP_DIGEST_MD5_CRC32, MD5HIP_DIGEST_CRC32};
        const struct md5hip_src src = {.kind = MD5HIP_SRC_PTRS, .ptrs = ptrs, .lens = g_lens};
        uint64_t tk[R];
        memset(out, 0x5a, sizeof g_rec);
        for (int r = 0; r < R; r++)
            CHECK((rc = md5hip_submit_src(b, kinds[r % 3], 0, &src, (uint64_t)r * PER, (uint64_t)(r + 1) * PER,
                                          &out[r * PER][0], &tk[r], 0)) == 0, "interleaved submit %d: %d", r, rc);
        for (int r = R - 1; r >= 0; r--) CHECK((rc = md5_batch_wait(b, tk[r])) == 0, "interleaved wait %d: %d", r, rc);
        for (int r = 0; r < R; r++) {
            const int k = kinds[r % 3];
            const unsigned char *o = &out[r * PER][0];
            for (int i = 0; i < PER; i++) {
                const int c = r * PER + i;
                if (k == MD5HIP_DIGEST_MD5) CHECK(same(o + 16 * i, g_md5[c], 16), "interleaved MD5 %d", c);
                else if (k == MD5HIP_DIGEST_CRC32) CHECK(same(o + 4 * i, &g_crc[c], 4), "interleaved CRC %d", c);
                else CHECK(same(o + 32 * i, g_rec[c], 32), "interleaved record %d", c);
            }
            /* nothing past the ticket's own digests (a slot of another kind would write 32-byte strides) */
            const size_t used = (size_t)md5hip_digest_size(k) * PER;
            CHECK(untouched(o + used, 32u * PER - used), "ticket %d wrote past its digests", r);
        }
    }

    /* verify over whole records: one md5 byte, one crc byte, one padding byte corrupted */
    unsigned char ok[NCH];
    memcpy(out, g_rec, sizeof g_rec);
    out[3][5] ^= 1;
    out[77][17] ^= 0x80;
    out[200][27] = 1;
    CHECK((rc = md5hip_batch_verify_iov(b, g_segs, g_first, NCH, out, ok)) == 3, "verify %d", rc);
    for (int i = 0; i < NCH; i++) CHECK(ok[i] == !(i == 3 || i == 77 || i == 200), "verify ok[%d]", i);

    /* upgrade: whatever kind the handle is set to (here CRC-32 with a window) */
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, 64) == 0, "CRC-32 window");
    uint32_t want[NCH];
    unsigned char md5s[NCH][16];
    memcpy(want, g_crc, sizeof want);
    want[0] ^= 1;
    want[299] ^= 0x80000000u;
    memset(ok, 0x5a, sizeof ok);
    memset(md5s, 0x5a, sizeof md5s);
    CHECK((rc = md5hip_batch_upgrade_iov(b, g_segs, g_first, NCH, want, ok, &md5s[0][0])) == 2, "upgrade %d", rc);
    for (int i = 0; i < NCH; i++) CHECK(ok[i] == !(i == 0 || i == 299), "upgrade ok[%d]", i);
    CHECK(same(md5s, g_md5, sizeof g_md5), "upgrade md5 of every block");
    CHECK(md5hip_batcher_get_digest(b, &kind, &fc) == 0 && kind == MD5HIP_DIGEST_CRC32 && fc == 64, "kind kept");
    CHECK(md5hip_batch_upgrade_iov(b, g_segs, g_first, 0, NULL, NULL, NULL) == 0, "empty upgrade");
    CHECK(md5hip_batch_upgrade_iov(NULL, g_segs, g_first, 1, want, ok, &md5s[0][0]) == -EINVAL, "NULL batcher");
    CHECK(md5hip_batch_upgrade_iov(b, g_segs, g_first, 1, NULL, ok, &md5s[0][0]) == -EINVAL, "NULL want");
    CHECK(md5hip_batch_upgrade_iov(b, g_segs, g_first, 1, want, NULL, &md5s[0][0]) == -EINVAL, "NULL ok");
    CHECK(md5hip_batch_upgrade_iov(b, g_segs, g_first, 1, want, ok, NULL) == -EINVAL, "NULL md5_out");
    CHECK(md5hip_batch_upgrade_iov(b, NULL, g_first, 1, want, ok, &md5s[0][0]) == -EINVAL, "NULL segs");
    free(out);
    md5hip_batcher_destroy(b);
    printf("batcher: every submit path, kind switches, interleaved kinds, verify and upgrade ok\n");
    return 0;
}

static int staging(void)
{
    /* a host_fixed call under the kind stages and copies what one MD5 call over the same buffer does */
    md5hip_batcher *b;
    CHECK(md5hip_batcher_create(0, 1u << 20, 3, &b) == 0, "create");
    const size_t bytes = (size_t)NF * FS;
    unsigned char *fx = malloc(bytes), *o = malloc((size_t)NF * 32);
    CHECK(fx && o, "alloc");
    memset(fx, 3, bytes);
    struct md5hip_batcher_stats s0, s1, s2;
    md5hip_batcher_get_stats(b, &s0);
    CHECK(md5hip_batch_host_fixed(b, fx, NF, FL, FS, o) == 0, "MD5");
    md5hip_batcher_get_stats(b, &s1);
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 0) == 0, "both");
    CHECK(md5hip_batch_host_fixed(b, fx, NF, FL, FS, o) == 0, "both");
    md5hip_batcher_get_stats(b, &s2);
    CHECK(s1.bytes_staged > s0.bytes_staged, "a pageable source is staged");
    CHECK(s2.bytes_staged - s1.bytes_staged == s1.bytes_staged - s0.bytes_staged, "staged %llu under the kind, %llu under MD5",
          (unsigned long long)(s2.bytes_staged - s1.bytes_staged), (unsigned long long)(s1.bytes_staged - s0.bytes_staged));
    CHECK(s2.launches - s1.launches == s1.launches - s0.launches, "launches");
    free(fx);
    free(o);
    md5hip_batcher_destroy(b);
    printf("staging: host_fixed stages the same bytes under the kind as under MD5\n");
    return 0;
}

static int pool_paths(void)
{
    const int devs[2] = {0, 1};
    md5hip_pool *p;
    int rc = md5hip_pool_create(devs, 2, 1u << 20, 3, &p);
    CHECK(rc == 0, "pool create %d", rc);
    CHECK(md5hip_pool_set_digest(p, MD5HIP_DIGEST_MD5_CRC32, 8) == -EINVAL, "window");
    CHECK(md5hip_pool_set_digest(p, 3, 0) == -EINVAL, "kind 3");
    CHECK(md5hip_pool_set_digest(p, MD5HIP_DIGEST_MD5_CRC32, 0) == 0, "set_digest");
    const void *ptrs[NCH];
    for (int i = 0; i < NCH; i++) ptrs[i] = g_heap + g_offs[i];
    unsigned char(*rec)[32] = malloc(sizeof g_rec);
    CHECK(rec, "alloc");
    uint64_t t = 0;
    for (int split = 0; split < 2; split++) {
        /* whole to one device, then cut over both (tickets of two batchers) */
        CHECK(md5hip_pool_set_split(p, split ? 64u << 10 : 1ull << 40) == 0, "set_split");
        FRESH();
        CHECK((rc = md5hip_pool_submit(p, ptrs, g_lens, NCH, &rec[0][0])) == 0 && same(rec, g_rec, sizeof g_rec), "pool ptrs %d", rc);
        FRESH();
        CHECK((rc = md5hip_pool_submit_iov(p, g_segs, g_first, NCH, &rec[0][0])) == 0 && same(rec, g_rec, sizeof g_rec), "pool iov %d", rc);
        FRESH();
        CHECK((rc = md5hip_pool_submit_async(p, ptrs, g_lens, NCH, &rec[0][0], &t)) == 0 && t, "pool async %d", rc);
        CHECK((rc = md5hip_pool_wait(p, t)) == 0 && same(rec, g_rec, sizeof g_rec), "pool async wait %d", rc);
        FRESH();
        CHECK((rc = md5hip_pool_submit_iov_async(p, g_segs, g_first, NCH, &rec[0][0], &t)) == 0 && t, "pool iov async %d", rc);
        CHECK((rc = md5hip_pool_wait(p, t)) == 0 && same(rec, g_rec, sizeof g_rec), "pool iov async wait %d", rc);
        unsigned char(*frec)[32] = malloc((size_t)400 * 32);
        CHECK(frec, "alloc");
        CHECK((rc = md5hip_pool_host_fixed(p, g_heap, 400, 4000, 4001, &frec[0][0])) == 0, "pool host_fixed %d", rc);
        for (int i = 0; i < 400; i++) {
            unsigned char w[32];
            record_of(g_heap + (size_t)i * 4001, 4000, w);
            CHECK(same(frec[i], w, 32), "pool host_fixed record %d", i);
        }
        free(frec);
        struct md5hip_pool_stats ps;
        md5hip_pool_get_stats(p, &ps);
        CHECK(split ? ps.split > 0 : ps.split == 0, "split submissions: %llu", (unsigned long long)ps.split);
    }
    unsigned char ok[NCH];
    memcpy(rec, g_rec, sizeof g_rec);
    rec[10][0] ^= 4;
    rec[11][19] ^= 4;
    rec[12][31] ^= 4;
    CHECK((rc = md5hip_pool_verify_iov(p, g_segs, g_first, NCH, rec, ok)) == 3, "pool verify %d", rc);
    for (int i = 0; i < NCH; i++) CHECK(ok[i] == !(i >= 10 && i <= 12), "pool verify ok[%d]", i);
    CHECK(md5hip_pool_set_digest(p, MD5HIP_DIGEST_MD5, 0) == 0, "pool to MD5");
    uint32_t want[NCH];
    unsigned char md5s[NCH][16];
    memcpy(want, g_crc, sizeof want);
    want[150] += 1;
    want[151] -= 1;
    CHECK((rc = md5hip_pool_upgrade_iov(p, g_segs, g_first, NCH, want, ok, &md5s[0][0])) == 2, "pool upgrade %d", rc);
    for (int i = 0; i < NCH; i++) CHECK(ok[i] == !(i == 150 || i == 151), "pool upgrade ok[%d]", i);
    CHECK(same(md5s, g_md5, sizeof g_md5), "pool upgrade md5");
    CHECK(md5hip_pool_submit(p, ptrs, g_lens, NCH, &rec[0][0]) == 0 && same(rec, g_md5, sizeof g_md5), "pool still MD5");
    CHECK(md5hip_pool_upgrade_iov(NULL, g_segs, g_first, 1, want, ok, &md5s[0][0]) == -EINVAL, "NULL pool");
    CHECK(md5hip_pool_upgrade_iov(p, g_segs, g_first, 1, want, ok, NULL) == -EINVAL, "NULL md5_out");
    free(rec);
    md5hip_pool_destroy(p);
    printf("pool: whole and split submissions, verify and upgrade ok\n");
    return 0;
}

static int failures(void)
{
    const void *ptrs[NCH];
    for (int i = 0; i < NCH; i++) ptrs[i] = g_heap + g_offs[i];
    unsigned char(*rec)[32] = malloc(sizeof g_rec);
    CHECK(rec, "alloc");
    /* NS chunks fit one slot, so a submission is one launch */
    enum { NS = 20 };
    md5hip_batcher *b;
    int rc;
    CHECK(md5hip_batcher_create(2, 1u << 20, 3, &b) == 0, "create");
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 0) == 0, "both");
    /* a launch that fails on a healthy device: its ticket -EIO, nothing written, the batcher usable */
    FRESH();
    __atomic_store_n(&fake_dual_fail_next, 1, __ATOMIC_RELAXED);
    CHECK((rc = md5_batch_submit(b, ptrs, g_lens, NS, &rec[0][0])) == -EIO, "failed launch %d", rc);
    CHECK(untouched(&rec[0][0], sizeof g_rec), "a failed launch wrote records");
    CHECK(md5hip_batcher_health(b) == 0, "healthy after a failed launch");
    CHECK((rc = md5_batch_submit(b, ptrs, g_lens, NS, &rec[0][0])) == 0 && same(rec, g_rec, 32 * NS), "after it %d", rc);
    /* the device lost after launch K = 2: launch 1 right, launch 2 -EIO, then -ENODEV with nothing enqueued */
    CHECK(md5hip_batcher_inject_fault(b, 2) == 0, "inject");
    FRESH();
    CHECK((rc = md5_batch_submit(b, ptrs, g_lens, NS, &rec[0][0])) == 0 && same(rec, g_rec, 32 * NS), "launch 1 %d", rc);
    FRESH();
    uint64_t t = 0;
    CHECK((rc = md5_batch_submit_async(b, ptrs, g_lens, NS, &rec[0][0], &t)) == 0, "launch 2 submit %d", rc);
    CHECK((rc = md5_batch_wait(b, t)) == -EIO, "launch 2's ticket %d", rc);
    CHECK(untouched(&rec[0][0], sizeof g_rec), "the lost launch wrote records");
    CHECK(md5hip_batcher_health(b) == -ENODEV, "failed");
    const unsigned long l0 = __atomic_load_n(&fake_dual_launches, __ATOMIC_RELAXED);
    CHECK((rc = md5_batch_submit(b, ptrs, g_lens, NS, &rec[0][0])) == -ENODEV, "later sync %d", rc);
    CHECK((rc = md5_batch_submit_iov_async(b, g_segs, g_first, NS, &rec[0][0], &t)) == -ENODEV && t == 0, "later async %d", rc);
    unsigned char ok[NCH], md5s[NCH][16];
    memset(ok, 0x5a, sizeof ok);
    memset(md5s, 0x5a, sizeof md5s);
    CHECK((rc = md5hip_batch_upgrade_iov(b, g_segs, g_first, NS, g_crc, ok, &md5s[0][0])) == -ENODEV, "upgrade %d", rc);
    CHECK(untouched(ok, sizeof ok) && untouched(&md5s[0][0], sizeof md5s), "upgrade wrote on -errno");
    CHECK(md5hip_batch_verify_iov(b, g_segs, g_first, NS, g_rec, ok) == -ENODEV && untouched(ok, sizeof ok), "verify");
    CHECK(untouched(&rec[0][0], sizeof g_rec), "records after the loss");
    CHECK(__atomic_load_n(&fake_dual_launches, __ATOMIC_RELAXED) == l0, "launched on a failed device");
    md5hip_batcher_destroy(b);

    /* a pool of one device losing it: -EIO / -ENODEV, nothing written */
    const int dev = 3;
    md5hip_pool *p;
    CHECK(md5hip_pool_create(&dev, 1, 1u << 20, 3, &p) == 0, "pool create");
    CHECK(md5hip_pool_set_digest(p, MD5HIP_DIGEST_MD5_CRC32, 0) == 0, "pool both");
    CHECK(md5hip_pool_submit(p, ptrs, g_lens, NS, &rec[0][0]) == 0 && same(rec, g_rec, 32 * NS), "pool healthy");
    CHECK(md5hip_pool_inject_fault(p, 0, 1) == 0, "pool inject");
    FRESH();
    rc = md5hip_pool_submit(p, ptrs, g_lens, NS, &rec[0][0]);
    CHECK(rc == -EIO || rc == -ENODEV, "pool lost launch %d", rc);
    CHECK(untouched(&rec[0][0], sizeof g_rec), "pool: the lost launch wrote records");
    memset(ok, 0x5a, sizeof ok);
    memset(md5s, 0x5a, sizeof md5s);
    CHECK((rc = md5hip_pool_upgrade_iov(p, g_segs, g_first, NS, g_crc, ok, &md5s[0][0])) == -ENODEV, "pool upgrade %d", rc);
    CHECK(untouched(ok, sizeof ok) && untouched(&md5s[0][0], sizeof md5s), "pool upgrade wrote on -errno");
    md5hip_pool_destroy(p);
    free(rec);
    printf("failures: failed launch -EIO, device lost after launch 2 -EIO / -ENODEV, no record written\n");
    return 0;
}
#else  /* NO_DUAL: the launchers are absent */
static int refusals(void)
{
    md5hip_batcher *b;
    CHECK(md5hip_batcher_create(0, 1u << 20, 3, &b) == 0, "create");
    struct md5hip_batcher_stats s0, s1;
    md5hip_batcher_get_stats(b, &s0);
    int rc;
    CHECK((rc = md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 0)) == -ENOSYS, "set_digest %d", rc);
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_MD5_CRC32, 4) == -EINVAL, "window");
    CHECK(md5hip_batcher_set_digest(b, 3, 0) == -EINVAL, "kind 3");
    int kind = -1;
    uint32_t fc = 9;
    CHECK(md5hip_batcher_get_digest(b, &kind, &fc) == 0 && kind == MD5HIP_DIGEST_MD5 && fc == 0, "kind unchanged");
    unsigned char ok[NCH], md5s[NCH][16];
    memset(ok, 0x5a, sizeof ok);
    memset(md5s, 0x5a, sizeof md5s);
    CHECK((rc = md5hip_batch_upgrade_iov(b, g_segs, g_first, NCH, g_crc, ok, &md5s[0][0])) == -ENOSYS, "upgrade %d", rc);
    CHECK(untouched(ok, sizeof ok) && untouched(&md5s[0][0], sizeof md5s), "upgrade wrote on -ENOSYS");
    CHECK((rc = md5hip_verify_iov_as(b, MD5HIP_DIGEST_MD5_CRC32, 0, g_segs, g_first, NCH, g_rec, ok)) == -ENOSYS,
          "verify_as %d", rc);
    md5hip_batcher_get_stats(b, &s1);
    CHECK(s1.launches == s0.launches && s1.submissions == s0.submissions, "something was enqueued");
    /* the other kinds as before */
    unsigned char(*out)[16] = malloc(sizeof g_md5);
    CHECK(out, "alloc");
    CHECK(md5_batch_submit_iov(b, g_segs, g_first, NCH, &out[0][0]) == 0 && same(out, g_md5, sizeof g_md5), "MD5");
    CHECK(md5hip_batcher_set_digest(b, MD5HIP_DIGEST_CRC32, 0) == 0, "CRC-32");
    CHECK(md5_batch_submit_iov(b, g_segs, g_first, NCH, &out[0][0]) == 0 && same(out, g_crc, sizeof g_crc), "CRCs");
    md5hip_batcher_destroy(b);

    const int devs[2] = {0, 1};
    md5hip_pool *p;
    CHECK(md5hip_pool_create(devs, 2, 1u << 20, 3, &p) == 0, "pool create");
    CHECK((rc = md5hip_pool_set_digest(p, MD5HIP_DIGEST_MD5_CRC32, 0)) == -ENOSYS, "pool set_digest %d", rc);
    CHECK(md5hip_pool_set_digest(p, 3, 0) == -EINVAL, "pool kind 3");
    CHECK((rc = md5hip_pool_upgrade_iov(p, g_segs, g_first, NCH, g_crc, ok, &md5s[0][0])) == -ENOSYS, "pool upgrade %d", rc);
    CHECK(untouched(ok, sizeof ok) && untouched(&md5s[0][0], sizeof md5s), "pool upgrade wrote on -ENOSYS");
    struct md5hip_pool_stats ps;
    md5hip_pool_get_stats(p, &ps);
    CHECK(ps.submissions == 0, "pool: something was submitted");
    CHECK(md5hip_pool_submit_iov(p, g_segs, g_first, NCH, &out[0][0]) == 0 && same(out, g_md5, sizeof g_md5), "pool MD5");
    md5hip_pool_destroy(p);
    free(out);
    printf("refusals: MD5_CRC32 without its launchers is -ENOSYS, nothing enqueued\n");
    return 0;
}
#endif

int main(void)
{
    setvbuf(stdout, NULL, _IOLBF, 0);
    if (setup()) return 2;
    make_iov();
#ifndef NO_DUAL
    if (batcher_paths() || staging() || pool_paths() || failures()) return 1;
#else
    if (refusals()) return 1;
#endif
    free(g_heap);
    printf("dual ok\n");
    return 0;
}
