/*
 * source_check.c -- the batcher's host chunk sources
 * (sproxy_amd/csrc/md5_source.h) driven on the host, built with ASan/UBSan by
 * tests/test_source_host.py.  Exits 0 when every check holds, else prints the
 * failing line.
 *
 * PTRS and IOV sources over the same bytes (chunks of many 1-byte segments,
 * empty segments, empty chunks, first != 0) against a flat copy: whole
 * chunks, every byte range of a 300-byte chunk, the staged form around the
 * fastcrc window, and the threaded gather cut into 1, 2, 5 and 32 parts.
 */
#include <stdio.h>

#include "../../sproxy_amd/csrc/md5_source.h"

#define CHECK(c)                                                   \
    do {                                                           \
        if (!(c)) {                                                \
            printf("FAIL line %d: %s\n", __LINE__, #c);            \
            return 1;                                              \
        }                                                          \
    } while (0)

enum { SKIP = 3, NCH = 40, MAXL = 700, GUARD = 256 };

/* chunk lengths: empty ones, 1, the lengths around F and 2F for F = 64 and
 * 128, and 300 once in each segmentation (build: by index % 3) */
static const uint32_t LEN[NCH] = {0,   1,   300, 63,  64,  65,  127, 128, 129, 0,   255, 256, 257, 2,
                                  5,   700, 0,   33,  128, 129, 257, 64,  1,   17,  300, 0,   511, 512,
                                  513, 90,  7,   256, 3,   0,   128, 640, 65,  300, 31,  1};

static unsigned char flat[(SKIP + NCH) * MAXL];      /* chunk c at flat + c * MAXL */
static const void *ptrs[SKIP + NCH];
static uint32_t lens[SKIP + NCH];
static struct md5hip_iov segs[(SKIP + NCH) * (MAXL + 8)];
static uint64_t seg_first[SKIP + NCH + 1];

/* chunk c as segments, by c % 3: 1-byte segments; pieces of 1, 2, 3, ...
 * bytes with an empty segment (NULL base) before each; one segment between
 * two empty ones */
static void build(void)
{
    uint64_t ns = 0;
    for (int c = 0; c < SKIP + NCH; c++) {
        const uint32_t L = c < SKIP ? 11 + c : LEN[c - SKIP];
        unsigned char *p = flat + (size_t)c * MAXL;
        for (uint32_t k = 0; k < L; k++) p[k] = (unsigned char)(1 + (c * 131 + k * 7 + (k >> 8)) % 251);
        ptrs[c] = L ? p : NULL;
        lens[c] = L;
        seg_first[c] = ns;
        if (c % 3 == 0) {
            for (uint32_t k = 0; k < L; k++) segs[ns++] = (struct md5hip_iov){p + k, 1};
        } else if (c % 3 == 1) {
            for (uint32_t k = 0, w = 1; k < L; k += w, w++) {
                segs[ns++] = (struct md5hip_iov){NULL, 0};
                segs[ns++] = (struct md5hip_iov){p + k, L - k < w ? L - k : w};
            }
        } else {
            segs[ns++] = (struct md5hip_iov){NULL, 0};
            segs[ns++] = (struct md5hip_iov){p, L};
            segs[ns++] = (struct md5hip_iov){p + L, 0};
        }
    }
    seg_first[SKIP + NCH] = ns;
}

static const unsigned char *chunk(uint64_t i) { return flat + (SKIP + i) * MAXL; }

/* `n` bytes at p all equal to v */
static int all(const unsigned char *p, size_t n, unsigned char v)
{
    for (size_t k = 0; k < n; k++)
        if (p[k] != v) return 0;
    return 1;
}

static int check_source(const struct md5hip_src *s)
{
    static unsigned char out[GUARD + MAXL + GUARD];
    unsigned char *dst = out + GUARD;
    CHECK(md5hip_src_check(s, NCH) == 0);
    for (uint64_t i = 0; i < NCH; i++) {
        const uint32_t L = LEN[i];
        CHECK(md5hip_src_len(s, i) == L);
        /* the segments, in order, are the chunk */
        uint64_t at = 0;
        for (uint64_t k = 0; k < src_nseg(s, i); k++) {
            const void *p;
            uint32_t l;
            src_seg(s, i, k, &p, &l);
            CHECK(at + l <= L && (l == 0 || memcmp(p, chunk(i) + at, l) == 0));
            at += l;
        }
        CHECK(at == L);
        /* whole */
        memset(out, 0, sizeof out);
        src_copy(s, i, dst);
        CHECK(memcmp(dst, chunk(i), L) == 0 && all(out, GUARD, 0) && all(dst + L, GUARD, 0));
        /* staged: whole up to 2F, else head || tail */
        for (uint32_t F = 0; F <= 128; F = F ? 2 * F : 64) {
            const uint64_t E = staged_len(F, L);
            CHECK(E == (F && L > 2 * F ? 2 * F : L));
            memset(out, 0, sizeof out);
            src_copy_staged(s, i, F, dst);
            if (E == L) {
                CHECK(memcmp(dst, chunk(i), L) == 0);
            } else {
                CHECK(memcmp(dst, chunk(i), F) == 0 && memcmp(dst + F, chunk(i) + L - F, F) == 0);
            }
            CHECK(all(out, GUARD, 0) && all(dst + E, GUARD, 0));
        }
    }
    /* every range [a, a + len) of a 300-byte chunk: the copy, and the walk's
     * pieces (non-empty, contiguous in the chunk, `len` bytes in all) */
    for (uint64_t i = 0; i < NCH; i++) {
        if (LEN[i] != 300) continue;
        for (uint64_t a = 0; a <= 300; a++)
            for (uint64_t len = 0; a + len <= 300; len++) {
                memset(dst - 1, 0, len + 2);
                src_copy_range(s, i, a, len, dst);
                CHECK(memcmp(dst, chunk(i) + a, len) == 0 && dst[-1] == 0 && dst[len] == 0);
                struct src_walk w = src_walk_range(s, i, a, len);
                const void *p;
                uint32_t take;
                uint64_t got = 0;
                while (src_walk_next(&w, &p, &take)) {
                    CHECK(take && got + take <= len && memcmp(p, chunk(i) + a + got, take) == 0);
                    got += take;
                }
                CHECK(got == len);
            }
    }
    return 0;
}

/* The gather of chunks [first, first + m) as the batcher stages them (each
 * on a 128-B line from `lo`), cut into T parts: the parts tile [0, m) in
 * order, and running them writes every chunk's staged bytes and nothing
 * else -- not the padding between chunks, nothing before lo or past used. */
static int check_gather(const struct md5hip_src *s, uint64_t first, uint64_t m, uint32_t F, uint64_t T)
{
    static unsigned char stage[GUARD + NCH * 768 + GUARD], want[sizeof stage];
    uint64_t off[NCH];
    const uint64_t lo = 384;
    uint64_t used = lo;
    memset(stage, 0xEE, sizeof stage);
    memset(want, 0xEE, sizeof want);
    for (uint64_t j = 0; j < m; j++) {
        const uint64_t L = LEN[first + j], E = staged_len(F, L);
        off[j] = used;
        if (E == L) {
            memcpy(want + used, chunk(first + j), L);
        } else {
            memcpy(want + used, chunk(first + j), F);
            memcpy(want + used + F, chunk(first + j) + L - F, F);
        }
        used += (E + 127) & ~127ull;
    }
    CHECK(used + GUARD <= sizeof stage);
    struct gather_part part[FAN_MAX];
    CHECK(T >= 1 && T <= FAN_MAX);
    gather_cut(part, T, s, first, m, off, stage, lo, used, F);
    uint64_t j = 0;
    for (uint64_t t = 0; t < T; t++) {
        CHECK(part[t].jlo == j && part[t].jhi >= j && part[t].jhi <= m);
        j = part[t].jhi;
    }
    CHECK(j == m);
    fan_out(gather_run, part, sizeof part[0], T);
    CHECK(memcmp(stage, want, sizeof stage) == 0);
    return 0;
}

int main(void)
{
    build();
    const struct md5hip_src sp = {.kind = MD5HIP_SRC_PTRS, .first = SKIP, .ptrs = ptrs, .lens = lens};
    const struct md5hip_src si = {.kind = MD5HIP_SRC_IOV, .first = SKIP, .segs = segs, .seg_first = seg_first};
    if (check_source(&sp) || check_source(&si)) return 1;

    static const uint64_t parts[] = {1, 2, 5, 32};
    for (int k = 0; k < 4; k++)
        for (uint32_t F = 0; F <= 128; F = F ? 2 * F : 64) {
            if (check_gather(&sp, 0, NCH, F, parts[k]) || check_gather(&si, 0, NCH, F, parts[k])) return 1;
            if (check_gather(&si, 7, 3, F, parts[k])) return 1;      /* more parts than chunks */
        }
    /* the entry the batcher calls (one part below the split threshold), and
     * the partition rule itself */
    {
        static unsigned char stage[1024], want[1024];
        const uint64_t off[2] = {128, 512};
        memset(stage, 0xEE, sizeof stage);
        memset(want, 0xEE, sizeof want);
        memcpy(want + 128, chunk(2), 300);
        memcpy(want + 512, chunk(3), 63);
        gather_range(&si, 2, 2, off, stage, 128, 640, 0);
        CHECK(memcmp(stage, want, sizeof stage) == 0);
        CHECK(fan_parts(GATHER_SPLIT_MIN - 1, 1000) == 1);
        CHECK(fan_parts(64ull << 20, 1000) == (uint64_t)g_gather_threads);
        CHECK(fan_parts(64ull << 20, 3) == 3 && fan_parts(64ull << 20, 0) == 1);
        CHECK(fan_parts(9ull << 20, 1000) == (g_gather_threads < 4 ? (uint64_t)g_gather_threads : 4));
    }
    /* copy_parallel below its threshold is one memcpy */
    {
        unsigned char a[300], z[302] = {0};
        memcpy(a, chunk(2), 300);
        copy_parallel(z + 1, a, 300);
        CHECK(memcmp(z + 1, a, 300) == 0 && z[0] == 0 && z[301] == 0);
    }
    puts("source ok");
    return 0;
}
