/*
 * md5_source.h -- the batcher's host chunk sources (md5_submit.c): a
 * struct md5hip_src (md5_internal.h) of the host kinds, PTRS and IOV, read as
 * segments, its chunks copied whole, by byte range or as staged (fastcrc
 * windows), and the fan-out of large host copies over threads.  Kept apart,
 * as md5_tickets.h is, so the host test drives exactly this code
 * (tests/c/source_check.c); `static` and included by md5_submit.c alone.
 * Nothing here touches HIP or the batcher's state.
 */
#ifndef SPROXY_AMD_MD5_SOURCE_H
#define SPROXY_AMD_MD5_SOURCE_H

#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "md5_internal.h"

/* struct md5hip_src (md5_internal.h); the host kinds, PTRS and IOV, as
 * segments: chunk i is entry s->first + i of the caller's arrays */
static uint64_t src_nseg(const struct md5hip_src *s, uint64_t i)
{
    i += s->first;
    return s->kind == MD5HIP_SRC_PTRS ? 1 : s->seg_first[i + 1] - s->seg_first[i];
}

static void src_seg(const struct md5hip_src *s, uint64_t i, uint64_t k, const void **base,
                    uint32_t *len)
{
    i += s->first;
    if (s->kind == MD5HIP_SRC_PTRS) { *base = s->ptrs[i]; *len = s->lens[i]; return; }
    *base = s->segs[s->seg_first[i] + k].base;
    *len = s->segs[s->seg_first[i] + k].len;
}

static void src_copy(const struct md5hip_src *s, uint64_t i, unsigned char *dst)
{
    i += s->first;
    if (s->kind == MD5HIP_SRC_PTRS) {
        if (s->lens[i]) memcpy(dst, s->ptrs[i], s->lens[i]);
        return;
    }
    for (uint64_t j = s->seg_first[i]; j < s->seg_first[i + 1]; j++) {
        if (s->segs[j].len) memcpy(dst, s->segs[j].base, s->segs[j].len);
        dst += s->segs[j].len;
    }
}

/* Bytes [a, a + len) of chunk i, one contiguous piece at a time:
 * src_walk_next yields the next (pointer, take) piece, 0 when the range is
 * done (or the chunk ends first).  Empty segments yield nothing. */
struct src_walk {
    const struct md5hip_src *s;
    uint64_t i, k, ns, a, left;
};

static inline struct src_walk src_walk_range(const struct md5hip_src *s, uint64_t i, uint64_t a, uint64_t len)
{
    return (struct src_walk){s, i, 0, len ? src_nseg(s, i) : 0, a, len};
}

static inline int src_walk_next(struct src_walk *w, const void **p, uint32_t *take)
{
    while (w->left && w->k < w->ns) {
        const void *base;
        uint32_t len;
        src_seg(w->s, w->i, w->k++, &base, &len);
        if (w->a >= len) {
            w->a -= len;
            continue;
        }
        *take = (uint32_t)(len - w->a < w->left ? len - w->a : w->left);
        *p = (const unsigned char *)base + w->a;
        w->a = 0;
        w->left -= *take;
        return 1;
    }
    return 0;
}

/* Bytes [a, a + len) of chunk i to dst. */
static void src_copy_range(const struct md5hip_src *s, uint64_t i, uint64_t a, uint64_t len, unsigned char *dst)
{
    struct src_walk w = src_walk_range(s, i, a, len);
    const void *p;
    uint32_t take;
    while (src_walk_next(&w, &p, &take)) {
        memcpy(dst, p, take);
        dst += take;
    }
}

/* What a digest reads of an L-byte chunk: netcache's CRC-32 with a fastcrc
 * window F < L reads only the first and the last F bytes (blk_io.c:408-424),
 * so for L > 2F only those 2F bytes are staged and sent, as ONE 2F-byte
 * chunk whose own fastcrc digest is the same crc(head) ^ crc(tail) (a 16 KiB
 * block with F = 128: 256 B over PCIe instead of 16 KiB).  Up to 2F, and
 * for F = 0 (MD5 too), the whole chunk: never more than L bytes, so a chunk
 * that passes submit()'s size check always fits an empty slot. */
static inline uint64_t staged_len(uint32_t F, uint64_t L) { return F && L > 2ull * F ? 2ull * F : L; }

/* Table entries a zero-copy chunk of `ns` segments may take: one per
 * segment, one more when it is sent as two windows (one segment may hold
 * both), plus two spare.  submit() sends a chunk zero-copy only if this fits
 * an empty slot (win = 1, whatever the digest), so reserve() always places
 * it. */
static inline uint64_t zc_pieces(uint64_t ns, int win) { return ns + (win ? 1 : 0) + 2; }

/* chunk i as staged: whole, or its head and tail windows */
static void src_copy_staged(const struct md5hip_src *s, uint64_t i, uint32_t F, unsigned char *dst)
{
    const uint64_t L = F ? md5hip_src_len(s, i) : 0;
    if (staged_len(F, L) == L) {
        src_copy(s, i, dst);
        return;
    }
    src_copy_range(s, i, 0, F, dst);
    src_copy_range(s, i, L - F, F, dst + F);
}

/* Large host copies are fanned out: one thread's memcpy from pageable
 * memory into pinned staging runs ~15 GB/s, well below PCIe,
 * so a copy past 8 MiB is cut into parts of at least 2 MiB for
 * MD5HIP_GATHER_THREADS threads (default 4, at most 32; the calling thread
 * takes the first part, and any part whose thread could not be created). */
static pthread_once_t g_gather_once = PTHREAD_ONCE_INIT;
static int g_gather_threads = 4;

static void gather_threads_init(void)
{
    const char *e = getenv("MD5HIP_GATHER_THREADS");
    if (e && *e) {
        const int t = atoi(e);
        g_gather_threads = t < 1 ? 1 : t > 32 ? 32 : t;
    }
}

#define GATHER_SPLIT_MIN (8ull << 20)   /* bytes per range before it is split */
#define GATHER_PART_MIN (2ull << 20)    /* and at least this many bytes per part */
enum { FAN_MAX = 32 };

/* how many parts for `bytes` in `units` indivisible pieces: 1 .. FAN_MAX */
static uint64_t fan_parts(uint64_t bytes, uint64_t units)
{
    pthread_once(&g_gather_once, gather_threads_init);
    uint64_t T = (uint64_t)g_gather_threads;
    if (bytes < GATHER_SPLIT_MIN) T = 1;
    if (T > bytes / GATHER_PART_MIN) T = bytes / GATHER_PART_MIN ? bytes / GATHER_PART_MIN : 1;
    if (T > units) T = units ? units : 1;
    return T < 1 ? 1 : T > FAN_MAX ? FAN_MAX : T;
}

/* run(part t) for the T <= FAN_MAX parts of `size` bytes each at `parts` */
static void fan_out(void *(*run)(void *), void *parts, size_t size, uint64_t T)
{
    pthread_t tid[FAN_MAX];
    int started[FAN_MAX] = {0};
    for (uint64_t t = 1; t < T; t++)
        started[t] = pthread_create(&tid[t], NULL, run, (char *)parts + t * size) == 0;
    run(parts);
    for (uint64_t t = 1; t < T; t++) {
        if (started[t]) pthread_join(tid[t], NULL);
        else run((char *)parts + t * size);      /* no thread: copy it here */
    }
}

/* Host gather of chunks [first, first + m) to dst + off[j], the range
 * [lo, used) of the staging cut by bytes at chunk boundaries. */
struct gather_part {
    const struct md5hip_src *src;
    uint64_t first, jlo, jhi;
    const uint64_t *off;
    unsigned char *dst;
    uint32_t win;                         /* fastcrc window of a CRC-32 slot (staged_len), else 0 */
};

static void *gather_run(void *arg)
{
    const struct gather_part *p = arg;
    for (uint64_t j = p->jlo; j < p->jhi; j++) src_copy_staged(p->src, p->first + j, p->win, p->dst + p->off[j]);
    return NULL;
}

/* the T parts of that gather: part t takes chunks [jlo, jhi), every chunk in
 * exactly one part */
static void gather_cut(struct gather_part *part, uint64_t T, const struct md5hip_src *src, uint64_t first,
                       uint64_t m, const uint64_t *off, unsigned char *dst, uint64_t lo, uint64_t used,
                       uint32_t win)
{
    const uint64_t bytes = used - lo;
    uint64_t j = 0;
    for (uint64_t t = 0; t < T; t++) {      /* part t: chunks whose offset < lo + (t+1) * bytes / T */
        const uint64_t lim = t + 1 == T ? UINT64_MAX : lo + (t + 1) * bytes / T;
        part[t] = (struct gather_part){src, first, j, j, off, dst, win};
        while (j < m && off[j] < lim) j++;
        part[t].jhi = j;
    }
}

static void gather_range(const struct md5hip_src *src, uint64_t first, uint64_t m,
                         const uint64_t *off, unsigned char *dst, uint64_t lo, uint64_t used, uint32_t win)
{
    const uint64_t T = fan_parts(used - lo, m);
    struct gather_part part[FAN_MAX];
    gather_cut(part, T, src, first, m, off, dst, lo, used, win);
    fan_out(gather_run, part, sizeof part[0], T);
}

/* memcpy of `bytes`, cut evenly */
struct copy_part {
    unsigned char *dst;
    const unsigned char *src;
    uint64_t len;
};

static void *copy_run(void *arg)
{
    const struct copy_part *c = arg;
    memcpy(c->dst, c->src, c->len);
    return NULL;
}

static void copy_parallel(void *dst, const void *src, uint64_t bytes)
{
    const uint64_t T = fan_parts(bytes, UINT64_MAX);
    struct copy_part part[FAN_MAX];
    for (uint64_t t = 0; t < T; t++) {
        const uint64_t a = bytes * t / T, z = bytes * (t + 1) / T;
        part[t] = (struct copy_part){(unsigned char *)dst + a, (const unsigned char *)src + a, z - a};
    }
    fan_out(copy_run, part, sizeof part[0], T);
}

#endif
