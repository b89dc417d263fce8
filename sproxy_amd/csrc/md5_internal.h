/* md5_internal.h -- entries shared between the library's own objects
 * (hidden: not part of the C ABI in include/). */
#ifndef SPROXY_AMD_MD5_INTERNAL_H
#define SPROXY_AMD_MD5_INTERNAL_H

#include <errno.h>
#include <stdint.h>
#include <string.h>

#include "../../include/md5hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One copy of the device-side gather: `len` bytes from the device-visible
 * address `src` (registered host memory) to d_dst + dst. */
struct md5hip_seg {
    uint64_t src;
    uint64_t dst;
    uint32_t len;
    uint32_t pad;
};

/* Gather kernel (md5_kernels.hip): one workgroup per segment. */
__attribute__((visibility("hidden")))
int md5hip_gather_launch(const struct md5hip_seg *d_segs, uint64_t nseg, unsigned char *d_dst,
                         void *stream);

/* Thresholds in 64-B blocks that the kernels (md5_kernels.h) and the planner
 * (md5_plan.cc) share: a fed pair needs a chunk of two whole blocks; a
 * HYBRID wave goes lane-direct from a longest chunk of 256 KiB. */
enum { MD5HIP_FED_MIN_BLOCKS = 2, MD5HIP_HYBRID_LONG_BLOCKS = 4096 };

/* Compute units of the current device, cached; 256 when it cannot be asked
 * (md5_kernels.hip).  The planner's only way to the device. */
__attribute__((visibility("hidden")))
int md5hip_cu_count(void);

/* The planner's entries for the launchers (md5_plan.cc): whether a batch of
 * `ngroups` 64-chunk groups is small enough for fed pairs, and whether a
 * full-CRC batch of n chunks of `len` bytes (0 = not known) runs split. */
__attribute__((visibility("hidden")))
int md5hip_fed_fits(uint64_t ngroups);
__attribute__((visibility("hidden")))
int md5hip_crc_split_fits(uint64_t n, uint64_t len);

/* CRC kernel variant (enum crc32hip_variant) for a full-CRC descriptor batch
 * of n chunks whose mean length is known (md5_plan.cc). */
__attribute__((visibility("hidden")))
int md5hip_crc_desc_choice(uint64_t n, uint64_t mean_len);

/* MD5 descriptor variant for a planned batch of `bytes` payload of which
 * `unlined_bytes` lie in chunks starting 16-B but not 128-B aligned: XDMA
 * becomes LINES past half (md5_plan.cc). */
__attribute__((visibility("hidden")))
int md5hip_lines_choice(int variant, uint64_t unlined_bytes, uint64_t bytes);

/* ------------------------------------------------------------------------
 * What a submission reads: exactly one of a flat host (ptr, len) list, page
 * lists with per-chunk segment ranges (seg_first has one entry more than
 * the caller has chunks, seg_first[0] = 0), device addresses (no bytes to
 * move), fixed-length chunks at a fixed stride from one base, or
 * device-resident page lists (a table of page addresses, per-chunk entry
 * ranges and lengths; page_first has one entry more than the caller has
 * chunks).  Chunk i of
 * the source is entry first + i of the caller's arrays, so a sub-range of a
 * caller's source is the same arrays with another `first`: nothing is copied
 * or re-based.
 * ------------------------------------------------------------------------ */
enum md5hip_src_kind { MD5HIP_SRC_PTRS, MD5HIP_SRC_IOV, MD5HIP_SRC_DEVICE, MD5HIP_SRC_FIXED, MD5HIP_SRC_PAGES };
struct md5hip_src {
    int kind;                            /* enum md5hip_src_kind */
    uint64_t first;
    const void *const *ptrs;             /* PTRS */
    const uint32_t *lens;                /* PTRS, DEVICE */
    const struct md5hip_iov *segs;       /* IOV */
    const uint64_t *seg_first;
    const uint64_t *dptrs;               /* DEVICE */
    const unsigned char *base;           /* FIXED: chunk i is (base + i * stride, len) */
    uint32_t len;
    uint64_t stride;
    int base_on_device;                  /* FIXED: device memory, read in place */
    const uint64_t *pages;               /* PAGES: device addresses; chunk i is lens[i] bytes in the */
    const uint64_t *page_first;          /* pages at entries page_first[i] .. of `pages`, page_bytes each */
    uint32_t page_bytes;
};

/* page_bytes of a paged batch: a multiple of 128 (no 64-B block and no
 * 128-B stage straddles two pages), at most 2^30 */
static inline int md5hip_page_bytes_ok(uint32_t page_bytes)
{
    return page_bytes != 0 && (page_bytes & 127u) == 0 && page_bytes <= MD5HIP_PAGE_BYTES_MAX;
}

/* table entries a chunk of len bytes reads */
static inline uint64_t md5hip_pages_of(uint32_t len, uint32_t page_bytes)
{
    return ((uint64_t)len + page_bytes - 1) / page_bytes;
}

/* 0, or -EINVAL: an array missing, a NULL pointer with a length, a seg_first
 * that does not start at 0 or decreases, len > stride, a page size off its
 * rules, a page_first that decreases or leaves a chunk fewer entries than its
 * length needs, a NULL page among those (chunks [0, n)). */
static inline int md5hip_src_check(const struct md5hip_src *s, uint64_t n)
{
    const uint64_t f = s->first;
    switch (s->kind) {
    case MD5HIP_SRC_PTRS:
        if (!s->ptrs || !s->lens) return -EINVAL;
        for (uint64_t i = f; i < f + n; i++)
            if (!s->ptrs[i] && s->lens[i]) return -EINVAL;
        return 0;
    case MD5HIP_SRC_DEVICE:
        if (!s->dptrs || !s->lens) return -EINVAL;
        for (uint64_t i = f; i < f + n; i++)
            if (!s->dptrs[i] && s->lens[i]) return -EINVAL;
        return 0;
    case MD5HIP_SRC_IOV:
        if (!s->segs || !s->seg_first || s->seg_first[0] != 0) return -EINVAL;
        for (uint64_t i = f; i < f + n; i++) {
            if (s->seg_first[i + 1] < s->seg_first[i]) return -EINVAL;
            for (uint64_t j = s->seg_first[i]; j < s->seg_first[i + 1]; j++)
                if (!s->segs[j].base && s->segs[j].len) return -EINVAL;
        }
        return 0;
    case MD5HIP_SRC_FIXED:
        return s->base && s->len <= s->stride ? 0 : -EINVAL;
    case MD5HIP_SRC_PAGES:
        if (!s->pages || !s->page_first || !s->lens || !md5hip_page_bytes_ok(s->page_bytes)) return -EINVAL;
        for (uint64_t i = f; i < f + n; i++) {
            const uint64_t need = md5hip_pages_of(s->lens[i], s->page_bytes);
            if (s->page_first[i + 1] < s->page_first[i] || s->page_first[i + 1] - s->page_first[i] < need)
                return -EINVAL;
            for (uint64_t j = 0; j < need; j++)
                if (!s->pages[s->page_first[i] + j]) return -EINVAL;
        }
        return 0;
    }
    return -EINVAL;
}

/* bytes of chunk i */
static inline uint64_t md5hip_src_len(const struct md5hip_src *s, uint64_t i)
{
    if (s->kind == MD5HIP_SRC_FIXED) return s->len;
    if (s->kind != MD5HIP_SRC_IOV) return s->lens[s->first + i];
    uint64_t L = 0;
    for (uint64_t j = s->seg_first[s->first + i]; j < s->seg_first[s->first + i + 1]; j++) L += s->segs[j].len;
    return L;
}

/* digest bytes per chunk (MD5_CRC32: one struct md5hip_md5crc32) */
static inline uint32_t md5hip_digest_size(int kind)
{
    return kind == MD5HIP_DIGEST_CRC32 ? 4 : kind == MD5HIP_DIGEST_MD5_CRC32 ? 32 : 16;
}

/* a digest kind with its fastcrc window: MD5 and MD5_CRC32 take none,
 * CRC-32's is a multiple of 4 (cfs_apix.c:2222-2236) */
static inline int md5hip_digest_valid(int kind, uint32_t fastcrc)
{
    return kind == MD5HIP_DIGEST_MD5 || kind == MD5HIP_DIGEST_MD5_CRC32
               ? fastcrc == 0
               : kind == MD5HIP_DIGEST_CRC32 && (fastcrc & 3u) == 0;
}

/* The MD5_CRC32 launchers are weak references for the host objects: linked
 * without the device library (the CPU tests' stand-in runtime has none) the
 * batcher and the pool refuse the kind with -ENOSYS before anything is
 * enqueued.  md5_kernels.hip defines them, so libmd5hip.so always has them. */
#ifndef MD5HIP_DEFINES_MD5CRC32
extern __typeof__(md5crc32hip_fixed) md5crc32hip_fixed __attribute__((weak));
extern __typeof__(md5crc32hip_desc) md5crc32hip_desc __attribute__((weak));
static inline int md5hip_md5crc32_present(void) { return &md5crc32hip_fixed && &md5crc32hip_desc; }
/* So are the entries that name the kernel, and the planner's choice between
 * them: a build with the plain launchers alone (tests/c/fake_dual.c) calls
 * those for every batch. */
extern __typeof__(md5crc32hip_fixed_variant) md5crc32hip_fixed_variant __attribute__((weak));
extern __typeof__(md5crc32hip_desc_variant) md5crc32hip_desc_variant __attribute__((weak));
extern __typeof__(md5crc32hip_plan) md5crc32hip_plan __attribute__((weak));
static inline int md5hip_md5crc32_variants_present(void)
{
    return &md5crc32hip_fixed_variant && &md5crc32hip_desc_variant && &md5crc32hip_plan;
}
#else
static inline int md5hip_md5crc32_present(void) { return 1; }
static inline int md5hip_md5crc32_variants_present(void) { return 1; }
#endif
/* 0, -EINVAL (no such kind / window) or -ENOSYS (MD5_CRC32 without its launchers) */
static inline int md5hip_digest_usable(int kind, uint32_t fastcrc)
{
    if (!md5hip_digest_valid(kind, fastcrc)) return -EINVAL;
    if (kind == MD5HIP_DIGEST_MD5_CRC32 && !md5hip_md5crc32_present()) return -ENOSYS;
    return 0;
}

/* So is the paged launcher (md5_pages.hip) for the host objects: without it
 * md5_batch_submit_device_pages returns -ENOSYS before anything is enqueued. */
#ifndef MD5HIP_DEFINES_PAGES
extern __typeof__(md5hip_digest_pages) md5hip_digest_pages __attribute__((weak));
static inline int md5hip_pages_present(void) { return &md5hip_digest_pages != 0; }
/* and the fastcrc windows over page lists, which a paged verify under a
 * CRC-32 window launches: -ENOSYS for that kind alone without it */
extern __typeof__(crc32hip_pages) crc32hip_pages __attribute__((weak));
static inline int md5hip_pages_fast_present(void) { return &crc32hip_pages != 0; }
#else
static inline int md5hip_pages_present(void) { return 1; }
static inline int md5hip_pages_fast_present(void) { return 1; }
#endif

/* One range of the digest-compare kernel's table form (md5_verify.hip): for
 * i in [0, count), ok[i] = (bytes [goff, goff + wsz) of record first + i of
 * the launch's digest array == want i), and *cnt = the range's mismatches
 * (stored, not added: a range is one workgroup's).  want: count x wsz bytes,
 * ok: count bytes, both device addresses of any alignment; cnt: a device
 * uint64.  The batcher cuts a long segment into ranges of at most
 * MD5HIP_CMP_PIECE records; the public entry cuts its n the same way. */
struct md5hip_cmp {
    uint64_t first, count;
    uint64_t want, ok, cnt;
    uint32_t goff, wsz;
};
enum { MD5HIP_CMP_PIECE = 4096 };

/* The table launcher, one workgroup per entry (md5_verify.hip): a weak
 * reference for the host objects, like the MD5_CRC32 launchers above --
 * without it the asynchronous verify entries return -ENOSYS before anything
 * is enqueued.  d_got: records of gsz bytes (4, 16 or 32), aligned to
 * min(gsz, 16).  0, -EINVAL, -EIO. */
__attribute__((visibility("hidden")))
int md5hip_compare_launch(const void *d_got, uint32_t gsz, const struct md5hip_cmp *d_tab, uint64_t nent,
                          void *stream);
#ifndef MD5HIP_DEFINES_COMPARE
extern __typeof__(md5hip_compare_launch) md5hip_compare_launch __attribute__((weak));
static inline int md5hip_compare_present(void) { return &md5hip_compare_launch != 0; }
#else
static inline int md5hip_compare_present(void) { return 1; }
#endif

/* verify: ok[i] = digest i of `got` equals that of `expected`; the number of
 * mismatches */
static inline int md5hip_verify_count(const unsigned char *got, const void *expected, uint32_t dsz, uint64_t n,
                                      unsigned char *ok)
{
    const unsigned char *e = (const unsigned char *)expected;
    int bad = 0;
    for (uint64_t i = 0; i < n; i++) {
        ok[i] = memcmp(got + (size_t)dsz * i, e + (size_t)dsz * i, dsz) == 0;
        bad += !ok[i];
    }
    return bad;
}

/* upgrade: from n MD5_CRC32 records, ok[i] = (crc i == want_crc[i]) and
 * md5_out + 16 i = md5 i (every chunk); the number of mismatches */
static inline int md5hip_upgrade_count(const unsigned char *rec, const uint32_t *want_crc, uint64_t n,
                                       unsigned char *ok, unsigned char *md5_out)
{
    int bad = 0;
    for (uint64_t i = 0; i < n; i++) {
        const unsigned char *r = rec + 32 * (size_t)i;
        const uint32_t crc = (uint32_t)r[16] | (uint32_t)r[17] << 8 | (uint32_t)r[18] << 16 | (uint32_t)r[19] << 24;
        memcpy(md5_out + 16 * (size_t)i, r, 16);
        ok[i] = crc == want_crc[i];
        bad += !ok[i];
    }
    return bad;
}

/* Batched verify with a digest kind of its own (md5_submit.c): the
 * batcher's setting is not touched, so concurrent submitters keep theirs. */
struct md5hip_batcher;
__attribute__((visibility("hidden")))
int md5hip_verify_iov_as(struct md5hip_batcher *b, int kind, uint32_t fastcrc,
                         const struct md5hip_iov *segs, const uint64_t *seg_first, uint64_t n,
                         const void *expected, unsigned char *ok);

/* For the multi-GPU pool's router (md5_pool.c), all in md5_submit.c:
 *   md5hip_batcher_load    weight (len + 64 per chunk) reserved in the
 *                          batcher's open and in-flight slots, read lock-free
 *   md5hip_batcher_slice   staging bytes per slot
 *   md5hip_submit_src      chunks [lo, hi) of a host source (PTRS, IOV or
 *                          FIXED) with an explicit digest kind, digests to
 *                          digests[0..]; ticket NULL = synchronous; urgent =
 *                          launched at once like a synchronous call (the
 *                          caller waits on the ticket right away; a FIXED
 *                          source has a launch of its own either way)
 *   md5hip_batcher_ticket_state  1 done (*err = its error), 0 pending,
 *                          -EINVAL unknown; never launches anything */
__attribute__((visibility("hidden")))
uint64_t md5hip_batcher_load(const struct md5hip_batcher *b);
__attribute__((visibility("hidden")))
uint64_t md5hip_batcher_slice(const struct md5hip_batcher *b);
__attribute__((visibility("hidden")))
int md5hip_submit_src(struct md5hip_batcher *b, int kind, uint32_t fastcrc, const struct md5hip_src *src,
                      uint64_t lo, uint64_t hi, unsigned char *digests, uint64_t *ticket, int urgent);
__attribute__((visibility("hidden")))
int md5hip_batcher_ticket_state(struct md5hip_batcher *b, uint64_t ticket, int *err);

/* What a verify submission compares and where its results go (all indexed
 * by the submission's chunk): expected = wsz bytes per chunk, compared with
 * bytes [goff, goff + wsz) of the chunk's digest; ok = one byte per chunk;
 * md5_out = 16 bytes per chunk or NULL (upgrade: the records' MD5s, host
 * only); nbad = a counter the mismatches are ADDED to, atomically, when a
 * launch retires, or NULL; on_device: expected and ok are device memory.
 *   md5hip_verify_src   md5hip_submit_src's sibling: chunks [lo, hi) of a
 *                       source as verify segments, results to ok + lo,
 *                       md5_out + 16 lo, expected from expected + wsz lo;
 *                       *nbad is not zeroed (the parts of a pool's
 *                       submission share it).  -ENOSYS without the compare
 *                       launcher, -ENOMEM if the batcher's verify buffers
 *                       cannot be allocated: nothing enqueued either way. */
struct md5hip_verify_opt {
    const void *expected;
    unsigned char *ok, *md5_out;
    uint64_t *nbad;
    uint32_t goff, wsz;
    int on_device;
};
__attribute__((visibility("hidden")))
int md5hip_verify_src(struct md5hip_batcher *b, int kind, uint32_t fastcrc, const struct md5hip_src *src,
                      uint64_t lo, uint64_t hi, const struct md5hip_verify_opt *v, uint64_t *ticket, int urgent);

#ifdef __cplusplus
}
#endif

#endif
