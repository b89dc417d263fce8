/*
 * pool_routes.c -- runs the scripts of tests/pool_cases.py on the multi-GPU
 * pool (sproxy_amd/csrc/md5_pool.c) with NO device and prints what the pool
 * did, one line per fact; tests/test_pool_routes.py holds the lines against
 * the table.  Only md5hip_pool_* entries are called.  The batcher entries
 * the pool calls are a scripted fake defined here (tests/c/pool_check.c has
 * another, for its long scenario):
 *
 *   per device a settable load and a queue of answers for its next
 *   submissions -- T take, N refuse -ENODEV and stay healthy, F refuse
 *   -ENODEV and fail, e take then complete -EIO and stay healthy, E take
 *   then complete -EIO and fail with it, D take then fail before the launch
 *   (the ticket completes -ENODEV), B refuse -E2BIG; an empty queue
 *   answers T, a failed device X (-ENODEV), an empty range Z; "seq CODES"
 *   answers the pool's next submissions whatever their device, so that a
 *   script can aim at a part; "failat G N" fails device G at its N-th health
 *   query from now (between the pool's count of healthy devices and its
 *   choice of them);
 *   md5hip_batcher_inject_fault(after) turns the after-th taken submission
 *   into E;
 *   tickets complete after a few polls, or ("manual 1") only on "finish" --
 *   a wait on a ticket still running then says so ("blocked") and completes
 *   it, so a wait that returns without one is seen;
 *   digests by the library's host MD5 / CRC-32 at the kind's true record
 *   width (32 B: md5, crc little-endian, 12 zero bytes), written at the
 *   submission (a launch that fails writes nothing);
 *   a "src" line per md5hip_submit_src call: submission, device, lo, hi,
 *   kind, fastcrc, urgent, byte offset of its digests in the caller's
 *   array, answer.
 *
 * Script (stdin, words): arena BYTES, then cases: case ID NDEV SLICE ...
 * end.  Steps: split B | digest KIND F | load G W | ans G CODES | fault G
 * AFTER | seq CODES | failat G N | manual 0/1 | finish K | sub ENTRY SYNC
 * NPLAN ... | wait K | poll K | waitnext K (the ticket after K's: never
 * issued) | twait HEX | tpoll HEX | stats | spread N.  Chunk i of a
 * submission lies in the arena after chunks [0, i).  A plain executable,
 * built with ASan + UBSan and run directly.
 */
#include <errno.h>
#include <inttypes.h>
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "md5.h"
#include "md5hip.h"
#include "nc_digest.h"
#include "../../sproxy_amd/csrc/md5_internal.h"

#define DIE(...)                                                             \
    do {                                                                     \
        printf("FAIL line %d: ", __LINE__);                                  \
        printf(__VA_ARGS__);                                                 \
        printf("\n");                                                        \
        exit(1);                                                             \
    } while (0)

#define GUARD 64
#define MAX_SUBS 256
#define MAX_DEV 8

/* the one-pass kind's launchers, so that the pool takes the kind: never called */
int md5crc32hip_fixed(const void *d_base, uint64_t n, uint32_t len, uint64_t stride, struct md5hip_md5crc32 *d_out,
                      void *stream)
{
    (void)d_base; (void)n; (void)len; (void)stride; (void)d_out; (void)stream;
    return -ENOSYS;
}

int md5crc32hip_desc(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens, const uint32_t *d_order,
                     uint64_t n, struct md5hip_md5crc32 *d_out, void *stream)
{
    (void)d_base; (void)d_offsets; (void)d_lens; (void)d_order; (void)n; (void)d_out; (void)stream;
    return -ENOSYS;
}

/* ------------------------------------------------------------------ digests */
static uint32_t dsz_of(int kind) { return kind == MD5HIP_DIGEST_CRC32 ? 4 : kind == MD5HIP_DIGEST_MD5_CRC32 ? 32 : 16; }

/* md5hip.h: the whole chunk's CRC for 'fastcrc == 0 || len <= fastcrc', else head ^ tail */
static uint32_t crc_of(const unsigned char *b, uint64_t L, uint32_t fastcrc)
{
    if (fastcrc == 0 || L <= fastcrc) return nc_crc32(b, L);
    return nc_crc32(b, fastcrc) ^ nc_crc32(b + L - fastcrc, fastcrc);
}

/* one record of `kind` for the bytes of segs[0..nseg) into out[0..dsz) */
static void digest_one(int kind, uint32_t fastcrc, const struct md5hip_iov *segs, uint64_t nseg, unsigned char *out)
{
    uint64_t L = 0;
    for (uint64_t k = 0; k < nseg; k++) L += segs[k].len;
    unsigned char *tmp = malloc(L ? L : 1);
    uint64_t at = 0;
    for (uint64_t k = 0; k < nseg; k++) {
        if (segs[k].len) memcpy(tmp + at, segs[k].base, segs[k].len);
        at += segs[k].len;
    }
    unsigned char rec[32] = {0};
    if (kind != MD5HIP_DIGEST_CRC32) {
        struct MD5Context ctx;
        MD5Init(&ctx);
        MD5Update(&ctx, tmp, (unsigned)L);
        MD5Final(rec, &ctx);
    }
    if (kind != MD5HIP_DIGEST_MD5) {
        const uint32_t c = crc_of(tmp, L, fastcrc);
        unsigned char *p = rec + (kind == MD5HIP_DIGEST_CRC32 ? 0 : 16);
        p[0] = (unsigned char)c; p[1] = (unsigned char)(c >> 8); p[2] = (unsigned char)(c >> 16); p[3] = (unsigned char)(c >> 24);
    }
    memcpy(out, rec, dsz_of(kind));
    free(tmp);
}

/* chunk c of a source as segments: their count (at most `cap`) */
static uint64_t src_chunk(const struct md5hip_src *s, uint64_t c, struct md5hip_iov *one, const struct md5hip_iov **segs)
{
    if (s->kind == MD5HIP_SRC_IOV) {
        *segs = s->segs + s->seg_first[c];
        return s->seg_first[c + 1] - s->seg_first[c];
    }
    if (s->kind == MD5HIP_SRC_PTRS) *one = (struct md5hip_iov){s->ptrs[c], s->lens[c]};
    else *one = (struct md5hip_iov){s->base + c * s->stride, s->len};
    *segs = one;
    return 1;
}

/* ------------------------------------------------------------------ the scripted fake batcher */
struct fake_ticket {
    int done, polls_left, err, fails_device;
    uint64_t weight, lo, hi;
    int owner;                         /* the submission it belongs to */
};

struct md5hip_batcher {
    int device, lost;
    uint64_t slice, base_load, load, lose_in;
    uint64_t submissions, chunks;
    char ans[256];
    size_t ans_at;
    uint64_t fail_at_query;            /* the device reads failed from this health query on */
    struct fake_ticket *tk;
    uint64_t ntk, captk;
};

static char g_seq[512];                /* answers for the pool's next submissions whatever their device */
static size_t g_seq_at;
static struct md5hip_batcher *g_b[MAX_DEV]; /* the pool's batchers by device index */
static int g_manual;                   /* tickets complete only on "finish" (or at a wait, which says so) */
static int g_cur = -1;                 /* the submission being made */
static int g_quiet;                    /* no src lines ("spread") */
static const unsigned char *g_cur_base; /* its digest array, NULL if the pool allocates one */

struct src_rec {
    int sub, dev, kind, urgent;
    uint32_t fastcrc;
    uint64_t lo, hi;
    const unsigned char *dig;
    char ans;
};
static struct src_rec g_rec[64];
static int g_nrec;

int md5hip_batcher_create(int device, uint64_t slice_bytes, uint32_t nslots, md5hip_batcher **out)
{
    (void)nslots;
    md5hip_batcher *b = calloc(1, sizeof *b);
    if (!b) return -ENOMEM;
    b->device = device;
    b->slice = slice_bytes;
    g_b[device] = b;
    *out = b;
    return 0;
}

void md5hip_batcher_destroy(md5hip_batcher *b)
{
    if (!b) return;
    free(b->tk);
    free(b);
}

int md5hip_batcher_set_gather(md5hip_batcher *b, int mode) { return b && mode >= 0 && mode <= 3 ? 0 : -EINVAL; }

int md5hip_batcher_health(const md5hip_batcher *cb)
{
    md5hip_batcher *b = g_b[cb->device];
    if (b->fail_at_query && --b->fail_at_query == 0) b->lost = -ENODEV;
    return b->lost;
}

uint64_t md5hip_batcher_load(const md5hip_batcher *b) { return b->base_load + b->load; }
uint64_t md5hip_batcher_slice(const md5hip_batcher *b) { return b->slice; }

int md5hip_batcher_inject_fault(md5hip_batcher *b, uint64_t after)
{
    if (b->lost) return b->lost;
    b->lose_in = after;
    return 0;
}

int md5hip_batcher_get_stats(md5hip_batcher *b, struct md5hip_batcher_stats *out)
{
    memset(out, 0, sizeof *out);
    out->submissions = b->submissions;
    out->launches = b->submissions;
    out->chunks = b->chunks;
    return 0;
}

static void fake_complete(md5hip_batcher *b, struct fake_ticket *k)
{
    if (k->done) return;
    k->done = 1;
    k->polls_left = 0;
    b->load -= k->weight;
    if (k->fails_device) b->lost = -ENODEV;
}

/* 1 done / 0 running / -EINVAL; advance = this call is a poll or a wait */
static int fake_state(md5hip_batcher *b, uint64_t t, int advance, int *err)
{
    *err = 0;
    if (t == 0 || t > b->ntk) return -EINVAL;
    struct fake_ticket *k = &b->tk[t - 1];
    if (!k->done && advance && !g_manual && --k->polls_left <= 0) fake_complete(b, k);
    if (k->done) *err = k->err;
    return k->done;
}

int md5hip_submit_src(md5hip_batcher *b, int kind, uint32_t fastcrc, const struct md5hip_src *src, uint64_t lo,
                      uint64_t hi, unsigned char *digests, uint64_t *ticket, int urgent)
{
    if (ticket) *ticket = 0;
    const uint64_t n = hi - lo;
    char a = 'T';
    if (n == 0) a = 'Z';
    else if (b->lost) a = 'X';
    else {
        if (g_seq[g_seq_at]) a = g_seq[g_seq_at++];
        else if (b->ans[b->ans_at]) a = b->ans[b->ans_at++];
        if ((a == 'T' || a == 'e' || a == 'E' || a == 'D') && b->lose_in && --b->lose_in == 0) a = 'E';
    }
    if (!g_quiet) {
        if (g_nrec == 64) DIE("more than 64 device submissions in one pool call");
        g_rec[g_nrec++] = (struct src_rec){g_cur, b->device, kind, urgent, fastcrc, lo, hi, digests, a};
    }
    switch (a) {
    case 'Z': return 0;
    case 'F': b->lost = -ENODEV; /* fall through */
    case 'X':
    case 'N': return -ENODEV;
    case 'B': return -E2BIG;
    default: break;
    }
    const int fails = a != 'T';
    const uint32_t dsz = dsz_of(kind);
    uint64_t weight = 0;
    for (uint64_t i = 0; i < n; i++) {
        struct md5hip_iov one;
        const struct md5hip_iov *segs;
        const uint64_t ns = src_chunk(src, src->first + lo + i, &one, &segs);
        for (uint64_t k = 0; k < ns; k++) weight += segs[k].len;
        weight += 64;
        if (!fails) digest_one(kind, fastcrc, segs, ns, digests + (size_t)dsz * i);
    }
    if (b->ntk == b->captk) {
        b->captk = b->captk ? 2 * b->captk : 64;
        b->tk = realloc(b->tk, b->captk * sizeof *b->tk);
        if (!b->tk) DIE("no memory");
    }
    const uint64_t id = ++b->ntk;
    b->tk[id - 1] = (struct fake_ticket){0, 1 + (int)(id % 3), a == 'D' ? -ENODEV : fails ? -EIO : 0, a == 'E' || a == 'D', weight, lo, hi, g_cur};
    b->load += weight;
    b->submissions++;
    b->chunks += n;
    if (!ticket) {
        fake_complete(b, &b->tk[id - 1]);
        return b->tk[id - 1].err;
    }
    *ticket = id;
    return 0;
}

int md5hip_batcher_ticket_state(md5hip_batcher *b, uint64_t ticket, int *err)
{
    *err = 0;
    if (ticket == 0) return 1;
    return fake_state(b, ticket, 0, err);
}

int md5_batch_wait(md5hip_batcher *b, uint64_t ticket)
{
    if (ticket == 0) return 0;
    int err = 0, r;
    while ((r = fake_state(b, ticket, 1, &err)) == 0) {
        if (!g_manual) continue;
        struct fake_ticket *k = &b->tk[ticket - 1];
        printf("blocked|%d|%" PRIu64 "|%" PRIu64 "\n", k->owner, k->lo, k->hi);
        fake_complete(b, k);
    }
    return r < 0 ? r : err;
}

int md5_batch_poll(md5hip_batcher *b, uint64_t ticket)
{
    if (ticket == 0) return 1;
    int err = 0;
    const int r = fake_state(b, ticket, 1, &err);
    if (r < 0) return r;
    return r == 1 && err ? err : r;
}

/* ------------------------------------------------------------------ the runner */
struct sub {
    char entry[16];
    int sync, kind;
    uint32_t fastcrc;
    uint64_t n, ticket;
    const void **ptrs;
    uint32_t *lens;
    struct md5hip_iov *segs;
    uint64_t *seg_first;
    uint32_t flen;
    uint64_t stride;
    unsigned char *dig;                /* GUARD + dsz * n + GUARD, 0xAA before the call */
};

static unsigned char *g_arena;
static uint64_t g_arena_bytes;
static md5hip_pool *g_pool;
static uint32_t g_ndev;
static struct sub g_sub[MAX_SUBS];
static int g_nsub;
static int g_kind;                     /* the pool's digest kind, as set by this script */
static uint32_t g_fastcrc;

static char g_word[64];

static const char *word(void)
{
    if (scanf("%63s", g_word) != 1) DIE("script ends inside a case");
    return g_word;
}

static uint64_t num(void) { return strtoull(word(), NULL, 0); }

static uint64_t chunk_segs(const struct sub *s, uint64_t i, struct md5hip_iov *one, const struct md5hip_iov **segs)
{
    if (s->segs) {
        *segs = s->segs + s->seg_first[i];
        return s->seg_first[i + 1] - s->seg_first[i];
    }
    if (s->ptrs) *one = (struct md5hip_iov){s->ptrs[i], s->lens[i]};
    else *one = (struct md5hip_iov){g_arena + i * s->stride, s->flen};
    *segs = one;
    return 1;
}

static void want_one(const struct sub *s, int kind, uint32_t fastcrc, uint64_t i, unsigned char *out)
{
    struct md5hip_iov one;
    const struct md5hip_iov *segs;
    const uint64_t ns = chunk_segs(s, i, &one, &segs);
    digest_one(kind, fastcrc, segs, ns, out);
}

static void print_digests(int k)
{
    const struct sub *s = &g_sub[k];
    const uint32_t dsz = dsz_of(s->kind);
    for (uint64_t i = 0; i < s->n; i++) {
        unsigned char w[32];
        want_one(s, s->kind, s->fastcrc, i, w);
        if (memcmp(w, s->dig + GUARD + (size_t)dsz * i, dsz)) {
            printf("digests|%d|bad@%" PRIu64 "\n", k, i);
            return;
        }
    }
    printf("digests|%d|ok\n", k);
}

static int guards_ok(const struct sub *s)
{
    if (!s->dig) return 1;
    const size_t body = (size_t)dsz_of(s->kind) * s->n;
    for (size_t k = 0; k < GUARD; k++)
        if (s->dig[k] != 0xAA || s->dig[GUARD + body + k] != 0xAA) return 0;
    return 1;
}

static void flush_records(uint32_t dsz)
{
    const unsigned char *base = g_cur_base;
    if (!base && g_nrec) base = g_rec[0].dig - (size_t)dsz * g_rec[0].lo;
    for (int r = 0; r < g_nrec; r++) {
        const struct src_rec *q = &g_rec[r];
        printf("src|%d|%d|%" PRIu64 "|%" PRIu64 "|%d|%u|%d|%lld|%c\n", q->sub, q->dev, q->lo, q->hi, q->kind,
               q->fastcrc, q->urgent, (long long)(q->dig - base), q->ans);
    }
    g_nrec = 0;
}

static void print_ticket(int k, int rc, uint64_t t)
{
    if (t == 0) printf("rc|%d|%d|0\n", k, rc);
    else if (t >> 63) printf("rc|%d|%d|s\n", k, rc);
    else printf("rc|%d|%d|w%u\n", k, rc, (unsigned)(t & 63));
}

/* sub ENTRY SYNC NPLAN: ptrs N len..., iov|verify|upgrade N (NSEG len...)... [BAD], fixed N LEN STRIDE */
static void do_sub(void)
{
    if (g_nsub == MAX_SUBS) DIE("too many submissions in one case");
    const int k = g_nsub++;
    struct sub *s = &g_sub[k];
    memset(s, 0, sizeof *s);
    snprintf(s->entry, sizeof s->entry, "%s", word());
    s->sync = (int)num();
    const uint32_t nplan = (uint32_t)num();
    s->n = num();
    const int iov = !strcmp(s->entry, "iov") || !strcmp(s->entry, "verify") || !strcmp(s->entry, "upgrade");
    uint32_t *tot = calloc(s->n + 1, sizeof *tot);
    uint64_t at = 0;
    if (!strcmp(s->entry, "ptrs")) {
        s->ptrs = calloc(s->n + 1, sizeof *s->ptrs);
        s->lens = calloc(s->n + 1, sizeof *s->lens);
        for (uint64_t i = 0; i < s->n; i++) {
            tot[i] = s->lens[i] = (uint32_t)num();
            s->ptrs[i] = g_arena + at;
            at += s->lens[i];
        }
    } else if (iov) {
        s->seg_first = calloc(s->n + 1, sizeof *s->seg_first);
        uint64_t cap = 16, ns = 0;
        s->segs = calloc(cap, sizeof *s->segs);
        for (uint64_t i = 0; i < s->n; i++) {
            s->seg_first[i] = ns;
            const uint64_t c = num();
            for (uint64_t j = 0; j < c; j++) {
                if (ns == cap) s->segs = realloc(s->segs, (cap *= 2) * sizeof *s->segs);
                const uint64_t len = num();
                s->segs[ns++] = (struct md5hip_iov){g_arena + at, len};
                at += len;
                tot[i] += (uint32_t)len;
            }
        }
        s->seg_first[s->n] = ns;
    } else if (!strcmp(s->entry, "fixed")) {
        s->flen = (uint32_t)num();
        s->stride = num();
        at = s->n ? (s->n - 1) * s->stride + s->flen : 0;
    } else DIE("entry %s", s->entry);
    if (at > g_arena_bytes) DIE("submission of %" PRIu64 " bytes, arena of %" PRIu64, at, g_arena_bytes);
    s->kind = g_kind;
    s->fastcrc = g_fastcrc;
    if (nplan > 1) {
        uint64_t first[MAX_DEV + 1];
        if (nplan > MAX_DEV) DIE("plan of %u parts", nplan);
        const int rc = md5hip_pool_plan(s->stride ? NULL : tot, s->n, nplan, first);
        printf("plan|%d|%d|", k, rc);
        for (uint32_t g = 0; g <= nplan; g++) printf("%s%" PRIu64, g ? "," : "", first[g]);
        printf("\n");
    }
    g_cur = k;
    int rc;
    if (!strcmp(s->entry, "verify") || !strcmp(s->entry, "upgrade")) {
        const int bad = (int)strtol(word(), NULL, 0);
        const int up = s->entry[0] == 'u';
        const uint32_t dsz = up ? 4 : dsz_of(g_kind);
        unsigned char *exp = calloc(s->n + 1, 32);
        unsigned char *ok = calloc(s->n + 1, 1), *md5s = calloc(s->n + 1, 16);
        for (uint64_t i = 0; i < s->n; i++)
            want_one(s, up ? MD5HIP_DIGEST_CRC32 : g_kind, up ? 0 : g_fastcrc, i, exp + (size_t)dsz * i);
        if (bad >= 0) exp[(size_t)dsz * (size_t)bad] ^= 1;
        g_cur_base = NULL;
        if (up) rc = md5hip_pool_upgrade_iov(g_pool, s->segs, s->seg_first, s->n, (const uint32_t *)(void *)exp, ok, md5s);
        else rc = md5hip_pool_verify_iov(g_pool, s->segs, s->seg_first, s->n, exp, ok);
        flush_records(up ? 32 : dsz);
        printf("%s|%d|%d|", s->entry, k, rc);
        for (uint64_t i = 0; i < s->n; i++) printf("%d", ok[i]);
        if (up) {
            int good = 1;
            for (uint64_t i = 0; i < s->n; i++) {
                unsigned char w[16];
                want_one(s, MD5HIP_DIGEST_MD5, 0, i, w);
                good &= !memcmp(w, md5s + 16 * i, 16);
            }
            printf("|md5=%s", good ? "ok" : "bad");
        }
        printf("\n");
        free(exp);
        free(ok);
        free(md5s);
        free(tot);
        return;
    }
    free(tot);
    const size_t body = (size_t)dsz_of(s->kind) * s->n;
    s->dig = malloc(2 * GUARD + body);
    memset(s->dig, 0xAA, 2 * GUARD + body);
    unsigned char *out = s->dig + GUARD;
    g_cur_base = out;
    s->ticket = 0xdead;                                  /* an asynchronous entry sets it, always */
    if (s->stride) rc = md5hip_pool_host_fixed(g_pool, g_arena, s->n, s->flen, s->stride, out);
    else if (s->ptrs && s->sync) rc = md5hip_pool_submit(g_pool, s->ptrs, s->lens, s->n, out);
    else if (s->ptrs) rc = md5hip_pool_submit_async(g_pool, s->ptrs, s->lens, s->n, out, &s->ticket);
    else if (s->sync) rc = md5hip_pool_submit_iov(g_pool, s->segs, s->seg_first, s->n, out);
    else rc = md5hip_pool_submit_iov_async(g_pool, s->segs, s->seg_first, s->n, out, &s->ticket);
    if (s->sync) s->ticket = 0;
    flush_records(dsz_of(s->kind));
    print_ticket(k, rc, s->ticket);
    if (s->sync && rc == 0) print_digests(k);
}

static void do_stats(void)
{
    struct md5hip_pool_stats st;
    struct md5hip_pool_health h;
    if (md5hip_pool_get_stats(g_pool, &st) || md5hip_pool_get_health(g_pool, &h)) DIE("stats");
    printf("stats|submissions=%" PRIu64 "|routed_whole=%" PRIu64 "|split=%" PRIu64 "|parts=%" PRIu64 "\n",
           st.submissions, st.routed_whole, st.split, st.parts);
    printf("health|ndev=%u|nfailed=%u|mask=%" PRIx64 "|failovers=%" PRIu64 "\n", h.ndev, h.nfailed, h.failed_mask,
           h.failovers);
    for (uint32_t g = 0; g < g_ndev; g++) {
        struct md5hip_batcher_stats bs;
        if (md5hip_pool_device_stats(g_pool, g, &bs)) DIE("device stats");
        printf("dev|%u|%d|submissions=%" PRIu64 "|chunks=%" PRIu64 "\n", g, md5hip_pool_device_health(g_pool, g),
               bs.submissions, bs.chunks);
    }
}

/* N synchronous whole submissions of 4 chunks of 100 bytes: where they went */
static void do_spread(void)
{
    const int reps = (int)num();
    const void *ptrs[4];
    uint32_t lens[4] = {100, 100, 100, 100};
    unsigned char want[4][16], got[4][16];
    for (int i = 0; i < 4; i++) {
        ptrs[i] = g_arena + 100 * i;
        const struct md5hip_iov one = {ptrs[i], 100};
        digest_one(MD5HIP_DIGEST_MD5, 0, &one, 1, want[i]);
    }
    uint64_t before[MAX_DEV];
    struct md5hip_batcher_stats bs;
    for (uint32_t g = 0; g < g_ndev; g++) {
        md5hip_pool_device_stats(g_pool, g, &bs);
        before[g] = bs.submissions;
    }
    int rcs = 0, bad = 0;
    g_quiet = 1;
    for (int r = 0; r < reps; r++) {
        memset(got, 0, sizeof got);
        rcs += md5hip_pool_submit(g_pool, ptrs, lens, 4, &got[0][0]) != 0;
        bad += memcmp(got, want, dsz_of(g_kind) == 16 ? sizeof got : 0) != 0;
    }
    g_quiet = 0;
    printf("spread|%d|%d|", rcs, bad);
    for (uint32_t g = 0; g < g_ndev; g++) {
        md5hip_pool_device_stats(g_pool, g, &bs);
        printf("%s%" PRIu64, g ? "," : "", bs.submissions - before[g]);
    }
    printf("|healthy=");
    for (uint32_t g = 0; g < g_ndev; g++) printf("%d", md5hip_pool_device_health(g_pool, g) == 0);
    printf("\n");
}

static struct sub *sub_arg(int *k)
{
    *k = (int)num();
    if (*k < 0 || *k >= g_nsub) DIE("no submission %d", *k);
    return &g_sub[*k];
}

static void run_case(void)
{
    printf("case %s\n", word());
    g_ndev = (uint32_t)num();
    const uint64_t slice = num();
    if (g_ndev == 0 || g_ndev > MAX_DEV) DIE("%u devices", g_ndev);
    int devs[MAX_DEV];
    for (uint32_t g = 0; g < g_ndev; g++) devs[g] = (int)g;
    g_nsub = 0;
    g_manual = 0;
    g_seq[0] = 0;
    g_seq_at = 0;
    g_kind = MD5HIP_DIGEST_MD5;
    g_fastcrc = 0;
    if (md5hip_pool_create(devs, g_ndev, slice, 2, &g_pool) || !g_pool) DIE("create");
    if (md5hip_pool_ndev(g_pool) != (int)g_ndev) DIE("ndev");
    for (;;) {
        const char *w = word();
        int k;
        if (!strcmp(w, "end")) break;
        if (!strcmp(w, "split")) {
            printf("split|%d\n", md5hip_pool_set_split(g_pool, num()));
        } else if (!strcmp(w, "digest")) {
            const int kind = (int)num();
            const uint32_t f = (uint32_t)num();
            const int rc = md5hip_pool_set_digest(g_pool, kind, f);
            if (rc == 0) g_kind = kind, g_fastcrc = f;
            printf("digest|%d\n", rc);
        } else if (!strcmp(w, "load")) {
            const uint64_t g = num();
            g_b[g]->base_load = num();
        } else if (!strcmp(w, "ans")) {
            md5hip_batcher *b = g_b[num()];
            snprintf(b->ans, sizeof b->ans, "%s", word());
            b->ans_at = 0;
        } else if (!strcmp(w, "seq")) {
            snprintf(g_seq, sizeof g_seq, "%s", word());
            g_seq_at = 0;
        } else if (!strcmp(w, "failat")) {
            const uint64_t g = num();
            g_b[g]->fail_at_query = num();
        } else if (!strcmp(w, "fault")) {
            const uint32_t g = (uint32_t)num();
            printf("fault|%d\n", md5hip_pool_inject_fault(g_pool, g, num()));
        } else if (!strcmp(w, "manual")) {
            g_manual = (int)num();
        } else if (!strcmp(w, "finish")) {
            sub_arg(&k);
            for (uint32_t g = 0; g < g_ndev; g++)
                for (uint64_t t = 0; t < g_b[g]->ntk; t++)
                    if (g_b[g]->tk[t].owner == k) fake_complete(g_b[g], &g_b[g]->tk[t]);
        } else if (!strcmp(w, "sub")) {
            do_sub();
        } else if (!strcmp(w, "wait") || !strcmp(w, "poll") || !strcmp(w, "waitnext")) {
            const int poll = w[0] == 'p', next = w[4] == 'n';
            const struct sub *s = sub_arg(&k);
            const uint64_t t = s->ticket + (uint64_t)next;
            const int rc = poll ? md5hip_pool_poll(g_pool, t) : md5hip_pool_wait(g_pool, t);
            printf("%s|%d|%d\n", poll ? "poll" : next ? "waitnext" : "wait", k, rc);
            if (!poll && !next && rc == 0) print_digests(k);
        } else if (!strcmp(w, "twait") || !strcmp(w, "tpoll")) {
            const int poll = w[1] == 'p';
            const uint64_t t = num();
            printf("%s|%" PRIx64 "|%d\n", poll ? "tpoll" : "twait", t, poll ? md5hip_pool_poll(g_pool, t) : md5hip_pool_wait(g_pool, t));
        } else if (!strcmp(w, "stats")) {
            do_stats();
        } else if (!strcmp(w, "spread")) {
            do_spread();
        } else DIE("step %s", w);
    }
    /* nothing may still run when the buffers go: the fake completes what is left */
    g_manual = 0;
    for (uint32_t g = 0; g < g_ndev; g++)
        for (uint64_t t = 0; t < g_b[g]->ntk; t++) fake_complete(g_b[g], &g_b[g]->tk[t]);
    int guards = 1;
    for (int k = 0; k < g_nsub; k++) guards &= guards_ok(&g_sub[k]);
    printf("guard|%s\n", guards ? "ok" : "bad");
    md5hip_pool_destroy(g_pool);
    g_pool = NULL;
    for (int k = 0; k < g_nsub; k++) {
        struct sub *s = &g_sub[k];
        free(s->ptrs);
        free(s->lens);
        free(s->segs);
        free(s->seg_first);
        free(s->dig);
    }
    printf("end\n");
}

int main(void)
{
    if (strcmp(word(), "arena")) DIE("the script starts with the arena size");
    g_arena_bytes = num();
    g_arena = malloc(g_arena_bytes + 1);
    /* tests/pool_cases.py arena(): byte k = (k * 2654435761 mod 2^32) >> 24 */
    for (uint64_t k = 0; k < g_arena_bytes; k++) g_arena[k] = (unsigned char)((uint32_t)(k * 2654435761u) >> 24);
    while (scanf("%63s", g_word) == 1) {
        if (strcmp(g_word, "case")) DIE("expected a case, not %s", g_word);
        run_case();
    }
    free(g_arena);
    printf("routes done\n");
    return 0;
}
