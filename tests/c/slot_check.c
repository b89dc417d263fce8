/*
 * slot_check.c -- TEST INFRASTRUCTURE: the batcher's slot routes with no
 * device (tests/test_slot_routes.py).  Links md5_submit.c, md5_stream.c and
 * nc_digest.c against the fake runtime (fake_hip.c, its record log on) and the
 * plain MD5_CRC32 stand-ins (fake_dual.c); the entries that name the one-pass
 * kernel, and its planner, are stand-ins here that log what they were given.
 *
 * Reads the cases of tests/slot_cases.py on stdin, one word at a time:
 *   arenas H D O              bytes of the host, "device" and device-output arenas
 *   case ID
 *   create B slice nslots     md5hip_batcher_create  | create Q max_chunks nslots
 *   digest kind fastcrc | gather mode | inflight target | refuse every
 *   reg off bytes | unreg off md5hip_host_register on the host arena
 *   hold | release            fake_hip_hold: every launch stays in flight
 *   mark                      a `mark` line in the log
 *   sub ENTRY sync outkind outoff n ...    one submission
 *        ENTRY ptrs: n x (off len)          host arena
 *              iov:  n x (nseg, nseg x (off len))
 *              dev:  n x (off len)          device arena
 *              hostfixed | devfixed: base len stride
 *        outkind h = a host array of the program's, d = device-output arena + outoff
 *   waitall                   md5_batch_wait on every asynchronous ticket
 *   end                       checks, stats, destroy
 * and prints per case the fake's records, `rc|k|value` per submission,
 * `digests|k|ok` (or `bad|chunk`) against the host MD5 / CRC-32 of the source
 * bytes, `guard|ok` when no byte of the output arena outside the submissions'
 * own records lost its 0xAA, and the batcher's counters.
 * Nothing here is part of the product.
 */
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "md5.h"
#include "md5hip.h"
#include "nc_digest.h"

extern FILE *fake_hip_log;
extern int fake_hip_hold;
extern unsigned fake_hip_sort_refuse_every;
void fake_hip_name(const void *p, size_t len, const char *name);
void fake_hip_logf(const char *fmt, ...);
const char *fake_hip_where(const void *p, char buf[64]);
void fake_hip_log_desc(const char *what, int variant, uint64_t n, uint32_t fastcrc, const void *base,
                       const uint64_t *off, const uint32_t *len, const uint32_t *ord, const void *out);

/* ------------------------------------------------ the one-pass kind's named entries */
enum { FAKE_CUS = 256 };

int md5crc32hip_plan(uint64_t n, uint64_t mean_len)
{
    fake_hip_logf("choice|dual|%llu|%llu", (unsigned long long)n, (unsigned long long)mean_len);
    return n && (n + 63) / 64 <= FAKE_CUS && mean_len >= MD5CRC32HIP_FEDSPLIT_MIN_LEN &&
                   n * 256 <= FAKE_CUS * mean_len
               ? MD5CRC32HIP_FEDSPLIT
               : MD5CRC32HIP_XDMA16;
}

int md5crc32hip_desc_variant(const void *d_base, const uint64_t *d_offsets, const uint32_t *d_lens,
                             const uint32_t *d_order, uint64_t n, struct md5hip_md5crc32 *d_out, void *stream,
                             int variant)
{
    fake_hip_log_desc("dual_desc", variant, n, 0, d_base, d_offsets, d_lens, d_order, d_out);
    return md5crc32hip_desc(d_base, d_offsets, d_lens, d_order, n, d_out, stream);
}

int md5crc32hip_fixed_variant(const void *d_base, uint64_t n, uint32_t len, uint64_t stride,
                              struct md5hip_md5crc32 *d_out, void *stream, int variant)
{
    char b0[64], b1[64];
    (void)variant;                    /* the batcher always passes AUTO */
    fake_hip_logf("hash|dual_fixed|%llu|%u|%llu|0|%s|%s", (unsigned long long)n, len, (unsigned long long)stride,
                  fake_hip_where(d_base, b0), fake_hip_where(d_out, b1));
    return md5crc32hip_fixed(d_base, n, len, stride, d_out, stream);
}

/* ------------------------------------------------ arenas and submissions */
static unsigned char *H, *D, *O, *omask;
static size_t nH, nD, nO;

struct piece { const unsigned char *p; uint32_t len; };
struct sub {
    uint64_t n, ticket;
    int async, rc, on_device;
    unsigned char *out;               /* host array (owned) or into O */
    struct piece *pieces;             /* every chunk's segments, in order */
    uint64_t *first;                  /* chunk i = pieces [first[i], first[i + 1]) */
    void *a0, *a1, *a2;               /* the arrays the call was given */
};
static struct sub subs[8192];
static unsigned nsubs;

static void die(const char *what)
{
    fflush(stdout);
    fprintf(stderr, "slot_check: %s\n", what);
    exit(2);
}

static unsigned long long num(void)
{
    unsigned long long v;
    if (scanf("%llu", &v) != 1) die("a number expected");
    return v;
}

static void *xalloc(size_t bytes)
{
    void *p = calloc(bytes ? bytes : 1, 1);
    if (!p) die("out of memory");
    return p;
}

static void fill(unsigned char *p, size_t n, uint64_t x)
{
    for (size_t i = 0; i < n; i++) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        p[i] = (unsigned char)(x >> 24);
    }
}

static unsigned char *in_arena(unsigned char *base, size_t size, unsigned long long off, unsigned long long len)
{
    if (off > size || len > size - off) die("a chunk outside its arena");
    return base + off;
}

/* the digest of `kind` of the bytes of chunk i of submission s, into out[32] */
static void want_digest(const struct sub *s, uint64_t i, int kind, uint32_t F, unsigned char *out)
{
    uint64_t L = 0;
    for (uint64_t k = s->first[i]; k < s->first[i + 1]; k++) L += s->pieces[k].len;
    unsigned char *buf = xalloc(L), *at = buf;
    for (uint64_t k = s->first[i]; k < s->first[i + 1]; k++) {
        if (s->pieces[k].len) memcpy(at, s->pieces[k].p, s->pieces[k].len);
        at += s->pieces[k].len;
    }
    memset(out, 0, 32);
    if (kind != MD5HIP_DIGEST_CRC32) {
        struct MD5Context c;
        MD5Init(&c);
        MD5Update(&c, buf, (unsigned)L);
        MD5Final(out, &c);
    }
    if (kind != MD5HIP_DIGEST_MD5) {
        const uint32_t crc = (F == 0 || L <= F) ? nc_crc32(buf, L) : nc_crc32(buf, F) ^ nc_crc32(buf + (L - F), F);
        unsigned char *c = out + (kind == MD5HIP_DIGEST_CRC32 ? 0 : 16);
        c[0] = (unsigned char)crc; c[1] = (unsigned char)(crc >> 8);
        c[2] = (unsigned char)(crc >> 16); c[3] = (unsigned char)(crc >> 24);
    }
    free(buf);
}

int main(void)
{
    char word[64], id[64] = "";
    md5hip_batcher *b = NULL;
    int kind = MD5HIP_DIGEST_MD5;
    uint32_t fastcrc = 0, dsz = 16;
    unsigned long long regs[64];
    unsigned nregs = 0;
    fake_hip_log = stdout;
    while (scanf("%63s", word) == 1) {
        if (!strcmp(word, "arenas")) {
            nH = num(); nD = num(); nO = num();
            if (posix_memalign((void **)&H, 4096, nH) || posix_memalign((void **)&D, 4096, nD) ||
                posix_memalign((void **)&O, 4096, nO))
                die("out of memory");
            omask = xalloc(nO);
            fill(H, nH, 0x9E3779B97F4A7C15ull);
            fill(D, nD, 0xD1B54A32D192ED03ull);
            fake_hip_name(H, nH, "H");
            fake_hip_name(D, nD, "D");
            fake_hip_name(O, nO, "O");
        } else if (!strcmp(word, "case")) {
            if (scanf("%63s", id) != 1) die("case id");
            printf("case %s\n", id);
            memset(O, 0xAA, nO);
            memset(omask, 0, nO);
            kind = MD5HIP_DIGEST_MD5; fastcrc = 0; dsz = 16;
            fake_hip_sort_refuse_every = 0;
        } else if (!strcmp(word, "create")) {
            if (scanf("%63s", word) != 1) die("create");
            const unsigned long long a = num(), slots = num();
            const int rc = word[0] == 'Q' ? md5hip_queue_create(0, a, (uint32_t)slots, &b)
                                          : md5hip_batcher_create(0, a, (uint32_t)slots, &b);
            if (rc) die("create failed");
        } else if (!strcmp(word, "digest")) {
            kind = (int)num(); fastcrc = (uint32_t)num();
            dsz = kind == MD5HIP_DIGEST_CRC32 ? 4 : kind == MD5HIP_DIGEST_MD5_CRC32 ? 32 : 16;
            if (md5hip_batcher_set_digest(b, kind, fastcrc)) die("set_digest failed");
        } else if (!strcmp(word, "gather")) {
            if (md5hip_batcher_set_gather(b, (int)num())) die("set_gather failed");
        } else if (!strcmp(word, "inflight")) {
            if (md5hip_batcher_set_inflight(b, (uint32_t)num())) die("set_inflight failed");
        } else if (!strcmp(word, "refuse")) {
            fake_hip_sort_refuse_every = (unsigned)num();
        } else if (!strcmp(word, "reg")) {
            const unsigned long long off = num(), len = num();
            if (nregs == 64 || md5hip_host_register(in_arena(H, nH, off, len), len)) die("register failed");
            regs[nregs++] = off;
        } else if (!strcmp(word, "hold")) {
            __atomic_store_n(&fake_hip_hold, 1, __ATOMIC_RELAXED);
        } else if (!strcmp(word, "release")) {
            __atomic_store_n(&fake_hip_hold, 0, __ATOMIC_RELAXED);
        } else if (!strcmp(word, "mark")) {
            fake_hip_logf("mark");
        } else if (!strcmp(word, "sub")) {
            if (nsubs == sizeof subs / sizeof subs[0]) die("too many submissions");
            struct sub *s = &subs[nsubs];
            memset(s, 0, sizeof *s);
            char entry[64], outkind[8];
            if (scanf("%63s", entry) != 1) die("sub entry");
            s->async = !num();
            if (scanf("%7s", outkind) != 1) die("sub outkind");
            const unsigned long long outoff = num();
            const uint64_t n = s->n = num();
            s->on_device = outkind[0] == 'd';
            if (s->on_device) {
                s->out = in_arena(O, nO, outoff, (unsigned long long)dsz * n);
                memset(omask + outoff, 1, (size_t)dsz * n);
            } else {
                s->out = xalloc((size_t)dsz * n);
            }
            s->first = xalloc(sizeof(uint64_t) * (n + 1));
            uint64_t *ticket = s->async ? &s->ticket : NULL;
            if (!strcmp(entry, "ptrs") || !strcmp(entry, "dev")) {
                const int dev = entry[0] == 'd';
                s->pieces = xalloc(sizeof(struct piece) * n);
                const void **ptrs = xalloc(sizeof(void *) * n);
                uint64_t *dptrs = xalloc(sizeof(uint64_t) * n);
                uint32_t *lens = xalloc(sizeof(uint32_t) * n);
                s->a0 = ptrs; s->a1 = dptrs; s->a2 = lens;
                for (uint64_t i = 0; i < n; i++) {
                    const unsigned long long off = num(), len = num();
                    ptrs[i] = dev ? in_arena(D, nD, off, len) : in_arena(H, nH, off, len);
                    dptrs[i] = (uint64_t)(uintptr_t)ptrs[i];
                    lens[i] = (uint32_t)len;
                    s->pieces[i] = (struct piece){ptrs[i], (uint32_t)len};
                    s->first[i] = i;
                }
                s->first[n] = n;
                s->rc = dev ? (s->async ? md5_batch_submit_device_async(b, dptrs, lens, n, s->out, s->on_device, ticket)
                                        : md5_batch_submit_device(b, dptrs, lens, n, s->out, s->on_device))
                            : (s->async ? md5_batch_submit_async(b, ptrs, lens, n, s->out, ticket)
                                        : md5_batch_submit(b, ptrs, lens, n, s->out));
            } else if (!strcmp(entry, "iov")) {
                size_t cap = 64, np = 0;
                struct md5hip_iov *segs = xalloc(sizeof *segs * cap);
                uint64_t *sf = xalloc(sizeof(uint64_t) * (n + 1));
                for (uint64_t i = 0; i < n; i++) {
                    const uint64_t ns = num();
                    sf[i] = np;
                    for (uint64_t k = 0; k < ns; k++) {
                        if (np == cap) {
                            segs = realloc(segs, sizeof *segs * (cap *= 2));
                            if (!segs) die("out of memory");
                        }
                        const unsigned long long off = num(), len = num();
                        segs[np++] = (struct md5hip_iov){in_arena(H, nH, off, len), (uint32_t)len};
                    }
                }
                sf[n] = np;
                s->pieces = xalloc(sizeof(struct piece) * np);
                for (size_t k = 0; k < np; k++) s->pieces[k] = (struct piece){segs[k].base, segs[k].len};
                memcpy(s->first, sf, sizeof(uint64_t) * (n + 1));
                s->a0 = segs; s->a1 = sf;
                s->rc = s->async ? md5_batch_submit_iov_async(b, segs, sf, n, s->out, ticket)
                                 : md5_batch_submit_iov(b, segs, sf, n, s->out);
            } else if (!strcmp(entry, "hostfixed") || !strcmp(entry, "devfixed")) {
                const int dev = entry[0] == 'd';
                const unsigned long long base = num(), len = num(), stride = num();
                const unsigned long long span = n ? (n - 1) * stride + len : 0;
                const unsigned char *p = dev ? in_arena(D, nD, base, span) : in_arena(H, nH, base, span);
                s->pieces = xalloc(sizeof(struct piece) * n);
                for (uint64_t i = 0; i < n; i++) {
                    s->pieces[i] = (struct piece){p + i * stride, (uint32_t)len};
                    s->first[i] = i;
                }
                s->first[n] = n;
                if (!dev && s->async) die("host_fixed is synchronous");
                s->rc = dev ? md5_batch_submit_device_fixed(b, p, n, (uint32_t)len, stride, s->out, s->on_device, NULL,
                                                            0, ticket)
                            : md5hip_batch_host_fixed(b, p, n, (uint32_t)len, stride, s->out);
            } else {
                die("unknown entry");
            }
            printf("rc|%u|%d\n", nsubs, s->rc);
            nsubs++;
        } else if (!strcmp(word, "waitall")) {
            for (unsigned k = 0; k < nsubs; k++)
                if (subs[k].async && subs[k].rc == 0) {
                    const int rc = md5_batch_wait(b, subs[k].ticket);
                    if (rc) printf("wait|%u|%d\n", k, rc);
                }
        } else if (!strcmp(word, "end")) {
            for (unsigned k = 0; k < nsubs; k++) {
                const struct sub *s = &subs[k];
                long bad = -1;
                unsigned char want[32];
                for (uint64_t i = 0; i < s->n && bad < 0 && s->rc == 0; i++) {
                    want_digest(s, i, kind, fastcrc, want);
                    if (memcmp(want, s->out + (size_t)dsz * i, dsz)) bad = (long)i;
                }
                if (bad < 0) printf("digests|%u|ok\n", k);
                else printf("digests|%u|bad|%ld\n", k, bad);
            }
            size_t hurt = nO;
            for (size_t i = 0; i < nO && hurt == nO; i++)
                if (!omask[i] && O[i] != 0xAA) hurt = i;
            if (hurt == nO) printf("guard|ok\n");
            else printf("guard|bad|%zu\n", hurt);
            struct md5hip_batcher_stats st;
            md5hip_batcher_get_stats(b, &st);
            printf("stats|submissions=%llu|launches=%llu|coalesced_launches=%llu|chunks=%llu|bytes_staged=%llu|"
                   "max_chunks_per_launch=%llu|max_tickets_per_launch=%llu\n",
                   (unsigned long long)st.submissions, (unsigned long long)st.launches,
                   (unsigned long long)st.coalesced_launches, (unsigned long long)st.chunks,
                   (unsigned long long)st.bytes_staged, (unsigned long long)st.max_chunks_per_launch,
                   (unsigned long long)st.max_tickets_per_launch);
            md5hip_batcher_destroy(b);
            b = NULL;
            for (unsigned k = 0; k < nregs; k++)
                if (md5hip_host_unregister(H + regs[k])) die("unregister failed");
            nregs = 0;
            for (unsigned k = 0; k < nsubs; k++) {
                struct sub *s = &subs[k];
                if (!s->on_device) free(s->out);
                free(s->pieces); free(s->first); free(s->a0); free(s->a1); free(s->a2);
            }
            nsubs = 0;
            printf("end\n");
        } else {
            die("unknown word");
        }
    }
    free(H); free(D); free(O); free(omask);
    return 0;
}
