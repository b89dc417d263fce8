/*
 * md5_pool.c -- multi-GPU host pool (include/md5hip.h): a
 * router over one coalescing batcher (md5_submit.c) per listed device.
 *
 * The reference calls its chunk checksum (blk_make_crc, blk_io.c:354) from
 * every ASIO pool thread at once, without a lock (asio_mgr.c:205,
 * :1050-1057), one vector of 64-1,024 blocks at a time, and completes the
 * vector as a unit (asio_read_vector_done_LOCK, asio_mgr.c:1414).  So the
 * pool keeps a vector whole: a submission goes to the device whose batcher
 * has the least outstanding weight, where it coalesces with the other
 * threads' vectors into that device's next launch.  Cutting a 64-block
 * vector eight ways would make eight launches, each bound by one 16 KiB
 * chunk's serial chain.  Only a submission heavier than the split threshold
 * (one batcher slice by default) is cut into contiguous byte-balanced ranges
 * (md5hip_pool_plan) over the least-loaded devices.
 *
 * Concurrency: routing reads each batcher's load lock-free and reserves the
 * submission's weight on the chosen device (`claim`) until the batcher has
 * taken the chunks, so concurrent callers spread instead of piling onto the
 * same idle device.  p->mu guards only the pool's own fields (digest kind,
 * counters, the multi-part ticket table) and is never held across a batcher
 * call that waits for the device.  No thread is created per call.
 *
 * A submission is one or more parts (struct pool_part): a contiguous chunk
 * range, its weight and, once placed, its device and batcher ticket.  One
 * routed whole is the single part [0, n); a split one is the k parts that
 * plan_next cuts, all claimed by one route call before the first is placed.
 *
 * Failed devices (md5hip_batcher_health): never routed to.  part_place puts
 * a part on its device and, while that device has failed and so refuses it
 * (-ENODEV before it took the part), on another.  part_settle waits for a
 * synchronous caller's part and, while its launch failed with its device,
 * places it again from the caller's buffers (still valid: the call has not
 * returned).  An asynchronous ticket keeps its -EIO (or -ENODEV if it was
 * still coalescing).  Each move off a failed device is one failover.
 *
 * Tickets: a submission routed whole is (batcher ticket << 6) | device; a
 * split one is bit 63 | id, its parts kept in `mt` (ascending ids) until all
 * of them have completed, then dropped (an error is kept in `failed`).
 */
#include <errno.h>
#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/md5hip.h"
#include "md5_internal.h"
#include "md5_tickets.h"

/* The batcher's verify submission is a weak reference here, as the compare
 * launcher is for the batcher (md5_internal.h): a pool linked over stand-in
 * batchers that have neither refuses the verify tickets with -ENOSYS. */
extern __typeof__(md5hip_verify_src) md5hip_verify_src __attribute__((weak));
static inline int verify_present(void) { return md5hip_compare_present() && &md5hip_verify_src; }

#define POOL_MAX_DEV 64
#define MT_BIT (1ull << 63)
#define FAILED_MAX (1u << 16)

struct pool_part {
    uint64_t lo, hi;                  /* chunks [lo, hi) of the submission */
    uint64_t w;                       /* their weight */
    uint32_t dev;                     /* once routed: the device, w claimed on it until placed */
    uint64_t t;                       /* once placed: the batcher's ticket */
};

struct mt_entry {                      /* one split submission */
    uint64_t id;
    uint32_t nparts;
    struct pool_part part[];
};

struct md5hip_pool {
    uint32_t ndev;
    md5hip_batcher *b[POOL_MAX_DEV];
    uint64_t claim[POOL_MAX_DEV];     /* weight routed to a device, not yet taken by its batcher */
    pthread_mutex_t mu;
    int kind;
    uint32_t fastcrc;
    uint64_t split_bytes;             /* 0 = one batcher slice */
    uint32_t rr;                      /* rotating start for ties */
    struct md5hip_pool_stats st;
    uint64_t st_failovers;            /* md5hip_pool_health.failovers */
    /* split tickets still running, ascending ids; [mt_lo, mt_lo + mt_n) of a ring */
    struct mt_entry **mt;
    uint64_t mt_cap, mt_lo, mt_n, mt_next;
    struct tk_failed_list failed;     /* split tickets that completed with an error */
};

/* Per-chunk weight for the byte balance: payload plus a fixed cost per chunk
 * (one descriptor and one padding block), so empty chunks still spread. */
static inline uint64_t chunk_weight(uint64_t len) { return len + 64; }

/* weight of chunks [0, n) */
static inline __attribute__((always_inline)) uint64_t src_total(const struct md5hip_src *s, uint64_t n)
{
    if (s->kind == MD5HIP_SRC_FIXED) return n * chunk_weight(s->len);
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) total += chunk_weight(md5hip_src_len(s, i));
    return total;
}

/* The one walk that cuts chunks [0, n) of weight `total` into k contiguous
 * byte-balanced parts: part g starts at the first chunk whose prefix weight
 * reaches g*total/k (a chunk that straddles the target goes to the side that
 * holds more of it).  A FIXED source has the closed form: equal counts. */
struct plan_walk {
    const struct md5hip_src *s;
    uint64_t n, total;
    uint32_t k, g;                    /* g: the part plan_next yields next */
    uint64_t i, acc;                  /* its first chunk, and the weight before that */
};

static inline __attribute__((always_inline)) struct pool_part plan_next(struct plan_walk *c)
{
    struct pool_part q = {.lo = c->i, .hi = c->n, .w = c->total - c->acc};
    const uint32_t g = ++c->g;
    if (g >= c->k) return q;                            /* the last part takes the rest */
    if (c->s->kind == MD5HIP_SRC_FIXED) {
        q.hi = c->n * g / c->k;
        q.w = (q.hi - q.lo) * chunk_weight(c->s->len);
    } else {
        const unsigned __int128 target = (unsigned __int128)c->total * g / c->k;
        uint64_t i = c->i, acc = c->acc;
        while (i < c->n) {
            const uint64_t w = chunk_weight(md5hip_src_len(c->s, i));
            if (acc + w / 2 >= target) break;
            acc += w;
            i++;
        }
        q.hi = i;
        q.w = acc - c->acc;
    }
    c->i = q.hi;
    c->acc += q.w;
    return q;
}

/* Inlined into its two callers, where the source kind is a constant: the
 * ABI entry's walk over a plain length array then costs what it did when it
 * was written out for one. */
static inline __attribute__((always_inline)) void plan_firsts(const struct md5hip_src *s, uint64_t n,
                                                              uint32_t nparts, uint64_t *first)
{
    struct plan_walk c = {.s = s, .n = n, .total = src_total(s, n), .k = nparts};
    for (uint32_t g = 0; g < nparts; g++) first[g] = plan_next(&c).lo;
    first[nparts] = n;
}

int md5hip_pool_plan(const uint32_t *lens, uint64_t n, uint32_t nparts, uint64_t *first)
{
    if (!first || nparts == 0) return -EINVAL;
    if (lens) plan_firsts(&(const struct md5hip_src){.kind = MD5HIP_SRC_PTRS, .lens = lens}, n, nparts, first);
    else plan_firsts(&(const struct md5hip_src){.kind = MD5HIP_SRC_FIXED}, n, nparts, first);   /* equal counts */
    return 0;
}

void md5hip_pool_destroy(md5hip_pool *p)
{
    if (!p) return;
    for (uint32_t g = 0; g < p->ndev; g++) md5hip_batcher_destroy(p->b[g]);
    for (uint64_t k = 0; k < p->mt_n; k++) free(p->mt[(p->mt_lo + k) % p->mt_cap]);
    free(p->mt);
    free(p->failed.e);
    pthread_mutex_destroy(&p->mu);
    free(p);
}

int md5hip_pool_create(const int *devices, uint32_t ndev, uint64_t slice_bytes, uint32_t nslots,
                       md5hip_pool **out)
{
    if (!out) return -EINVAL;
    *out = NULL;
    if (!devices || ndev == 0 || ndev > POOL_MAX_DEV) return -EINVAL;
    md5hip_pool *p = calloc(1, sizeof *p);
    if (!p) return -ENOMEM;
    pthread_mutex_init(&p->mu, NULL);
    p->kind = MD5HIP_DIGEST_MD5;
    p->mt_next = 1;
    p->failed.max = FAILED_MAX;
    for (uint32_t g = 0; g < ndev; g++) {
        int rc = md5hip_batcher_create(devices[g], slice_bytes, nslots, &p->b[g]);
        if (rc) {
            p->ndev = g;
            md5hip_pool_destroy(p);
            return rc;
        }
        p->ndev = g + 1;
    }
    *out = p;
    return 0;
}

int md5hip_pool_ndev(const md5hip_pool *p) { return p ? (int)p->ndev : -EINVAL; }

int md5hip_pool_set_digest(md5hip_pool *p, int kind, uint32_t fastcrc)
{
    if (!p) return -EINVAL;
    const int u = md5hip_digest_usable(kind, fastcrc);
    if (u) return u;
    pthread_mutex_lock(&p->mu);
    p->kind = kind;
    p->fastcrc = fastcrc;
    pthread_mutex_unlock(&p->mu);
    return 0;
}

int md5hip_pool_set_gather(md5hip_pool *p, int mode)
{
    if (!p) return -EINVAL;
    int rc = 0;
    for (uint32_t g = 0; g < p->ndev && rc == 0; g++) rc = md5hip_batcher_set_gather(p->b[g], mode);
    return rc;
}

int md5hip_pool_set_split(md5hip_pool *p, uint64_t bytes)
{
    if (!p) return -EINVAL;
    pthread_mutex_lock(&p->mu);
    p->split_bytes = bytes;
    pthread_mutex_unlock(&p->mu);
    return 0;
}

int md5hip_pool_get_stats(md5hip_pool *p, struct md5hip_pool_stats *out)
{
    if (!p || !out) return -EINVAL;
    pthread_mutex_lock(&p->mu);
    *out = p->st;
    pthread_mutex_unlock(&p->mu);
    return 0;
}

int md5hip_pool_device_stats(md5hip_pool *p, uint32_t g, struct md5hip_batcher_stats *out)
{
    if (!p || !out || g >= p->ndev) return -EINVAL;
    return md5hip_batcher_get_stats(p->b[g], out);
}

int md5hip_pool_device_health(md5hip_pool *p, uint32_t g)
{
    if (!p || g >= p->ndev) return -EINVAL;
    return md5hip_batcher_health(p->b[g]);
}

int md5hip_pool_get_health(md5hip_pool *p, struct md5hip_pool_health *out)
{
    if (!p || !out) return -EINVAL;
    memset(out, 0, sizeof *out);
    out->ndev = p->ndev;
    for (uint32_t g = 0; g < p->ndev; g++)
        if (md5hip_batcher_health(p->b[g])) {
            out->nfailed++;
            if (g < 64) out->failed_mask |= 1ull << g;
        }
    pthread_mutex_lock(&p->mu);
    out->failovers = p->st_failovers;
    pthread_mutex_unlock(&p->mu);
    return 0;
}

int md5hip_pool_inject_fault(md5hip_pool *p, uint32_t g, uint64_t after)
{
    if (!p || g >= p->ndev) return -EINVAL;
    return md5hip_batcher_inject_fault(p->b[g], after);
}

/* ------------------------------------------------------------------------
 * Routing
 * ------------------------------------------------------------------------ */
static uint64_t dev_load(md5hip_pool *p, uint32_t g)
{
    return md5hip_batcher_load(p->b[g]) + __atomic_load_n(&p->claim[g], __ATOMIC_RELAXED);
}

static int dev_ok(md5hip_pool *p, uint32_t g) { return md5hip_batcher_health(p->b[g]) == 0; }

/* The k least-loaded healthy devices (ties from a rotating start) for
 * part[0..k): part j's device, its weight claimed there.  Returns how many
 * were chosen: fewer than k when fewer devices are healthy (0: every device
 * failed). */
static uint32_t route(md5hip_pool *p, uint32_t k, struct pool_part *part)
{
    const uint32_t G = p->ndev;
    const uint32_t r0 = __atomic_fetch_add(&p->rr, 1, __ATOMIC_RELAXED);
    uint64_t load[POOL_MAX_DEV];
    int used[POOL_MAX_DEV];
    for (uint32_t g = 0; g < G; g++) {
        used[g] = !dev_ok(p, g);                      /* a failed device is never picked */
        load[g] = dev_load(p, g);
    }
    for (uint32_t j = 0; j < k; j++) {
        uint32_t best = G;
        for (uint32_t q = 0; q < G; q++) {
            const uint32_t g = (r0 + q) % G;
            if (!used[g] && (best == G || load[g] < load[best])) best = g;
        }
        if (best == G) return j;
        used[best] = 1;
        part[j].dev = best;
        __atomic_fetch_add(&p->claim[best], part[j].w, __ATOMIC_RELAXED);
    }
    return k;
}

static void unclaim(md5hip_pool *p, const struct pool_part *q)
{
    __atomic_fetch_sub(&p->claim[q->dev], q->w, __ATOMIC_RELAXED);
}

/* ------------------------------------------------------------------------
 * Tickets
 * ------------------------------------------------------------------------ */
/* wait for (block = 1) or poll (block = 0) ticket t of device g's batcher:
 * 1 done and *err its error, 0 running, -EINVAL no such ticket */
static int ticket_step(md5hip_pool *p, uint32_t g, uint64_t t, int block, int *err)
{
    const int r = block ? md5_batch_wait(p->b[g], t) : md5_batch_poll(p->b[g], t);
    *err = 0;
    if (r == -EINVAL) return -EINVAL;
    if (!block && r >= 0) return r;
    *err = r;
    return 1;
}

/* ticket_step over parts that this pool placed: 1 every part done, 0 some
 * running (each has been hastened); the first part error into *err if it
 * holds none yet */
static int parts_step(md5hip_pool *p, const struct pool_part *part, uint32_t np, int block, int *err)
{
    int done = 1;
    for (uint32_t j = 0; j < np; j++) {
        int e;
        const int s = ticket_step(p, part[j].dev, part[j].t, block, &e);
        if (s < 0) e = s;
        else if (s == 0) done = 0;
        if (e && !*err) *err = e;
    }
    return done;
}

/* 1 = every part done (*err = the first part error), 0 = running; launches
 * and waits for nothing (p->mu held) */
static int mt_state(md5hip_pool *p, const struct mt_entry *e, int *err)
{
    *err = 0;
    for (uint32_t j = 0; j < e->nparts; j++) {
        int pe = 0;
        const int s = md5hip_batcher_ticket_state(p->b[e->part[j].dev], e->part[j].t, &pe);
        if (s < 0) pe = s;
        else if (s == 0) return 0;
        if (pe && !*err) *err = pe;
    }
    return 1;
}

/* Drop completed entries from the low end (their errors are looked up in
 * p->failed from then on); p->mu held. */
static void mt_reap(md5hip_pool *p)
{
    while (p->mt_n) {
        struct mt_entry *e = p->mt[p->mt_lo % p->mt_cap];
        int err;
        if (!mt_state(p, e, &err)) break;
        if (err) tk_failed_add(&p->failed, e->id, err);
        free(e);
        p->mt_lo++;
        p->mt_n--;
    }
}

/* p->mu held */
static int mt_push(md5hip_pool *p, struct mt_entry *e)
{
    if (p->mt_n == p->mt_cap) {
        const uint64_t nc = p->mt_cap ? 2 * p->mt_cap : 64;
        struct mt_entry **m = malloc(nc * sizeof *m);
        if (!m) return -ENOMEM;
        for (uint64_t k = 0; k < p->mt_n; k++) m[k] = p->mt[(p->mt_lo + k) % p->mt_cap];
        free(p->mt);
        p->mt = m;
        p->mt_cap = nc;
        p->mt_lo = 0;
    }
    p->mt[(p->mt_lo + p->mt_n) % p->mt_cap] = e;
    p->mt_n++;
    return 0;
}

/* the live entry with this id, or NULL (completed and dropped, or unknown);
 * p->mu held */
static struct mt_entry *mt_find(md5hip_pool *p, uint64_t id)
{
    uint64_t a = 0, z = p->mt_n;
    while (a < z) {
        const uint64_t mid = (a + z) / 2;
        if (p->mt[(p->mt_lo + mid) % p->mt_cap]->id < id) a = mid + 1;
        else z = mid;
    }
    if (a < p->mt_n) {
        struct mt_entry *e = p->mt[(p->mt_lo + a) % p->mt_cap];
        if (e->id == id) return e;
    }
    return NULL;
}

/* wait (block = 1) or poll (block = 0) on a pool ticket: 1 done / 0 running
 * and *err its error, or -EINVAL */
static int pool_ticket(md5hip_pool *p, uint64_t ticket, int block, int *err)
{
    *err = 0;
    if (ticket == 0) return 1;
    if (!(ticket & MT_BIT)) {
        const uint32_t g = (uint32_t)(ticket & 63u);
        return g < p->ndev ? ticket_step(p, g, ticket >> 6, block, err) : -EINVAL;
    }
    const uint64_t id = ticket & ~MT_BIT;
    struct pool_part parts[POOL_MAX_DEV];
    uint32_t np = 0;
    pthread_mutex_lock(&p->mu);
    const int known = id != 0 && id < p->mt_next;
    const struct mt_entry *e = known ? mt_find(p, id) : NULL;
    if (e) {
        np = e->nparts;
        memcpy(parts, e->part, np * sizeof *parts);
    } else if (known) {
        *err = tk_failed_find(&p->failed, id);        /* completed and dropped */
    }
    pthread_mutex_unlock(&p->mu);
    if (!e) return known ? 1 : -EINVAL;
    /* the batcher calls may block: p->mu is not held */
    const int done = parts_step(p, parts, np, block, err);
    if (done) {
        pthread_mutex_lock(&p->mu);
        mt_reap(p);
        pthread_mutex_unlock(&p->mu);
    }
    return done;
}

int md5hip_pool_wait(md5hip_pool *p, uint64_t ticket)
{
    if (!p) return -EINVAL;
    int err;
    const int r = pool_ticket(p, ticket, 1, &err);
    return r < 0 ? r : err;
}

int md5hip_pool_poll(md5hip_pool *p, uint64_t ticket)
{
    if (!p) return -EINVAL;
    int err;
    const int r = pool_ticket(p, ticket, 0, &err);
    if (r < 0) return r;
    return r == 1 && err ? err : r;
}

/* ------------------------------------------------------------------------
 * Submission
 * ------------------------------------------------------------------------ */
struct pool_sub {                      /* what every part of one submission shares */
    md5hip_pool *p;
    const struct md5hip_src *s;
    unsigned char *digests;
    const struct md5hip_verify_opt *v; /* a verify submission (digests NULL): compared on each part's device */
    int kind;
    uint32_t fastcrc;
    int sync;                          /* the caller has no ticket: it waits in the call */
};

/* Opens the submission: the pool's digest kind unless the caller named one
 * (kind >= 0); returns the split threshold in bytes. */
static uint64_t sub_open(struct pool_sub *u, int kind, uint32_t fastcrc)
{
    md5hip_pool *p = u->p;
    pthread_mutex_lock(&p->mu);
    u->kind = kind < 0 ? p->kind : kind;
    u->fastcrc = kind < 0 ? p->fastcrc : fastcrc;
    const uint64_t split = p->split_bytes;
    p->st.submissions++;
    pthread_mutex_unlock(&p->mu);
    return split ? split : md5hip_batcher_slice(p->b[0]);
}

/* parts to cut n chunks of weight `total` into: 1 = whole (the common
 * case), 0 = no device is healthy */
static uint32_t part_count(md5hip_pool *p, uint64_t n, uint64_t total, uint64_t split)
{
    uint32_t healthy = 0;
    for (uint32_t g = 0; g < p->ndev; g++) healthy += dev_ok(p, g);
    if (total <= split || healthy <= 1) return healthy != 0;
    const uint64_t want = (total + split - 1) / split;
    const uint64_t k = want < healthy ? want : healthy;
    return (uint32_t)(k < n ? k : n);
}

static void count_failover(md5hip_pool *p)
{
    pthread_mutex_lock(&p->mu);
    p->st_failovers++;
    pthread_mutex_unlock(&p->mu);
}

static void count_routed(md5hip_pool *p, int split, uint32_t parts)
{
    pthread_mutex_lock(&p->mu);
    if (split) p->st.split++;
    else p->st.routed_whole++;
    p->st.parts += parts;
    pthread_mutex_unlock(&p->mu);
}

/* Places part q: on the device already claimed for it (claimed, by the
 * split's route), else on one routed here.  The batcher takes it
 * asynchronously even for a synchronous caller, so the claim ends with the
 * submit attempt (the batcher's own load counts the chunks from then on);
 * urgent for a synchronous caller, who waits right away.  While the device
 * refuses the part because it has failed, the part moves to another: one
 * failover each.  -ENODEV once no device is healthy. */
static int part_place(const struct pool_sub *u, struct pool_part *q, int claimed)
{
    md5hip_pool *p = u->p;
    for (;; claimed = 0) {
        if (!claimed && !route(p, 1, q)) return -ENODEV;
        q->t = 0;
        const int rc = u->v ? md5hip_verify_src(p->b[q->dev], u->kind, u->fastcrc, u->s, q->lo, q->hi, u->v, &q->t,
                                                u->sync)
                            : md5hip_submit_src(p->b[q->dev], u->kind, u->fastcrc, u->s, q->lo, q->hi,
                                                u->digests + (size_t)md5hip_digest_size(u->kind) * q->lo, &q->t,
                                                u->sync);
        unclaim(p, q);
        if (rc != -ENODEV || dev_ok(p, q->dev)) return rc;
        count_failover(p);
    }
}

static int part_wait(md5hip_pool *p, const struct pool_part *q)
{
    int err = 0;
    parts_step(p, q, 1, 1, &err);
    return err;
}

/* Settles placed part q for a synchronous caller: waits for it and, while
 * its launch failed because its device did, places it again (one failover)
 * from the caller's buffers and waits again. */
static int part_settle(const struct pool_sub *u, struct pool_part *q)
{
    for (;;) {
        int rc = part_wait(u->p, q);
        if ((rc != -EIO && rc != -ENODEV) || dev_ok(u->p, q->dev)) return rc;
        count_failover(u->p);
        if ((rc = part_place(u, q, 0))) return rc;
    }
}

/* The placed parts finish before the caller may reuse its buffers: settled
 * for a synchronous caller while no part has failed for good (rc, the error
 * so far), else only waited for.  Returns the first error. */
static int parts_finish(const struct pool_sub *u, struct pool_part *part, uint32_t np, int rc)
{
    for (uint32_t j = 0; j < np; j++) {
        const int r = u->sync && rc == 0 ? part_settle(u, &part[j]) : part_wait(u->p, &part[j]);
        if (r && !rc) rc = r;
    }
    return rc;
}

static int submit_whole(const struct pool_sub *u, uint64_t n, uint64_t total, uint64_t *ticket)
{
    struct pool_part q = {.lo = 0, .hi = n, .w = total};
    int rc = part_place(u, &q, 0);
    if (rc == 0 && u->sync) rc = part_settle(u, &q);
    count_routed(u->p, 0, 1);
    if (ticket && rc == 0 && q.t) *ticket = (q.t << 6) | q.dev;
    return rc;
}

/* Places part[0..k), of which route claimed a device for the first `got`,
 * and moves the placed ones to the front: their count into *np.  A part for
 * which no device was left (a device failed since part_count) goes to any
 * healthy one.  After one part's error no further part is placed. */
static int parts_place(const struct pool_sub *u, struct pool_part *part, uint32_t k, uint32_t got, uint32_t *np)
{
    int rc = 0;
    *np = 0;
    for (uint32_t j = 0; j < k; j++) {
        struct pool_part *q = &part[j];
        if (rc || q->hi == q->lo) {
            if (j < got) unclaim(u->p, q);
            continue;
        }
        rc = part_place(u, q, j < got);
        if (rc == 0 && q->t) part[(*np)++] = *q;
    }
    return rc;
}

/* Hands out the split ticket of entry e, whose parts run; without table
 * space they finish here.  Owns e. */
static int mt_publish(const struct pool_sub *u, struct mt_entry *e, uint64_t *ticket)
{
    md5hip_pool *p = u->p;
    pthread_mutex_lock(&p->mu);
    mt_reap(p);
    e->id = p->mt_next++;
    const int rc = mt_push(p, e);
    if (rc == 0) *ticket = MT_BIT | e->id;
    pthread_mutex_unlock(&p->mu);
    if (rc) {
        parts_finish(u, e->part, e->nparts, rc);
        free(e);
    }
    return rc;
}

/* contiguous byte-balanced ranges over the k least-loaded devices */
static int submit_split(const struct pool_sub *u, uint64_t n, uint64_t total, uint32_t k, uint64_t *ticket)
{
    struct mt_entry *e = malloc(sizeof *e + k * sizeof *e->part);
    if (!e) return -ENOMEM;
    struct plan_walk c = {.s = u->s, .n = n, .total = total, .k = k};
    for (uint32_t j = 0; j < k; j++) e->part[j] = plan_next(&c);
    const uint32_t got = route(u->p, k, e->part);     /* every claim before the first part is placed */
    int rc = parts_place(u, e->part, k, got, &e->nparts);
    count_routed(u->p, 1, e->nparts);
    if (rc == 0 && !u->sync) return mt_publish(u, e, ticket);
    rc = parts_finish(u, e->part, e->nparts, rc);
    free(e);
    return rc;
}

/* n > 0 valid chunks, *ticket zeroed (pool_enter); ticket NULL =
 * synchronous; kind < 0 = the pool's current digest kind */
static int pool_submit_as(md5hip_pool *p, const struct md5hip_src *s, uint64_t n, unsigned char *digests,
                          const struct md5hip_verify_opt *v, uint64_t *ticket, int kind, uint32_t fastcrc)
{
    struct pool_sub u = {.p = p, .s = s, .digests = digests, .v = v, .sync = ticket == NULL};
    const uint64_t split = sub_open(&u, kind, fastcrc);
    const uint64_t total = src_total(s, n);
    const uint32_t k = part_count(p, n, total, split);
    if (k == 0) return -ENODEV;
    return k == 1 ? submit_whole(&u, n, total, ticket) : submit_split(&u, n, total, k, ticket);
}

static int pool_submit(md5hip_pool *p, const struct md5hip_src *s, uint64_t n, unsigned char *digests,
                       uint64_t *ticket, int kind, uint32_t fastcrc)
{
    return pool_submit_as(p, s, n, digests, NULL, ticket, kind, fastcrc);
}

/* ------------------------------------------------------------------------
 * Entries
 * ------------------------------------------------------------------------ */
/* What every submit entry does once it has named its source: async = the
 * entry has a ticket argument, which must not be NULL. */
static int pool_enter(md5hip_pool *p, const struct md5hip_src *s, uint64_t n, unsigned char *digests,
                      uint64_t *ticket, int async)
{
    if (ticket) *ticket = 0;
    if (!p || (async && !ticket)) return -EINVAL;
    if (n == 0) return 0;
    if (!digests) return -EINVAL;
    const int rc = md5hip_src_check(s, n);
    return rc ? rc : pool_submit(p, s, n, digests, ticket, -1, 0);
}

int md5hip_pool_submit_async(md5hip_pool *p, const void *const *ptrs, const uint32_t *lens,
                             uint64_t n, unsigned char *digests, uint64_t *ticket)
{
    const struct md5hip_src s = {.kind = MD5HIP_SRC_PTRS, .ptrs = ptrs, .lens = lens};
    return pool_enter(p, &s, n, digests, ticket, 1);
}

int md5hip_pool_submit_iov_async(md5hip_pool *p, const struct md5hip_iov *segs,
                                 const uint64_t *seg_first, uint64_t n, unsigned char *digests,
                                 uint64_t *ticket)
{
    const struct md5hip_src s = {.kind = MD5HIP_SRC_IOV, .segs = segs, .seg_first = seg_first};
    return pool_enter(p, &s, n, digests, ticket, 1);
}

int md5hip_pool_submit(md5hip_pool *p, const void *const *ptrs, const uint32_t *lens, uint64_t n,
                       unsigned char *digests)
{
    const struct md5hip_src s = {.kind = MD5HIP_SRC_PTRS, .ptrs = ptrs, .lens = lens};
    return pool_enter(p, &s, n, digests, NULL, 0);
}

int md5hip_pool_submit_iov(md5hip_pool *p, const struct md5hip_iov *segs, const uint64_t *seg_first,
                           uint64_t n, unsigned char *digests)
{
    const struct md5hip_src s = {.kind = MD5HIP_SRC_IOV, .segs = segs, .seg_first = seg_first};
    return pool_enter(p, &s, n, digests, NULL, 0);
}

int md5hip_pool_host_fixed(md5hip_pool *p, const void *h_base, uint64_t n, uint32_t len,
                           uint64_t stride, unsigned char *digests)
{
    const struct md5hip_src s = {.kind = MD5HIP_SRC_FIXED, .base = h_base, .len = len, .stride = stride};
    return pool_enter(p, &s, n, digests, NULL, 0);
}

int md5hip_pool_verify_iov(md5hip_pool *p, const struct md5hip_iov *segs, const uint64_t *seg_first,
                           uint64_t n, const void *expected, unsigned char *ok)
{
    if (!p) return -EINVAL;
    if (n == 0) return 0;
    if (!expected || !ok) return -EINVAL;
    const struct md5hip_src s = {.kind = MD5HIP_SRC_IOV, .segs = segs, .seg_first = seg_first};
    int rc = md5hip_src_check(&s, n);
    if (rc) return rc;
    /* one snapshot of the kind for the digest size and the submission */
    pthread_mutex_lock(&p->mu);
    const int kind = p->kind;
    const uint32_t fastcrc = p->fastcrc;
    pthread_mutex_unlock(&p->mu);
    const uint32_t dsz = md5hip_digest_size(kind);
    unsigned char *got = malloc((size_t)dsz * n);
    if (!got) return -ENOMEM;
    rc = pool_submit(p, &s, n, got, NULL, kind, fastcrc);
    if (rc == 0) rc = md5hip_verify_count(got, expected, dsz, n, ok);
    free(got);
    return rc;
}

/* md5hip_batch_upgrade_iov on the pool: one MD5_CRC32 submission of this
 * call's own, routed and split as any other. */
int md5hip_pool_upgrade_iov(md5hip_pool *p, const struct md5hip_iov *segs, const uint64_t *seg_first,
                            uint64_t n, const uint32_t *want_crc, unsigned char *ok,
                            unsigned char *md5_out)
{
    if (!p) return -EINVAL;
    int rc = md5hip_digest_usable(MD5HIP_DIGEST_MD5_CRC32, 0);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!want_crc || !ok || !md5_out) return -EINVAL;
    const struct md5hip_src s = {.kind = MD5HIP_SRC_IOV, .segs = segs, .seg_first = seg_first};
    if ((rc = md5hip_src_check(&s, n))) return rc;
    unsigned char *rec = malloc(32 * (size_t)n);
    if (!rec) return -ENOMEM;
    rc = pool_submit(p, &s, n, rec, NULL, MD5HIP_DIGEST_MD5_CRC32, 0);
    if (rc == 0) rc = md5hip_upgrade_count(rec, want_crc, n, ok, md5_out);
    free(rec);
    return rc;
}

/* The ticket forms of verify and upgrade: the submission routed and split as
 * any other, each part compared on its own device (md5hip_verify_src) and
 * adding its mismatches into the one *nbad, zeroed here.  kind < 0: the
 * pool's digest kind, whole digests (v->wsz is set from it). */
static int pool_enter_verify(md5hip_pool *p, const struct md5hip_iov *segs, const uint64_t *seg_first, uint64_t n,
                             int kind, struct md5hip_verify_opt *v, uint64_t *ticket)
{
    if (ticket) *ticket = 0;
    if (!p || !ticket) return -EINVAL;
    if (v->nbad) *v->nbad = 0;
    if (!verify_present()) return -ENOSYS;
    if (n == 0) return 0;
    if (!v->expected || !v->ok) return -EINVAL;
    uint32_t fastcrc = 0;
    if (kind < 0) {                               /* one snapshot for the digest size and the submission */
        pthread_mutex_lock(&p->mu);
        kind = p->kind;
        fastcrc = p->fastcrc;
        pthread_mutex_unlock(&p->mu);
        v->wsz = md5hip_digest_size(kind);
    }
    int rc = md5hip_digest_usable(kind, fastcrc);
    if (rc) return rc;
    const struct md5hip_src s = {.kind = MD5HIP_SRC_IOV, .segs = segs, .seg_first = seg_first};
    if ((rc = md5hip_src_check(&s, n))) return rc;
    return pool_submit_as(p, &s, n, NULL, v, ticket, kind, fastcrc);
}

int md5hip_pool_verify_iov_async(md5hip_pool *p, const struct md5hip_iov *segs, const uint64_t *seg_first,
                                 uint64_t n, const void *expected, unsigned char *ok, uint64_t *nbad,
                                 uint64_t *ticket)
{
    struct md5hip_verify_opt v = {.expected = expected, .ok = ok, .nbad = nbad};
    return pool_enter_verify(p, segs, seg_first, n, -1, &v, ticket);
}

int md5hip_pool_upgrade_iov_async(md5hip_pool *p, const struct md5hip_iov *segs, const uint64_t *seg_first,
                                  uint64_t n, const uint32_t *want_crc, unsigned char *ok, unsigned char *md5_out,
                                  uint64_t *nbad, uint64_t *ticket)
{
    struct md5hip_verify_opt v = {.expected = want_crc, .ok = ok, .md5_out = md5_out, .nbad = nbad, .goff = 16, .wsz = 4};
    if (p && ticket && n && !md5_out) {
        *ticket = 0;
        return -EINVAL;
    }
    return pool_enter_verify(p, segs, seg_first, n, MD5HIP_DIGEST_MD5_CRC32, &v, ticket);
}
