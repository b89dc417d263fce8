/*
 * md5_submit.c -- the batcher: a thread-safe, coalescing submission queue in
 * front of the batched kernels (include/md5hip.h).
 *
 * Serves the netcache block-completion checksum site (blk_make_crc,
 * netcache/common/blk_io.c:354-430, called from ASIO pool threads,
 * asio_mgr.c:1054-1057): chunks live in host memory (cache pages, socket
 * buffers) or already in HBM, and each caller wants its own digests back.
 *
 * A batcher owns `nslots` pipeline slots.  Slot k has its own HIP stream,
 * pinned staging, device buffers, descriptor arrays and completion event.
 * At most one slot is OPEN at a time: submissions (from any thread) append
 * their chunks to it -- host chunks are gathered into its pinned staging,
 * device-resident chunks only add a descriptor -- and the slot is launched
 * as ONE planned descriptor batch (md5hip_plan_desc) when
 *   - it is full (bytes, descriptors or gather segments), or
 *   - fewer than `target` slots are in flight (an idle pipeline takes work at
 *     once: no added latency when the device is not busy), or
 *   - a caller waits on / polls / flushes a ticket it holds.
 * So while the device is busy, everything submitted meanwhile is coalesced
 * into the next launch: a 1 MiB chunk's serial chain (~10 ms) then runs
 * beside the bytes of many later submissions instead of ending its launch
 * alone.
 *
 * Completion is per ticket and out of order: a ticket completes when every
 * slot holding its chunks has finished, whatever earlier tickets are doing.
 * A progress thread per batcher polls the in-flight slots' events, delivers
 * host digests (D2H staging -> the caller's array), retires slots and
 * launches the open slot when the pipeline drains below `target`.
 *
 * Locking: b->mu guards all batcher state; HIP enqueue calls are made under
 * it (they are asynchronous); host gathers (memcpy) run outside it, the slot
 * held open by a writer count.  Lock order: b->mu, then g_reg_lock.
 *
 * Every entry saves and restores the calling thread's HIP device.
 * Errors: 0 / negative errno (include/md5hip.h); -E2BIG when one chunk
 * exceeds the slot's staging; -EFAULT when registered memory vanished
 * under a zero-copy submission.
 *
 * Device failure.  blk_make_crc cannot fail (blk_io.c:354-430); this can.
 * A launch whose completion event reports an error, or an enqueue failure
 * after which the slot's stream reports one, marks the batcher FAILED
 * (sticky): that launch's tickets get -EIO, tickets still coalescing in the
 * open slot and every later submission get -ENODEV at once, and nothing is
 * enqueued on the device again.  Launches already in flight complete as
 * their events say.  No digest of a failed launch is delivered.  The pool
 * (md5_pool.c) routes around a failed batcher; what the call site does with
 * -EIO / -ENODEV is INTEGRATION.md §2j.
 *
 * The parts, in the file's order:
 *   registered host ranges   the table behind zero-copy input; the device guard
 *   slots and tickets        the structures; descriptors and plan (slot_prepare);
 *                            a launch as bytes in, kernel, digests out
 *                            (slot_enqueue); retire, failure, the launch
 *                            decision (slot_try_launch); the open slot and
 *                            claiming a free one
 *   progress thread          retire what finished, linger or sleep, prepare
 *                            the open slot ahead, chain it, poll interval
 *   blocked callers          the watcher of a launch, wait_ticket
 *   create / destroy / settings
 *   submission               reserve (descriptors, histogram, zero-copy
 *                            tables), the engines submit and fixed_submit,
 *                            wait / poll / flush
 *   entries                  the C ABI's submit calls; the pool's; verify
 *   asynchronous verify      the ticket forms: verify segments compared on
 *                            the device (enqueue_verify), their buffers
 * The ticket table is md5_tickets.h, the host chunk sources (segments,
 * copies, the threaded gather) md5_source.h: both included here alone.
 */
#include <errno.h>
#include <pthread.h>
#include <sys/prctl.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <hip/hip_runtime_api.h>

#include "../../include/md5hip.h"
#include "md5_internal.h"
#include "md5_tickets.h"
#include "md5_source.h"

/* ------------------------------------------------------------------------
 * Registered host ranges (zero-copy input).  netcache allocates its cache
 * pages in 4 KiB-aligned bulks (bc_mgr.c:1260-1290); a bulk registered here
 * is pinned and mapped for every device, so the batcher can let the device
 * (or the DMA engine) pull the pages directly instead of memcpy'ing them into
 * the pinned staging slice on the host.
 * ------------------------------------------------------------------------ */
#define REG_MAXDEV 16
struct reg_range {
    uintptr_t lo, hi;
    intptr_t delta[REG_MAXDEV];       /* device-visible address - host address */
};
static struct reg_range *g_reg;
static size_t g_nreg, g_capreg;
static pthread_rwlock_t g_reg_lock = PTHREAD_RWLOCK_INITIALIZER;

/* index of the range containing [p, p+len), or -1 (caller holds the lock) */
static long reg_find(uintptr_t p, uint64_t len)
{
    size_t lo = 0, hi = g_nreg;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        if (g_reg[mid].hi <= p) lo = mid + 1;
        else hi = mid;
    }
    if (lo < g_nreg && g_reg[lo].lo <= p && p + len <= g_reg[lo].hi) return (long)lo;
    return -1;
}

/* The caller's HIP device, restored on every exit from an entry. */
struct dev_guard { int prev; int ok; };
static void dev_save(struct dev_guard *g)
{
    g->ok = hipGetDevice(&g->prev) == hipSuccess;
}
static int dev_enter(struct dev_guard *g, int device)
{
    dev_save(g);
    if (hipSetDevice(device) != hipSuccess) {
        (void)hipGetLastError();      /* ours: returned as -ENODEV, not left for the caller's next check */
        if (g->ok) (void)hipSetDevice(g->prev);
        return -ENODEV;
    }
    return 0;
}
static void dev_leave(const struct dev_guard *g)
{
    if (g->ok) (void)hipSetDevice(g->prev);
}

int md5hip_host_register(void *base, uint64_t bytes)
{
    if (!base || bytes == 0) return -EINVAL;
    const uintptr_t lo = (uintptr_t)base, hi = lo + bytes;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return -ENODEV;
    if (ndev > REG_MAXDEV) ndev = REG_MAXDEV;
    struct dev_guard g;
    dev_save(&g);                     /* the loop below visits every device */
    pthread_rwlock_wrlock(&g_reg_lock);
    int rc = 0;
    size_t at = 0;
    while (at < g_nreg && g_reg[at].hi <= lo) at++;
    if (at < g_nreg && g_reg[at].lo < hi) { rc = -EEXIST; goto out; }     /* overlap */
    if (g_nreg == g_capreg) {
        size_t cap = g_capreg ? 2 * g_capreg : 64;
        struct reg_range *r = realloc(g_reg, cap * sizeof *r);
        if (!r) { rc = -ENOMEM; goto out; }
        g_reg = r;
        g_capreg = cap;
    }
    /* coarse-grained: the batcher reads a range only between the caller's
     * writes, and DMA from coarse-grained pages runs 44 vs 34 GB/s
     * (DESIGN.md §5); MD5HIP_REGISTER_COARSE=0 turns it off */
    unsigned flags = hipHostRegisterPortable | hipHostRegisterMapped;
    const char *coarse = getenv("MD5HIP_REGISTER_COARSE");
    if (!coarse || atoi(coarse)) flags |= hipExtHostRegisterCoarseGrained;
    if (hipHostRegister(base, bytes, flags) != hipSuccess) {
        rc = -ENODEV;
        goto out;
    }
    struct reg_range r = {lo, hi, {0}};
    for (int d = 0; d < ndev; d++) {
        void *dp = NULL;
        if (hipSetDevice(d) == hipSuccess && hipHostGetDevicePointer(&dp, base, 0) == hipSuccess)
            r.delta[d] = (intptr_t)((uintptr_t)dp - lo);
    }
    memmove(&g_reg[at + 1], &g_reg[at], (g_nreg - at) * sizeof *g_reg);
    g_reg[at] = r;
    g_nreg++;
out:
    pthread_rwlock_unlock(&g_reg_lock);
    dev_leave(&g);
    return rc;
}

int md5hip_host_unregister(void *base)
{
    if (!base) return -EINVAL;
    pthread_rwlock_wrlock(&g_reg_lock);
    int rc = -ENOENT;
    for (size_t k = 0; k < g_nreg; k++) {
        if (g_reg[k].lo == (uintptr_t)base) {
            rc = hipHostUnregister(base) == hipSuccess ? 0 : -EIO;
            memmove(&g_reg[k], &g_reg[k + 1], (g_nreg - k - 1) * sizeof *g_reg);
            g_nreg--;
            break;
        }
    }
    pthread_rwlock_unlock(&g_reg_lock);
    return rc;
}

/* ------------------------------------------------------------------------
 * Slots and tickets
 * ------------------------------------------------------------------------ */
enum slot_state { SLOT_FREE = 0, SLOT_OPEN, SLOT_INFLIGHT };
enum slot_mode { MODE_NONE = 0, MODE_STAGED, MODE_ZEROCOPY, MODE_FIXED, MODE_PAGES };

/* One ticket's chunks in one slot: slot chunks [first, first+count) deliver
 * into `user` (host array, or device memory when on_device). */
struct seg {
    uint64_t ticket, first, count;
    unsigned char *user;
    int on_device;
    /* a verify segment (ok != NULL, user == NULL): its chunks' digests are
     * compared on the device (enqueue_verify) instead of delivered.  ok / the
     * expected values at `want` are host memory, or (on_device) the caller's
     * device memory; a host caller's expected values were copied into the
     * slot's table buffer at submit time (want = their offset there).
     * md5_out: upgrade, the records' MD5s (host).  The range's compare
     * entries are [ent, ent + nent) of the slot's table. */
    unsigned char *ok, *md5_out;
    uint64_t *nbad;
    uint64_t want;
    uint32_t goff, wsz, ent, nent;
};

struct slot {
    hipStream_t stream;
    hipEvent_t done;
    hipEvent_t kdone;                 /* right after the hash kernel: what a chained launch waits on
                                         (the digest scatter / D2H behind it need not) */
    unsigned char *h_data, *d_data;   /* staging, `cap` bytes */
    uint64_t *h_off, *d_off;          /* descriptors, `maxn` entries */
    uint32_t *h_len, *d_len;
    const uint64_t *dh_off;           /* h_off / h_len as the device sees them (fine-grained) */
    const uint32_t *dh_len;
    int desc_direct;                  /* the planned launch reads dh_off / dh_len in place */
    uint32_t *h_ord, *d_ord;
    unsigned char *h_dig, *d_dig;     /* 32 * maxn (the largest digest, MD5_CRC32's record) */
    int direct;                       /* the kernel wrote the one device segment in place */
    struct md5hip_seg *h_seg, *d_seg; /* zero-copy gather table, `segcap` entries */
    void **b_dst, **b_src;            /* DMA-batch gather arrays (plain host memory) */
    size_t *b_len;
    long *b_reg;                      /* registration each DMA entry lies in */
    struct md5hip_seg *h_dsc, *d_dsc; /* device-digest scatter table, `segcap` entries */
    struct seg *segs;                 /* ticket segments */
    uint32_t nsegs, capsegs;
    int state, mode, writers, full, flush, err;
    uint64_t n, used, nseg, ndma, ndsc;
    uint32_t kind, fastcrc, dsz;
    /* MODE_FIXED (md5hip_batch_host_fixed): one contiguous host range, or
     * (fx_dev, md5_batch_submit_device_fixed) one device range read in place */
    const unsigned char *fx_src;
    int fx_dev;
    uint64_t fx_bytes, fx_stride;
    uint32_t fx_len;
    /* MODE_PAGES (md5_batch_submit_device_pages): one slice of a paged
     * submission.  Its pg_n table entries are in h_pg, chunk i's from entry
     * h_off[i] on, its lengths in h_len, its longest-first order (use_order)
     * in h_ord; h_pg / d_pg are the slot's share of the batcher's page
     * tables: NULL until the first paged submission (pages_buffers) */
    uint64_t *h_pg, *d_pg;
    uint64_t pg_n;
    uint32_t pg_bytes;
    uint64_t tickets_in;              /* distinct tickets (stats) */
    /* descriptors already on the device / the plan they were ordered by:
     * prepared ahead while another slot's launch runs (slot_prepare) */
    uint64_t copied_n, planned_n, seen_n;
    int plan_var;
    /* key histogram of the reserved chunks (k = (len >> 6) + 1, md5hip.h
     * md5hip_plan_hist): the plan is made from counts and the order built on
     * the device; hovf = a chunk past MD5HIP_HIST_KMAX (host sort instead) */
    uint32_t *hh, hkmax, *h_bkt, *d_bkt;
    void *d_sort;                     /* md5hip_order_device_stable scratch (NULL: order_scatter) */
    uint64_t sort_bytes;
    int hovf;
    /* keys already non-increasing in reservation order (a vector of full
     * blocks with a short last one, a single equal-length batch): then the
     * identity IS the longest-first order, and no order is built or used */
    uint32_t last_key;
    int unsorted, use_order;
    uint64_t opened_us, launched_us;  /* first chunk reserved / went in flight */
    uint64_t gen;                     /* launches of this slot so far (a waiter's check) */
    uint64_t load;                    /* this slot's share of b->load_bytes */
    /* payload bytes, and those in device-resident chunks starting 16-B but not
     * 128-B aligned (md5hip_lines_choice: LINES instead of XDMA) */
    uint64_t payload, unlined;
    /* callers blocked on tickets held here sleep on `cv` (nwait of them):
     * broadcast when the slot retires, signalled once when it goes in flight
     * (one sleeper then watches the launch).  watch: WATCH_NONE / _ACTIVE (one
     * waiter sleeps through or spins on this launch) / _GAVE_UP (the spin
     * ended first: the progress thread retires it, polling fast) */
    pthread_cond_t cv;
    uint32_t nwait;
    int watch;
    /* chained launch: its hash kernel waits on the last launch's event
     * (device-side order), so it starts the moment that one ends instead of
     * after the host has seen it end and enqueued it (~1.3 ms per C3 step,
     * profiles/r04b/c3q_gaps.json); chain_at = when it should start */
    hipEvent_t chain_ev;
    uint64_t chain_at;
    /* chain mode 2, both launches BALANCED: no device-side wait -- this
     * launch's workgroups take CUs as the running one's finish (a BALANCED
     * workgroup holds 96 KiB of LDS, so two never share a CU) */
    int chain_overlap;
    /* a synchronous caller's chunks are here: the slot goes while a slot is
     * left over to coalesce the callers behind it (slot_try_launch) */
    int urgent;
    /* md5hip_batcher_inject_fault: this launch completes as a device fault */
    int inject;
    /* verify segments (struct seg): how many the slot holds, the bytes of host
     * callers' expected values copied into h_vin so far, and the compare
     * entries of its launch.  h_vin / d_vin (expected values, then the table)
     * and h_vout / d_vout (one count per entry, then an ok byte per chunk) are
     * the slot's share of the batcher's verify buffers: NULL until the first
     * verify submission (verify_buffers) */
    uint32_t nverify, nvent;
    uint64_t vwant;
    unsigned char *h_vin, *d_vin, *h_vout, *d_vout;
};
enum { WATCH_NONE = 0, WATCH_ACTIVE, WATCH_GAVE_UP };

struct md5hip_batcher {
    int device;
    int kind;          /* enum md5hip_digest_kind */
    uint32_t fastcrc;  /* CRC-32 head^tail window (blk_io.c:408-424), 0 = whole block */
    uint32_t nslots;
    uint64_t cap;      /* staging bytes per slot */
    uint64_t maxn;     /* chunks per slot */
    uint64_t segcap;   /* gather segments per slot (zero-copy modes) */
    int gather;        /* enum md5hip_gather_mode */
    uint32_t target;   /* launch the open slot at once while fewer slots are in flight */
    uint32_t linger_max_us;  /* idle pipeline: hold a slot up to this long for more work */
    double launch_ema_us;    /* recent launches' wall time (submit to retire) */
    struct slot *s;
    int open;          /* index of the OPEN slot new chunks go to, -1 = none */
    uint32_t inflight;
    struct tk_ring tk; /* tickets: live ids, their references and errors (md5_tickets.h), under mu */
    uint64_t load_bytes;      /* weight (len + 64 per chunk) reserved and not yet retired:
                                 read without the lock by md5hip_batcher_load (the pool's router) */
    struct md5hip_batcher_stats st;
    pthread_mutex_t mu;
    pthread_cond_t done_cv;   /* a slot retired / a ticket completed */
    pthread_cond_t work_cv;   /* a slot went in flight / stop */
    pthread_t progress;
    int progress_started, stop;
    int poll_fast;            /* the progress thread polls launches every 10 us now */
    uint32_t slot_waiters;    /* submitters waiting for a slot to retire (slot_wait) */
    int chain;                /* chain the open slot behind the running launch: 0 off, 1 on, 2 (default) on + BALANCED tails overlap */
    hipEvent_t after_ev;     /* recorded on a producer's stream (md5_batch_submit_device_on) */
    int failed;               /* 0, or -ENODEV once the device failed (sticky; read lock-free by the pool) */
    uint64_t inject_at;       /* md5hip_batcher_inject_fault: launch number that faults, 0 = none */
    /* verify buffers of all slots, allocated by the first verify submission
     * (verify_buffers): pinned host and device, `vin_sz` / `vout_sz` per slot */
    unsigned char *vb_hin, *vb_din, *vb_hout, *vb_dout;
    uint64_t vin_sz, vout_sz;
    int vready;
    /* page tables of all slots, allocated by the first paged submission
     * (pages_buffers): pinned host and device, `pgcap` entries per slot */
    uint64_t *pb_h, *pb_d;
    uint64_t pgcap;
    int pready;
};

#define CK(x) do { if ((x) != hipSuccess) { rc = -ENODEV; goto fail; } } while (0)

/* the earliest a slot is chained behind the running launch: this long
 * before that launch's expected end (at most; a quarter of a launch for
 * short ones), so late submissions still coalesce into it */
#define CHAIN_LEAD_MAX_US 2000.0

static uint64_t now_us(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (uint64_t)ts.tv_sec * 1000000u + (uint64_t)ts.tv_nsec / 1000u;
}

/* How long an idle pipeline holds an open slot for more work: 1/8 of the
 * recent launches' wall time, at most linger_max_us.  A burst of vectors
 * submitted back to back then goes out as one launch instead of its first
 * vector alone (a mixed vector alone is bound by its longest chains, DESIGN.md
 * §5.4), and the added latency stays a fraction of the work itself. */
static uint64_t linger_us(const md5hip_batcher *b)
{
    const double l = b->launch_ema_us / 8.0;
    return l < (double)b->linger_max_us ? (uint64_t)l : (uint64_t)b->linger_max_us;
}

/* pthread_cond_timedwait on cv until `us` microseconds from now (mu held) */
static void wait_cv_us(md5hip_batcher *b, pthread_cond_t *cv, uint64_t us)
{
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    ts.tv_sec += (time_t)(us / 1000000u);
    ts.tv_nsec += (long)(us % 1000000u) * 1000;
    if (ts.tv_nsec >= 1000000000L) { ts.tv_sec++; ts.tv_nsec -= 1000000000L; }
    pthread_cond_timedwait(cv, &b->mu, &ts);
}
static void wait_work_us(md5hip_batcher *b, uint64_t us) { wait_cv_us(b, &b->work_cv, us); }

/* One segment per (ticket, slot): a submission fills a slot until it is full
 * before it moves on, so its chunks in one slot are one contiguous run.  The
 * slot holds a reference on the ticket from here until it retires (mu held). */
static int seg_push(md5hip_batcher *b, struct slot *sl, struct seg sg)
{
    if (sl->nsegs == sl->capsegs) {
        const uint32_t nc = sl->capsegs ? 2 * sl->capsegs : 64;
        struct seg *p = realloc(sl->segs, nc * sizeof *p);
        if (!p) return -ENOMEM;
        sl->segs = p;
        sl->capsegs = nc;
    }
    sl->segs[sl->nsegs++] = sg;
    sl->tickets_in++;
    tk_ring_ref(&b->tk, sg.ticket);
    return 0;
}

/* Weight w (len + 64 per chunk) more in slot `sl` and in the batcher's load,
 * which the pool's router reads without the lock (mu held).  A retiring slot
 * takes its whole share out again: w = -sl->load, modulo 2^64. */
static void load_add(md5hip_batcher *b, struct slot *sl, uint64_t w)
{
    sl->load += w;
    __atomic_store_n(&b->load_bytes, b->load_bytes + w, __ATOMIC_RELAXED);
}

static int seg_has(const struct slot *sl, uint64_t t)
{
    for (uint32_t k = 0; k < sl->nsegs; k++)
        if (sl->segs[k].ticket == t) return 1;
    return 0;
}

/* Descriptors in and the plan (mu held): the new descriptor entries
 * [copied_n, n) go to the device, the whole slot is ordered longest-first
 * (md5hip_plan_desc) and the order follows, all on the slot's own stream.
 * Descriptors are final once reserved (append-only), so this may run while
 * the slot is still OPEN -- the progress thread does it while another slot's
 * launch keeps the device busy, and the launch then only enqueues the kernel.
 * Chunks appended after it are copied and the slot re-planned at launch (an
 * order copy still in flight is overwritten by the later one, same stream). */
/* Small slots (a netcache vector) skip the two descriptor copies: the kernel
 * reads the fine-grained pinned arrays in place, one PCIe round trip per wave
 * instead of two copy operations ahead of the launch on the slot's stream. */
enum { DESC_DIRECT_MAX = 4096, EARLY_COPY_MIN = 8192 };

/* The stable device order of a large slot: 0 done; 1 = refused before any
 * device work (scratch sized at creation too small for this slot's n /
 * kmax, an argument the sort does not take): fall back to order_scatter,
 * never a failed ticket for it; < 0 = the sort's launch failed (-EIO): the
 * slot fails, and no hash kernel runs on an order never written. */
static int stable_order(struct slot *sl, uint64_t n)
{
    const int e = md5hip_order_device_stable(sl->d_len, n, sl->hkmax, sl->d_sort, sl->sort_bytes,
                                             sl->d_ord, sl->stream);
    return e == -ENOSPC || e == -EINVAL ? 1 : e;
}

/* The descriptor entries not yet on the device, [copied_n, n), go there on
 * the slot's stream (mu held, n > copied_n). */
static int desc_copy(struct slot *sl)
{
    const uint64_t c0 = sl->copied_n, cn = sl->n - c0;
    if (hipMemcpyAsync(sl->d_off + c0, sl->h_off + c0, 8 * cn, hipMemcpyHostToDevice, sl->stream) ||
        hipMemcpyAsync(sl->d_len + c0, sl->h_len + c0, 4 * cn, hipMemcpyHostToDevice, sl->stream))
        return -EIO;
    sl->copied_n = sl->n;
    return 0;
}

static int slot_prepare(struct slot *sl)
{
    const uint64_t n = sl->n;
    if (sl->planned_n == n) return 0;
    sl->desc_direct = n <= DESC_DIRECT_MAX;
    if (!sl->desc_direct && n > sl->copied_n && desc_copy(sl)) return -EIO;
    int dvar, e = 0;
    if (!sl->unsorted) {
        dvar = sl->hovf ? md5hip_plan_desc(sl->h_len, n, sl->h_ord)
                        : md5hip_plan_hist(sl->hh, sl->hkmax, n, NULL);
        if (dvar < 0) return dvar;
        sl->use_order = 0;
    } else if (!sl->hovf && !sl->desc_direct && sl->d_sort &&
               (dvar = md5hip_plan_hist(sl->hh, sl->hkmax, n, NULL)) >= 0 &&
               (e = stable_order(sl, n)) <= 0) {
        /* from the histogram: O(keys) on the host; the STABLE order on the
         * device (equal keys in chunk order: a 6-batch C3 BALANCED launch
         * ran 5-6 % longer in order_scatter's wave-arrival order,
         * profiles/r06e/order_ab.json) */
        if (e) return e;
    } else if (!sl->hovf) {
        /* small slots (lengths read in place from mapped host memory), and
         * large ones whose stable sort was refused: one scatter launch */
        dvar = md5hip_plan_hist(sl->hh, sl->hkmax, n, sl->h_bkt);
        if (dvar < 0) return dvar;
        if (hipMemcpyAsync(sl->d_bkt, sl->h_bkt, 4 * ((size_t)sl->hkmax + 1), hipMemcpyHostToDevice,
                           sl->stream))
            return -EIO;
        e = md5hip_order_device(sl->desc_direct ? sl->dh_len : sl->d_len, n, sl->hkmax, sl->d_bkt,
                                sl->d_ord, sl->stream);
        if (e) return e;
    } else {
        dvar = md5hip_plan_desc(sl->h_len, n, sl->h_ord);
        if (dvar < 0) return dvar;
        if (hipMemcpyAsync(sl->d_ord, sl->h_ord, 4 * n, hipMemcpyHostToDevice, sl->stream)) return -EIO;
    }
    if (sl->unsorted) sl->use_order = 1;
    /* host-staged chunks sit on 128-B lines; device-resident ones as placed */
    sl->plan_var = md5hip_lines_choice(dvar, sl->unlined, sl->payload);
    sl->planned_n = n;
    return 0;
}

/* Bytes in for a staged or zero-copy slot: one H2D copy of the pinned
 * staging, or the registered pages by the gather kernel or by DMA per run. */
static int enqueue_bytes(md5hip_batcher *b, struct slot *sl)
{
    if (sl->mode == MODE_STAGED && sl->used) {
        if (hipMemcpyAsync(sl->d_data, sl->h_data, sl->used, hipMemcpyHostToDevice, sl->stream))
            return -EIO;
    } else if (sl->mode == MODE_ZEROCOPY && sl->nseg) {
        int mode = b->gather;
        if (mode == MD5HIP_GATHER_AUTO)
            /* measured: per-copy DMA beats the PCIe-reading
             * gather kernel once copies average more than ~192 KiB */
            mode = sl->ndma * (256u << 10) <= sl->used ? MD5HIP_GATHER_DMA : MD5HIP_GATHER_DEVICE;
        if (mode == MD5HIP_GATHER_DEVICE) {
            if (hipMemcpyAsync(sl->d_seg, sl->h_seg, sizeof(struct md5hip_seg) * sl->nseg,
                               hipMemcpyHostToDevice, sl->stream))
                return -EIO;
            return md5hip_gather_launch(sl->d_seg, sl->nseg, sl->d_data, sl->stream);
        }
        /* one async copy per run (hipMemcpyBatchAsync is newer than the
         * HIP runtime torch ships, which this library shares) */
        for (uint64_t q = 0; q < sl->ndma; q++)
            if (hipMemcpyAsync(sl->b_dst[q], sl->b_src[q], sl->b_len[q], hipMemcpyHostToDevice,
                               sl->stream) != hipSuccess)
                return -EIO;
    }
    return 0;
}

/* The MD5_CRC32 launches: the kernel is md5crc32hip_plan's (small vectors
 * run as fed pairs beside split CRCs); a build that has the plain launchers
 * only (md5_internal.h) calls those. */
static int dual_fixed(const void *src, uint64_t n, uint32_t len, uint64_t stride, struct md5hip_md5crc32 *dst,
                      void *stream)
{
    return md5hip_md5crc32_variants_present()
               ? md5crc32hip_fixed_variant(src, n, len, stride, dst, stream, MD5CRC32HIP_AUTO)
               : md5crc32hip_fixed(src, n, len, stride, dst, stream);
}

static int dual_desc(const void *base, const uint64_t *off, const uint32_t *len, const uint32_t *ord, uint64_t n,
                     uint64_t mean_len, struct md5hip_md5crc32 *dst, void *stream)
{
    return md5hip_md5crc32_variants_present()
               ? md5crc32hip_desc_variant(base, off, len, ord, n, dst, stream, md5crc32hip_plan(n, mean_len))
               : md5crc32hip_desc(base, off, len, ord, n, dst, stream);
}

/* The hash kernel, digests to `dst`, and `kdone` behind it. */
static int enqueue_kernel(struct slot *sl, unsigned char *dst)
{
    int rc;
    const uint64_t n = sl->n;
    /* a chained launch: bytes in and plan made beside the running launch,
     * the hash kernel after it.  Never a FIXED slot: chain_ev is set on the
     * open slot only (chain_open), and a FIXED slot is never b->open */
    if (sl->chain_ev && !sl->chain_overlap && hipStreamWaitEvent(sl->stream, sl->chain_ev, 0) != hipSuccess)
        return -EIO;
    if (sl->mode == MODE_FIXED) {
        /* host_fixed: the bytes are on their way already (its copy was
         * enqueued on this stream outside b->mu); device_fixed: they are
         * read where the caller keeps them */
        const void *src = sl->fx_dev ? (const void *)sl->fx_src : (const void *)sl->d_data;
        rc = sl->kind == MD5HIP_DIGEST_CRC32
                 ? crc32hip_fixed(src, n, sl->fx_len, sl->fx_stride, sl->fastcrc, (uint32_t *)dst, sl->stream)
             : sl->kind == MD5HIP_DIGEST_MD5_CRC32
                 ? dual_fixed(src, n, sl->fx_len, sl->fx_stride, (struct md5hip_md5crc32 *)dst, sl->stream)
                 : md5hip_digest_fixed(src, n, sl->fx_len, sl->fx_stride, dst, sl->stream);
    } else if (sl->mode == MODE_PAGES) {
        /* the pages are read where they lie, through the tables just sent
         * (enqueue_tables); under a fastcrc window (a paged verify: the submit
         * entry refuses one) only the windows' granules */
        const uint32_t *ord = sl->use_order ? sl->d_ord : NULL;
        rc = sl->fastcrc ? crc32hip_pages(sl->d_pg, sl->d_off, sl->d_len, ord, n, sl->pg_bytes, sl->fastcrc,
                                          (uint32_t *)dst, sl->stream)
                         : md5hip_digest_pages((int)sl->kind, sl->d_pg, sl->d_off, sl->d_len, ord, n, sl->pg_bytes,
                                               dst, sl->stream);
    } else {
        const uint32_t *ord = sl->use_order ? sl->d_ord : NULL;
        const uint64_t *doff = sl->desc_direct ? sl->dh_off : sl->d_off;
        const uint32_t *dlen = sl->desc_direct ? sl->dh_len : sl->d_len;
        rc = sl->kind == MD5HIP_DIGEST_CRC32
                 ? crc32hip_desc_variant(sl->d_data, doff, dlen, ord, n, sl->fastcrc,
                                         (uint32_t *)dst, sl->stream,
                                         md5hip_crc_desc_choice(sl->fastcrc ? 2 * n : n,
                                                                sl->fastcrc ? sl->fastcrc
                                                                            : sl->load / n - 64))
             : sl->kind == MD5HIP_DIGEST_MD5_CRC32      /* the plan's order; the kernel by the mean length */
                 ? dual_desc(sl->d_data, doff, dlen, ord, n, sl->load / n - 64, (struct md5hip_md5crc32 *)dst,
                             sl->stream)
                 : md5hip_digest_desc_variant(sl->d_data, doff, dlen, ord, n,
                                              dst, sl->stream, sl->plan_var);
    }
    if (rc) return rc;
    return hipEventRecord(sl->kdone, sl->stream) ? -EIO : 0;
}

/* A paged slot's tables to the device: the page addresses, each chunk's first
 * entry, the lengths and, when the slice is not longest-first as it came,
 * the order (the submitter filled the pinned arrays: pages_fill). */
static int enqueue_tables(struct slot *sl)
{
    const uint64_t n = sl->n;
    if ((sl->pg_n && hipMemcpyAsync(sl->d_pg, sl->h_pg, 8 * sl->pg_n, hipMemcpyHostToDevice, sl->stream)) ||
        hipMemcpyAsync(sl->d_off, sl->h_off, 8 * n, hipMemcpyHostToDevice, sl->stream) ||
        hipMemcpyAsync(sl->d_len, sl->h_len, 4 * n, hipMemcpyHostToDevice, sl->stream) ||
        (sl->use_order && hipMemcpyAsync(sl->d_ord, sl->h_ord, 4 * n, hipMemcpyHostToDevice, sl->stream)))
        return -EIO;
    return 0;
}

/* The slot's verify segments, compared where the digests are (behind kdone,
 * like the scatter: a chained launch does not wait on it): the table of
 * compare entries -- a segment cut into ranges of MD5HIP_CMP_PIECE chunks,
 * one workgroup each -- goes up behind the host callers' expected values in
 * ONE copy, ONE launch compares over d_dig, and the entries' counts and the
 * host callers' ok bytes come back in ONE copy.  Device callers' expected
 * values are read and their ok bytes written in place.  The table has room:
 * verify_buffers sized it for maxn chunks in segcap segments. */
static int enqueue_verify(struct slot *sl)
{
    uint32_t nent = 0;
    int host_ok = 0;
    for (uint32_t k = 0; k < sl->nsegs; k++)
        if (sl->segs[k].ok) nent += (uint32_t)((sl->segs[k].count + MD5HIP_CMP_PIECE - 1) / MD5HIP_CMP_PIECE);
    const uint64_t tab_at = (sl->vwant + 15) & ~15ull;
    struct md5hip_cmp *tab = (struct md5hip_cmp *)(sl->h_vin + tab_at);
    unsigned char *d_ok = sl->d_vout + 8 * (size_t)nent;      /* ok byte of slot chunk c: d_ok + c */
    uint32_t e = 0;
    for (uint32_t k = 0; k < sl->nsegs; k++) {
        struct seg *g = &sl->segs[k];
        if (!g->ok) continue;
        const uint64_t want = g->on_device ? g->want : (uint64_t)(uintptr_t)sl->d_vin + g->want;
        const uint64_t ok = (uint64_t)(uintptr_t)(g->on_device ? g->ok : d_ok + g->first);
        host_ok |= !g->on_device;
        g->ent = e;
        for (uint64_t at = 0; at < g->count; at += MD5HIP_CMP_PIECE, e++) {
            const uint64_t c = g->count - at < MD5HIP_CMP_PIECE ? g->count - at : MD5HIP_CMP_PIECE;
            tab[e] = (struct md5hip_cmp){g->first + at, c, want + (uint64_t)g->wsz * at, ok + at,
                                         (uint64_t)(uintptr_t)(sl->d_vout + 8 * (size_t)e), g->goff, g->wsz};
        }
        g->nent = e - g->ent;
    }
    sl->nvent = nent;
    if (hipMemcpyAsync(sl->d_vin, sl->h_vin, tab_at + sizeof(struct md5hip_cmp) * nent, hipMemcpyHostToDevice,
                       sl->stream))
        return -EIO;
    const int rc = md5hip_compare_launch(sl->d_dig, sl->dsz, (const struct md5hip_cmp *)(sl->d_vin + tab_at), nent,
                                         sl->stream);
    if (rc) return rc;
    return hipMemcpyAsync(sl->h_vout, sl->d_vout, 8 * (size_t)nent + (host_ok ? sl->n : 0), hipMemcpyDeviceToHost,
                          sl->stream)
               ? -EIO
               : 0;
}

/* Digests out: one D2H for the host segments, one scatter for the device
 * ones, then `done`.  The scatter kernel runs one workgroup per entry, so a
 * long segment is cut into pieces of DSC_PIECE bytes as the table has room
 * (6 tickets of 79 K digests as 6 entries took 145 us) */
static int enqueue_digests(md5hip_batcher *b, struct slot *sl)
{
    int rc;
    const uint64_t n = sl->n;
    enum { DSC_PIECE = 64 << 10 };
    int any_host = 0;
    sl->ndsc = 0;
    uint64_t ndev = 0;
    for (uint32_t k = 0; k < sl->nsegs && !sl->direct; k++) ndev += sl->segs[k].on_device && !sl->segs[k].ok;
    uint64_t spare = b->segcap - ndev;                   /* nsegs < segcap (slot_open) */
    for (uint32_t k = 0; k < sl->nsegs && !sl->direct; k++) {
        const struct seg *g = &sl->segs[k];
        /* a verify segment takes no digests, but an upgrade's MD5s (host) */
        if (g->ok) { any_host |= g->md5_out != NULL; continue; }
        if (!g->on_device) { any_host = 1; continue; }
        const uint64_t len = (uint64_t)sl->dsz * g->count;
        if (len == 0) continue;
        uint64_t extra = (len + DSC_PIECE - 1) / DSC_PIECE - 1;
        if (extra > spare) extra = spare;
        spare -= extra;
        const uint64_t piece = ((len + extra) / (extra + 1) + 15) & ~15ull;   /* 16-B multiples */
        for (uint64_t at = 0; at < len; at += piece) {
            const uint64_t l = len - at < piece ? len - at : piece;
            sl->h_dsc[sl->ndsc++] = (struct md5hip_seg){
                (uint64_t)(uintptr_t)(sl->d_dig + (size_t)sl->dsz * g->first + at),
                (uint64_t)((uintptr_t)g->user + at - (uintptr_t)sl->d_dig),   /* relative to d_dig (mod 2^64) */
                (uint32_t)l, 0};
        }
    }
    if (sl->ndsc) {
        if (hipMemcpyAsync(sl->d_dsc, sl->h_dsc, sizeof(struct md5hip_seg) * sl->ndsc,
                           hipMemcpyHostToDevice, sl->stream))
            return -EIO;
        if ((rc = md5hip_gather_launch(sl->d_dsc, sl->ndsc, sl->d_dig, sl->stream))) return rc;
    }
    if (sl->nverify && (rc = enqueue_verify(sl))) return rc;
    if (any_host &&
        hipMemcpyAsync(sl->h_dig, sl->d_dig, (size_t)sl->dsz * n, hipMemcpyDeviceToHost, sl->stream))
        return -EIO;
    return hipEventRecord(sl->done, sl->stream) ? -EIO : 0;
}

/* Enqueue slot `sl` (mu held, writers == 0): bytes in, kernel, digests out. */
static int slot_enqueue(md5hip_batcher *b, struct slot *sl)
{
    int rc;
    /* one submission whose digests stay on the device and fill the slot in
     * order: the kernel writes them in place (no scatter launch) */
    const struct seg *g0 = sl->nsegs == 1 ? &sl->segs[0] : NULL;
    unsigned char *dst = sl->d_dig;
    if (g0 && g0->on_device && !g0->ok && g0->first == 0 && g0->count == sl->n && ((uintptr_t)g0->user & 15u) == 0) {
        dst = g0->user;
        sl->direct = 1;
    }
    /* a FIXED slot has no descriptors, and its bytes are in (enqueue_kernel);
     * a PAGES slot has its tables, ordered by its submitter */
    if (sl->mode == MODE_PAGES) {
        if ((rc = enqueue_tables(sl))) return rc;
    } else if (sl->mode != MODE_FIXED && ((rc = slot_prepare(sl)) || (rc = enqueue_bytes(b, sl)))) {
        return rc;
    }
    if ((rc = enqueue_kernel(sl, dst))) return rc;
    return enqueue_digests(b, sl);
}

static void slot_reset(struct slot *sl)
{
    sl->state = SLOT_FREE;
    sl->watch = WATCH_NONE;
    sl->chain_ev = NULL;
    sl->chain_at = 0;
    sl->chain_overlap = 0;
    sl->urgent = 0;
    sl->inject = 0;
    sl->fx_dev = 0;
    sl->pg_n = 0;
    sl->mode = MODE_NONE;
    sl->writers = sl->full = sl->flush = sl->err = sl->direct = 0;
    sl->n = sl->used = sl->nseg = sl->ndma = sl->ndsc = 0;
    sl->nsegs = 0;
    sl->nverify = sl->nvent = 0;
    sl->vwant = 0;
    sl->tickets_in = 0;
    sl->copied_n = sl->planned_n = sl->seen_n = 0;
    sl->load = 0;
    sl->payload = sl->unlined = 0;
    sl->last_key = UINT32_MAX;
    sl->unsorted = sl->use_order = 0;
    if (sl->hh) memset(sl->hh, 0, sizeof(uint32_t) * ((size_t)sl->hkmax + 1));
    sl->hkmax = 0;
    sl->hovf = 0;
}

/* A finished launch's verify segment to its caller: ok (host callers), the
 * upgrade's MD5s from the records, then its entries' mismatches added into
 * *nbad -- atomically: the parts of a pool's submission share the counter,
 * and retire on several batchers. */
static void verify_deliver(const struct slot *sl, const struct seg *g)
{
    if (!g->on_device) memcpy(g->ok, sl->h_vout + 8 * (size_t)sl->nvent + g->first, g->count);
    for (uint64_t i = 0; g->md5_out && i < g->count; i++)
        memcpy(g->md5_out + 16 * i, sl->h_dig + 32 * (size_t)(g->first + i), 16);
    if (!g->nbad) return;
    uint64_t bad = 0, c;
    for (uint32_t e = g->ent; e < g->ent + g->nent; e++) {
        memcpy(&c, sl->h_vout + 8 * (size_t)e, 8);
        bad += c;
    }
    __atomic_fetch_add(g->nbad, bad, __ATOMIC_RELAXED);
}

/* Deliver a finished (or failed) slot to its tickets and free it (mu held). */
static void slot_retire(md5hip_batcher *b, struct slot *sl, int err)
{
    for (uint32_t k = 0; k < sl->nsegs; k++) {
        const struct seg *g = &sl->segs[k];
        if (g->ok) {
            if (!err) verify_deliver(sl, g);
        } else if (!err && !g->on_device)
            memcpy(g->user, sl->h_dig + (size_t)sl->dsz * g->first, (size_t)sl->dsz * g->count);
        tk_ring_put(&b->tk, g->ticket, err);
    }
    load_add(b, sl, -sl->load);
    if (sl->state == SLOT_INFLIGHT) {
        b->inflight--;
        /* a chained launch's start is estimated (chain_at): one that retires
         * before it (a BALANCED overlap started early) gives no sample */
        const uint64_t t = now_us();
        if (t > sl->launched_us) {
            const double d = (double)(t - sl->launched_us);
            b->launch_ema_us = b->launch_ema_us > 0 ? 0.75 * b->launch_ema_us + 0.25 * d : d;
        }
    }
    slot_reset(sl);
    if (sl->nwait) pthread_cond_broadcast(&sl->cv);   /* its waiters only */
    pthread_cond_broadcast(&b->done_cv);              /* slot_wait / drain / destroy */
}

/* The OPEN slot new chunks go to, or NULL; `sl` is it no longer (mu held). */
static struct slot *open_slot(const md5hip_batcher *b) { return b->open >= 0 ? &b->s[b->open] : NULL; }
static void unopen(md5hip_batcher *b, const struct slot *sl)
{
    if (b->open == (int)(sl - b->s)) b->open = -1;
}

/* Is the device behind this HIP status gone (a fault, a lost or reset
 * device) rather than the call merely refused?  Completion events report
 * only these; an enqueue error is classified by the stream's state after it. */
static int hip_lost(hipError_t e)
{
    switch (e) {
    case hipSuccess: case hipErrorNotReady:
    case hipErrorInvalidValue: case hipErrorOutOfMemory: case hipErrorInvalidDevicePointer:
    case hipErrorInvalidMemcpyDirection: case hipErrorInvalidConfiguration:
    case hipErrorInvalidResourceHandle: case hipErrorNotSupported:
        return 0;
    default:
        return 1;
    }
}

/* The device failed (mu held): sticky.  Tickets coalescing in the open slot
 * are retired with -ENODEV (or when their writers are done: sl->err); slots
 * in flight finish as their events say; callers blocked on a slot are woken
 * by its retire, everything waiting for a free slot by done_cv. */
static void batcher_fail(md5hip_batcher *b)
{
    if (b->failed) return;
    __atomic_store_n(&b->failed, -ENODEV, __ATOMIC_RELEASE);
    b->inject_at = 0;
    for (uint32_t k = 0; k < b->nslots; k++) {
        struct slot *sl = &b->s[k];
        if (sl->state != SLOT_OPEN) continue;
        unopen(b, sl);
        sl->full = 1;
        if (!sl->err) sl->err = -ENODEV;
        if (!sl->writers) slot_retire(b, sl, sl->err);
    }
    pthread_cond_broadcast(&b->done_cv);
    pthread_cond_broadcast(&b->work_cv);
}

/* A launch's completion (mu not needed): its event, or the injected fault
 * once the launch has really finished. */
static hipError_t launch_status(hipEvent_t ev, int inject)
{
    const hipError_t e = hipEventQuery(ev);
    return e == hipSuccess && inject ? hipErrorLaunchFailure : e;
}

/* Retire in-flight slot `sl` whose completion status is `e` (mu held). */
static void slot_complete(md5hip_batcher *b, struct slot *sl, hipError_t e)
{
    slot_retire(b, sl, e == hipSuccess ? 0 : -EIO);
    if (e != hipSuccess) batcher_fail(b);
}

/* Launch slot `sl` if it may go now (mu held). */
static void slot_try_launch(md5hip_batcher *b, struct slot *sl)
{
    if (sl->state != SLOT_OPEN || sl->writers) return;
    /* callers blocked on its tickets: no linger once the device is idle (as
     * md5_batch_wait's hasten, re-applied whenever the slot is looked at,
     * since they sleep until it goes) */
    if (sl->nwait && b->inflight == 0) sl->flush = 1;
    /* synchronous callers: up to nslots - 1 launches run at once (a netcache
     * vector is a wave or two: concurrent small launches cost the device
     * nothing), the last slot coalesces whoever comes while they run */
    if (sl->urgent && b->inflight + 1 < b->nslots) sl->flush = 1;
    if (sl->n == 0) {                 /* nothing reserved (all chunks failed) */
        unopen(b, sl);
        slot_retire(b, sl, sl->err);
        return;
    }
    if (!(sl->full || sl->flush || sl->chain_ev || b->inflight < b->target)) return;
    if (!sl->full && !sl->flush && b->inflight == 0 && now_us() - sl->opened_us < linger_us(b)) {
        pthread_cond_broadcast(&b->work_cv);        /* the progress thread times the linger */
        return;
    }
    unopen(b, sl);
    const int rc = sl->err ? sl->err : b->failed ? b->failed : slot_enqueue(b, sl);
    if (rc) {
        /* an enqueue (here, or a descriptor copy or ordering made earlier:
         * sl->err) that failed because the device did: the stream says so */
        const int lost = !b->failed && rc != -ENODEV && hip_lost(hipStreamQuery(sl->stream));
        slot_retire(b, sl, rc);
        if (lost) batcher_fail(b);
        return;
    }
    if (b->inject_at && b->st.launches + 1 == b->inject_at) {
        sl->inject = 1;
        b->inject_at = 0;
    }
    sl->state = SLOT_INFLIGHT;
    sl->launched_us = now_us();
    if (sl->chain_ev && sl->chain_at > sl->launched_us) sl->launched_us = sl->chain_at;   /* its real start */
    sl->gen++;
    b->inflight++;
    b->st.launches++;
    b->st.chunks += sl->n;
    b->st.bytes_staged += sl->used;
    if (sl->n > b->st.max_chunks_per_launch) b->st.max_chunks_per_launch = sl->n;
    if (sl->tickets_in > 1) b->st.coalesced_launches++;
    if (sl->tickets_in > b->st.max_tickets_per_launch) b->st.max_tickets_per_launch = sl->tickets_in;
    if (sl->nwait) pthread_cond_signal(&sl->cv);      /* one sleeper becomes its watcher */
    pthread_cond_broadcast(&b->work_cv);
}

/* A submitter waits for a slot to retire (mu held).  The progress thread
 * polls the launches every 10 us meanwhile instead of its idle 20-200 us:
 * nobody else may be waiting on a ticket (an asynchronous stream whose
 * every slot is in flight), and the retire it waits for gates its whole
 * submission -- a stream of 1 M-block fastcrc launches (~55 us each) lost
 * half its time to that poll before. */
static void slot_wait(md5hip_batcher *b)
{
    b->slot_waiters++;
    if (!b->poll_fast) pthread_cond_broadcast(&b->work_cv);
    pthread_cond_wait(&b->done_cv, &b->mu);
    b->slot_waiters--;
}

/* The open slot, looked at again / flushed (no linger, no inflight target) /
 * closed: full, no longer b->open, launched once its writers are done
 * (mu held; nothing when no slot is open). */
static void try_open(md5hip_batcher *b)
{
    struct slot *o = open_slot(b);
    if (o) slot_try_launch(b, o);
}

static void flush_open(md5hip_batcher *b)
{
    struct slot *o = open_slot(b);
    if (!o) return;
    o->flush = 1;
    slot_try_launch(b, o);
}

static void close_open(md5hip_batcher *b)
{
    struct slot *o = open_slot(b);
    if (!o) return;
    o->full = 1;
    b->open = -1;
    slot_try_launch(b, o);
}

/* A FREE slot made OPEN in `mode` for digests of `kind`, or NULL (mu held). */
static struct slot *slot_claim(md5hip_batcher *b, int mode, int kind, uint32_t fastcrc)
{
    for (uint32_t k = 0; k < b->nslots; k++) {
        struct slot *sl = &b->s[k];
        if (sl->state != SLOT_FREE) continue;
        slot_reset(sl);
        sl->state = SLOT_OPEN;
        sl->mode = mode;
        sl->kind = (uint32_t)kind;
        sl->fastcrc = fastcrc;
        sl->dsz = md5hip_digest_size(kind);
        return sl;
    }
    return NULL;
}

/* A slot of the caller's own, not b->open (mu held; waits for one to retire). */
static struct slot *slot_take(md5hip_batcher *b, int mode, int kind, uint32_t fastcrc)
{
    struct slot *sl;
    while (!(sl = slot_claim(b, mode, kind, fastcrc))) {
        close_open(b);                /* all busy: make sure the open slot can go */
        slot_wait(b);
    }
    return sl;
}

/* The OPEN slot that accepts chunks of `mode` and digest `kind` (mu held). */
/* The open slot is re-examined after every wait for a free one: another
 * submitter may have opened one meanwhile, and taking a second slot then
 * would leave the first OPEN but no longer b->open -- launched by nobody
 * (its asynchronous tickets stranded until a wait on them). */
static struct slot *slot_open(md5hip_batcher *b, int mode, int kind, uint32_t fastcrc)
{
    for (;;) {
        struct slot *o = open_slot(b);
        if (o) {
            const int compatible = (o->mode == mode || mode == MODE_NONE || o->mode == MODE_NONE) &&
                                   o->kind == (uint32_t)kind && o->fastcrc == fastcrc;
            if (!o->full && compatible && o->nsegs < b->segcap) {
                if (o->mode == MODE_NONE) o->mode = mode;
                return o;
            }
            close_open(b);
        }
        if ((o = slot_claim(b, mode, kind, fastcrc))) {
            b->open = (int)(o - b->s);
            return o;
        }
        slot_wait(b);                                 /* all busy: wait for a retire */
    }
}

/* The slot the next chunks of a submission go to (mu held): one of its own
 * for MODE_FIXED (straight from the caller's buffer; the open slot keeps
 * coalescing other work), else the open slot.  NULL once the device has
 * failed -- before, or while this waited for a slot: the empty slot it was
 * given then retires. */
static struct slot *slot_for(md5hip_batcher *b, int mode, int kind, uint32_t fastcrc)
{
    if (b->failed) return NULL;
    struct slot *sl = (mode == MODE_FIXED || mode == MODE_PAGES ? slot_take : slot_open)(b, mode, kind, fastcrc);
    if (!b->failed) return sl;
    slot_try_launch(b, sl);
    return NULL;
}

/* ------------------------------------------------------------------------
 * Progress thread: retire finished slots, launch coalesced work.
 * ------------------------------------------------------------------------ */
/* Retire every in-flight slot whose launch has finished; were there any? */
static int retire_finished(md5hip_batcher *b)
{
    int any = 0;
    for (uint32_t k = 0; k < b->nslots; k++) {
        struct slot *sl = &b->s[k];
        if (sl->state != SLOT_INFLIGHT) continue;
        const hipError_t e = launch_status(sl->done, sl->inject);
        if (e == hipErrorNotReady) continue;
        slot_complete(b, sl, e);
        any = 1;
    }
    return any;
}

/* Nothing in flight: time the open slot's linger and launch it, or sleep
 * until there is work. */
static void idle_wait(md5hip_batcher *b)
{
    struct slot *o = open_slot(b);
    if (o && o->state == SLOT_OPEN && o->n > 0 && !o->writers) {
        const uint64_t waited = now_us() - o->opened_us, l = linger_us(b);
        if (waited >= l) slot_try_launch(b, o);    /* lingered long enough */
        else wait_work_us(b, l - waited);
    } else {
        pthread_cond_wait(&b->work_cv, &b->mu);
    }
}

/* The device is busy: get open slot `o`'s descriptors over and its plan
 * made now, once no chunk arrived since the last poll, so its launch is
 * only the kernel when the running one retires. */
static void prepare_ahead(struct slot *o)
{
    if (o->state != SLOT_OPEN || o->mode == MODE_FIXED || o->n <= o->planned_n) return;
    if (o->n == o->seen_n) {
        const int e = slot_prepare(o);
        if (e && !o->err) o->err = e;
    }
    o->seen_n = o->n;
}

/* Open slot `o` planned and quiet, the pipeline at its target, and the last
 * launch due to end within min(2 ms, a quarter of a launch): chain it there
 * (its kernel waits on that launch's event).  Not behind a launch overdue by
 * more than that: its end is unknown, and the open slot keeps coalescing
 * until it retires.  Did it chain? */
static int chain_open(md5hip_batcher *b, struct slot *o)
{
    if (!(b->chain && o->state == SLOT_OPEN && o->n && !o->writers && !o->err && !o->chain_ev &&
          o->mode != MODE_FIXED && o->planned_n == o->n && b->inflight == b->target &&
          b->launch_ema_us > 0))
        return 0;
    struct slot *last = NULL;
    for (uint32_t k = 0; k < b->nslots; k++)
        if (b->s[k].state == SLOT_INFLIGHT && (!last || b->s[k].launched_us > last->launched_us))
            last = &b->s[k];
    const double lead = b->launch_ema_us / 4 < CHAIN_LEAD_MAX_US ? b->launch_ema_us / 4
                                                                 : CHAIN_LEAD_MAX_US;
    const uint64_t end = last ? last->launched_us + (uint64_t)b->launch_ema_us : 0;
    const uint64_t now = now_us();
    if (!(last && (double)now + lead >= (double)end && (double)now <= (double)end + lead)) return 0;
    o->chain_ev = last->kdone;
    o->chain_at = end > now ? end : now;
    o->chain_overlap = b->chain == 2 && last->mode != MODE_FIXED &&
                       last->kind == MD5HIP_DIGEST_MD5 && o->kind == MD5HIP_DIGEST_MD5 &&
                       last->plan_var == MD5HIP_DESC_BALANCED &&
                       o->plan_var == MD5HIP_DESC_BALANCED;
    slot_try_launch(b, o);
    return 1;
}

/* Poll interval: idle_us (20 -> 200 us) while nobody waits; blocked callers
 * pin it at 10 us (a short launch is not delivered up to 200 us late)
 * unless each of their launches has a watcher of its own: callers on an
 * open slot (it goes when a launch retires), or on a launch with no watcher
 * yet or whose watcher's spin ran out. */
static unsigned poll_interval_us(md5hip_batcher *b, unsigned idle_us)
{
    int fast = b->slot_waiters > 0;
    for (uint32_t k = 0; k < b->nslots; k++)
        fast |= b->s[k].nwait && !(b->s[k].state == SLOT_INFLIGHT && b->s[k].watch == WATCH_ACTIVE);
    b->poll_fast = fast;
    return fast ? 10u : idle_us;
}

static void *progress_main(void *arg)
{
    md5hip_batcher *b = arg;
    (void)hipSetDevice(b->device);
    /* this thread's timed waits are the event polls (10 us while a caller
     * waits): the default 50 us timer slack would stretch each to ~60 us and
     * deliver a finished launch that much late */
    (void)prctl(PR_SET_TIMERSLACK, 1000UL, 0, 0, 0);
    pthread_mutex_lock(&b->mu);
    unsigned idle_us = 20;
    while (!b->stop) {
        b->poll_fast = 0;
        if (retire_finished(b)) {
            try_open(b);
            idle_us = 20;
        } else if (b->inflight == 0) {
            idle_wait(b);
            idle_us = 20;
        } else {
            struct slot *o = open_slot(b);
            if (o) {
                prepare_ahead(o);
                chain_open(b, o);
            }
            wait_work_us(b, poll_interval_us(b, idle_us));
            if (idle_us < 200) idle_us += 20;
        }
    }
    pthread_mutex_unlock(&b->mu);
    return NULL;
}

/* ------------------------------------------------------------------------
 * Blocked callers.  A caller blocked on ticket t sleeps on the condition
 * variable of a slot holding t, so a retire wakes only that slot's callers
 * (the netcache ASIO pool runs 4-512 threads into this site at once,
 * asio_mgr.c:86-91, :205, :1050-1057, and a coalesced launch holds many of
 * their vectors).  Waiting for the progress thread alone, a synchronous call
 * returns up to one poll (10 us) plus a wake-up after its kernel ends -- for
 * a netcache vector (a ~140 us kernel) 20-30 us of each call -- so ONE caller
 * per launch watches it: a launch expected to end soon (recent launches' wall
 * time) has its event polled by that caller, who retires the slot the moment
 * it completes; a longer one is slept through first.  Every other caller on
 * the launch sleeps until the retire.  The spin is bounded; past it the
 * watcher sleeps too and the progress thread (polling fast meanwhile)
 * retires the launch.  Every sleep re-checks its condition under b->mu, and
 * every state change that ends one (retire, launch) is made under b->mu and
 * broadcast or signalled, so no wake-up is lost.
 * ------------------------------------------------------------------------ */
enum { WATCH_TAIL_US = 50, WATCH_TAIL_SPIN_US = 150 };

static void cpu_relax(void)
{
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}

/* The watcher's sleep on the slot's condition variable until `us` from now
 * ends within a few us of its deadline, not the default 50 us timer slack
 * later (the caller's own slack is put back after). */
static void watch_sleep(md5hip_batcher *b, struct slot *sl, uint64_t us)
{
    const int old = prctl(PR_GET_TIMERSLACK, 0, 0, 0, 0);
    if (old > 2000) (void)prctl(PR_SET_TIMERSLACK, 2000UL, 0, 0, 0);
    sl->nwait++;
    wait_cv_us(b, &sl->cv, us);
    sl->nwait--;
    if (old > 2000) (void)prctl(PR_SET_TIMERSLACK, (unsigned long)old, 0, 0, 0);
}

/* Watch in-flight slot `sl` (mu held on entry and exit, watch == NONE):
 * sleep on the slot until 50 us before the launch is due (recent launches'
 * wall time), then poll its event for at most 150 us; past that the watcher
 * gives up and sleeps too, and the progress thread (polling every 10 us
 * meanwhile) retires it.  Two other policies were measured against this one
 * and removed (profiles/r05e/asio_watch.json, profiles/r05f/; git history):
 * polling a launch due within 300 us for up to 500 us cost a call's thread
 * 122 us of CPU at 8 callers instead of 33-39, same latency; and
 * hipEventSynchronize on a blocking-sync event woke up ~1 ms late per call
 * for ~190 us of CPU. */
static void watch_launch(md5hip_batcher *b, struct slot *sl)
{
    const uint64_t gen = sl->gen;
    sl->watch = WATCH_ACTIVE;
    for (;;) {                                  /* long launch: sleep most of it */
        const uint64_t now = now_us(), end = sl->launched_us + (uint64_t)b->launch_ema_us;
        if (end <= now + WATCH_TAIL_US) break;
        watch_sleep(b, sl, end - now - WATCH_TAIL_US);
        if (sl->state != SLOT_INFLIGHT || sl->gen != gen) return;     /* retired meanwhile */
    }
    const hipEvent_t ev = sl->done;
    const int inject = sl->inject;
    pthread_mutex_unlock(&b->mu);
    hipError_t e;
    const uint64_t t0 = now_us();
    while ((e = launch_status(ev, inject)) == hipErrorNotReady && now_us() - t0 < WATCH_TAIL_SPIN_US) cpu_relax();
    pthread_mutex_lock(&b->mu);
    /* the same launch still in flight? (the progress thread may have retired
     * it, and the slot may even be in flight again with other work: then
     * `watch` belongs to that launch and is left alone) */
    if (sl->state != SLOT_INFLIGHT || sl->gen != gen) return;
    if (e == hipErrorNotReady) {
        sl->watch = WATCH_GAVE_UP;              /* nobody spins on it again */
        return;
    }
    slot_complete(b, sl, e);
    try_open(b);
    pthread_cond_broadcast(&b->work_cv);
}

/* Block until ticket t is complete (mu held on entry and exit); its error.
 * An open slot holding t is hastened: launched at once while nothing is in
 * flight (no linger), else by the usual policy (md5_batch_wait's rule; a
 * synchronous submission's too, so that callers arriving while the device is
 * busy coalesce into one launch instead of one launch each). */
static int wait_ticket(md5hip_batcher *b, uint64_t t)
{
    int err = 0;
    while (!tk_ring_done(&b->tk, t, &err)) {
        struct slot *in = NULL, *open = NULL;
        for (uint32_t k = 0; k < b->nslots; k++) {
            struct slot *sl = &b->s[k];
            if (sl->state == SLOT_FREE || !seg_has(sl, t)) continue;
            if (sl->state == SLOT_OPEN) {
                if (b->inflight == 0) sl->flush = 1;
                slot_try_launch(b, sl);
            }
            if (sl->state == SLOT_INFLIGHT && !in) in = sl;
            else if (sl->state == SLOT_OPEN && !open) open = sl;
        }
        if (tk_ring_done(&b->tk, t, &err)) break;
        if (in && in->watch == WATCH_NONE) {
            watch_launch(b, in);
            continue;
        }
        struct slot *sl = in ? in : open;
        if (!sl) {                  /* not held by any slot yet (cannot happen for a
                                       returned ticket): re-check shortly */
            wait_cv_us(b, &b->done_cv, 1000);
            continue;
        }
        sl->nwait++;
        if (!b->poll_fast) pthread_cond_broadcast(&b->work_cv);   /* it may need to now */
        pthread_cond_wait(&sl->cv, &b->mu);
        sl->nwait--;
    }
    return err;
}

/* ------------------------------------------------------------------------
 * Create / destroy / settings
 * ------------------------------------------------------------------------ */
static void batcher_free(md5hip_batcher *b)
{
    for (uint32_t k = 0; b->s && k < b->nslots; k++) {
        struct slot *sl = &b->s[k];
        if (sl->state == SLOT_INFLIGHT) hipEventSynchronize(sl->done);
        if (sl->stream) hipStreamDestroy(sl->stream);
        if (sl->done) hipEventDestroy(sl->done);
        if (sl->kdone) hipEventDestroy(sl->kdone);
        hipHostFree(sl->h_data); hipHostFree(sl->h_off); hipHostFree(sl->h_len);
        hipHostFree(sl->h_ord); hipHostFree(sl->h_dig);
        hipFree(sl->d_data); hipFree(sl->d_off); hipFree(sl->d_len);
        hipFree(sl->d_ord); hipFree(sl->d_dig);
        hipHostFree(sl->h_seg); hipFree(sl->d_seg);
        hipHostFree(sl->h_dsc); hipFree(sl->d_dsc);
        free(sl->b_dst); free(sl->b_src); free(sl->b_len); free(sl->b_reg);
        free(sl->segs);
        free(sl->hh);
        hipHostFree(sl->h_bkt); hipFree(sl->d_bkt);
        if (sl->d_sort) hipFree(sl->d_sort);
        pthread_cond_destroy(&sl->cv);
    }
    free(b->s);
    if (b->vb_hin) hipHostFree(b->vb_hin);
    if (b->vb_hout) hipHostFree(b->vb_hout);
    if (b->vb_din) hipFree(b->vb_din);
    if (b->vb_dout) hipFree(b->vb_dout);
    if (b->pb_h) hipHostFree(b->pb_h);
    if (b->pb_d) hipFree(b->pb_d);
    if (b->after_ev) hipEventDestroy(b->after_ev);
    tk_ring_free(&b->tk);
    pthread_mutex_destroy(&b->mu);
    pthread_cond_destroy(&b->done_cv);
    pthread_cond_destroy(&b->work_cv);
    free(b);
}

void md5hip_batcher_destroy(md5hip_batcher *b)
{
    if (!b) return;
    struct dev_guard g;
    if (dev_enter(&g, b->device)) g.ok = 0;
    if (b->progress_started) {
        pthread_mutex_lock(&b->mu);
        /* launch what is still open so every ticket completes, then drain */
        flush_open(b);
        while (b->inflight) pthread_cond_wait(&b->done_cv, &b->mu);
        b->stop = 1;
        pthread_cond_broadcast(&b->work_cv);
        pthread_mutex_unlock(&b->mu);
        pthread_join(b->progress, NULL);
    }
    batcher_free(b);
    dev_leave(&g);
}

static int batcher_new(int device, uint64_t slice_bytes, uint32_t nslots, uint64_t maxn,
                       md5hip_batcher **out)
{
    int rc = 0;
    if (!out) return -EINVAL;
    *out = NULL;
    if (nslots == 0) nslots = 4;
    if (nslots > 16) return -EINVAL;
    slice_bytes = (slice_bytes + 4095) & ~4095ull;
    if (slice_bytes == 0) slice_bytes = 4096;
    struct dev_guard g;
    if (dev_enter(&g, device)) return -ENODEV;
    md5hip_batcher *b = calloc(1, sizeof *b);
    if (!b) { dev_leave(&g); return -ENOMEM; }
    pthread_mutex_init(&b->mu, NULL);
    pthread_cond_init(&b->done_cv, NULL);
    pthread_cond_init(&b->work_cv, NULL);
    b->device = device;
    b->kind = MD5HIP_DIGEST_MD5;
    b->nslots = nslots;
    b->cap = slice_bytes;
    b->maxn = maxn;
    b->segcap = slice_bytes / 1024 < 4096 ? 4096 : slice_bytes / 1024;
    b->pgcap = MD5HIP_PAGES_PER_SLOT(maxn);
    b->gather = MD5HIP_GATHER_AUTO;
    b->target = nslots > 2 ? 2 : 1;
    b->linger_max_us = 5000;
    b->chain = 2;
    b->open = -1;
    b->s = calloc(nslots, sizeof *b->s);
    /* ticket 0 = "nothing": complete at once */
    if (!b->s || tk_ring_init(&b->tk, 1)) { rc = -ENOMEM; goto fail; }
    for (uint32_t k = 0; k < nslots; k++) pthread_cond_init(&b->s[k].cv, NULL);
    CK(hipEventCreateWithFlags(&b->after_ev, hipEventDisableTiming));
    for (uint32_t k = 0; k < nslots; k++) {
        struct slot *sl = &b->s[k];
        CK(hipStreamCreateWithFlags(&sl->stream, hipStreamNonBlocking));
        CK(hipEventCreateWithFlags(&sl->done, hipEventDisableTiming));
        CK(hipEventCreateWithFlags(&sl->kdone, hipEventDisableTiming));
        CK(hipHostMalloc((void **)&sl->h_data, b->cap, hipHostMallocDefault));
        /* fine-grained: a small slot's kernel reads them in place (slot_prepare) */
        CK(hipHostMalloc((void **)&sl->h_off, 8 * b->maxn, hipHostMallocCoherent));
        CK(hipHostMalloc((void **)&sl->h_len, 4 * b->maxn, hipHostMallocCoherent));
        CK(hipHostGetDevicePointer((void **)&sl->dh_off, sl->h_off, 0));
        CK(hipHostGetDevicePointer((void **)&sl->dh_len, sl->h_len, 0));
        CK(hipHostMalloc((void **)&sl->h_ord, 4 * b->maxn, hipHostMallocDefault));
        CK(hipHostMalloc((void **)&sl->h_dig, 32 * b->maxn, hipHostMallocDefault));
        CK(hipMalloc((void **)&sl->d_data, b->cap));
        CK(hipMalloc((void **)&sl->d_off, 8 * b->maxn));
        CK(hipMalloc((void **)&sl->d_len, 4 * b->maxn));
        CK(hipMalloc((void **)&sl->d_ord, 4 * b->maxn));
        CK(hipMalloc((void **)&sl->d_dig, 32 * b->maxn));
        CK(hipHostMalloc((void **)&sl->h_seg, sizeof(struct md5hip_seg) * b->segcap, hipHostMallocDefault));
        CK(hipMalloc((void **)&sl->d_seg, sizeof(struct md5hip_seg) * b->segcap));
        CK(hipHostMalloc((void **)&sl->h_dsc, sizeof(struct md5hip_seg) * b->segcap, hipHostMallocDefault));
        CK(hipMalloc((void **)&sl->d_dsc, sizeof(struct md5hip_seg) * b->segcap));
        sl->b_dst = malloc(sizeof(void *) * b->segcap);
        sl->b_src = malloc(sizeof(void *) * b->segcap);
        sl->b_len = malloc(sizeof(size_t) * b->segcap);
        sl->b_reg = malloc(sizeof(long) * b->segcap);
        sl->hh = calloc((size_t)MD5HIP_HIST_KMAX + 2, sizeof(uint32_t));
        CK(hipHostMalloc((void **)&sl->h_bkt, sizeof(uint32_t) * ((size_t)MD5HIP_HIST_KMAX + 2),
                         hipHostMallocDefault));
        CK(hipMalloc((void **)&sl->d_bkt, sizeof(uint32_t) * ((size_t)MD5HIP_HIST_KMAX + 2)));
        /* the stable order's scratch for slots past DESC_DIRECT_MAX chunks
         * (none: those slots keep order_scatter) */
        sl->sort_bytes = b->maxn > DESC_DIRECT_MAX ? md5hip_order_stable_scratch(b->maxn, 0) : 0;
        if (sl->sort_bytes && hipMalloc(&sl->d_sort, sl->sort_bytes) != hipSuccess) {
            (void)hipGetLastError();
            sl->d_sort = NULL;
        }
        if (!sl->b_dst || !sl->b_src || !sl->b_len || !sl->b_reg || !sl->hh) { rc = -ENOMEM; goto fail; }
    }
    if (pthread_create(&b->progress, NULL, progress_main, b) != 0) { rc = -EAGAIN; goto fail; }
    b->progress_started = 1;
    *out = b;
    dev_leave(&g);
    return 0;
fail:
    (void)hipGetLastError();          /* a failed allocation is returned as rc, not left sticky */
    batcher_free(b);
    dev_leave(&g);
    return rc;
}

int md5hip_batcher_create(int device, uint64_t slice_bytes, uint32_t nslots, md5hip_batcher **out)
{
    /* defaults sized for MD5's serial chains: a slice of B-byte chunks keeps
     * slice/B lanes busy for B/110 MB/s (one chain), so the bytes in flight
     * must cover PCIe rate x chain time -- 4 x 128 MiB reaches the H2D rate
     * for 256 KiB blocks where 3 x 64 MiB stalls at ~34 GB/s */
    if (slice_bytes == 0) slice_bytes = 128ull << 20;
    uint64_t maxn = slice_bytes / 64 < 4096 ? 4096 : slice_bytes / 64;
    if (maxn > (1u << 20)) maxn = 1u << 20;      /* descriptors: 32 B per chunk */
    return batcher_new(device, slice_bytes, nslots, maxn, out);
}

int md5hip_queue_create(int device, uint64_t max_chunks, uint32_t nslots, md5hip_batcher **out)
{
    if (max_chunks == 0) max_chunks = 1u << 20;
    if (max_chunks > (1ull << 26)) return -EINVAL;
    /* a small staging slice keeps host-memory submissions possible */
    return batcher_new(device, 16ull << 20, nslots, max_chunks, out);
}

/* An entry that may launch the open slot from the caller's thread
 * (slot_enqueue's device-keyed state: the BALANCED counter, CU counts) runs
 * on the batcher's device, like submit -- a pool waits on a ticket of one
 * device from a thread whose current device is another.  In: that device,
 * then b->mu; out: both back. */
static int batcher_enter(md5hip_batcher *b, struct dev_guard *g)
{
    if (dev_enter(g, b->device)) return -ENODEV;
    pthread_mutex_lock(&b->mu);
    return 0;
}

static void batcher_leave(md5hip_batcher *b, const struct dev_guard *g)
{
    pthread_mutex_unlock(&b->mu);
    dev_leave(g);
}

/* Wait until nothing is open or in flight (mu held). */
static void drain(md5hip_batcher *b)
{
    for (;;) {
        flush_open(b);
        int busy = 0;
        for (uint32_t k = 0; k < b->nslots; k++) busy |= b->s[k].state != SLOT_FREE;
        if (!busy) return;
        pthread_cond_wait(&b->done_cv, &b->mu);
    }
}

int md5hip_batcher_set_digest(md5hip_batcher *b, int kind, uint32_t fastcrc)
{
    if (!b) return -EINVAL;
    const int u = md5hip_digest_usable(kind, fastcrc);
    if (u) return u;
    struct dev_guard g;
    if (batcher_enter(b, &g)) return -ENODEV;    /* drain may launch the open slot */
    drain(b);                                    /* never change kind under queued work */
    b->kind = kind;
    b->fastcrc = fastcrc;
    batcher_leave(b, &g);
    return 0;
}

int md5hip_batcher_get_digest(const md5hip_batcher *b, int *kind, uint32_t *fastcrc)
{
    if (!b || !kind || !fastcrc) return -EINVAL;
    pthread_mutex_lock((pthread_mutex_t *)&b->mu);
    *kind = b->kind;
    *fastcrc = b->fastcrc;
    pthread_mutex_unlock((pthread_mutex_t *)&b->mu);
    return 0;
}

int md5hip_batcher_set_gather(md5hip_batcher *b, int mode)
{
    if (!b || mode < MD5HIP_GATHER_HOST || mode > MD5HIP_GATHER_AUTO) return -EINVAL;
    pthread_mutex_lock(&b->mu);
    __atomic_store_n(&b->gather, mode, __ATOMIC_RELAXED);
    pthread_mutex_unlock(&b->mu);
    return 0;
}

int md5hip_batcher_set_inflight(md5hip_batcher *b, uint32_t target)
{
    if (!b || target == 0 || target > b->nslots) return -EINVAL;
    struct dev_guard g;
    if (batcher_enter(b, &g)) return -ENODEV;
    b->target = target;
    try_open(b);
    batcher_leave(b, &g);
    return 0;
}

int md5hip_batcher_set_linger(md5hip_batcher *b, uint32_t max_us)
{
    if (!b) return -EINVAL;
    pthread_mutex_lock(&b->mu);
    b->linger_max_us = max_us;
    pthread_cond_broadcast(&b->work_cv);
    pthread_mutex_unlock(&b->mu);
    return 0;
}

int md5hip_batcher_set_chain(md5hip_batcher *b, int mode)
{
    if (!b || mode < 0 || mode > 2) return -EINVAL;
    pthread_mutex_lock(&b->mu);
    b->chain = mode;
    pthread_mutex_unlock(&b->mu);
    return 0;
}

int md5hip_batcher_health(const md5hip_batcher *b)
{
    if (!b) return -EINVAL;
    return __atomic_load_n(&b->failed, __ATOMIC_ACQUIRE);
}

int md5hip_batcher_inject_fault(md5hip_batcher *b, uint64_t after)
{
    if (!b) return -EINVAL;
    pthread_mutex_lock(&b->mu);
    int rc = b->failed;
    if (!rc) b->inject_at = after ? b->st.launches + after : 0;
    pthread_mutex_unlock(&b->mu);
    return rc;
}

int md5hip_batcher_get_stats(md5hip_batcher *b, struct md5hip_batcher_stats *out)
{
    if (!b || !out) return -EINVAL;
    pthread_mutex_lock(&b->mu);
    *out = b->st;
    out->inflight_target = b->target;
    out->nslots = b->nslots;
    out->max_chunks_per_slot = b->maxn;
    pthread_mutex_unlock(&b->mu);
    return 0;
}

/* ------------------------------------------------------------------------
 * Submission (the host chunk sources themselves: md5_source.h)
 * ------------------------------------------------------------------------ */
/* Every non-empty segment of the call in registered memory? */
static int src_registered(const struct md5hip_src *s, uint64_t n)
{
    int ok = 1;
    pthread_rwlock_rdlock(&g_reg_lock);
    for (uint64_t i = 0; i < n && ok; i++)
        for (uint64_t k = 0; k < src_nseg(s, i) && ok; k++) {
            const void *p;
            uint32_t L;
            src_seg(s, i, k, &p, &L);
            if (L && reg_find((uintptr_t)p, L) < 0) ok = 0;
        }
    pthread_rwlock_unlock(&g_reg_lock);
    return ok;
}

/* Chunk key k = (len >> 6) + 1 into the key histogram hh and its running
 * values (md5hip.h md5hip_plan_hist): the largest key, whether a key past
 * MD5HIP_HIST_KMAX was seen (host sort instead), and whether the keys so far
 * were non-increasing (then no order is built).  reserve_device passes
 * locals, so its loop keeps them in registers. */
static inline void hist_add(uint32_t *hh, uint32_t key, uint32_t *last, uint32_t *kmax, int *unsorted, int *hovf)
{
    *unsorted |= key > *last;
    *last = key;
    if (key > MD5HIP_HIST_KMAX) {
        *hovf = 1;
    } else {
        hh[key]++;
        if (key > *kmax) *kmax = key;
    }
}

/* Device-resident chunks [i, i + m) into slot `sl` (mu held, m fits): the
 * descriptors, payload and key histogram in one pass with the running
 * values in registers -- no bytes to stage.  While a burst of C3 vectors is
 * submitted to an idle queue this pass is the device's idle time (bench.py
 * --config c3q `drained`): ~97 us of a 79 K-chunk vector's submission on
 * the box's host, the rest of the call ~3 us of HIP calls (rocprofv3
 * --hip-trace, profiles/r04k/).  Neither threads (slower at every count,
 * profiles/r04f/) nor non-temporal stores (2.4x in isolation,
 * profiles/r04i/, no change in the submission, profiles/r04j/) shortened
 * it, so it stays one plain pass on the calling thread.  A function of its
 * own on a 64-byte boundary: inlined into submit() the loop moved with every
 * edit before it, and sitting across three 64-byte lines instead of two it
 * cost the call 6 % (profiles/batcher_split/ab.json). */
__attribute__((noinline, aligned(64)))
static void reserve_device(md5hip_batcher *b, struct slot *sl, const struct md5hip_src *src, uint64_t i,
                           uint64_t m)
{
    uint64_t *ho = sl->h_off + sl->n;
    uint32_t *hl = sl->h_len + sl->n;
    uint32_t *hh = sl->hh;
    const uint64_t *dp = src->dptrs + src->first + i;
    const uint32_t *ln = src->lens + src->first + i;
    const uint64_t dbase = (uint64_t)(uintptr_t)sl->d_data;
    uint64_t pay = 0, unl = 0;
    uint32_t last = sl->last_key, kmax = sl->hkmax;
    int unsorted = sl->unsorted, hovf = sl->hovf;
    for (uint64_t k = 0; k < m; k++) {
        const uint64_t p = dp[k];
        const uint32_t L = ln[k];
        ho[k] = p - dbase;
        hl[k] = L;
        pay += L;
        unl += ((p & 127u) != 0 && (p & 15u) == 0) ? L : 0;
        hist_add(hh, (L >> 6) + 1, &last, &kmax, &unsorted, &hovf);   /* L < 2^32: no overflow */
    }
    sl->last_key = last;
    sl->hkmax = kmax;
    sl->unsorted = unsorted;
    sl->hovf = hovf;
    sl->payload += pay;
    sl->unlined += unl;
    load_add(b, sl, pay + 64 * m);
    sl->n += m;
}

/* One piece of a zero-copy chunk -- `len` registered bytes at host address
 * p (registration r) -- to staging offset `at` of the slot's gather tables. */
static void zc_piece(struct slot *sl, int dev, const void *p, uint32_t len, long r, uint64_t at)
{
    const uint64_t dsrc = (uint64_t)((uintptr_t)p + g_reg[r].delta[dev]);
    /* device table: contiguous pieces merged up to 64 KiB, so a slice keeps
     * >= ~1000 workgroups of gather work */
    struct md5hip_seg *prev = sl->nseg ? &sl->h_seg[sl->nseg - 1] : NULL;
    if (prev && prev->src + prev->len == dsrc && prev->dst + prev->len == at &&
        (uint64_t)prev->len + len <= (64u << 10)) {
        prev->len += len;
    } else {
        sl->h_seg[sl->nseg++] = (struct md5hip_seg){dsrc, at, len, 0};
    }
    /* DMA list: merged without limit (a copy has a fixed cost), but only
     * within one registered range (one pinned allocation) */
    const uint64_t q1 = sl->ndma;
    if (q1 && sl->b_reg[q1 - 1] == r &&
        (const unsigned char *)sl->b_src[q1 - 1] + sl->b_len[q1 - 1] == (const unsigned char *)p &&
        (unsigned char *)sl->b_dst[q1 - 1] + sl->b_len[q1 - 1] == sl->d_data + at) {
        sl->b_len[q1 - 1] += len;
    } else {
        sl->b_dst[q1] = sl->d_data + at;
        sl->b_src[q1] = (void *)p;
        sl->b_len[q1] = len;
        sl->b_reg[q1] = r;
        sl->ndma++;
    }
}

/* Chunk j of `src` -- L bytes, E of them staged: all of it, or its two
 * F-byte windows -- into the slot's zero-copy tables at staging offset
 * sl->used (mu and g_reg_lock held).  0; 1 when the tables have no room for
 * it; -EFAULT when a piece is registered no longer. */
static int reserve_zc(md5hip_batcher *b, struct slot *sl, const struct md5hip_src *src, uint64_t j,
                      uint64_t L, uint64_t E, uint32_t F)
{
    const int win = E != L;
    const uint64_t need = zc_pieces(src_nseg(src, j), win);
    if (sl->nseg + need > b->segcap || sl->ndma + need > b->segcap) return 1;
    const uint64_t ra[2] = {0, win ? L - F : 0}, rl[2] = {win ? F : L, win ? F : 0};
    uint64_t at = sl->used;
    for (int w = 0; w < 2; w++) {
        struct src_walk walk = src_walk_range(src, j, ra[w], rl[w]);
        const void *p;
        uint32_t take;
        while (src_walk_next(&walk, &p, &take)) {
            const long r = reg_find((uintptr_t)p, take);
            if (r < 0) return -EFAULT;
            zc_piece(sl, b->device, p, take, r, at);
            at += take;
        }
    }
    return 0;
}

/* Reserve chunks [i, n) of `src` into the open slot (mu held): descriptors,
 * staging offsets, zero-copy tables.  Returns the number reserved (the slot
 * is marked full when a chunk did not fit) or -errno.  A CRC-32 slot with a
 * fastcrc window stages each longer chunk's two windows only (staged_len). */
static long reserve(md5hip_batcher *b, struct slot *sl, const struct md5hip_src *src, uint64_t i,
                    uint64_t n, int zc)
{
    const uint32_t F = sl->kind == MD5HIP_DIGEST_CRC32 ? sl->fastcrc : 0;
    uint64_t j = i;
    if (sl->n == 0 && i < n) sl->opened_us = now_us();
    if (src->kind == MD5HIP_SRC_DEVICE) {
        const uint64_t m = n - i < b->maxn - sl->n ? n - i : b->maxn - sl->n;
        reserve_device(b, sl, src, i, m);
        if (i + m < n) sl->full = 1;
        return (long)m;
    }
    if (zc) pthread_rwlock_rdlock(&g_reg_lock);
    while (j < n && sl->n < b->maxn) {
        const uint64_t L = md5hip_src_len(src, j);
        const uint64_t E = staged_len(F, L);
        /* chunks packed on 128-B lines: the LDS-DMA loaders read 128-B
         * stages, and a stage off the line shares a line with the next
         * one (the nt policy is then off, md5_kernels.h) */
        const uint64_t sz = (E + 127) & ~127ull;
        if (sl->used + sz > b->cap) break;
        const int e = zc ? reserve_zc(b, sl, src, j, L, E, F) : 0;
        if (e < 0) {                                /* unregistered under us */
            pthread_rwlock_unlock(&g_reg_lock);
            return e;
        }
        if (e) break;
        sl->h_off[sl->n] = sl->used;
        sl->used += sz;
        sl->h_len[sl->n] = (uint32_t)E;
        sl->payload += E;
        load_add(b, sl, E + 64);
        /* E < 2^32 (submit's size check): the key fits */
        hist_add(sl->hh, (uint32_t)(E >> 6) + 1, &sl->last_key, &sl->hkmax, &sl->unsorted, &sl->hovf);
        sl->n++;
        j++;
    }
    if (zc) pthread_rwlock_unlock(&g_reg_lock);
    if (j < n) sl->full = 1;
    return (long)(j - i);
}

/* What a submission asks for beside its chunks; an entry names what it sets,
 * the rest is 0 / NULL.
 *   digests, on_device   where the digests go: a host array, or device memory
 *   async   0 = synchronous (returns when the digests are delivered);
 *           1 = asynchronous (*ticket; the slot may linger and coalesce);
 *           2 = asynchronous but launched at once like a synchronous call
 *               (the caller waits on *ticket right away: the pool's
 *               synchronous entries)
 *   kind    KIND_BATCHER: the batcher's current digest kind; else this
 *           submission's own, with `fastcrc` (it never changes the
 *           batcher's setting)
 *   after   != NULL: *after is the producer's stream (NULL there = the null
 *           stream) -- every slot taking chunks of this submission waits on
 *           the producer's work enqueued so far before its kernel (an event
 *           recorded on *after, waited on by the slot's stream) */
enum { KIND_BATCHER = -1 };
struct sub_opt {
    unsigned char *digests;
    int on_device, async;
    uint64_t *ticket;
    int kind;
    uint32_t fastcrc;
    const hipStream_t *after;
    const struct md5hip_verify_opt *verify;   /* verify segments (digests NULL): enter_verify */
};

/* One submission between sub_begin and sub_end: the caller's device (entered
 * by the engine before sub_begin), its ticket and its digest kind. */
struct sub {
    struct dev_guard g;
    uint64_t t;
    int kind;
    uint32_t fastcrc, dsz;
};

/* Takes b->mu and opens the submission: the digest kind, a ticket,
 * `after` checked to be a stream of this device.  On an error nothing is
 * held any more: mu released, the caller's device put back. */
static int sub_begin(md5hip_batcher *b, struct sub *s, const struct sub_opt *o)
{
    pthread_mutex_lock(&b->mu);
    s->kind = o->kind < 0 ? b->kind : o->kind;
    s->fastcrc = o->kind < 0 ? b->fastcrc : o->fastcrc;
    s->dsz = md5hip_digest_size(s->kind);
    s->t = 0;
    int rc = b->failed ? b->failed : tk_ring_new(&b->tk, &s->t);
    if (rc == 0 && o->after && hipEventRecord(b->after_ev, *o->after) != hipSuccess) {
        tk_ring_put(&b->tk, s->t, 0);
        rc = -EINVAL;                              /* not a stream of this device */
    }
    if (rc) {
        batcher_leave(b, &s->g);
        return rc;
    }
    b->st.submissions++;
    return 0;
}

/* Closes the submission (mu held) with the engine's rc: drops its own
 * reference on the ticket, hands the ticket out, waits when the call is
 * synchronous or failed, releases mu and the device. */
static int sub_end(md5hip_batcher *b, struct sub *s, int rc, uint64_t *ticket, int wait)
{
    tk_ring_put(&b->tk, s->t, rc);
    if (ticket) *ticket = s->t;
    if (wait || rc) {
        const int err = wait_ticket(b, s->t);
        if (!rc) rc = err;
    }
    batcher_leave(b, &s->g);
    return rc;
}

/* A submitter's copy into slot `sl` runs outside b->mu, between these two:
 * the slot is held by a writer count (slot_try_launch waits for
 * writers == 0) while other submitters reserve behind it. */
static void write_begin(md5hip_batcher *b, struct slot *sl)
{
    sl->writers++;
    pthread_mutex_unlock(&b->mu);
}

static void write_end(md5hip_batcher *b, struct slot *sl)
{
    pthread_mutex_lock(&b->mu);
    sl->writers--;
}

/* The producer's work enqueued so far, before slot `sl`'s kernel (mu held).
 * Recorded and waited on under one hold of b->mu -- recorded again per slot:
 * slot_open / slot_take may have let another producer record the event
 * meanwhile -- and before the slot's kernel can be enqueued. */
static void slot_after(md5hip_batcher *b, struct slot *sl, const hipStream_t *after)
{
    if (after && (hipEventRecord(b->after_ev, *after) != hipSuccess ||
                  hipStreamWaitEvent(sl->stream, b->after_ev, 0) != hipSuccess) && !sl->err)
        sl->err = -EIO;
}

/* Makes `sg` -- chunks [i, i + sg->count) of a verify submission, going into
 * slot `sl` -- a verify segment (mu held).  A host caller's expected values
 * are copied into the slot's table buffer here, so the caller may reuse its
 * array on return (16 to 32 bytes a chunk: beside the chunk's own bytes,
 * nothing); they fit: verify_buffers sized it for maxn chunks in segcap
 * segments. */
static void seg_verify(struct slot *sl, struct seg *sg, const struct md5hip_verify_opt *v, uint64_t i)
{
    const unsigned char *want = (const unsigned char *)v->expected + (size_t)v->wsz * i;
    sg->ok = v->ok + i;
    sg->md5_out = v->md5_out ? v->md5_out + 16 * (size_t)i : NULL;
    sg->nbad = v->nbad;
    sg->goff = v->goff;
    sg->wsz = v->wsz;
    if (v->on_device) {
        sg->want = (uint64_t)(uintptr_t)want;
    } else {
        const uint64_t bytes = (uint64_t)v->wsz * sg->count;
        sg->want = sl->vwant;
        memcpy(sl->h_vin + sl->vwant, want, bytes);
        sl->vwant += (bytes + 15) & ~15ull;
    }
    sl->nverify++;
}

/* The submission engine: chunks [0, n) of a PTRS, IOV or DEVICE source into
 * the open slot, as many slots as they take. */
static int submit(md5hip_batcher *b, const struct md5hip_src *src, uint64_t n, const struct sub_opt *o)
{
    const int urgent = o->async != 1, dev_src = src->kind == MD5HIP_SRC_DEVICE;
    for (uint64_t i = 0; !dev_src && i < n; i++) {      /* device chunks: uint32 lengths, no staging */
        const uint64_t L = md5hip_src_len(src, i);
        if (L > 0xffffffffull) return -E2BIG;
        if ((L + 127) / 128 * 128 > b->cap) return -E2BIG;
    }
    struct sub s;
    if (dev_enter(&s.g, b->device)) return -ENODEV;
    int zc = 0;
    /* gather is read here without mu (set_gather may change it meanwhile):
     * it only decides whether this submission may go zero-copy */
    if (!dev_src && __atomic_load_n(&b->gather, __ATOMIC_RELAXED) != MD5HIP_GATHER_HOST &&
        b->device < REG_MAXDEV &&
        src_registered(src, n)) {
        zc = 1;
        for (uint64_t i = 0; i < n; i++)
            if (zc_pieces(src_nseg(src, i), 1) > b->segcap) zc = 0;   /* too fragmented for one table */
    }
    const int mode = dev_src ? MODE_NONE : zc ? MODE_ZEROCOPY : MODE_STAGED;
    int rc = sub_begin(b, &s, o);
    if (rc) return rc;
    uint64_t i = 0;
    while (i < n) {
        struct slot *sl = slot_for(b, mode, s.kind, s.fastcrc);
        if (!sl) { rc = -ENODEV; break; }
        const uint64_t at = sl->n;
        const uint64_t lo = sl->used;
        const long got = reserve(b, sl, src, i, n, zc);
        if (got < 0) { rc = (int)got; break; }
        if (got == 0) {                      /* nothing fit: close it and take a fresh one */
            close_open(b);
            continue;
        }
        const uint64_t m = (uint64_t)got;
        const uint64_t hi = sl->used;
        /* a large device-resident range: its descriptors go over now, on the
         * slot's idle stream, instead of after the burst's last submission
         * (a drained c3q step's 6 vectors: ~0.12 ms of copies that no longer
         * sit between the burst and its kernel); appended descriptors are
         * final, slot_prepare copies only what follows */
        if (dev_src && m >= EARLY_COPY_MIN && sl->n > DESC_DIRECT_MAX && sl->n > sl->copied_n &&
            desc_copy(sl) && !sl->err)
            sl->err = -EIO;
        slot_after(b, sl, o->after);
        struct seg sg = {s.t, at, m, o->verify ? NULL : o->digests + (size_t)s.dsz * i, o->on_device};
        if (o->verify) seg_verify(sl, &sg, o->verify, i);
        if ((rc = seg_push(b, sl, sg))) {
            sl->err = rc;                    /* its reserved chunks have no segment */
            break;
        }
        if (mode == MODE_STAGED && hi > lo) {
            write_begin(b, sl);
            gather_range(src, i, m, sl->h_off + at, sl->h_data, lo, hi,
                         sl->kind == MD5HIP_DIGEST_CRC32 ? sl->fastcrc : 0);
            write_end(b, sl);
        }
        i += m;
        /* the caller waits right away: no linger; the slot goes while fewer
         * than nslots - 1 launches run, else it coalesces in the last slot
         * (slot_try_launch) -- forcing every synchronous call out at once
         * made one launch per vector at ASIO scale (profiles/r04b/), and
         * holding them to `target` launches cost the 8-thread call site a
         * fifth of its throughput (profiles/r04d/asio_threads.json) */
        if (urgent && i >= n) sl->urgent = 1;
        slot_try_launch(b, sl);
    }
    return sub_end(b, &s, rc, o->ticket, !o->async);
}

/* A waiter or poller on `ticket` (mu held): if its chunks sit in the open
 * slot and nothing is in flight, launch that slot now (no linger).  While
 * launches are in flight the slot keeps coalescing and goes out as soon as
 * one retires (the inflight target holds; its plan is made meanwhile) --
 * forcing it out beside a running launch only splits the device between
 * them. */
static void hasten(md5hip_batcher *b, uint64_t ticket)
{
    for (uint32_t k = 0; k < b->nslots; k++)
        if (b->s[k].state == SLOT_OPEN && seg_has(&b->s[k], ticket)) {
            if (b->inflight == 0) b->s[k].flush = 1;
            slot_try_launch(b, &b->s[k]);
        }
}

/* Wait, poll and flush may launch the open slot from the caller's thread:
 * batcher_enter. */
int md5_batch_wait(md5hip_batcher *b, uint64_t ticket)
{
    if (!b) return -EINVAL;
    if (ticket == 0) return 0;               /* "nothing submitted" */
    struct dev_guard g;
    if (batcher_enter(b, &g)) return -ENODEV;
    const int rc = ticket >= b->tk.hi ? -EINVAL : wait_ticket(b, ticket);
    batcher_leave(b, &g);
    return rc;
}

int md5_batch_poll(md5hip_batcher *b, uint64_t ticket)
{
    if (!b) return -EINVAL;
    if (ticket == 0) return 1;
    struct dev_guard g;
    if (batcher_enter(b, &g)) return -ENODEV;
    int rc, err = 0;
    if (ticket >= b->tk.hi) {
        rc = -EINVAL;
    } else if (tk_ring_done(&b->tk, ticket, &err)) {
        rc = err ? err : 1;
    } else {
        hasten(b, ticket);                   /* progress without the caller blocking */
        rc = 0;
    }
    batcher_leave(b, &g);
    return rc;
}

int md5_batch_flush(md5hip_batcher *b)
{
    if (!b) return -EINVAL;
    struct dev_guard g;
    if (batcher_enter(b, &g)) return -ENODEV;
    flush_open(b);
    batcher_leave(b, &g);
    return 0;
}

/* Is the byte at p page-locked host memory known to the runtime? */
static int pinned_at(const void *p)
{
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();                  /* pageable: not an error of ours */
        return 0;
    }
    return a.type == hipMemoryTypeHost;
}

/* Is [p, p + len) page-locked host memory the DMA engine can read in place
 * (hipHostMalloc'd, hipHostRegister'ed, or registered here)?  The whole
 * range, not its first byte: a source that starts in a pinned block and runs
 * on into pageable memory is staged.  Both ends must be pinned, and the
 * runtime's allocation holding the first byte must hold the last too (HIP's
 * RANGE_START/RANGE_SIZE attribute, else hipMemGetAddressRange); a range
 * whose extent the runtime will not tell is staged. */
static int host_pinned(const void *p, uint64_t len)
{
    if (!len) return 0;
    pthread_rwlock_rdlock(&g_reg_lock);
    const int reg = reg_find((uintptr_t)p, len) >= 0;
    pthread_rwlock_unlock(&g_reg_lock);
    if (reg) return 1;
    const uintptr_t lo = (uintptr_t)p, hi = lo + len;      /* [lo, hi) */
    if (!pinned_at(p) || !pinned_at((const void *)(hi - 1))) return 0;
    void *start = NULL;
    size_t size = 0;
    if (hipPointerGetAttribute(&start, HIP_POINTER_ATTRIBUTE_RANGE_START_ADDR, (hipDeviceptr_t)p) == hipSuccess &&
        hipPointerGetAttribute(&size, HIP_POINTER_ATTRIBUTE_RANGE_SIZE, (hipDeviceptr_t)p) == hipSuccess &&
        start && size)
        return (uintptr_t)start <= lo && hi <= (uintptr_t)start + size;
    (void)hipGetLastError();
    if (hipMemGetAddressRange((hipDeviceptr_t *)&start, &size, (hipDeviceptr_t)p) == hipSuccess && start && size)
        return (uintptr_t)start <= lo && hi <= (uintptr_t)start + size;
    (void)hipGetLastError();
    return 0;
}

/* Fixed-length chunks from one contiguous range (MODE_FIXED, a FIXED
 * source), one slot per slice of it: host memory (one H2D copy per slot, no
 * host gather) or device memory (base_on_device: read in place, no per-chunk
 * descriptor -- md5_batch_submit_device_fixed).  Synchronous when the options
 * name no ticket. */
static int fixed_submit(md5hip_batcher *b, const struct md5hip_src *fx, uint64_t n, const struct sub_opt *o)
{
    const int dev_src = fx->base_on_device;
    const uint32_t len = fx->len;
    const uint64_t stride = fx->stride;
    if (!dev_src && stride > b->cap) return -E2BIG;
    struct sub s;
    if (dev_enter(&s.g, b->device)) return -ENODEV;
    const unsigned char *src = fx->base + fx->first * stride;
    uint64_t per = dev_src || !stride ? b->maxn : b->cap / stride;   /* stride 0: empty chunks */
    if (per > b->maxn) per = b->maxn;
    /* a pageable source is copied into the slot's pinned staging by this
     * thread: HIP's own pageable H2D path stalls other threads' HIP calls on
     * the device while it runs (submitters' p90 +2.7 ms beside 128 MiB
     * slices, profiles/r05f/) */
    const int pinned = !dev_src && n && host_pinned(src, (n - 1) * stride + len);
    int rc = sub_begin(b, &s, o);
    if (rc) return rc;
    for (uint64_t i = 0; i < n && !rc; i += per) {
        const uint64_t m = n - i < per ? n - i : per;
        struct slot *sl = slot_for(b, MODE_FIXED, s.kind, s.fastcrc);
        if (!sl) { rc = -ENODEV; break; }
        sl->n = m;
        sl->fx_src = src + i * stride;
        sl->fx_dev = dev_src;
        sl->fx_bytes = (m - 1) * stride + len;
        sl->fx_len = len;
        sl->fx_stride = stride;
        sl->full = 1;
        load_add(b, sl, m * ((uint64_t)len + 64));      /* the slot is fresh: load == 0 */
        if ((rc = seg_push(b, sl, (struct seg){s.t, 0, m, o->digests + (size_t)s.dsz * i, o->on_device}))) {
            slot_retire(b, sl, rc);
            break;
        }
        slot_after(b, sl, o->after);         /* the slot is fresh: err == 0 */
        if (!dev_src) {
            /* the copy outside the lock, the slot held by this writer: a
             * pageable source through the pinned staging (host_pinned), a
             * pinned one by DMA in place; every other submitter and waiter
             * needs b->mu meanwhile.  Nothing else touches a FIXED slot's
             * stream or staging until its writers are done (slot_try_launch
             * waits for writers == 0). */
            write_begin(b, sl);
            const void *from = sl->fx_src;
            if (!pinned) {
                copy_parallel(sl->h_data, sl->fx_src, sl->fx_bytes);
                from = sl->h_data;
            }
            const hipError_t ce = hipMemcpyAsync(sl->d_data, from, sl->fx_bytes, hipMemcpyHostToDevice, sl->stream);
            write_end(b, sl);
            if (!pinned) b->st.bytes_staged += sl->fx_bytes;
            if (ce != hipSuccess && !sl->err) sl->err = -EIO;
            if (ce != hipSuccess && hip_lost(hipStreamQuery(sl->stream))) batcher_fail(b);
        }
        slot_try_launch(b, sl);
    }
    return sub_end(b, &s, rc, o->ticket, !o->ticket);
}

/* ------------------------------------------------------------------------
 * Entries
 * ------------------------------------------------------------------------ */
/* What every submit entry does once it has named its source and options:
 * the argument checks, then the engine the source goes to.  A non-zero
 * `async` takes a ticket, which is zeroed first (an empty batch is complete
 * at once, and no error leaves a stale ticket). */
static int enter(md5hip_batcher *b, const struct md5hip_src *src, uint64_t n, const struct sub_opt *o)
{
    if (o->ticket) *o->ticket = 0;
    if (!b || (o->async && !o->ticket)) return -EINVAL;
    if (n == 0) return 0;
    if (!o->digests) return -EINVAL;
    const int rc = md5hip_src_check(src, n);
    if (rc) return rc;
    return src->kind == MD5HIP_SRC_FIXED ? fixed_submit(b, src, n, o) : submit(b, src, n, o);
}

static struct md5hip_src src_ptrs(const void *const *ptrs, const uint32_t *lens)
{
    return (struct md5hip_src){.kind = MD5HIP_SRC_PTRS, .ptrs = ptrs, .lens = lens};
}

static struct md5hip_src src_iov(const struct md5hip_iov *segs, const uint64_t *seg_first)
{
    return (struct md5hip_src){.kind = MD5HIP_SRC_IOV, .segs = segs, .seg_first = seg_first};
}

static struct md5hip_src src_device(const uint64_t *d_ptrs, const uint32_t *lens)
{
    return (struct md5hip_src){.kind = MD5HIP_SRC_DEVICE, .dptrs = d_ptrs, .lens = lens};
}

int md5_batch_submit(md5hip_batcher *b, const void *const *ptrs, const uint32_t *lens, uint64_t n,
                     unsigned char *digests)
{
    const struct md5hip_src src = src_ptrs(ptrs, lens);
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .kind = KIND_BATCHER});
}

int md5_batch_submit_async(md5hip_batcher *b, const void *const *ptrs, const uint32_t *lens,
                           uint64_t n, unsigned char *digests, uint64_t *ticket)
{
    const struct md5hip_src src = src_ptrs(ptrs, lens);
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .async = 1, .ticket = ticket, .kind = KIND_BATCHER});
}

int md5_batch_submit_iov(md5hip_batcher *b, const struct md5hip_iov *segs,
                         const uint64_t *seg_first, uint64_t n, unsigned char *digests)
{
    const struct md5hip_src src = src_iov(segs, seg_first);
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .kind = KIND_BATCHER});
}

int md5_batch_submit_iov_async(md5hip_batcher *b, const struct md5hip_iov *segs,
                               const uint64_t *seg_first, uint64_t n, unsigned char *digests,
                               uint64_t *ticket)
{
    const struct md5hip_src src = src_iov(segs, seg_first);
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .async = 1, .ticket = ticket, .kind = KIND_BATCHER});
}

int md5_batch_submit_device_async(md5hip_batcher *b, const uint64_t *d_ptrs, const uint32_t *lens,
                                  uint64_t n, unsigned char *digests, int digests_on_device,
                                  uint64_t *ticket)
{
    const struct md5hip_src src = src_device(d_ptrs, lens);
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .on_device = digests_on_device != 0,
                                               .async = 1, .ticket = ticket, .kind = KIND_BATCHER});
}

int md5_batch_submit_device(md5hip_batcher *b, const uint64_t *d_ptrs, const uint32_t *lens,
                            uint64_t n, unsigned char *digests, int digests_on_device)
{
    const struct md5hip_src src = src_device(d_ptrs, lens);
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .on_device = digests_on_device != 0,
                                               .kind = KIND_BATCHER});
}

int md5_batch_submit_device_after(md5hip_batcher *b, const uint64_t *d_ptrs, const uint32_t *lens,
                                  uint64_t n, unsigned char *digests, int digests_on_device,
                                  void *producer_stream, int order, uint64_t *ticket)
{
    const struct md5hip_src src = src_device(d_ptrs, lens);
    const hipStream_t after = (hipStream_t)producer_stream;
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .on_device = digests_on_device != 0,
                                               .async = ticket != NULL, .ticket = ticket, .kind = KIND_BATCHER,
                                               .after = order ? &after : NULL});
}

int md5_batch_submit_device_on(md5hip_batcher *b, const uint64_t *d_ptrs, const uint32_t *lens,
                               uint64_t n, unsigned char *digests, int digests_on_device,
                               void *producer_stream, uint64_t *ticket)
{
    return md5_batch_submit_device_after(b, d_ptrs, lens, n, digests, digests_on_device,
                                         producer_stream, producer_stream != NULL, ticket);
}

int md5_batch_submit_device_fixed(md5hip_batcher *b, const void *d_base, uint64_t n, uint32_t len,
                                  uint64_t stride, unsigned char *digests, int digests_on_device,
                                  void *producer_stream, int order, uint64_t *ticket)
{
    const struct md5hip_src src = {.kind = MD5HIP_SRC_FIXED, .base = d_base, .len = len, .stride = stride,
                                   .base_on_device = 1};
    const hipStream_t after = (hipStream_t)producer_stream;
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .on_device = digests_on_device != 0,
                                               .async = ticket != NULL, .ticket = ticket, .kind = KIND_BATCHER,
                                               .after = order ? &after : NULL});
}

int md5hip_batch_host_fixed(md5hip_batcher *b, const void *h_base, uint64_t n, uint32_t len,
                            uint64_t stride, unsigned char *digests)
{
    const struct md5hip_src src = {.kind = MD5HIP_SRC_FIXED, .base = h_base, .len = len, .stride = stride};
    return enter(b, &src, n, &(struct sub_opt){.digests = digests, .kind = KIND_BATCHER});
}

/* ------------------------------------------------------------------------
 * Device-resident page lists (md5hip.h: md5_batch_submit_device_pages)
 * ------------------------------------------------------------------------ */
/* The page tables of every slot, allocated once by the first paged
 * submission (a batcher that never gets one allocates nothing for it): pgcap
 * entries per slot, pinned host and device.  0, -ENODEV, or -ENOMEM with
 * nothing allocated. */
static int pages_buffers(md5hip_batcher *b)
{
    if (__atomic_load_n(&b->pready, __ATOMIC_ACQUIRE)) return 0;
    struct dev_guard g;
    if (batcher_enter(b, &g)) return -ENODEV;
    int rc = 0;
    if (!b->pready) {
        const uint64_t bytes = 8 * b->pgcap * b->nslots;
        void *h = NULL, *d = NULL;
        if (hipHostMalloc(&h, bytes, hipHostMallocDefault) != hipSuccess || hipMalloc(&d, bytes) != hipSuccess) {
            (void)hipGetLastError();
            if (h) hipHostFree(h);
            rc = -ENOMEM;
        } else {
            b->pb_h = h;
            b->pb_d = d;
            for (uint32_t k = 0; k < b->nslots; k++) {
                b->s[k].h_pg = b->pb_h + b->pgcap * k;
                b->s[k].d_pg = b->pb_d + b->pgcap * k;
            }
            __atomic_store_n(&b->pready, 1, __ATOMIC_RELEASE);
        }
    }
    batcher_leave(b, &g);
    return rc;
}

/* Chunks [i, i + m) of a paged source into the pinned arrays of slot `sl`,
 * the submitter's own (outside b->mu): of each chunk the table entries its
 * length reads, packed, its first entry among them and its length; then the
 * longest-first order, unless the keys are non-increasing as they came (the
 * identity then is that order).  0, or the planner's -errno. */
static int pages_fill(struct slot *sl, const struct md5hip_src *pg, uint64_t i, uint64_t m)
{
    const uint32_t *lens = pg->lens + pg->first + i;
    const uint64_t *pfirst = pg->page_first + pg->first + i;
    uint64_t at = 0;
    int sorted = 1;
    for (uint64_t k = 0; k < m; k++) {
        const uint64_t need = md5hip_pages_of(lens[k], pg->page_bytes);
        if (need) memcpy(sl->h_pg + at, pg->pages + pfirst[k], 8 * need);
        sl->h_off[k] = at;
        sl->h_len[k] = lens[k];
        at += need;
        if (k && (lens[k] >> 6) > (lens[k - 1] >> 6)) sorted = 0;
    }
    sl->use_order = !sorted;
    const int rc = sorted ? 0 : md5hip_plan_desc(sl->h_len, m, sl->h_ord);
    return rc < 0 ? rc : 0;
}

/* A paged source, one slot of its own per slice (MODE_PAGES), each slice one
 * launch: a slice ends at maxn chunks or at pgcap table entries, whichever
 * comes first (every chunk fits an empty table: the entry checked).
 * Synchronous when the options name no ticket.  With o->verify every slice
 * is one verify segment (the entry made sure of verify_buffers). */
static int pages_submit(md5hip_batcher *b, const struct md5hip_src *pg, uint64_t n, const struct sub_opt *o)
{
    struct sub s;
    if (dev_enter(&s.g, b->device)) return -ENODEV;
    int rc = sub_begin(b, &s, o);
    if (rc) return rc;
    for (uint64_t i = 0; i < n && !rc;) {
        uint64_t m = 0, ents = 0, weight = 0;
        while (i + m < n && m < b->maxn) {
            const uint32_t len = pg->lens[pg->first + i + m];
            const uint64_t need = md5hip_pages_of(len, pg->page_bytes);
            if (ents + need > b->pgcap) break;
            ents += need;
            weight += (uint64_t)len + 64;
            m++;
        }
        struct slot *sl = slot_for(b, MODE_PAGES, s.kind, s.fastcrc);
        if (!sl) { rc = -ENODEV; break; }
        sl->n = m;
        sl->pg_n = ents;
        sl->pg_bytes = pg->page_bytes;
        sl->full = 1;
        load_add(b, sl, weight);                        /* the slot is fresh: load == 0 */
        struct seg sg = {s.t, 0, m, o->verify ? NULL : o->digests + (size_t)s.dsz * i, o->on_device};
        if (o->verify) seg_verify(sl, &sg, o->verify, i);
        if ((rc = seg_push(b, sl, sg))) {
            slot_retire(b, sl, rc);
            break;
        }
        slot_after(b, sl, o->after);                    /* the slot is fresh: err == 0 */
        /* the caller's arrays are copied outside the lock, the slot held by
         * this writer (as fixed_submit's bytes) */
        write_begin(b, sl);
        const int fe = pages_fill(sl, pg, i, m);
        write_end(b, sl);
        if (fe && !sl->err) sl->err = fe;
        slot_try_launch(b, sl);
        i += m;
    }
    return sub_end(b, &s, rc, o->ticket, !o->ticket);
}

int md5_batch_submit_device_pages(md5hip_batcher *b, const uint64_t *pages, const uint64_t *page_first,
                                  const uint32_t *lens, uint64_t n, uint32_t page_bytes, unsigned char *digests,
                                  int digests_on_device, void *producer_stream, int order, uint64_t *ticket)
{
    if (ticket) *ticket = 0;
    if (!b) return -EINVAL;
    if (n == 0) return 0;
    if (!digests) return -EINVAL;
    const struct md5hip_src src = {.kind = MD5HIP_SRC_PAGES, .lens = lens, .pages = pages,
                                   .page_first = page_first, .page_bytes = page_bytes};
    int rc = md5hip_src_check(&src, n);
    if (rc) return rc;
    /* the batcher's kind at the call, named to the engine (as the verify
     * entries): whole chunks only, so no CRC-32 window */
    int kind = MD5HIP_DIGEST_MD5;
    uint32_t fastcrc = 0;
    md5hip_batcher_get_digest(b, &kind, &fastcrc);
    if (fastcrc) return -EINVAL;
    if (!md5hip_pages_present()) return -ENOSYS;
    for (uint64_t i = 0; i < n; i++)
        if (md5hip_pages_of(lens[i], page_bytes) > b->pgcap) return -E2BIG;
    if ((rc = pages_buffers(b))) return rc;
    const hipStream_t after = (hipStream_t)producer_stream;
    return pages_submit(b, &src, n,
                        &(struct sub_opt){.digests = digests, .on_device = digests_on_device != 0,
                                          .async = ticket != NULL, .ticket = ticket, .kind = kind,
                                          .after = order ? &after : NULL});
}

/* ------------------------------------------------------------------------
 * Entries for the multi-GPU pool (md5_internal.h)
 * ------------------------------------------------------------------------ */
uint64_t md5hip_batcher_load(const md5hip_batcher *b)
{
    return __atomic_load_n(&b->load_bytes, __ATOMIC_RELAXED);
}

uint64_t md5hip_batcher_slice(const md5hip_batcher *b) { return b->cap; }

int md5hip_submit_src(md5hip_batcher *b, int kind, uint32_t fastcrc, const struct md5hip_src *src,
                      uint64_t lo, uint64_t hi, unsigned char *digests, uint64_t *ticket, int urgent)
{
    struct md5hip_src part = *src;
    part.first += lo;
    return enter(b, &part, hi - lo, &(struct sub_opt){.digests = digests, .async = ticket ? (urgent ? 2 : 1) : 0,
                                                      .ticket = ticket, .kind = kind, .fastcrc = fastcrc});
}

int md5hip_batcher_ticket_state(md5hip_batcher *b, uint64_t ticket, int *err)
{
    *err = 0;
    if (ticket == 0) return 1;
    pthread_mutex_lock(&b->mu);
    int rc = ticket >= b->tk.hi ? -EINVAL : tk_ring_done(&b->tk, ticket, err);
    pthread_mutex_unlock(&b->mu);
    return rc;
}

/* The digests of `kind` of n page-list chunks, by one synchronous submission
 * of this call's own kind (the batcher's setting is untouched, so concurrent
 * users are unaffected), in a fresh array the caller frees: *out, NULL on an
 * error. */
static int iov_digests(md5hip_batcher *b, int kind, uint32_t fastcrc, const struct md5hip_iov *segs,
                       const uint64_t *seg_first, uint64_t n, unsigned char **out)
{
    *out = NULL;
    const struct md5hip_src src = src_iov(segs, seg_first);
    int rc = md5hip_src_check(&src, n);
    if (rc) return rc;
    unsigned char *got = malloc((size_t)md5hip_digest_size(kind) * n);
    if (!got) return -ENOMEM;
    rc = submit(b, &src, n, &(struct sub_opt){.digests = got, .kind = kind, .fastcrc = fastcrc});
    if (rc) free(got);
    else *out = got;
    return rc;
}

/* Batched verify for the cache-read / write-verify sites (blk_io.c:665-704,
 * bc_mgr.c:1464-1492): ok[i] = digest(chunk i) == expected[i]; returns the
 * number of mismatching chunks (>= 0) or -errno.  A mismatch is what
 * dm_verify_block_crc (diskcache.c:3245-3265) reports per block; the caller
 * applies its own EAGAIN / inode-reset policy per flagged block.
 * md5hip_verify_iov_as: with an explicit digest kind for this call only. */
int md5hip_verify_iov_as(md5hip_batcher *b, int kind, uint32_t fastcrc,
                         const struct md5hip_iov *segs, const uint64_t *seg_first, uint64_t n,
                         const void *expected, unsigned char *ok)
{
    if (!b) return -EINVAL;
    if (n == 0) return 0;
    if (!expected || !ok) return -EINVAL;
    int rc;
    if ((rc = md5hip_digest_usable(kind, fastcrc))) return rc;
    unsigned char *got;
    if ((rc = iov_digests(b, kind, fastcrc, segs, seg_first, n, &got))) return rc;
    rc = md5hip_verify_count(got, expected, md5hip_digest_size(kind), n, ok);
    free(got);
    return rc;
}

int md5hip_batch_verify_iov(md5hip_batcher *b, const struct md5hip_iov *segs,
                            const uint64_t *seg_first, uint64_t n, const void *expected,
                            unsigned char *ok)
{
    if (!b) return -EINVAL;
    int kind;
    uint32_t fastcrc;
    md5hip_batcher_get_digest(b, &kind, &fastcrc);
    return md5hip_verify_iov_as(b, kind, fastcrc, segs, seg_first, n, expected, ok);
}

/* Verify the stored CRC-32 and produce the MD5 of every chunk in one pass:
 * the MD5_CRC32 records of the chunks, then counted. */
int md5hip_batch_upgrade_iov(md5hip_batcher *b, const struct md5hip_iov *segs,
                             const uint64_t *seg_first, uint64_t n, const uint32_t *want_crc,
                             unsigned char *ok, unsigned char *md5_out)
{
    if (!b) return -EINVAL;
    int rc = md5hip_digest_usable(MD5HIP_DIGEST_MD5_CRC32, 0);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!want_crc || !ok || !md5_out) return -EINVAL;
    unsigned char *rec;
    if ((rc = iov_digests(b, MD5HIP_DIGEST_MD5_CRC32, 0, segs, seg_first, n, &rec))) return rc;
    rc = md5hip_upgrade_count(rec, want_crc, n, ok, md5_out);
    free(rec);
    return rc;
}

/* ------------------------------------------------------------------------
 * Asynchronous verify and upgrade: the digests compared on the device
 * ------------------------------------------------------------------------ */
/* The verify buffers of every slot, allocated once by the first verify
 * submission (a batcher that never verifies allocates nothing for it):
 *   in    host callers' expected values (at most 32 B a chunk, each segment's
 *         on a 16-B boundary), then the table: a segment of c chunks is
 *         ceil(c / MD5HIP_CMP_PIECE) entries, so a slot's maxn chunks in
 *         fewer than segcap segments are fewer than `ents`;
 *   out   a count per entry, then an ok byte per chunk.
 * 0, -ENODEV, or -ENOMEM with nothing allocated. */
static int verify_buffers(md5hip_batcher *b)
{
    if (__atomic_load_n(&b->vready, __ATOMIC_ACQUIRE)) return 0;
    struct dev_guard g;
    if (batcher_enter(b, &g)) return -ENODEV;
    int rc = 0;
    if (!b->vready) {
        const uint64_t ents = b->segcap + b->maxn / MD5HIP_CMP_PIECE + 1;
        const uint64_t vin = 32 * b->maxn + 16 * b->segcap + 16 + sizeof(struct md5hip_cmp) * ents;
        const uint64_t vout = (8 * ents + b->maxn + 15) & ~15ull;
        void *hin = NULL, *din = NULL, *hout = NULL, *dout = NULL;
        if (hipHostMalloc(&hin, vin * b->nslots, hipHostMallocDefault) != hipSuccess ||
            hipHostMalloc(&hout, vout * b->nslots, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(&din, vin * b->nslots) != hipSuccess || hipMalloc(&dout, vout * b->nslots) != hipSuccess) {
            (void)hipGetLastError();
            if (hin) hipHostFree(hin);
            if (hout) hipHostFree(hout);
            if (din) hipFree(din);
            if (dout) hipFree(dout);
            rc = -ENOMEM;
        } else {
            b->vb_hin = hin; b->vb_din = din; b->vb_hout = hout; b->vb_dout = dout;
            b->vin_sz = vin;
            b->vout_sz = vout;
            for (uint32_t k = 0; k < b->nslots; k++) {
                b->s[k].h_vin = b->vb_hin + vin * k;
                b->s[k].d_vin = b->vb_din + vin * k;
                b->s[k].h_vout = b->vb_hout + vout * k;
                b->s[k].d_vout = b->vb_dout + vout * k;
            }
            __atomic_store_n(&b->vready, 1, __ATOMIC_RELEASE);
        }
    }
    batcher_leave(b, &g);
    return rc;
}

/* What every verify entry does once it has named its source, its digest
 * kind and what is compared: the checks (in the order in which the errors
 * win: arguments, the launcher, the buffers), then the engine.  Verify
 * segments never go the FIXED way. */
static int enter_verify(md5hip_batcher *b, const struct md5hip_src *src, uint64_t n, int kind, uint32_t fastcrc,
                        const struct md5hip_verify_opt *v, int async, uint64_t *ticket, const hipStream_t *after)
{
    if (ticket) *ticket = 0;
    if (!b || (async && !ticket)) return -EINVAL;
    int rc = md5hip_digest_usable(kind, fastcrc);
    if (rc) return rc;
    if (!md5hip_compare_present()) return -ENOSYS;
    if (n == 0) return 0;
    if (!v->expected || !v->ok || v->wsz == 0 || ((v->goff | v->wsz) & 3u) ||
        (uint64_t)v->goff + v->wsz > md5hip_digest_size(kind) || (v->md5_out && v->on_device))
        return -EINVAL;
    if ((rc = md5hip_src_check(src, n)) || (rc = verify_buffers(b))) return rc;
    return submit(b, src, n, &(struct sub_opt){.on_device = v->on_device, .async = async, .ticket = ticket,
                                               .kind = kind, .fastcrc = fastcrc, .after = after, .verify = v});
}

int md5hip_verify_src(md5hip_batcher *b, int kind, uint32_t fastcrc, const struct md5hip_src *src, uint64_t lo,
                      uint64_t hi, const struct md5hip_verify_opt *v, uint64_t *ticket, int urgent)
{
    struct md5hip_src part = *src;
    part.first += lo;
    struct md5hip_verify_opt pv = *v;
    if (pv.expected) pv.expected = (const unsigned char *)v->expected + (size_t)v->wsz * lo;
    if (pv.ok) pv.ok = v->ok + lo;
    if (pv.md5_out) pv.md5_out = v->md5_out + 16 * (size_t)lo;
    return enter_verify(b, &part, hi - lo, kind, fastcrc, &pv, ticket ? (urgent ? 2 : 1) : 0, ticket, NULL);
}

/* The ticket forms: *nbad is zeroed by the call, the mismatches added as
 * each launch holding the submission's chunks retires. */
int md5hip_batch_verify_iov_async(md5hip_batcher *b, const struct md5hip_iov *segs, const uint64_t *seg_first,
                                  uint64_t n, const void *expected, unsigned char *ok, uint64_t *nbad,
                                  uint64_t *ticket)
{
    if (ticket) *ticket = 0;
    if (!b || !ticket) return -EINVAL;
    if (nbad) *nbad = 0;
    if (n && (!expected || !ok)) return -EINVAL;
    int kind = MD5HIP_DIGEST_MD5;
    uint32_t fastcrc = 0;
    if (n) md5hip_batcher_get_digest(b, &kind, &fastcrc);
    const struct md5hip_src src = src_iov(segs, seg_first);
    return enter_verify(b, &src, n, kind, fastcrc,
                        &(struct md5hip_verify_opt){.expected = expected, .ok = ok, .nbad = nbad,
                                                    .wsz = md5hip_digest_size(kind)},
                        1, ticket, NULL);
}

int md5hip_batch_upgrade_iov_async(md5hip_batcher *b, const struct md5hip_iov *segs, const uint64_t *seg_first,
                                   uint64_t n, const uint32_t *want_crc, unsigned char *ok, unsigned char *md5_out,
                                   uint64_t *nbad, uint64_t *ticket)
{
    if (ticket) *ticket = 0;
    if (!b || !ticket) return -EINVAL;
    if (nbad) *nbad = 0;
    if (n && (!want_crc || !ok || !md5_out)) return -EINVAL;
    const struct md5hip_src src = src_iov(segs, seg_first);
    return enter_verify(b, &src, n, MD5HIP_DIGEST_MD5_CRC32, 0,
                        &(struct md5hip_verify_opt){.expected = want_crc, .ok = ok, .md5_out = md5_out, .nbad = nbad,
                                                    .goff = 16, .wsz = 4},
                        1, ticket, NULL);
}

int md5_batch_verify_device(md5hip_batcher *b, const uint64_t *d_ptrs, const uint32_t *lens, uint64_t n,
                            const void *expected, unsigned char *ok, int on_device, void *producer_stream,
                            int order, uint64_t *nbad, uint64_t *ticket)
{
    if (ticket) *ticket = 0;
    if (!b) return -EINVAL;
    if (nbad) *nbad = 0;
    if (n && (!expected || !ok)) return -EINVAL;
    int kind = MD5HIP_DIGEST_MD5;
    uint32_t fastcrc = 0;
    if (n) md5hip_batcher_get_digest(b, &kind, &fastcrc);
    const struct md5hip_src src = src_device(d_ptrs, lens);
    const hipStream_t after = (hipStream_t)producer_stream;
    return enter_verify(b, &src, n, kind, fastcrc,
                        &(struct md5hip_verify_opt){.expected = expected, .ok = ok, .nbad = nbad,
                                                    .wsz = md5hip_digest_size(kind), .on_device = on_device != 0},
                        ticket != NULL, ticket, order ? &after : NULL);
}

/* What both paged verify entries do once they have named what is compared
 * (n > 0): the checks in the order in which the errors win (arguments and
 * page rules -- before the batcher is touched --, the launchers, one chunk
 * against a slot's table, the buffers), then the paged engine with verify
 * segments.  kind KIND_BATCHER: the batcher's kind and window at the call,
 * whole digests compared (v->wsz is set here). */
static int enter_verify_pages(md5hip_batcher *b, const struct md5hip_src *src, uint64_t n, int kind,
                              struct md5hip_verify_opt *v, void *producer_stream, int order, uint64_t *ticket)
{
    int rc;
    uint32_t fastcrc = 0;
    if (!v->expected || !v->ok || (v->md5_out && v->on_device)) return -EINVAL;
    if ((rc = md5hip_src_check(src, n))) return rc;
    if (kind == KIND_BATCHER) {
        md5hip_batcher_get_digest(b, &kind, &fastcrc);
        v->wsz = md5hip_digest_size(kind);
    }
    if ((rc = md5hip_digest_usable(kind, fastcrc))) return rc;
    if (!md5hip_pages_present() || !md5hip_compare_present() || (fastcrc && !md5hip_pages_fast_present()))
        return -ENOSYS;
    for (uint64_t i = 0; i < n; i++)
        if (md5hip_pages_of(src->lens[i], src->page_bytes) > b->pgcap) return -E2BIG;
    if ((rc = pages_buffers(b)) || (rc = verify_buffers(b))) return rc;
    const hipStream_t after = (hipStream_t)producer_stream;
    return pages_submit(b, src, n,
                        &(struct sub_opt){.on_device = v->on_device, .async = ticket != NULL, .ticket = ticket,
                                          .kind = kind, .fastcrc = fastcrc, .after = order ? &after : NULL,
                                          .verify = v});
}

int md5_batch_verify_device_pages(md5hip_batcher *b, const uint64_t *pages, const uint64_t *page_first,
                                  const uint32_t *lens, uint64_t n, uint32_t page_bytes, const void *expected,
                                  unsigned char *ok, int on_device, void *producer_stream, int order, uint64_t *nbad,
                                  uint64_t *ticket)
{
    if (ticket) *ticket = 0;
    if (!b) return -EINVAL;
    if (nbad) *nbad = 0;
    if (n == 0) return 0;
    const struct md5hip_src src = {.kind = MD5HIP_SRC_PAGES, .lens = lens, .pages = pages,
                                   .page_first = page_first, .page_bytes = page_bytes};
    return enter_verify_pages(b, &src, n, KIND_BATCHER,
                              &(struct md5hip_verify_opt){.expected = expected, .ok = ok, .nbad = nbad,
                                                          .on_device = on_device != 0},
                              producer_stream, order, ticket);
}

int md5_batch_upgrade_device_pages(md5hip_batcher *b, const uint64_t *pages, const uint64_t *page_first,
                                   const uint32_t *lens, uint64_t n, uint32_t page_bytes, const uint32_t *want_crc,
                                   unsigned char *ok, unsigned char *md5_out, void *producer_stream, int order,
                                   uint64_t *nbad, uint64_t *ticket)
{
    if (ticket) *ticket = 0;
    if (!b) return -EINVAL;
    if (nbad) *nbad = 0;
    if (n == 0) return 0;
    if (!md5_out) return -EINVAL;
    const struct md5hip_src src = {.kind = MD5HIP_SRC_PAGES, .lens = lens, .pages = pages,
                                   .page_first = page_first, .page_bytes = page_bytes};
    return enter_verify_pages(b, &src, n, MD5HIP_DIGEST_MD5_CRC32,
                              &(struct md5hip_verify_opt){.expected = want_crc, .ok = ok, .md5_out = md5_out,
                                                          .nbad = nbad, .goff = 16, .wsz = 4},
                              producer_stream, order, ticket);
}
