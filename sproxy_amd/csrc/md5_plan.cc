// md5_plan.cc -- the batch planner of include/md5hip.h: the longest-first
// order of a descriptor batch and the kernel variant it runs.  Host
// arithmetic only; the device enters through md5hip_cu_count()
// (md5_internal.h, defined in md5_kernels.hip), so the file builds with the
// host compiler and runs stand-alone (tests/c/plan_check.cc).
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>

#include <thread>

#define MD5HIP_DEFINES_MD5CRC32   // md5crc32hip_plan is defined here, not weakly referenced
#include "md5_internal.h"

namespace {

uint64_t cus() { return (uint64_t)md5hip_cu_count(); }

// Small batches (at most two 64-chunk groups per CU: the netcache call
// site's vectors of 16-1,024 blocks) run lane-direct.  There each wave is
// nearly alone on its SIMD and the launch lasts one chunk's serial chain; the
// 8-block register ring keeps HBM latency off that chain, where XDMA's
// per-stage DMA wait and LDS round trip stay on it: 147 vs 163 us for
// 64-4,096 x 16 KiB, 162 vs 171 us at 32,768; past two groups per CU the
// lane-direct loads crowd the address units (65,536 x 16 KiB: 228 vs
// 206 us; profiles/r03/small_batch_kernels_*.json).
constexpr uint64_t kLaneGroupsPerCu = 2;

// Of those, batches of at most one group per CU (md5hip_fed_fits; also the
// fixed-length AUTO launch and md5hip_update_ctx) run as fed pairs (FED: the
// chain wave's 5th VALU per step moves to a feeder wave on another SIMD;
// 147 -> 138 us at 64-4,096 x 16 KiB, 150.6 -> 141 at 16,384;
// profiles/r03q/small_fed_16k.json) when some chunk has two whole blocks.
constexpr uint64_t kFedGroupsPerCu = 1;

// The decision past the small batches, from four order statistics: the
// longest chunk's blocks, the median group's first key, the summed first
// keys of all groups (work), and the blocks of the chunk two waves per CU deep.
int plan_choice(uint32_t bmax, uint64_t median, uint64_t total, uint32_t probe_blocks) {
  if (8u * median <= (uint64_t)bmax + 1) {
    const uint64_t simds = 4ull * cus();
    if (10u * total >= 4u * simds * ((uint64_t)bmax + 1)) return MD5HIP_DESC_BALANCED;
  }
  return 4ull * probe_blocks <= bmax ? MD5HIP_DESC_HYBRID : MD5HIP_DESC_XDMA;
}

// What both planners know of a non-empty batch in longest-first order:
// md5hip_plan_desc reads it off the order, md5hip_plan_hist off the histogram.
struct BatchStats {
  uint64_t ngroups;        // 64-chunk groups
  uint32_t bmax;           // whole blocks of the longest chunk
  uint64_t median;         // key of the median group's first chunk
  uint64_t total;          // work in block-steps: a group runs as long as its first lane
  uint32_t probe_blocks;   // whole blocks of the chunk two waves per CU deep (or the last)
};

// rank of that probe chunk
uint64_t probe_rank(uint64_t n) {
  const uint64_t depth = cus() * 128u;
  return depth < n - 1 ? depth : n - 1;
}

// Planner for descriptor batches (md5hip.h):
//  - FED / LANE for small batches (above);
//  - BALANCED for a mixed batch (longest chunk >= 256 KiB, median 64-chunk
//    group <= 1/8 of it) holding >= 0.4 x (SIMDs x longest chain) of work:
//    several waves per SIMD, where LPT placement beats the hardware's
//    (coalesced C3 submissions, profiles/r02_c3_trace.json);
//  - HYBRID when the longest chunks stand out -- the chunk two waves per CU
//    deep in the order is at most a quarter as long -- so their serial chains
//    bound the launch (one C3 batch; fewer long chunks than two waves per CU);
//  - XDMA otherwise (equal-length netcache blocks).  DESIGN.md §5.
int decide(const BatchStats& s) {
  if (s.ngroups <= kLaneGroupsPerCu * cus())
    return md5hip_fed_fits(s.ngroups) && s.bmax >= MD5HIP_FED_MIN_BLOCKS ? MD5HIP_DESC_FED : MD5HIP_DESC_LANE;
  if (s.bmax < MD5HIP_HYBRID_LONG_BLOCKS) return MD5HIP_DESC_XDMA;
  return plan_choice(s.bmax, s.median, s.total, s.probe_blocks);
}

}  // namespace

extern "C" {

int md5hip_fed_fits(uint64_t ngroups) { return ngroups <= kFedGroupsPerCu * cus(); }

// CRC-32 of a full-CRC batch, split across a wave per chunk (crc32_split)
// or streamed one lane per chunk.  The streaming launch lasts one chunk's
// serial chain, ~13 ns per byte (220 us at 16 KiB, 12.9 ms at 1 MiB) with an
// ~18 us floor; the split one moves ~2.8 TB/s with ~3 ns per chunk of fixed
// work.  Measured crossovers (profiles/r03aa/, profiles/r03u/): ~36 K chunks
// at 16 KiB, ~38 K at 64 KiB, none up to 4 K at 1 MiB, ~3.5 K at 1 KiB.  So
// with the chunk length known, split up to 128 chunks per CU when chunks are
// >= 2 KiB and up to 12 per CU below; with it unknown (device-side lengths),
// up to kCrcSplitPerCu.
constexpr uint64_t kCrcSplitPerCu = 16;
int md5hip_crc_split_fits(uint64_t n, uint64_t len) {
  if (len == 0) return n <= kCrcSplitPerCu * cus();
  return len >= 2048 ? n <= 128 * cus() : n <= 12 * cus();
}

// The CRC variant for a descriptor batch whose mean chunk length the caller
// knows (the batcher does).  Not split = XDMA16 named explicitly: AUTO would
// decide again with the length unknown (kCrcSplitPerCu per CU) and split
// short-chunk batches past the crossover.
int md5hip_crc_desc_choice(uint64_t n, uint64_t mean_len) {
  return md5hip_crc_split_fits(n, mean_len ? mean_len : 1) ? CRC32HIP_SPLIT : CRC32HIP_XDMA16;
}
// (with fastcrc the batcher passes 2n windows of fastcrc bytes; windows under
// the launchers' kCrcSplitMinWindow keep the window kernels whatever the
// variant says)

// The one-pass MD5 + CRC-32 kind (md5hip.h).  XDMA16 keeps one lane per chunk
// for both chains, ~20 ns per byte of chunk whatever the count: a batch of at
// most one 64-chunk group per CU is a lone wave per workgroup running them
// back to back (325 us at 16 KiB, 45 us at 2 KiB, 25 us at 1 KiB).  FEDSPLIT
// gives such a batch the two small-batch kernels in one launch: the MD5s as
// fed pairs (135 us at 16 KiB) beside two CRC waves per CU, each taking a
// chunk in ~5.5 us of mostly fixed work (the split's tree of shifts), so the
// CRC role lasts ceil(n / (2 x CUs)) x 5.5 us and bounds the launch once the
// chunks are many and short: 16,384 x 1 KiB ran 170 us against XDMA16's 26,
// 1,024 x 1 KiB 15 against 25.  Hence two bounds beside the fed pairs' own:
// chunks of >= MD5CRC32HIP_FEDSPLIT_MIN_LEN bytes (below, FEDSPLIT's ~15 us
// floor is XDMA16's whole launch), and at most CUs x mean_len / 256 chunks --
// the CRC role then lasts about half of XDMA16's time (2,048 chunks at
// 2 KiB: 25 us against 46; every fed-pair batch from 16 KiB on).  profiles/dual_small/ab.json,
// DESIGN.md §5.8.
constexpr uint64_t kDualLenPerChunkCu = 256;
int md5crc32hip_plan(uint64_t n, uint64_t mean_len) {
  return n && md5hip_fed_fits((n + 63) / 64) && mean_len >= MD5CRC32HIP_FEDSPLIT_MIN_LEN &&
                 n * kDualLenPerChunkCu <= cus() * mean_len
             ? MD5CRC32HIP_FEDSPLIT
             : MD5CRC32HIP_XDMA16;
}

int md5hip_plan_order(const uint32_t* lens, uint64_t n, uint32_t* order) {
  if (n == 0) return 0;
  if (!lens || !order || n > 0xffffffffull) return -EINVAL;
  // counting sort on block count, descending; block counts are < 2^26
  // (len < 2^32), bucket by the bit length of nblocks then by value within
  // small buckets -- a two-level key keeps the histogram tiny.
  uint32_t maxb = 0;
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t b = (lens[i] >> 6) + 1;
    if (b > maxb) maxb = b;
  }
  if (maxb <= (1u << 20)) {
    // T contiguous index ranges, one histogram each; range t's chunks of key
    // k go after every earlier range's chunks of key k: stable, and the
    // batcher's large coalesced slots (~1 M chunks) plan on several cores.
    constexpr uint32_t kPlanThreads = 8;
    const uint64_t per = 1u << 17;
    const uint32_t T = n >= 2 * per ? (uint32_t)(n / per < kPlanThreads ? n / per : kPlanThreads) : 1u;
    const size_t nb = (size_t)maxb + 1;
    uint32_t* cnt = (uint32_t*)calloc(nb * T, sizeof(uint32_t));
    if (!cnt) return -ENOMEM;
    auto range = [&](uint32_t t, uint64_t& lo, uint64_t& hi) {
      lo = n * t / T;
      hi = n * (t + 1) / T;
    };
    auto hist = [&](uint32_t t) {
      uint64_t lo, hi;
      range(t, lo, hi);
      uint32_t* c = cnt + nb * t;
      for (uint64_t i = lo; i < hi; ++i) c[maxb - ((lens[i] >> 6) + 1)]++;
    };
    auto scatter = [&](uint32_t t) {
      uint64_t lo, hi;
      range(t, lo, hi);
      uint32_t* c = cnt + nb * t;
      for (uint64_t i = lo; i < hi; ++i) order[c[maxb - ((lens[i] >> 6) + 1)]++] = (uint32_t)i;
    };
    // ranges 1..T-1 on helper threads; a range whose thread cannot be
    // started runs here (no exception leaves this extern "C" entry)
    auto fan_out = [&](auto&& fn) {
      std::thread th[kPlanThreads];
      for (uint32_t t = 1; t < T; ++t) {
        try {
          th[t] = std::thread(fn, t);
        } catch (...) {
        }
      }
      fn(0u);
      for (uint32_t t = 1; t < T; ++t) {
        if (th[t].joinable()) th[t].join();
        else fn(t);
      }
    };
    fan_out(hist);
    uint32_t run = 0;
    for (size_t k = 0; k < nb; ++k)
      for (uint32_t t = 0; t < T; ++t) {
        const uint32_t c = cnt[nb * t + k];
        cnt[nb * t + k] = run;
        run += c;
      }
    fan_out(scatter);
    free(cnt);
    return 0;
  }
  // very long chunks: fall back to a comparison sort
  for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;
  struct Cmp {
    static int f(const void* a, const void* b, void* ctx) {
      const uint32_t* L = (const uint32_t*)ctx;
      const uint32_t x = L[*(const uint32_t*)a] >> 6, y = L[*(const uint32_t*)b] >> 6;
      if (x != y) return x > y ? -1 : 1;
      return *(const uint32_t*)a < *(const uint32_t*)b ? -1 : 1;
    }
  };
  qsort_r(order, (size_t)n, sizeof(uint32_t), Cmp::f, (void*)lens);
  return 0;
}

int md5hip_plan_desc(const uint32_t* lens, uint64_t n, uint32_t* order) {
  if (int e = md5hip_plan_order(lens, n, order)) return e;
  if (n == 0) return MD5HIP_DESC_XDMA;
  auto blocks = [&](uint64_t rank) { return lens[order[rank]] >> 6; };
  BatchStats s{};
  s.ngroups = (n + 63) / 64;
  s.bmax = blocks(0);
  s.median = (uint64_t)blocks((s.ngroups / 2) * 64) + 1;
  for (uint64_t g = 0; g < s.ngroups; ++g) s.total += (uint64_t)blocks(g * 64) + 1;
  s.probe_blocks = blocks(probe_rank(n));
  return decide(s);
}

// XDMA becomes LINES when more than half the batch's bytes lie in chunks
// that start 16-B but not 128-B aligned (their stages would straddle lines).
// Line-aligned and uniform batches keep XDMA, whose four waves per SIMD
// LINES' extra line of registers does not allow.
int md5hip_lines_choice(int variant, uint64_t unlined_bytes, uint64_t bytes) {
  return variant == MD5HIP_DESC_XDMA && 2 * unlined_bytes > bytes ? MD5HIP_DESC_LINES : variant;
}

int md5hip_plan_desc_at(const uint32_t* lens, const uint64_t* addrs, uint64_t n, uint32_t* order) {
  if (!addrs && n) return -EINVAL;
  const int v = md5hip_plan_desc(lens, n, order);
  if (v != MD5HIP_DESC_XDMA) return v;
  uint64_t bytes = 0, unlined = 0;
  for (uint64_t i = 0; i < n; ++i) {
    bytes += lens[i];
    if ((addrs[i] & 127u) != 0 && (addrs[i] & 15u) == 0) unlined += lens[i];
  }
  return md5hip_lines_choice(v, unlined, bytes);
}

int md5hip_plan_hist(const uint32_t* hist, uint32_t kmax, uint64_t n, uint32_t* bucket_start) {
  if (!hist || kmax > MD5HIP_HIST_KMAX) return -EINVAL;
  // walk the keys longest-first; rank r of the sorted order holds key k for
  // r in [start(k), start(k) + hist[k])
  BatchStats s{};
  s.ngroups = (n + 63) / 64;
  const uint64_t rmed = (s.ngroups / 2) * 64;
  const uint64_t rprobe = n ? probe_rank(n) : 0;
  uint64_t r = 0, probe = 0;
  uint32_t top = 0;
  for (uint32_t k = kmax; k >= 1; --k) {
    const uint64_t c = hist[k];
    if (bucket_start) bucket_start[kmax - k] = (uint32_t)r;
    if (!c) continue;
    if (!top) top = k;
    // group firsts 64 g in [r, r + c)
    const uint64_t g0 = (r + 63) / 64, g1 = (r + c - 1) / 64;
    if (g1 >= g0) s.total += (g1 - g0 + 1) * (uint64_t)k;
    if (rmed >= r && rmed < r + c) s.median = k;
    if (rprobe >= r && rprobe < r + c) probe = k;
    r += c;
  }
  if (bucket_start) bucket_start[kmax] = (uint32_t)r;   // key 0 (never used): the end
  if (n == 0 || !top) return MD5HIP_DESC_XDMA;
  s.bmax = top - 1;
  s.probe_blocks = (uint32_t)(probe - 1);
  return decide(s);
}

}  // extern "C"
