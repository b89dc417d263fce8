// md5_kernels.hip -- instantiates the batched-MD5 kernels (md5_kernels.h)
// and exports the launchers of the C ABI (include/md5hip.h), the batch arenas
// and the device-side order.  Which kernel a batch runs is md5_plan.cc's.
#define MD5HIP_DEFINES_MD5CRC32   // the launchers are defined here (md5_internal.h)
#include "md5_kernels.h"

namespace md5hip {
// Explicit instantiations: kernels referenced only from host templates are
// otherwise not emitted by hipcc (host stub and device code both missing).
template __global__ void md5_desc<false>(const uint8_t*, const uint64_t*, const uint32_t*,
                                         const uint32_t*, uint64_t, uint64_t, uint32_t, uint4*);
template __global__ void md5_desc<true>(const uint8_t*, const uint64_t*, const uint32_t*,
                                        const uint32_t*, uint64_t, uint64_t, uint32_t, uint4*);
template __global__ void crc32_desc<true>(const uint8_t*, const uint64_t*, const uint32_t*,
                                          const uint32_t*, uint64_t, uint64_t, uint32_t,
                                          uint32_t*);

}  // namespace md5hip

// ===========================================================================
// C ABI (include/md5hip.h)
// ===========================================================================
#include <errno.h>
#include <atomic>
#include <map>
#include <tuple>
#include <mutex>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/md5hip.h"
#include "md5_internal.h"

using namespace md5hip;

namespace {

constexpr int kBlock = 256;
constexpr int kDescBlock = 64;

int launched() { return hipGetLastError() == hipSuccess ? 0 : -EIO; }

// One launcher branch: launch, then 0 or -EIO.  The arguments convert to the
// kernel's own parameter types, so a branch passes nullptr, 0 and the ABI's
// void pointers as they are.
template <typename... P, typename... A>
int launch(void (*kern)(P...), uint64_t grid, uint32_t block, uint32_t lds, void* stream, A... args) {
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(block), lds, (hipStream_t)stream,
                     static_cast<P>(args)...);
  return launched();
}

// What a launcher checks once its batch is not empty (that returns 0 before
// anything else), in the order in which the errors win: the caller's
// arguments (-EINVAL) before the device is asked for (-ENODEV: a machine
// without one still reports a wrong argument), the grid limit (-EINVAL) last.
int ready(bool args_ok, uint64_t grid = 0) {
  int dev = -1;
  if (!args_ok) return -EINVAL;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -ENODEV;
  return grid > 0x7fffffffull ? -EINVAL : 0;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

// BALANCED's self-resetting group counters: one pair per (device, stream),
// allocated and zeroed on first use (launches on one stream are ordered, so
// a counter reset by the last wave of launch k is zero for launch k+1).
// hipStreamPerThread is one handle that names a different stream in every
// thread, so it is keyed by a per-thread id as well (ids are never reused,
// so a finished thread's launch still in flight keeps its own counter).
std::mutex g_ctr_mu;
std::map<std::tuple<int, hipStream_t, uint64_t>, uint32_t*> g_ctr;
std::atomic<uint64_t> g_thread_ids{0};

uint64_t this_thread_id() {
  thread_local const uint64_t id = ++g_thread_ids;
  return id;
}

uint32_t* balanced_counter(hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  const auto key = std::make_tuple(dev, s, s == hipStreamPerThread ? this_thread_id() : 0ull);
  std::lock_guard<std::mutex> lk(g_ctr_mu);
  auto it = g_ctr.find(key);
  if (it != g_ctr.end()) return it->second;
  uint32_t* c = nullptr;
  if (hipMalloc(&c, 4 * sizeof(uint32_t)) != hipSuccess) return nullptr;
  if (hipMemset(c, 0, 4 * sizeof(uint32_t)) != hipSuccess) { (void)hipFree(c); return nullptr; }
  g_ctr[key] = c;
  return c;
}

// A kernel's dynamic-LDS limit raised once per device (the attribute is set
// on the current device; a pool drives several from one process).
bool dyn_lds_ready(const void* kern, uint32_t lds) {
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, bool> done;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return false;
  std::lock_guard<std::mutex> lk(mu);
  auto it = done.find({dev, kern});
  if (it != done.end()) return it->second;
  const bool ok = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) ==
                  hipSuccess;
  done[{dev, kern}] = ok;
  return ok;
}

// One workgroup of `threads` per CU, grid-stride over 64-chunk groups.
uint32_t per_cu_grid(uint64_t n) {
  const uint64_t need = (n + 63) / 64;
  const uint64_t cap = (uint64_t)md5hip_cu_count();
  return (uint32_t)(need < cap ? need : cap);
}

// 4 chunks (waves) per 256-thread workgroup; grid-stride past 8 per CU
uint32_t crc_split_grid(uint64_t n) {
  const uint64_t need = (n + 3) / 4;
  const uint64_t cap = 2ull * (uint64_t)md5hip_cu_count();
  return (uint32_t)(need < cap ? need : cap);
}

}  // namespace

extern "C" {

int md5hip_abi_version(void) { return MD5HIP_ABI_VERSION; }

// md5_internal.h: compute units of the current device (grid sizing of
// one-workgroup-per-CU kernels, HYBRID's long-wave count, the planner's
// thresholds).  Cached per device: a small launch asks several times
// (planner, grid, the CRC choice), and the attribute query is a runtime call
// each time.
int md5hip_cu_count(void) {
  static std::atomic<int> cached[64];
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  if (dev >= 0 && dev < 64 && (cus = cached[dev].load(std::memory_order_relaxed)) > 0) return cus;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    return 256;
  if (dev >= 0 && dev < 64) cached[dev].store(cus, std::memory_order_relaxed);
  return cus;
}

// The shipped kernels are fixed: the round-1 A/B variants live in the
// diagnostic library (removed in round 4; git history at 993ee7d), and no environment
// variable re-routes a product launch.
int md5hip_resolve_variant(int v) { return v == MD5HIP_AUTO ? MD5HIP_XDMA1NT : v; }
int crc32hip_resolve_variant(int v) { return v == CRC32HIP_AUTO ? CRC32HIP_XDMA16 : v; }

const char* md5hip_variant_name(int v) {
  switch (v) {
    case MD5HIP_AUTO: return "auto";
    case MD5HIP_DIRECT2: return "direct2";
    case MD5HIP_XDMA1NT: return "xdma1nt";
    default: return "?";
  }
}

int md5hip_digest_desc(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                       const uint32_t* d_order, uint64_t n, unsigned char* d_digests,
                       void* stream) {
  return md5hip_digest_desc_variant(d_base, d_offsets, d_lens, d_order, n, d_digests, stream,
                                    MD5HIP_DESC_AUTO);
}

int md5hip_digest_desc_variant(const void* d_base, const uint64_t* d_offsets,
                               const uint32_t* d_lens, const uint32_t* d_order, uint64_t n,
                               unsigned char* d_digests, void* stream, int variant) {
  if (n == 0) return 0;
  const bool known = variant == MD5HIP_DESC_AUTO || variant == MD5HIP_DESC_LANE ||
                     variant == MD5HIP_DESC_HYBRID || variant == MD5HIP_DESC_XDMA ||
                     variant == MD5HIP_DESC_BALANCED || variant == MD5HIP_DESC_FED ||
                     variant == MD5HIP_DESC_LINES;
  const uint64_t g = (n + 63) / 64;
  if (int e = ready(d_base && d_offsets && d_lens && d_digests && aligned(d_digests, 16) && known, g))
    return e;
  uint4* out = (uint4*)d_digests;
  switch (variant) {
    case MD5HIP_DESC_HYBRID:
      // the first waves (one per CU: the longest chunks in longest-first order)
      // run their chains lane-direct (md5hip_plan_desc picks HYBRID)
      return launch(md5_desc_hybrid, g, 64, 0, stream, d_base, d_offsets, d_lens, d_order, n, out,
                    md5hip_cu_count());
    case MD5HIP_DESC_BALANCED: {
      uint32_t* ctr = balanced_counter((hipStream_t)stream);
      if (!ctr) return -ENOMEM;
      constexpr int WPB = kBalancedWaves;
      constexpr uint32_t lds = BalancedCfg<WPB, kBalancedImages>::kLds;
      auto kern = md5_desc_balanced_t<WPB, kBalancedImages, kBalancedPolicy>;
      if (!dyn_lds_ready(reinterpret_cast<const void*>(kern), lds)) return -ENODEV;
      // the kernel resets its counter on exit; zero it on the stream anyway, so
      // a launch that never finished (a fault) cannot poison the next one
      if (hipMemsetAsync(ctr, 0, 4 * sizeof(uint32_t), (hipStream_t)stream) != hipSuccess) return -EIO;
      return launch(kern, (uint64_t)md5hip_cu_count(), 64 * WPB, lds, stream, d_base, d_offsets, d_lens,
                    d_order, n, out, ctr);
    }
    case MD5HIP_DESC_FED:
      // chain + feeder wave per 64-chunk group (md5_kernels.h md5_desc_fed)
      return launch(md5_desc_fed<false>, g, 128, 0, stream, d_base, d_offsets, d_lens, d_order, n, 0, 0,
                    out);
    case MD5HIP_DESC_LINES:
      return launch(md5_desc_lines, g, 64, 0, stream, d_base, d_offsets, d_lens, d_order, n, out);
    case MD5HIP_DESC_LANE:
      // One wave per workgroup: a mixed batch has few waves, and the
      // dispatcher then spreads them one per CU instead of packing 4 onto one CU
      // where the long chunks' lane-direct loads contend for the CU's address unit
      // (scripts/c3_trace.py, deleted in 4de68d0: 28.7 -> 13.2 ms on the C3 batch).
      return launch(md5_desc<false>, g, kDescBlock, 0, stream, d_base, d_offsets, d_lens, d_order, n, 0,
                    0, out);
    default:   // AUTO, XDMA
      return launch(md5_desc_xdma, g, 64, 0, stream, d_base, d_offsets, d_lens, d_order, n, out);
  }
}

int md5hip_digest_fixed_variant(const void* d_base, uint64_t n, uint32_t len, uint64_t stride,
                                unsigned char* d_digests, void* stream, int variant) {
  if (n == 0) return 0;
  const bool known = variant == MD5HIP_AUTO || variant == MD5HIP_DIRECT2 || variant == MD5HIP_XDMA1NT;
  const uint64_t grid = (n + kBlock - 1) / kBlock, g = (n + 63) / 64;
  // chunk starts off the 16-B grid launch g workgroups, the others `grid`
  const bool off_grid = !aligned(d_base, 16) || (stride & 15u) != 0;
  if (int e = ready(d_base && d_digests && len <= stride && aligned(d_digests, 16) && known, off_grid ? g : grid))
    return e;
  uint4* out = (uint4*)d_digests;
  if (off_grid)
    // chunk starts not 16-B aligned: descriptor kernel with implicit offsets
    return launch(md5_desc<true>, g, kDescBlock, 0, stream, d_base, nullptr, nullptr, nullptr, n, stride,
                  len, out);
  // xdma1nt addresses a 64-chunk group with 32-bit buffer offsets
  if (variant == MD5HIP_DIRECT2 || stride >= (1ull << 31) / 64)
    return launch(md5_fixed_direct, grid, kBlock, 0, stream, d_base, n, len, stride, out);
  if (variant == MD5HIP_AUTO && md5hip_fed_fits(g) && (len >> 6) >= kFedMinBlocks)
    // a small batch: its launch is one chunk's chain, which fed pairs shorten
    return launch(md5_desc_fed<true>, g, 128, 0, stream, d_base, nullptr, nullptr, nullptr, n, stride,
                  len, out);
  return launch(md5_fixed_xdma1nt, grid, kBlock, 0, stream, d_base, n, len, stride, out);
}

int md5hip_digest_fixed(const void* d_base, uint64_t n, uint32_t len, uint64_t stride,
                        unsigned char* d_digests, void* stream) {
  return md5hip_digest_fixed_variant(d_base, n, len, stride, d_digests, stream, MD5HIP_AUTO);
}

// (The CRC helpers stand here, not with the others above: crc32_split is
// first used after md5_desc_fed, and the code object lays kernels out in that
// order.  static: inside extern "C" the unnamed namespace alone exports them.)
namespace {
// Where a CRC batch's chunks lie: descriptor arrays, or with none chunk i at
// base + i * stride, flen bytes.
struct CrcSrc {
  const uint64_t* offs;
  const uint32_t* lens;
  const uint32_t* order;
  uint64_t stride;
  uint32_t flen;
};

static bool crc_variant_known(int v) { return v == CRC32HIP_AUTO || v == CRC32HIP_XDMA16 || v == CRC32HIP_SPLIT; }
constexpr uint32_t kCrcSplitMinWindow = 2048;    // fastcrc windows split from this size
constexpr int kCrcWhole = 1;                     // crc_ladder launched nothing (no errno is positive)

// The CRC kernels both entries share.  Split (md5_plan.cc has the
// crossovers): full-CRC batches, and windowed ones (two messages of fastcrc
// bytes per chunk) with windows of >= 2 KiB; shorter windows are chains short
// enough for the window kernels (F = 1000: split 28-48 us against 30-32 us,
// F = 4096: 15-31 against 57-60; profiles/r03af/).  `split_len` is the
// message length the split decision may count on, 0 when the caller has none.
// Whole chunks that do not split are left to the entry: kCrcWhole.
static int crc_ladder(const void* base, const CrcSrc& c, uint64_t n, uint32_t fastcrc, bool windows,
                      uint64_t split_len, int variant, uint32_t* out, void* stream) {
  const bool split = variant == CRC32HIP_SPLIT ||
                     (variant == CRC32HIP_AUTO && md5hip_crc_split_fits(windows ? 2 * n : n, split_len));
  if ((!windows || fastcrc >= kCrcSplitMinWindow) && split)
    return launch(!c.offs ? crc32_split<true> : crc32_split<false>, crc_split_grid(n), 256, 0, stream,
                  base, c.offs, c.lens, c.order, n, c.stride, c.flen, fastcrc, out);
  if (!windows) return kCrcWhole;
  // one- or two-block windows: lane loads, next group in flight; longer ones:
  // head and tail windows as 2n rows through the LDS-DMA loader
  const bool pipe = fastcrc == 64 || fastcrc == 128;
  return launch(pipe ? crc32_fast_pipe : crc32_fast_xdma16, per_cu_grid(2 * n), pipe ? 1024 : 768, 0,
                stream, base, c.offs, c.lens, n, c.stride, c.flen, fastcrc, out);
}

}  // namespace

// The two CRC entries share crc_ladder and differ in two things: the fixed
// one knows the chunk length for the split decision, and only it has the
// fixed-stride loader ahead of the descriptor kernel for whole chunks.
int crc32hip_fixed_variant(const void* d_base, uint64_t n, uint32_t len, uint64_t stride,
                           uint32_t fastcrc, uint32_t* d_crcs, void* stream, int variant) {
  if (n == 0) return 0;
  const uint64_t g = (n + kDescBlock - 1) / kDescBlock;
  if (int e = ready(d_base && d_crcs && len <= stride && !(fastcrc & 3u) && aligned(d_crcs, 4) && crc_variant_known(variant), g))
    return e;
  const bool windows = fastcrc && len > fastcrc;
  const int rc = crc_ladder(d_base, CrcSrc{nullptr, nullptr, nullptr, stride, len}, n, fastcrc, windows,
                            windows ? fastcrc : (len ? len : 1), variant, d_crcs, stream);
  if (rc != kCrcWhole) return rc;
  if (aligned(d_base, 16) && (stride & 15u) == 0 && stride < (1ull << 31) / 64)
    // one 768-thread workgroup per CU (160 KiB LDS), grid-stride, wave-major
    return launch(crc32_fixed_xdma16, per_cu_grid(n), 768, 0, stream, d_base, n, len, stride, d_crcs);
  return launch(crc32_desc<true>, g, kDescBlock, 0, stream, d_base, nullptr, nullptr, nullptr, n, stride,
                len, d_crcs);
}

int crc32hip_fixed(const void* d_base, uint64_t n, uint32_t len, uint64_t stride,
                   uint32_t fastcrc, uint32_t* d_crcs, void* stream) {
  return crc32hip_fixed_variant(d_base, n, len, stride, fastcrc, d_crcs, stream, CRC32HIP_AUTO);
}

int crc32hip_desc(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                  const uint32_t* d_order, uint64_t n, uint32_t fastcrc, uint32_t* d_crcs,
                  void* stream) {
  return crc32hip_desc_variant(d_base, d_offsets, d_lens, d_order, n, fastcrc, d_crcs, stream,
                               CRC32HIP_AUTO);
}

int crc32hip_desc_variant(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                          const uint32_t* d_order, uint64_t n, uint32_t fastcrc, uint32_t* d_crcs,
                          void* stream, int variant) {
  if (n == 0) return 0;
  if (int e = ready(d_base && d_offsets && d_lens && d_crcs && !(fastcrc & 3u) && aligned(d_crcs, 4) && crc_variant_known(variant),
                    (n + kDescBlock - 1) / kDescBlock))
    return e;
  // the lengths are on the device: windows whenever fastcrc is set (the
  // kernels take a chunk no longer than the window whole), and the split
  // decision has no length (0)
  const int rc = crc_ladder(d_base, CrcSrc{d_offsets, d_lens, d_order, 0, 0}, n, fastcrc, fastcrc != 0, 0,
                            variant, d_crcs, stream);
  if (rc != kCrcWhole) return rc;
  // XDMA16: one 768-thread workgroup per CU, LDS-DMA images
  return launch(crc32_desc_xdma16, per_cu_grid(n), 768, 0, stream, d_base, d_offsets, d_lens, d_order, n,
                d_crcs);
}

// MD5 + CRC-32 in one pass (32-B records, md5hip.h).  One frame for every
// batch: XDMA16's 768-thread workgroup per CU.  Chunk starts off the 16-B
// grid, or a stride past the fixed loader's 32-bit offsets, take the
// descriptor kernel with implicit offsets (its lane-direct branch covers the
// unaligned waves).
int md5crc32hip_fixed(const void* d_base, uint64_t n, uint32_t len, uint64_t stride,
                      struct md5hip_md5crc32* d_out, void* stream) {
  static_assert(sizeof(md5hip_md5crc32) == sizeof(Md5Crc32Record) && sizeof(Md5Crc32Record) == 32,
                "record layout");
  if (n == 0) return 0;
  if (int e = ready(d_base && d_out && len <= stride && aligned(d_out, 16), (n + 63) / 64)) return e;
  Md5Crc32Record* out = reinterpret_cast<Md5Crc32Record*>(d_out);
  if (aligned(d_base, 16) && (stride & 15u) == 0 && stride < (1ull << 31) / 64)
    return launch(md5crc32_fixed_xdma16, per_cu_grid(n), 768, 0, stream, d_base, n, len, stride, out);
  return launch(md5crc32_desc_xdma16<true>, per_cu_grid(n), 768, 0, stream, d_base, nullptr, nullptr,
                nullptr, n, stride, len, out);
}

int md5crc32hip_desc(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                     const uint32_t* d_order, uint64_t n, struct md5hip_md5crc32* d_out,
                     void* stream) {
  if (n == 0) return 0;
  if (int e = ready(d_base && d_offsets && d_lens && d_out && aligned(d_out, 16), (n + 63) / 64)) return e;
  return launch(md5crc32_desc_xdma16<false>, per_cu_grid(n), 768, 0, stream, d_base, d_offsets, d_lens,
                d_order, n, 0, 0, reinterpret_cast<Md5Crc32Record*>(d_out));
}

// Batched MD5Init / MD5Update / MD5Final on caller-owned contexts.
int md5hip_init_ctx(struct MD5Context* d_ctxs, uint64_t n, void* stream) {
  if (n == 0) return 0;
  const uint64_t g = (n + kBlock - 1) / kBlock;
  if (int e = ready(d_ctxs && aligned(d_ctxs, 4), g)) return e;
  return launch(md5_init_ctx, g, kBlock, 0, stream, reinterpret_cast<uint32_t*>(d_ctxs), n);
}

int md5hip_update_ctx(struct MD5Context* d_ctxs, const void* const* d_ptrs, const uint32_t* d_lens,
                      uint64_t n, void* stream) {
  if (n == 0) return 0;
  const uint64_t g = (n + 63) / 64;                   // one wave per 64 contexts
  if (int e = ready(d_ctxs && d_ptrs && d_lens && aligned(d_ctxs, 4), g)) return e;
  // few contexts: one update's chain bounds the launch; fed pairs shorten it
  const bool fed = md5hip_fed_fits(g);
  return launch(fed ? md5_update_ctx_fed : md5_update_ctx, g, fed ? 128 : 64, 0, stream,
                reinterpret_cast<uint32_t*>(d_ctxs), reinterpret_cast<const uint64_t*>(d_ptrs), d_lens, n);
}

int md5hip_final_ctx(struct MD5Context* d_ctxs, uint64_t n, unsigned char* d_digests, void* stream) {
  if (n == 0) return 0;
  const uint64_t g = (n + kBlock - 1) / kBlock;
  if (int e = ready(d_ctxs && d_digests && aligned(d_ctxs, 4) && aligned(d_digests, 16), g)) return e;
  return launch(md5_final_ctx, g, kBlock, 0, stream, reinterpret_cast<uint32_t*>(d_ctxs), n,
                reinterpret_cast<uint4*>(d_digests));
}

int md5hip_gather_launch(const struct md5hip_seg* d_segs, uint64_t nseg, unsigned char* d_dst,
                         void* stream) {
  static_assert(sizeof(md5hip_seg) == sizeof(GatherSeg), "segment layout");
  if (nseg == 0) return 0;
  return launch(gather_segments<4>, nseg < 65536 ? nseg : 65536, 256, 0, stream,
                reinterpret_cast<const GatherSeg*>(d_segs), nseg, d_dst);
}

int md5hip_fill_synthetic(void* d_dst, uint64_t nbytes, uint64_t seed, void* stream) {
  if (nbytes == 0) return 0;
  if (int e = ready(d_dst && (nbytes & 15u) == 0 && aligned(d_dst, 16))) return e;
  const uint64_t n16 = nbytes / 16;
  const uint64_t grid = (n16 + kBlock - 1) / kBlock;
  return launch(fill_synthetic, grid < 8192 ? grid : 8192, kBlock, 0, stream, (uint4*)d_dst, n16, seed);
}

int md5hip_order_device(const uint32_t* d_lens, uint64_t n, uint32_t kmax, uint32_t* d_next,
                        uint32_t* d_order, void* stream) {
  if (n == 0) return 0;
  const uint64_t g = (n + 255) / 256;
  if (int e = ready(d_lens && d_next && d_order && kmax <= MD5HIP_HIST_KMAX, g)) return e;
  return launch(order_scatter, g, 256, 0, stream, d_lens, n, kmax, d_next, d_order);
}

// ---------------------------------------------------------------------------
// Batch arenas: device memory whose virtual range is reserved with 1 GiB
// alignment (hipMemAddressReserve + hipMemCreate + hipMemMap), so the page
// tables can use large fragments throughout.  A lane-direct chain walks its
// own chunk, so a wave touches 64 distinct pages per load; HYBRID's long
// chains on C3 ran 9.7 ms in a 16 MiB-aligned buffer and 10.4-11.5 ms in a
// 2 MiB-aligned one (scripts/alloc_probe.py, deleted in 4de68d0).  The whole-line
// loaders are indifferent.
// ---------------------------------------------------------------------------
namespace {
struct Arena {
  void* ptr;       // mapped, kArenaAlign-aligned
  size_t size;
  void* base;      // the reservation (the runtime ignores a reservation's
  size_t rsize;    // alignment argument, so it is over-reserved by kArenaAlign)
  hipMemGenericAllocationHandle_t h;
  int device;
};
std::mutex g_arena_mu;
std::vector<Arena> g_arenas;
constexpr size_t kArenaAlign = size_t(1) << 30;
}  // namespace

int md5hip_arena_alloc(int device, uint64_t bytes, void** out) {
  if (!out || bytes == 0) return -EINVAL;
  *out = nullptr;
  hipMemAllocationProp prop = {};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended) !=
          hipSuccess || gran == 0)
    return -ENODEV;
  if (gran < (size_t(2) << 20)) gran = size_t(2) << 20;
  const size_t size = (size_t)((bytes + gran - 1) / gran * gran);
  void* base = nullptr;
  const size_t rsize = size + kArenaAlign;
  hipMemGenericAllocationHandle_t h{};
  if (hipMemAddressReserve(&base, rsize, kArenaAlign, nullptr, 0) != hipSuccess) return -ENOMEM;
  void* ptr = (void*)(((uintptr_t)base + kArenaAlign - 1) & ~(uintptr_t)(kArenaAlign - 1));
  if (hipMemCreate(&h, size, &prop, 0) != hipSuccess) {
    (void)hipMemAddressFree(base, rsize);
    return -ENOMEM;
  }
  hipMemAccessDesc acc = {};
  acc.location = prop.location;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  if (hipMemMap(ptr, size, 0, h, 0) != hipSuccess) {
    (void)hipMemRelease(h);
    (void)hipMemAddressFree(base, rsize);
    return -ENOMEM;
  }
  if (hipMemSetAccess(ptr, size, &acc, 1) != hipSuccess) {
    (void)hipMemUnmap(ptr, size);
    (void)hipMemRelease(h);
    (void)hipMemAddressFree(base, rsize);
    return -EIO;
  }
  {
    std::lock_guard<std::mutex> lk(g_arena_mu);
    g_arenas.push_back(Arena{ptr, size, base, rsize, h, device});
  }
  *out = ptr;
  return 0;
}

int md5hip_arena_free(void* ptr) {
  if (!ptr) return -EINVAL;
  Arena a{};
  {
    std::lock_guard<std::mutex> lk(g_arena_mu);
    size_t k = 0;
    while (k < g_arenas.size() && g_arenas[k].ptr != ptr) ++k;
    if (k == g_arenas.size()) return -ENOENT;
    a = g_arenas[k];
    g_arenas.erase(g_arenas.begin() + (long)k);
  }
  // Not stream-ordered like torch's allocator: a kernel still queued on any
  // stream of the device may read the arena, so drain the device before the
  // pages go (md5hip.h: freeing an arena synchronizes its device).
  int rc = 0, prev = -1;
  const bool had = hipGetDevice(&prev) == hipSuccess;
  if (hipSetDevice(a.device) != hipSuccess || hipDeviceSynchronize() != hipSuccess) rc = -EIO;
  if (hipMemUnmap(a.ptr, a.size) != hipSuccess) rc = -EIO;
  if (hipMemRelease(a.h) != hipSuccess) rc = -EIO;
  if (hipMemAddressFree(a.base, a.rsize) != hipSuccess) rc = -EIO;
  if (had) (void)hipSetDevice(prev);
  return rc;
}

// The stable longest-first order (ABI 5): rocPRIM's LSD radix sort of
// (kmax - key, chunk index) pairs, the key computed from the length as it is
// read (no key array), the index from a counting iterator; radix sort is
// stable, so equal keys keep chunk-index (= address) order -- exactly
// md5hip_plan_desc's host order.  order_scatter's wave-arrival order within a
// key cost a 6-batch C3 BALANCED launch 5-6 % against this order
// (profiles/r06d/, r06e/ order_ab.json).  Scratch: the sorted keys (4 n B,
// 256-B aligned) then rocPRIM's temporary storage.
}  // extern "C"

namespace {
struct BucketOf {
  uint32_t kmax;
  __host__ __device__ uint32_t operator()(uint32_t len) const {
    const uint32_t k = (len >> 6) + 1u;
    return k <= kmax ? kmax - k : kmax;        // a key past kmax: after every bucket
  }
};
unsigned sort_bits(uint32_t kmax) { return 32u - (unsigned)__builtin_clz(kmax | 1u); }
uint64_t keys_bytes(uint64_t n) { return (4 * n + 255) & ~255ull; }
hipError_t order_sort(void* temp, size_t& temp_bytes, const uint32_t* d_lens, uint32_t n, uint32_t kmax,
                      uint32_t* keys_out, uint32_t* d_order, hipStream_t s) {
  auto keys_in = rocprim::make_transform_iterator(d_lens, BucketOf{kmax});
  return rocprim::radix_sort_pairs(temp, temp_bytes, keys_in, keys_out, rocprim::counting_iterator<uint32_t>(0u),
                                   d_order, n, 0u, sort_bits(kmax), s);
}
}  // namespace

extern "C" {

uint64_t md5hip_order_stable_scratch(uint64_t n, uint32_t kmax) {
  if (n == 0) return 0;
  if (n > 0x7fffffffull || kmax > MD5HIP_HIST_KMAX) return 0;
  size_t temp = 0;
  if (order_sort(nullptr, temp, nullptr, (uint32_t)n, kmax ? kmax : MD5HIP_HIST_KMAX, nullptr, nullptr,
                 nullptr) != hipSuccess)
    return 0;
  return keys_bytes(n) + temp;
}

int md5hip_order_device_stable(const uint32_t* d_lens, uint64_t n, uint32_t kmax, void* d_scratch,
                               uint64_t scratch_bytes, uint32_t* d_order, void* stream) {
  if (n == 0) return 0;
  if (int e = ready(d_lens && d_order && d_scratch && kmax != 0 && kmax <= MD5HIP_HIST_KMAX &&
                    n <= 0x7fffffffull))
    return e;
  size_t temp = 0;
  if (order_sort(nullptr, temp, d_lens, (uint32_t)n, kmax, nullptr, d_order, (hipStream_t)stream) != hipSuccess)
    return -EINVAL;
  if (scratch_bytes < keys_bytes(n) + temp) return -ENOSPC;
  uint32_t* keys_out = (uint32_t*)d_scratch;
  void* tmp = (uint8_t*)d_scratch + keys_bytes(n);
  if (order_sort(tmp, temp, d_lens, (uint32_t)n, kmax, keys_out, d_order, (hipStream_t)stream) != hipSuccess)
    return -EIO;
  return launched();
}

// The one-pass kind with the kernel named.  (At the end of the file, so that
// md5crc32_fedsplit is the code object's last kernel and every other one
// keeps its place.)  FEDSPLIT: ceil(n/64) MD5 workgroups, then CRC workgroups
// of two waves, one chunk per wave, at most one per CU.
static uint64_t fedsplit_grid(uint64_t n) {
  const uint64_t half = (n + 1) / 2, cap = (uint64_t)md5hip_cu_count();
  return (n + 63) / 64 + (half < cap ? half : cap);
}

static int fedsplit_launch(const void* base, const uint64_t* offs, const uint32_t* lens,
                           const uint32_t* order, uint64_t n, uint64_t stride, uint32_t flen,
                           struct md5hip_md5crc32* d_out, void* stream) {
  return launch(offs ? md5crc32_fedsplit<false> : md5crc32_fedsplit<true>, fedsplit_grid(n), 128, 0, stream,
                base, offs, lens, order, n, stride, flen, reinterpret_cast<Md5Crc32Record*>(d_out));
}

static bool dual_variant_known(int v) { return v >= MD5CRC32HIP_AUTO && v < MD5CRC32HIP_NUM_VARIANTS; }

int md5crc32hip_fixed_variant(const void* d_base, uint64_t n, uint32_t len, uint64_t stride,
                              struct md5hip_md5crc32* d_out, void* stream, int variant) {
  if (n == 0) return 0;
  if (int e = ready(d_base && d_out && len <= stride && aligned(d_out, 16) && dual_variant_known(variant),
                    fedsplit_grid(n)))
    return e;
  if (variant == MD5CRC32HIP_AUTO)
    variant = aligned(d_base, 16) && (stride & 15u) == 0 && stride < (1ull << 31) / 64
                  ? md5crc32hip_plan(n, len)
                  : MD5CRC32HIP_XDMA16;
  if (variant == MD5CRC32HIP_FEDSPLIT)
    return fedsplit_launch(d_base, nullptr, nullptr, nullptr, n, stride, len, d_out, stream);
  return md5crc32hip_fixed(d_base, n, len, stride, d_out, stream);
}

int md5crc32hip_desc_variant(const void* d_base, const uint64_t* d_offsets, const uint32_t* d_lens,
                             const uint32_t* d_order, uint64_t n, struct md5hip_md5crc32* d_out,
                             void* stream, int variant) {
  if (n == 0) return 0;
  if (int e = ready(d_base && d_offsets && d_lens && d_out && aligned(d_out, 16) && dual_variant_known(variant),
                    fedsplit_grid(n)))
    return e;
  // AUTO: the lengths are on the device, so the caller names FEDSPLIT
  if (variant == MD5CRC32HIP_FEDSPLIT)
    return fedsplit_launch(d_base, d_offsets, d_lens, d_order, n, 0, 0, d_out, stream);
  return md5crc32hip_desc(d_base, d_offsets, d_lens, d_order, n, d_out, stream);
}

}  // extern "C"
