// md5_pages.hip -- digests of device-resident chunks laid out as page lists
// (md5hip_digest_pages, include/md5hip.h): a chunk is a run of entries of a
// page table, each the device address of a page of page_bytes, as netcache
// keeps a block (nc_page_ctrl_t lists).  The pages are hashed where they lie.
// Also blk_make_crc's fastcrc windows over such lists (crc32hip_pages), of
// which only the windows' bytes are read, and MD5Update on caller-owned
// contexts from such lists (md5hip_update_ctx_pages).
// A translation unit of its own, linked after md5_kernels.o and md5_verify.o:
// the hash kernels' code object stays the first gfx950 bundle of the library,
// byte for byte.
//
// The loaders and hashers are md5_kernels.h's.  That header also defines the
// library's kernels, which md5_kernels.o already holds under their external
// names: here it is included inside an unnamed namespace, so nothing of it
// clashes at link time.  The host side of this object emits none of those
// kernels (unused, internal linkage); its code object carries unreachable
// copies of the non-template ones, which cost file size and nothing else.
#define MD5HIP_DEFINES_PAGES   // the launcher is defined here (md5_internal.h)
#include <errno.h>
#include <stdint.h>

#include <type_traits>
#include <utility>

#include <hip/hip_runtime.h>

#include "../../include/md5hip.h"
#include "md5_internal.h"

namespace {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"   // the kernels this object does not launch
#include "md5_kernels.h"
#pragma clang diagnostic pop

using namespace md5hip;

// A paged batch: chunk c = order ? order[i] : i has lens[c] bytes, byte k of
// it being byte k % page_bytes of the page at pages[first[c] + k / page_bytes].
struct PageBatch {
  const uint64_t* __restrict__ pages;
  const uint64_t* __restrict__ first;
  const uint32_t* __restrict__ lens;
  const uint32_t* __restrict__ order;
  uint32_t page_bytes;                 // a multiple of 128
};

// pages_group: one wave hashes the 64-chunk group whose first position in
// `order` is `first` (< n); the hasher is set up by the caller.  The wave
// walks the page index p up to its largest page count.  Page p of every lane
// that still has one is a row of an LDS-DMA image (row_set<true>: per-row
// 64-bit addresses), loaded 128-B stage by stage with the hasher state
// carried over from page p - 1 (run_stages); lanes whose chunk ended on an
// earlier page, dead lanes and empty chunks have no stage and alias the
// wave's longest row.  A page index at which some lane's page is off the
// 16-B grid is hashed lane-direct instead, each lane its own page.  What is
// left after a lane's last page -- an odd 64-B block, then len % 64 bytes,
// both inside that page -- is finished as in desc_xpose_group.
//
// A lane reads only the table entries [first[c], first[c] + ceil(len / page_bytes))
// of its own chunk, and of a page only whole 128-B stages and 64-B blocks
// that hold chunk bytes, then (load_tail) the 16-B granules up to the one
// holding the chunk's last byte.
template <class H>
__device__ __forceinline__ void pages_group(H& h, const PageBatch& pb, uint64_t n, uint64_t first,
                                            typename H::Out* __restrict__ out, uint8_t* img) {
  const uint64_t i = first + (threadIdx.x & 63u);
  const bool live = i < n;
  const uint64_t c = live ? (pb.order ? (uint64_t)pb.order[i] : i) : 0;
  const uint32_t len = live ? pb.lens[c] : 0u;
  const uint64_t pf = live ? pb.first[c] : 0;
  const uint32_t P = pb.page_bytes;
  const uint32_t np = (uint32_t)(((uint64_t)len + P - 1u) / P);   // this lane's pages
  const uint32_t pmax = wave_max(np);
  chain_prio(wave_max(len >> 6));
  typename H::State st = h.init();
  uint64_t last = 0;                   // this lane's last page
  uint32_t lastb = 0;                  // and the chunk's bytes in it
  // the entry of page p is asked for one page ahead, so its round trip runs
  // under page p - 1's stages
  uint64_t next = np ? pb.pages[pf] : 0;
  for (uint32_t p = 0; p < pmax; ++p) {
    const bool own = p < np;
    const uint64_t addr = next;
    next = p + 1u < np ? pb.pages[pf + p + 1u] : 0;
    const uint64_t rest = own ? (uint64_t)len - (uint64_t)p * P : 0;
    const uint32_t bytes = rest < P ? (uint32_t)rest : P;          // of the chunk in page p
    const uint32_t nst = bytes >> 7;                               // whole 128-B stages
    if (own && p + 1u == np) {
      last = addr;
      lastb = bytes;
    }
    if (__ballot(own && ((uint32_t)addr & 15u) != 0) != 0) {
      // some page off the 16-B grid: every lane its own page, the same blocks
      if (nst) {
        const uint8_t* page = reinterpret_cast<const uint8_t*>((uintptr_t)addr);
        if (((uint32_t)addr & 15u) == 0) {
          ring_range<H, 2, false>(h, st, reinterpret_cast<const uint4*>(page), 2u * nst);
        } else {
          for (uint32_t blk = 0; blk < 2u * nst; ++blk) {
            uint4 w[4];
            load_block_unaligned(w, page + ((uint64_t)blk << 6));
            h.block(st, w);
          }
        }
      }
      continue;
    }
    const uint32_t smax = wave_max(nst);
    if (smax == 0) continue;           // remainders only: finished below
    // nt only when every row of the page starts on a 128-B line (otherwise a
    // stage shares a line with the row's next one, which must stay in L2)
    const bool lined = __ballot(nst != 0 && ((uint32_t)addr & 127u) != 0) == 0;
    const RowSet rs = row_set<true>(nullptr, addr, nst, smax, img);
    if (lined) run_stages<2>(h, st, rs);
    else run_stages<0>(h, st, rs);
  }
  if (live) {
    const uint8_t* page = reinterpret_cast<const uint8_t*>((uintptr_t)last);
    const uint32_t nfull = lastb >> 6;
    if (nfull & 1u) {
      uint4 w[4];
      const uint8_t* blk = page + ((uint64_t)(nfull - 1u) << 6);
      if (((uint32_t)last & 15u) == 0) load_block(w, reinterpret_cast<const uint4*>(blk));
      else load_block_unaligned(w, blk);
      h.block(st, w);
    }
    h.finish(st, page + ((uint64_t)nfull << 6), len & 63u, len);
    h.store(out, c, st);
  }
}

// MD5: one wave per workgroup with its 8 KiB image, held at 4 waves per SIMD
// by the register file, as md5_desc_xdma.
__global__ void __launch_bounds__(64)
md5_pages_xdma(PageBatch pb, uint64_t n, uint4* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t img[8192];
  asm volatile("" ::: "v127");
  Md5Hasher<true> h;
  const uint64_t first = (uint64_t)blockIdx.x * 64u;
  if (first >= n) return;
  pages_group(h, pb, n, first, out, img);
}

// CRC-32 of the whole chunk, and MD5 + CRC-32 in one pass: XDMA16's frame,
// the 64 KiB tables beside twelve waves' images, one workgroup per CU.
template <class H>
__global__ void __launch_bounds__(768)
pages_xdma16(PageBatch pb, uint64_t n, typename H::Out* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[kXdma16Lds<H>];
  xdma16_frame<H>(lds, n, [&](auto& h, uint64_t first, uint8_t* img) __attribute__((always_inline)) {
    pages_group(h, pb, n, first, out, img);
  });
}

// ---------------------------------------------------------------------------
// blk_make_crc's fastcrc windows (blk_io.c:408-424) over page lists
// (crc32hip_pages): crcs[k] = CRC(first F bytes) ^ CRC(last F bytes) of chunk
// k, the whole chunk's CRC when it has at most F bytes.  The rows are
// FastWindows': row 2k = chunk k's head window, row 2k + 1 its tail window
// (empty for a chunk of <= F bytes: CRC 0, the XOR identity), lanes 2k and
// 2k + 1 combine.  crc32_fast_pipe's frame: the perm tables alone in LDS,
// sixteen waves per CU, persistent, groups wave-major; the next group's
// windows are loaded into VGPRs before the current group is hashed.
// ---------------------------------------------------------------------------
// A lane's window: `len` bytes from `at`, which lies `room` bytes before the
// end of its page, entry `ent` of the table; what does not fit goes on at
// byte 0 of entries ent + 1, ...  Neither `at` nor `ent` means anything when
// len == 0, and no table entry is read for such a row.
struct PageWin {
  const uint8_t* at;
  uint64_t ent;
  uint32_t room, len;
  bool live;
  bool pipe;           // wave-uniform: every live row is F bytes inside one page on the 16-B grid
};

__device__ __forceinline__ PageWin page_window(const PageBatch& pb, uint64_t rows, uint64_t gi, uint32_t F,
                                               bool pipeF) {
  PageWin w;
  const uint64_t i = gi * 64u + (threadIdx.x & 63u);
  w.live = i < rows;
  const uint64_t k = i >> 1;
  const uint32_t L = w.live ? pb.lens[k] : 0u;
  const bool tail = (i & 1u) != 0;
  w.len = L <= F ? (tail ? 0u : L) : F;
  const uint32_t start = tail && L > F ? L - F : 0u;     // the window's first byte in its chunk
  const uint32_t P = pb.page_bytes;
  const uint32_t e = start / P, q = start - e * P;
  w.room = P - q;
  w.ent = 0;
  uint64_t addr = 0;
  if (w.len) {
    w.ent = pb.first[k] + e;
    addr = pb.pages[w.ent] + q;
  }
  const bool simple = !w.live || (w.len == F && F <= w.room && ((uint32_t)addr & 15u) == 0);
  w.pipe = pipeF && __ballot(!simple) == 0;
  // dead lanes of a pipelined group load the group's first window (row 0 is
  // live, and simple there)
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)addr, 0, 64);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(addr >> 32), 0, 64);
  if (!w.live) addr = ((uint64_t)hi << 32) | lo;
  w.at = reinterpret_cast<const uint8_t*>((uintptr_t)addr);
  return w;
}

// A window of any shape by its own lane: page by page, each piece hashed and
// finished by lane_range (any alignment; of a piece only the 64-B blocks, and
// then the 16-B or 4-B granules, that hold its bytes are read).  CRC-32 runs
// over a byte stream, so a piece may end anywhere: finish's complement is
// taken back, and the raw register goes on into the next page.
__device__ __forceinline__ void page_window_lane(Crc32PermHasher& h, Crc32State& st, const PageBatch& pb,
                                                 const PageWin& w) {
  const uint8_t* p = w.at;
  uint64_t ent = w.ent;
  uint32_t left = w.len, room = w.room;
  for (;;) {
    const uint32_t piece = left < room ? left : room;
    lane_range<Crc32PermHasher, 2>(h, st, p, piece);
    left -= piece;
    if (left == 0) break;
    st.c = ~st.c;
    p = reinterpret_cast<const uint8_t*>((uintptr_t)pb.pages[++ent]);
    room = pb.page_bytes;
  }
}

// The ring of loaded groups is fast_pipe_body's, written out here: that body
// hashes FastWindows rows, one address each, where a row of a paged batch may
// be several pieces, and it stays as md5_kernels.o compiled it.
__global__ void __launch_bounds__(1024)
crc32_pages_fast(PageBatch pb, uint64_t n, uint32_t F, uint32_t* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[Crc32PermHasher::kLdsBytes];
  constexpr int D = 2;                                    // window groups in flight per wave
  Crc32PermHasher h;
  h.setup(lds);
  const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint64_t rows = 2 * n;
  const uint64_t ngroups = (rows + 63) / 64;
  const uint64_t step = (uint64_t)gridDim.x * (blockDim.x >> 6);
  const bool pipeF = F == 64u || F == 128u;               // windows of one or two whole blocks
  const uint32_t nb = F >> 6;
  auto fetch = [&](const PageWin& w, uint4 (&W)[2][4]) __attribute__((always_inline)) {
    const uint4* q = reinterpret_cast<const uint4*>(w.at);
    if (nb == 2) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {      // a line's halves in alternating instructions (fast_pipe_body)
        W[0][k] = ld16(q + k);
        __builtin_amdgcn_sched_barrier(0);
        W[1][k] = ld16(q + 4 + k);
        __builtin_amdgcn_sched_barrier(0);
      }
    } else {
      load_block(W[0], q);
    }
  };
  auto hash = [&](const PageWin& w, uint64_t gi, uint4 (&W)[2][4]) __attribute__((always_inline)) {
    Crc32State st = h.init();
    if (w.pipe) {
      h.block(st, W[0]);
      if (nb == 2) h.block(st, W[1]);
      h.finish(st, w.at, 0u, F);
    } else if (w.live) {
      // placed again: a window's table entry and room in its page are not
      // kept in flight beside the loaded group (VGPRs: 128 at 16 waves per CU)
      page_window_lane(h, st, pb, page_window(pb, rows, gi, F, pipeF));
    }
    if (w.live) {                        // pairs are live together
      const uint64_t i = gi * 64u + (threadIdx.x & 63u);
      const uint32_t v = st.c ^ (uint32_t)__shfl_xor((int)st.c, 1, 64);
      if (!(i & 1u)) out[i >> 1] = v;
    }
  };
  uint64_t g0 = (uint64_t)wave * gridDim.x + blockIdx.x;
  if (g0 >= ngroups) return;
  uint4 buf[D][2][4];
  PageWin win[D];
#pragma unroll
  for (int j = 0; j < D - 1; ++j) {
    const uint64_t g = g0 + (uint64_t)j * step;
    win[j] = PageWin{};
    if (g < ngroups) {
      win[j] = page_window(pb, rows, g, F, pipeF);
      if (win[j].pipe) fetch(win[j], buf[j]);
    }
  }
  for (;;) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      const int pj = (j + D - 1) % D;                   // the slot freed one group ago
      const uint64_t gp = g0 + (uint64_t)(j + D - 1) * step;
      win[pj] = PageWin{};
      if (gp < ngroups) {
        win[pj] = page_window(pb, rows, gp, F, pipeF);
        if (win[pj].pipe) fetch(win[pj], buf[pj]);
      }
      const uint64_t g = g0 + (uint64_t)j * step;
      if (g < ngroups) hash(win[j], g, buf[j]);
    }
    g0 += (uint64_t)D * step;
    if (g0 >= ngroups) break;
  }
}

// ---------------------------------------------------------------------------
// MD5Update on caller-owned contexts over page lists (md5hip_update_ctx_pages):
// context i takes chunk i of a paged batch as md5.c:169-215 takes a buffer,
// all 88 bytes of it left as MD5Update leaves them (md5_kernels.h, "MD5Update
// / MD5Final on caller-owned contexts").  One wave per 64 contexts, a context's
// index its lane; a group takes one of two routes, wave-uniformly.
//
// Loader: no lane that gets bytes has any pending (t == 0 wherever len > 0).
// The lanes' 64-B blocks are then the pages' own, and pages_group walks them
// as it does for a digest -- LDS-DMA stages, a page index with a page off the
// 16-B grid lane by lane -- from each lane's own buf[] and with nothing
// appended (CtxHasher).  Across the walk a lane holds its state and what
// pages_group holds; bits[] and in[] are read and built after it.
//
// Lane: some lane has pending bytes, so its blocks sit 64 - t bytes into the
// stream and one a page straddles two pages.  Every lane walks its own byte
// stream, block by block; a straddling block is put together from its two
// pages byte by byte (put_bytes).  Correct, slower.
// ---------------------------------------------------------------------------
// pages_group's finish is handed where the walk ended -- the first byte after
// the last whole block of the lane's last page -- and keeps it for the tail.
struct CtxPagesHasher : CtxHasher {
  const uint8_t* tail;
  __device__ __forceinline__ void finish(State&, const uint8_t* t, uint32_t, uint64_t) { tail = t; }
};

__device__ __forceinline__ void block_words(uint32_t (&w)[16], const uint8_t* p) {
  uint4 v[4];
  if (((uintptr_t)p & 15u) == 0) load_block(v, reinterpret_cast<const uint4*>(p));
  else load_block_unaligned(v, p);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w[4 * k] = v[k].x; w[4 * k + 1] = v[k].y;
    w[4 * k + 2] = v[k].z; w[4 * k + 3] = v[k].w;
  }
}

// Word j of in[] as md5.c:214 leaves it: the r tail bytes (tw), then the bytes
// of `keep` -- the last block compressed, or in[] as it was.
__device__ __forceinline__ uint32_t in_word(uint32_t tw, uint32_t keep, uint32_t r, int j) {
  const uint32_t m = tail_mask((int)r - 4 * j);
  return (tw & m) | (keep & ~m);
}

// The lane route for one context with len > 0: buf and in[] of the context
// at cp (the caller advances the bit count).  The stream position is (e, q):
// byte q < P of the chunk's table entry e.  An entry is read only when a byte
// of it is.
__device__ __forceinline__ void ctx_pages_lane(uint32_t* __restrict__ cp, const PageBatch& pb, uint64_t pf,
                                               uint32_t len, const CtxSpan& sp) {
  const uint32_t P = pb.page_bytes;
  auto page = [&](uint32_t e) __attribute__((always_inline)) {
    return reinterpret_cast<const uint8_t*>((uintptr_t)pb.pages[pf + e]);
  };
  uint32_t keep[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) keep[j] = cp[6 + j];
  if (sp.append_only) {                                // md5.c:189-192; t + len < 64 <= P: one page
    put_bytes(keep, sp.t, page(0), len);
#pragma unroll
    for (int j = 0; j < 16; ++j) cp[6 + j] = keep[j];
    return;
  }
  State st{cp[0], cp[1], cp[2], cp[3]};
  if (sp.t) {                                          // md5.c:194-199: complete the pending block
    put_bytes(keep, sp.t, page(0), 64u - sp.t);
    compress<true>(st, [&](int k) __attribute__((always_inline)) { return keep[k]; });
  }
  uint32_t e = 0, q = sp.pos;                          // pos < 64 <= P
  uint32_t w[16];
  for (uint32_t b = 0; b < sp.nblk; ++b) {
    if (q + 64u <= P) {
      block_words(w, page(e) + q);
    } else {                                           // P - q bytes end page e, the rest start page e + 1
#pragma unroll
      for (int j = 0; j < 16; ++j) w[j] = 0u;
      put_bytes(w, 0u, page(e) + q, P - q);
      put_bytes(w, P - q, page(e + 1u), 64u - (P - q));
    }
    compress<true>(st, [&](int k) __attribute__((always_inline)) { return w[k]; });
    q += 64u;
    if (q >= P) {
      q -= P;
      ++e;
    }
  }
  if (sp.nblk) {
#pragma unroll
    for (int j = 0; j < 16; ++j) keep[j] = w[j];
  }
  const uint32_t r = len - sp.pos - (sp.nblk << 6);    // md5.c:214: memcpy(in, buf, r)
  uint32_t tw[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) tw[j] = 0u;
  if (r) {
    const uint32_t c1 = r < P - q ? r : P - q;
    put_bytes(tw, 0u, page(e) + q, c1);
    if (r > c1) put_bytes(tw, c1, page(e + 1u), r - c1);
  }
#pragma unroll
  for (int j = 0; j < 16; ++j) cp[6 + j] = in_word(tw[j], keep[j], r, j);
  cp[0] = st.a; cp[1] = st.b; cp[2] = st.c; cp[3] = st.d;
}

// One-wave workgroups with the loader's 8 KiB image, held at 4 waves per SIMD
// by the register file, as md5_pages_xdma and md5_update_ctx.
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4)))
md5_update_ctx_pages(uint32_t* __restrict__ ctxs, PageBatch pb, uint64_t n) {
  __shared__ __attribute__((aligned(16))) uint8_t img[8192];
  asm volatile("" ::: "v127");
  const uint64_t first = (uint64_t)blockIdx.x * 64u;
  if (first >= n) return;
  const uint64_t i = first + (threadIdx.x & 63u);
  const bool live = i < n;
  uint32_t* cp = ctxs + 22 * (live ? i : first);
  const uint32_t len = live ? pb.lens[i] : 0u;
  const uint32_t t0 = cp[4];
  const CtxSpan sp = ctx_span(t0, len);
  const uint32_t lo = t0 + (len << 3);                 // md5.c:179-182
  const uint32_t carry = (lo < t0 ? 1u : 0u) + (len >> 29);
  if (__ballot(len != 0 && sp.t != 0) != 0) {          // wave-uniform: the lane route
    if (len == 0) return;                              // no update: the context is not written
    ctx_pages_lane(cp, pb, pb.first[i], len, sp);
    cp[4] = lo;
    cp[5] += carry;
    return;
  }
  CtxPagesHasher h;
  h.s0 = State{cp[0], cp[1], cp[2], cp[3]};
  h.res = h.s0;
  h.tail = nullptr;
  pages_group(h, pb, n, first, static_cast<uint4*>(nullptr), img);
  if (len == 0) return;
  // t == 0: len >> 6 blocks were compressed, and len & 63 bytes are left at
  // h.tail.  The last block compressed ends there, unless the last page holds
  // fewer than 64 bytes (len = kP + 1 .. kP + 63): then it ends the page
  // before, whose table entry is read a second time.
  const uint32_t P = pb.page_bytes, r = len & 63u;
  uint32_t keep[16];
  if (len < 64u) {
#pragma unroll
    for (int j = 0; j < 16; ++j) keep[j] = cp[6 + j];
  } else {
    const uint32_t np = (uint32_t)(((uint64_t)len + P - 1u) / P);
    const uint32_t lastb = len - (np - 1u) * P;        // the chunk's bytes in its last page
    const uint8_t* blk = h.tail - 64;
    if (lastb < 64u) blk = reinterpret_cast<const uint8_t*>((uintptr_t)pb.pages[pb.first[i] + np - 2u]) + (P - 64u);
    block_words(keep, blk);
  }
  uint32_t tw[16];
  load_tail(h.tail, r, tw);
#pragma unroll
  for (int j = 0; j < 16; ++j) cp[6 + j] = in_word(tw[j], keep[j], r, j);
  cp[0] = h.res.a; cp[1] = h.res.b; cp[2] = h.res.c; cp[3] = h.res.d;
  cp[4] = lo;
  cp[5] += carry;
}

template <typename... P, typename... A>
int launch(void (*kern)(P...), uint64_t grid, uint32_t block, void* stream, A... args) {
  hipLaunchKernelGGL(kern, dim3((uint32_t)grid), dim3(block), 0, (hipStream_t)stream, static_cast<P>(args)...);
  return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

}  // namespace

extern "C" int md5hip_digest_pages(int kind, const uint64_t* d_pages, const uint64_t* d_first,
                                   const uint32_t* d_lens, const uint32_t* d_order, uint64_t n,
                                   uint32_t page_bytes, void* d_out, void* stream) {
  static_assert(sizeof(md5hip_md5crc32) == sizeof(Md5Crc32Record), "record layout");
  const bool known = kind == MD5HIP_DIGEST_MD5 || kind == MD5HIP_DIGEST_CRC32 || kind == MD5HIP_DIGEST_MD5_CRC32;
  if (n == 0) return 0;
  if (!known) return -EINVAL;
  const uintptr_t align = kind == MD5HIP_DIGEST_CRC32 ? 4 : 16;
  if (!d_pages || !d_first || !d_lens || !d_out || ((uintptr_t)d_out & (align - 1)) || page_bytes == 0 ||
      (page_bytes & 127u) || page_bytes > MD5HIP_PAGE_BYTES_MAX)
    return -EINVAL;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -ENODEV;
  const uint64_t groups = (n + 63) / 64;
  if (groups > 0x7fffffffull) return -EINVAL;
  const PageBatch pb{d_pages, d_first, d_lens, d_order, page_bytes};
  if (kind == MD5HIP_DIGEST_MD5) return launch(md5_pages_xdma, groups, 64, stream, pb, n, (uint4*)d_out);
  // one 768-thread workgroup per CU, grid-stride over the groups
  const uint64_t cus = (uint64_t)md5hip_cu_count();
  const uint64_t grid = groups < cus ? groups : cus;
  if (kind == MD5HIP_DIGEST_CRC32)
    return launch(pages_xdma16<Crc32PermHasher>, grid, 768, stream, pb, n, (uint32_t*)d_out);
  return launch(pages_xdma16<Md5Crc32Hasher>, grid, 768, stream, pb, n, (Md5Crc32Record*)d_out);
}

extern "C" int crc32hip_pages(const uint64_t* d_pages, const uint64_t* d_first, const uint32_t* d_lens,
                              const uint32_t* d_order, uint64_t n, uint32_t page_bytes, uint32_t fastcrc,
                              uint32_t* d_crcs, void* stream) {
  // whole chunks: the paged CRC-32 kernel itself
  if (fastcrc == 0)
    return md5hip_digest_pages(MD5HIP_DIGEST_CRC32, d_pages, d_first, d_lens, d_order, n, page_bytes, d_crcs, stream);
  if (n == 0) return 0;
  if (!d_pages || !d_first || !d_lens || !d_crcs || ((uintptr_t)d_crcs & 3u) || (fastcrc & 3u) || page_bytes == 0 ||
      (page_bytes & 127u) || page_bytes > MD5HIP_PAGE_BYTES_MAX)
    return -EINVAL;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -ENODEV;
  const uint64_t groups = (n + 31) / 32;                 // 64 window rows each
  if (groups > 0x7fffffffull) return -EINVAL;
  // every window is fastcrc bytes (or the whole of a shorter chunk) whatever
  // the order, and crcs[k] is chunk k's: d_order changes nothing, and is not read
  const PageBatch pb{d_pages, d_first, d_lens, nullptr, page_bytes};
  const uint64_t cus = (uint64_t)md5hip_cu_count();
  return launch(crc32_pages_fast, groups < cus ? groups : cus, 1024, stream, pb, n, fastcrc, d_crcs);
}

extern "C" int md5hip_update_ctx_pages(struct MD5Context* d_ctxs, const uint64_t* d_pages, const uint64_t* d_first,
                                       const uint32_t* d_lens, uint64_t n, uint32_t page_bytes, void* stream) {
  if (n == 0) return 0;
  const uint64_t groups = (n + 63) / 64;                 // one wave per 64 contexts
  if (!d_ctxs || !d_pages || !d_first || !d_lens || ((uintptr_t)d_ctxs & 3u) || page_bytes == 0 ||
      (page_bytes & 127u) || page_bytes > MD5HIP_PAGE_BYTES_MAX || groups > 0x7fffffffull)
    return -EINVAL;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -ENODEV;
  const PageBatch pb{d_pages, d_first, d_lens, nullptr, page_bytes};
  return launch(md5_update_ctx_pages, groups, 64, stream, reinterpret_cast<uint32_t*>(d_ctxs), pb, n);
}
