// md5_verify.hip -- the digest-compare kernel and its two launchers: the
// public md5hip_digest_compare (include/md5hip.h) and the batcher's table form
// md5hip_compare_launch (md5_internal.h).  A translation unit of its own,
// linked after md5_kernels.o: the hash kernels' code object stays the first
// gfx950 bundle of the library.
#define MD5HIP_DEFINES_COMPARE   // the table launcher is defined here (md5_internal.h)
#include <errno.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "../../include/md5hip.h"
#include "md5_internal.h"

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kWaves = kBlock / 64;

// One workgroup per range: entry blockIdx.x of `tab`, or (tab == nullptr)
// piece blockIdx.x of `one`, MD5HIP_CMP_PIECE records long.  A lane compares
// one record per trip: its wsz bytes at goff against want i, words of 4 bytes
// (the record side is 4-B aligned by contract; the want side is read by
// bytes when it is not).  Mismatches are counted per wave from a 64-bit
// ballot, summed over the workgroup's waves in LDS, and leave as ONE store
// (a table range owns its count) or ONE atomic add (the public entry's
// pieces share *d_nbad).
__global__ __launch_bounds__(kBlock) void digest_compare(const uint8_t* __restrict__ got, uint32_t gsz,
                                                         const md5hip_cmp* __restrict__ tab, md5hip_cmp one) {
  __shared__ uint32_t wave_bad[kWaves];
  const md5hip_cmp e = tab ? tab[blockIdx.x] : one;
  const uint64_t lo = tab ? 0 : (uint64_t)blockIdx.x * MD5HIP_CMP_PIECE;
  const uint64_t hi = tab ? e.count : (e.count - lo < MD5HIP_CMP_PIECE ? e.count : lo + MD5HIP_CMP_PIECE);
  const uint8_t* want = (const uint8_t*)(uintptr_t)e.want;
  uint8_t* ok = (uint8_t*)(uintptr_t)e.ok;
  const uint32_t words = e.wsz >> 2;
  const bool want_words = ((e.want | e.wsz) & 3u) == 0;   // wsz is a multiple of 4: every want i then is
  uint32_t bad = 0;                                       // the wave's mismatches (the same in every lane)
  for (uint64_t base = lo; base < hi; base += kBlock) {   // uniform trips: every lane reaches the ballot
    const uint64_t i = base + threadIdx.x;
    bool mis = false;
    if (i < hi) {
      const uint32_t* g = (const uint32_t*)(got + (size_t)gsz * (e.first + i) + e.goff);
      const uint8_t* w = want + (size_t)e.wsz * i;
      uint32_t diff = 0;
      for (uint32_t k = 0; k < words; k++) {
        const uint32_t wv = want_words ? ((const uint32_t*)w)[k]
                                       : (uint32_t)w[4 * k] | (uint32_t)w[4 * k + 1] << 8 |
                                             (uint32_t)w[4 * k + 2] << 16 | (uint32_t)w[4 * k + 3] << 24;
        diff |= g[k] ^ wv;
      }
      mis = diff != 0;
      ok[i] = mis ? 0 : 1;
    }
    bad += (uint32_t)__popcll(__ballot(mis));
  }
  if ((threadIdx.x & 63u) == 0) wave_bad[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0 && e.cnt) {
    uint64_t total = 0;
    for (uint32_t w = 0; w < kWaves; w++) total += wave_bad[w];
    unsigned long long* cnt = (unsigned long long*)(uintptr_t)e.cnt;
    if (tab) *cnt = total;
    else if (total) atomicAdd(cnt, (unsigned long long)total);
  }
}

bool shape_ok(uint32_t gsz, uint32_t goff, uint32_t wsz) {
  return (gsz == 4 || gsz == 16 || gsz == 32) && wsz != 0 && (goff & 3u) == 0 && (wsz & 3u) == 0 &&
         (uint64_t)goff + wsz <= gsz;
}

bool got_ok(const void* d_got, uint32_t gsz) {
  return d_got && ((uintptr_t)d_got & ((gsz < 16 ? gsz : 16u) - 1)) == 0;
}

int launch(const void* d_got, uint32_t gsz, const md5hip_cmp* d_tab, const md5hip_cmp& one, uint64_t grid,
           void* stream) {
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -ENODEV;
  if (grid > 0x7fffffffull) return -EINVAL;
  hipLaunchKernelGGL(digest_compare, dim3((uint32_t)grid), dim3(kBlock), 0, (hipStream_t)stream,
                     (const uint8_t*)d_got, gsz, d_tab, one);
  return hipGetLastError() == hipSuccess ? 0 : -EIO;
}

}  // namespace

extern "C" int md5hip_digest_compare(const void* d_got, uint32_t gsz, uint32_t goff, uint32_t wsz,
                                     const void* d_want, uint64_t n, unsigned char* d_ok, uint64_t* d_nbad,
                                     void* stream) {
  if (n == 0) return 0;
  if (!shape_ok(gsz, goff, wsz) || !got_ok(d_got, gsz) || !d_want || !d_ok || ((uintptr_t)d_nbad & 7u)) return -EINVAL;
  const md5hip_cmp one = {0, n, (uint64_t)(uintptr_t)d_want, (uint64_t)(uintptr_t)d_ok,
                          (uint64_t)(uintptr_t)d_nbad, goff, wsz};
  return launch(d_got, gsz, nullptr, one, (n + MD5HIP_CMP_PIECE - 1) / MD5HIP_CMP_PIECE, stream);
}

// The entries' shapes are the batcher's own (checked where a submission is
// taken); here only what the launch itself needs.
extern "C" int md5hip_compare_launch(const void* d_got, uint32_t gsz, const struct md5hip_cmp* d_tab, uint64_t nent,
                                     void* stream) {
  if (nent == 0) return 0;
  if (!(gsz == 4 || gsz == 16 || gsz == 32) || !got_ok(d_got, gsz) || !d_tab) return -EINVAL;
  return launch(d_got, gsz, d_tab, md5hip_cmp{}, nent, stream);
}
