// launch_args.h -- bytes of each kernel argument, in order, by kernel name
// without its template arguments (sproxy_amd/csrc/md5_kernels.h has the
// signatures): hipLaunchKernel gets an array of pointers to the arguments and
// no sizes, so the recording runtime (fake_hip_rt.cc) cuts them by this table.
// A kernel that is not listed aborts the harness.  An argument of kPageBatch
// bytes is md5_pages.hip's PageBatch, passed by value: it is recorded field by
// field (pages, first, lens, order, page_bytes -- the 4 bytes of padding after
// page_bytes are not).  Test infrastructure.
#ifndef SPROXY_AMD_TESTS_LAUNCH_ARGS_H
#define SPROXY_AMD_TESTS_LAUNCH_ARGS_H

#include <string.h>

enum { kPageBatch = 40 };    // sizeof(PageBatch): four pointers, a uint32_t, padding

struct LaunchArgs {
  const char* kernel;
  int nargs;
  unsigned char size[9];
};

static const LaunchArgs kLaunchArgs[] = {
    // base, n, len, stride, out
    {"md5hip::md5_fixed_direct", 5, {8, 8, 4, 8, 8}},
    {"md5hip::md5_fixed_xdma1nt", 5, {8, 8, 4, 8, 8}},
    {"md5hip::crc32_fixed_xdma16", 5, {8, 8, 4, 8, 8}},
    {"md5hip::md5crc32_fixed_xdma16", 5, {8, 8, 4, 8, 8}},
    // base, offs, lens, order, n, stride, flen, out
    {"md5hip::md5_desc", 8, {8, 8, 8, 8, 8, 8, 4, 8}},
    {"md5hip::md5_desc_fed", 8, {8, 8, 8, 8, 8, 8, 4, 8}},
    {"md5hip::crc32_desc", 8, {8, 8, 8, 8, 8, 8, 4, 8}},
    {"md5hip::md5crc32_desc_xdma16", 8, {8, 8, 8, 8, 8, 8, 4, 8}},
    {"md5hip::md5crc32_fedsplit", 8, {8, 8, 8, 8, 8, 8, 4, 8}},
    // base, offs, lens, order, n, out
    {"md5hip::md5_desc_xdma", 6, {8, 8, 8, 8, 8, 8}},
    {"md5hip::md5_desc_lines", 6, {8, 8, 8, 8, 8, 8}},
    {"md5hip::crc32_desc_xdma16", 6, {8, 8, 8, 8, 8, 8}},
    // ... out, nlong / ... out, ctr
    {"md5hip::md5_desc_hybrid", 7, {8, 8, 8, 8, 8, 8, 4}},
    {"md5hip::md5_desc_balanced_t", 7, {8, 8, 8, 8, 8, 8, 8}},
    // base, offs, lens, n, stride, flen, F, out
    {"md5hip::crc32_fast_xdma16", 8, {8, 8, 8, 8, 8, 4, 4, 8}},
    {"md5hip::crc32_fast_pipe", 8, {8, 8, 8, 8, 8, 4, 4, 8}},
    // base, offs, lens, order, n, stride, flen, F, out
    {"md5hip::crc32_split", 9, {8, 8, 8, 8, 8, 8, 4, 4, 8}},
    // ctxs, ptrs, lens, n / ctxs, n, digests / ctxs, n
    {"md5hip::md5_update_ctx", 4, {8, 8, 8, 8}},
    {"md5hip::md5_update_ctx_fed", 4, {8, 8, 8, 8}},
    {"md5hip::md5_final_ctx", 3, {8, 8, 8}},
    {"md5hip::md5_init_ctx", 2, {8, 8}},
    // lens, n, kmax, next, order
    {"md5hip::order_scatter", 5, {8, 8, 4, 8, 8}},
    // segs, nseg, dst / dst, n16, seed
    {"md5hip::gather_segments", 3, {8, 8, 8}},
    {"md5hip::fill_synthetic", 3, {8, 8, 8}},
    // md5_pages.hip (an unnamed namespace, fake_hip_rt.cc's short_name): pb, n, out
    {"md5_pages_xdma", 3, {kPageBatch, 8, 8}},
    {"pages_xdma16", 3, {kPageBatch, 8, 8}},
    // pb, n, F, out / ctxs, pb, n
    {"crc32_pages_fast", 4, {kPageBatch, 8, 4, 8}},
    {"md5_update_ctx_pages", 3, {8, kPageBatch, 8}},
};

// `name` may carry template arguments: "md5hip::md5_desc_fed<true>"
static inline const LaunchArgs* launch_args_of(const char* name) {
  const size_t len = strcspn(name, "<");
  for (const LaunchArgs& a : kLaunchArgs)
    if (strlen(a.kernel) == len && memcmp(a.kernel, name, len) == 0) return &a;
  return nullptr;
}

#endif
