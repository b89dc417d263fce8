// launch_check.cc -- TEST INFRASTRUCTURE: calls the real launchers of
// sproxy_amd/csrc/md5_kernels.hip and md5_pages.hip (build/obj/md5_kernels.o
// and md5_pages.o, with md5_plan.o) over the recording runtime tests/c/fake_hip_rt.cc and prints what each call
// launched.  No GPU, no libamdhip64: no kernel runs, so the pointers are
// whatever numbers the case gives (the launchers test them for NULL and
// alignment and never read through them).
//
// One case per line of stdin, all numbers in C notation (0x.., decimal):
//   <id> <device> <cus> <entry> <argument> ...
// with the entry's arguments in the order of include/md5hip.h, the stream
// included.  The launchers cache the CU count, the dynamic-LDS attribute and
// BALANCED's counter per device, so the device number says what a case
// inherits: a fresh number starts from nothing.  Output per case:
//   case <id> rc <return code>
//   <the records, fake_hip_rt.h>
//   end
// With --kernels it prints every kernel the object registered instead, the
// mangled name and the name as the records spell it.
// tests/test_launch_routes.py compares them with tests/launch_cases.py.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/md5hip.h"
#include "../../sproxy_amd/csrc/md5_internal.h"
#include "fake_hip_rt.h"

namespace {

typedef const std::vector<uint64_t>& Args;
template <typename T> T* ptr(uint64_t v) { return reinterpret_cast<T*>((uintptr_t)v); }
const void* cvp(uint64_t v) { return ptr<const void>(v); }
const uint64_t* u64p(uint64_t v) { return ptr<const uint64_t>(v); }
const uint32_t* u32p(uint64_t v) { return ptr<const uint32_t>(v); }
md5hip_md5crc32* recp(uint64_t v) { return ptr<md5hip_md5crc32>(v); }
MD5Context* ctxp(uint64_t v) { return ptr<MD5Context>(v); }

struct Entry {
  const char* name;
  size_t nargs;
  int (*call)(Args);
};

const Entry kEntries[] = {
    {"md5hip_digest_fixed", 6,
     [](Args a) { return md5hip_digest_fixed(cvp(a[0]), a[1], (uint32_t)a[2], a[3], ptr<unsigned char>(a[4]), ptr<void>(a[5])); }},
    {"md5hip_digest_fixed_variant", 7,
     [](Args a) {
       return md5hip_digest_fixed_variant(cvp(a[0]), a[1], (uint32_t)a[2], a[3], ptr<unsigned char>(a[4]),
                                          ptr<void>(a[5]), (int)a[6]);
     }},
    {"md5hip_digest_desc", 7,
     [](Args a) {
       return md5hip_digest_desc(cvp(a[0]), u64p(a[1]), u32p(a[2]), u32p(a[3]), a[4], ptr<unsigned char>(a[5]),
                                 ptr<void>(a[6]));
     }},
    {"md5hip_digest_desc_variant", 8,
     [](Args a) {
       return md5hip_digest_desc_variant(cvp(a[0]), u64p(a[1]), u32p(a[2]), u32p(a[3]), a[4],
                                         ptr<unsigned char>(a[5]), ptr<void>(a[6]), (int)a[7]);
     }},
    {"crc32hip_fixed", 7,
     [](Args a) {
       return crc32hip_fixed(cvp(a[0]), a[1], (uint32_t)a[2], a[3], (uint32_t)a[4], ptr<uint32_t>(a[5]),
                             ptr<void>(a[6]));
     }},
    {"crc32hip_fixed_variant", 8,
     [](Args a) {
       return crc32hip_fixed_variant(cvp(a[0]), a[1], (uint32_t)a[2], a[3], (uint32_t)a[4], ptr<uint32_t>(a[5]),
                                     ptr<void>(a[6]), (int)a[7]);
     }},
    {"crc32hip_desc", 8,
     [](Args a) {
       return crc32hip_desc(cvp(a[0]), u64p(a[1]), u32p(a[2]), u32p(a[3]), a[4], (uint32_t)a[5],
                            ptr<uint32_t>(a[6]), ptr<void>(a[7]));
     }},
    {"crc32hip_desc_variant", 9,
     [](Args a) {
       return crc32hip_desc_variant(cvp(a[0]), u64p(a[1]), u32p(a[2]), u32p(a[3]), a[4], (uint32_t)a[5],
                                    ptr<uint32_t>(a[6]), ptr<void>(a[7]), (int)a[8]);
     }},
    {"md5crc32hip_fixed", 6,
     [](Args a) { return md5crc32hip_fixed(cvp(a[0]), a[1], (uint32_t)a[2], a[3], recp(a[4]), ptr<void>(a[5])); }},
    {"md5crc32hip_fixed_variant", 7,
     [](Args a) {
       return md5crc32hip_fixed_variant(cvp(a[0]), a[1], (uint32_t)a[2], a[3], recp(a[4]), ptr<void>(a[5]), (int)a[6]);
     }},
    {"md5crc32hip_desc", 7,
     [](Args a) {
       return md5crc32hip_desc(cvp(a[0]), u64p(a[1]), u32p(a[2]), u32p(a[3]), a[4], recp(a[5]), ptr<void>(a[6]));
     }},
    {"md5crc32hip_desc_variant", 8,
     [](Args a) {
       return md5crc32hip_desc_variant(cvp(a[0]), u64p(a[1]), u32p(a[2]), u32p(a[3]), a[4], recp(a[5]),
                                       ptr<void>(a[6]), (int)a[7]);
     }},
    {"md5hip_init_ctx", 3, [](Args a) { return md5hip_init_ctx(ctxp(a[0]), a[1], ptr<void>(a[2])); }},
    {"md5hip_update_ctx", 5,
     [](Args a) { return md5hip_update_ctx(ctxp(a[0]), ptr<const void* const>(a[1]), u32p(a[2]), a[3], ptr<void>(a[4])); }},
    // sproxy_amd/csrc/md5_pages.hip (build/obj/md5_pages.o)
    {"md5hip_digest_pages", 9,
     [](Args a) {
       return md5hip_digest_pages((int)a[0], u64p(a[1]), u64p(a[2]), u32p(a[3]), u32p(a[4]), a[5], (uint32_t)a[6],
                                  ptr<void>(a[7]), ptr<void>(a[8]));
     }},
    {"crc32hip_pages", 9,
     [](Args a) {
       return crc32hip_pages(u64p(a[0]), u64p(a[1]), u32p(a[2]), u32p(a[3]), a[4], (uint32_t)a[5], (uint32_t)a[6],
                             ptr<uint32_t>(a[7]), ptr<void>(a[8]));
     }},
    {"md5hip_update_ctx_pages", 7,
     [](Args a) {
       return md5hip_update_ctx_pages(ctxp(a[0]), u64p(a[1]), u64p(a[2]), u32p(a[3]), a[4], (uint32_t)a[5],
                                      ptr<void>(a[6]));
     }},
    {"md5hip_final_ctx", 4,
     [](Args a) { return md5hip_final_ctx(ctxp(a[0]), a[1], ptr<unsigned char>(a[2]), ptr<void>(a[3])); }},
    {"md5hip_gather_launch", 4,
     [](Args a) { return md5hip_gather_launch(ptr<const md5hip_seg>(a[0]), a[1], ptr<unsigned char>(a[2]), ptr<void>(a[3])); }},
    {"md5hip_fill_synthetic", 4, [](Args a) { return md5hip_fill_synthetic(ptr<void>(a[0]), a[1], a[2], ptr<void>(a[3])); }},
    {"md5hip_order_device", 6,
     [](Args a) {
       return md5hip_order_device(u32p(a[0]), a[1], (uint32_t)a[2], ptr<uint32_t>(a[3]), ptr<uint32_t>(a[4]),
                                  ptr<void>(a[5]));
     }},
    // argument errors only: past them it runs rocPRIM's host code
    {"md5hip_order_device_stable", 7,
     [](Args a) {
       return md5hip_order_device_stable(u32p(a[0]), a[1], (uint32_t)a[2], ptr<void>(a[3]), a[4], ptr<uint32_t>(a[5]),
                                         ptr<void>(a[6]));
     }},
};

int fail(const char* what, const char* line) {
  fprintf(stderr, "launch_check: %s: %s\n", what, line);
  return 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc > 1 && strcmp(argv[1], "--kernels") == 0) {   // "<mangled>\t<name>" per kernel
    fake_hip_rt_kernels(stdout);
    return 0;
  }
  char line[4096];
  while (fgets(line, sizeof line, stdin)) {
    std::vector<std::string> tok;
    for (char* t = strtok(line, " \t\n"); t; t = strtok(nullptr, " \t\n")) tok.push_back(t);
    if (tok.empty() || tok[0][0] == '#') continue;
    if (tok.size() < 4) return fail("short line", tok[0].c_str());
    const Entry* e = nullptr;
    for (const Entry& k : kEntries)
      if (tok[3] == k.name) e = &k;
    if (!e) return fail("no such entry", tok[3].c_str());
    if (tok.size() != 4 + e->nargs) return fail("wrong number of arguments", tok[0].c_str());
    std::vector<uint64_t> a;
    for (size_t k = 4; k < tok.size(); ++k) {
      char* end = nullptr;
      a.push_back(strtoull(tok[k].c_str(), &end, 0));
      if (*end) return fail("not a number", tok[k].c_str());
    }
    fake_hip_rt_set_device(atoi(tok[1].c_str()), atoi(tok[2].c_str()));
    const int rc = e->call(a);
    printf("case %s rc %d\n", tok[0].c_str(), rc);
    fake_hip_rt_flush(stdout);
    printf("end\n");
  }
  return 0;
}
