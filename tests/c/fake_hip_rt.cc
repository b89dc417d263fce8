// fake_hip_rt.cc -- TEST INFRASTRUCTURE: a recording stand-in for the HIP
// runtime, just the entries the host halves of md5_kernels.o and md5_pages.o
// call.  Linked statically with the real objects and md5_plan.o into tests/c/launch_check.cc
// (never preloaded, never loaded into Python), it lets the launchers of
// sproxy_amd/csrc/md5_kernels.hip run on a machine without a GPU: no kernel
// executes, every launch is written down.
//
//   - the "device" is a number the harness sets, with a compute-unit count of
//     its own (hipDeviceGetAttribute); the launchers cache the count, the
//     dynamic-LDS attribute and BALANCED's counter per device, so a harness
//     that wants a case to start from nothing gives it a device of its own;
//   - __hipRegisterFunction keeps each host stub's kernel name; the table is
//     built on first use, since registration runs from a static constructor
//     of md5_kernels.o that may come before this file's;
//   - hipLaunchKernel records the demangled kernel name, grid, block, dynamic
//     LDS, stream and the raw argument bytes, cut by launch_args.h's table of
//     argument sizes; hipFuncSetAttribute, hipMemsetAsync, hipMalloc and
//     hipMemset are recorded in the same list, in call order;
//   - the virtual-memory calls of the batch arenas fail (arenas are not under
//     test), as do the device queries of rocPRIM's host code.
// Nothing here is part of the product.
#include <cxxabi.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "fake_hip_rt.h"
#include "launch_args.h"

namespace {

std::map<const void*, std::string>& names() {
  static std::map<const void*, std::string>* t = new std::map<const void*, std::string>;   // first use
  return *t;
}
std::vector<std::string>& records() {
  static std::vector<std::string>* r = new std::vector<std::string>;
  return *r;
}

int g_device = 0;
int g_cus = 256;
uint64_t g_next_alloc = 0x7f0000000000ull;

struct CallConfig {
  dim3 grid, block;
  size_t lds;
  hipStream_t stream;
};
thread_local std::vector<CallConfig> g_config;

std::string demangled(const char* mangled) {
  int status = 0;
  char* d = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
  std::string s = status == 0 && d ? d : mangled;
  free(d);
  return s;
}

// "void md5hip::md5_desc_fed<true>(unsigned char const*, ...)" -> "md5hip::md5_desc_fed<true>"
// A kernel of an unnamed namespace (md5_pages.o's) loses that prefix, in its
// template arguments too, before the parameter list is cut off at its "(":
// "void (anonymous namespace)::pages_xdma16<(anonymous namespace)::md5hip::Crc32PermHasher>((anonymous ..."
// -> "pages_xdma16<md5hip::Crc32PermHasher>"
std::string short_name(const std::string& full) {
  static const std::string anon = "(anonymous namespace)::";
  std::string s = full.compare(0, 5, "void ") == 0 ? full.substr(5) : full;
  for (size_t at = s.find(anon); at != std::string::npos; at = s.find(anon, at)) s.erase(at, anon.size());
  const size_t paren = s.find('(');
  return paren == std::string::npos ? s : s.substr(0, paren);
}

std::string kernel_of(const void* host_stub) {
  auto it = names().find(host_stub);
  return it == names().end() ? std::string("?") : short_name(demangled(it->second.c_str()));
}

void record(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void record(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  records().push_back(buf);
}

}  // namespace

// ---- the harness's side (fake_hip_rt.h)
void fake_hip_rt_set_device(int device, int cus) {
  g_device = device;
  g_cus = cus;
}
void fake_hip_rt_flush(FILE* out) {
  for (const std::string& r : records()) fprintf(out, "%s\n", r.c_str());
  records().clear();
}

void fake_hip_rt_kernels(FILE* out) {
  for (const auto& kv : names()) {
    fprintf(out, "%s\t%s\n", kv.second.c_str(), short_name(demangled(kv.second.c_str())).c_str());
  }
}

extern "C" {

// ---- registration (called from md5_kernels.o's static constructor)
void** __hipRegisterFatBinary(const void*) {
  static void* handle;
  return &handle;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_stub, char*, const char* device_name, unsigned, void*,
                           void*, void*, void*, int*) {
  names()[host_stub] = device_name;
}

hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t lds, hipStream_t stream) {
  g_config.push_back(CallConfig{grid, block, lds, stream});
  return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* lds, hipStream_t* stream) {
  if (g_config.empty()) return hipErrorInvalidValue;
  const CallConfig c = g_config.back();
  g_config.pop_back();
  *grid = c.grid;
  *block = c.block;
  *lds = c.lds;
  *stream = c.stream;
  return hipSuccess;
}

hipError_t hipLaunchKernel(const void* host_stub, dim3 grid, dim3 block, void** args, size_t lds,
                           hipStream_t stream) {
  const std::string name = kernel_of(host_stub);
  const LaunchArgs* la = launch_args_of(name.c_str());
  if (!la) {
    fprintf(stderr, "fake_hip_rt: no argument sizes for kernel %s (tests/c/launch_args.h)\n", name.c_str());
    abort();
  }
  std::string a;
  auto field = [&a](const void* at, size_t size) {
    uint64_t v = 0;
    memcpy(&v, at, size);                      // little-endian host: the low bytes
    char buf[24];
    snprintf(buf, sizeof buf, "%s0x%llx", a.empty() ? "" : ",", (unsigned long long)v);
    a += buf;
  };
  for (int k = 0; k < la->nargs; ++k) {
    if (la->size[k] == kPageBatch) {           // by value: four pointers and page_bytes
      const char* pb = static_cast<const char*>(args[k]);
      for (int f = 0; f < 4; ++f) field(pb + 8 * f, 8);
      field(pb + 32, 4);
    } else {
      field(args[k], la->size[k]);
    }
  }
  record("launch|%s|%u,%u,%u|%u,%u,%u|%zu|0x%llx|%s", name.c_str(), grid.x, grid.y, grid.z, block.x, block.y,
         block.z, lds, (unsigned long long)(uintptr_t)stream, a.c_str());
  return hipSuccess;
}

hipError_t hipFuncSetAttribute(const void* host_stub, hipFuncAttribute attr, int value) {
  record("attr|%s|%d|%d", kernel_of(host_stub).c_str(), (int)attr, value);
  return hipSuccess;
}

hipError_t hipMemsetAsync(void* dst, int value, size_t bytes, hipStream_t stream) {
  record("memset_async|0x%llx|%d|%zu|0x%llx", (unsigned long long)(uintptr_t)dst, value, bytes,
         (unsigned long long)(uintptr_t)stream);
  return hipSuccess;
}
hipError_t hipMemset(void* dst, int value, size_t bytes) {
  record("memset|0x%llx|%d|%zu", (unsigned long long)(uintptr_t)dst, value, bytes);
  return hipSuccess;
}
hipError_t hipMalloc(void** p, size_t bytes) {
  *p = (void*)(uintptr_t)g_next_alloc;         // never dereferenced: no kernel runs
  g_next_alloc += (bytes + 255) & ~(size_t)255;
  record("malloc|0x%llx|%zu", (unsigned long long)(uintptr_t)*p, bytes);
  return hipSuccess;
}
hipError_t hipFree(void*) { return hipSuccess; }

hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipGetDevice(int* device) {
  *device = g_device;
  return hipSuccess;
}
hipError_t hipSetDevice(int device) {
  g_device = device;
  return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* value, hipDeviceAttribute_t attr, int) {
  if (attr != hipDeviceAttributeMultiprocessorCount) return hipErrorInvalidValue;
  *value = g_cus;
  return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) { return hipSuccess; }
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }

// rocPRIM's host code asks these before it launches; it is not under test
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600*, int) { return hipErrorNoDevice; }
int hipGetStreamDeviceId(hipStream_t) { return -1; }

// the batch arenas: not under test
hipError_t hipMemGetAllocationGranularity(size_t*, const hipMemAllocationProp*, hipMemAllocationGranularity_flags) {
  return hipErrorNotSupported;
}
hipError_t hipMemAddressReserve(void**, size_t, size_t, void*, unsigned long long) { return hipErrorOutOfMemory; }
hipError_t hipMemAddressFree(void*, size_t) { return hipErrorInvalidValue; }
hipError_t hipMemCreate(hipMemGenericAllocationHandle_t*, size_t, const hipMemAllocationProp*, unsigned long long) {
  return hipErrorOutOfMemory;
}
hipError_t hipMemMap(void*, size_t, size_t, hipMemGenericAllocationHandle_t, unsigned long long) {
  return hipErrorInvalidValue;
}
hipError_t hipMemUnmap(void*, size_t) { return hipErrorInvalidValue; }
hipError_t hipMemRelease(hipMemGenericAllocationHandle_t) { return hipErrorInvalidValue; }
hipError_t hipMemSetAccess(void*, size_t, const hipMemAccessDesc*, size_t) { return hipErrorInvalidValue; }

}  // extern "C"
