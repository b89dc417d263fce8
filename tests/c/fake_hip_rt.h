// fake_hip_rt.h -- what tests/c/launch_check.cc asks of the recording
// runtime (tests/c/fake_hip_rt.cc).  Test infrastructure.
#ifndef SPROXY_AMD_TESTS_FAKE_HIP_RT_H
#define SPROXY_AMD_TESTS_FAKE_HIP_RT_H

#include <stdio.h>

// the current device and its compute-unit count
void fake_hip_rt_set_device(int device, int cus);
// print the records made since the last flush, one per line, and forget them:
//   launch|<kernel>|gx,gy,gz|bx,by,bz|<dynamic LDS>|<stream>|<arg>,<arg>,...
//   attr|<kernel>|<attribute>|<value>
//   memset_async|<ptr>|<value>|<bytes>|<stream>
//   memset|<ptr>|<value>|<bytes>
//   malloc|<ptr>|<bytes>
void fake_hip_rt_flush(FILE* out);
// "<mangled name>\t<name as the records spell it>" for every registered kernel
void fake_hip_rt_kernels(FILE* out);

#endif
