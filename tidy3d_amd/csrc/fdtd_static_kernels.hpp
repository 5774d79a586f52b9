// For the translation units beside fdtd_capi.hip.  fdtd_kernels.hpp defines its kernels in the header (it was written for one
// translation unit); the other units only need its types and device helpers: included behind this, every kernel gets internal
// linkage, and the ones a unit does not launch are dropped.
#pragma once
#include <hip/hip_runtime.h>
#undef __global__
#if defined(__HIPCC__)
#define __global__ static __attribute__((global))
#else
#define __global__ static
#endif
