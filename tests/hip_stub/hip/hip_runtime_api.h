// A stand-in for the handful of HIP calls csrc/bufs.h uses, backed by malloc / free: tests/bufs_main.cpp is compiled against it
// with the host compiler and the address and undefined-behaviour sanitizers, no GPU and no ROCm involved.  It counts the live
// allocations and can fail "the n-th allocation from now".
#pragma once
#include <stddef.h>
#include <stdlib.h>

typedef int hipError_t;
#define hipSuccess 0
#define hipErrorOutOfMemory 2
#define hipErrorInvalidValue 1
#define hipHostMallocDefault 0u
#define hipHostMallocMapped 2u

namespace hip_stub {
inline int live_dev = 0, live_host = 0;
inline long allocs = 0, frees = 0;
inline int fail_in = 0;                 // > 0: the fail_in-th allocation from now fails
inline unsigned last_host_flags = ~0u;
inline void fail_nth_from_now(int n) { fail_in = n; }
inline bool take_failure() { return fail_in > 0 && --fail_in == 0; }
}   // namespace hip_stub

inline hipError_t hipMalloc(void **p, size_t bytes)
{
    *p = nullptr;
    if (hip_stub::take_failure()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    ++hip_stub::live_dev; ++hip_stub::allocs;
    return hipSuccess;
}
inline hipError_t hipFree(void *p)
{
    if (!p) return hipSuccess;
    free(p);
    --hip_stub::live_dev; ++hip_stub::frees;
    return hipSuccess;
}
inline hipError_t hipHostMalloc(void **p, size_t bytes, unsigned flags)
{
    *p = nullptr;
    if (hip_stub::take_failure()) return hipErrorOutOfMemory;
    *p = malloc(bytes ? bytes : 1);
    hip_stub::last_host_flags = flags;
    ++hip_stub::live_host; ++hip_stub::allocs;
    return hipSuccess;
}
inline hipError_t hipHostFree(void *p)
{
    if (!p) return hipSuccess;
    free(p);
    --hip_stub::live_host; ++hip_stub::frees;
    return hipSuccess;
}
// the device view of mapped memory: here the host address itself
inline hipError_t hipHostGetDevicePointer(void **dev, void *host, unsigned)
{
    *dev = host;
    return host ? hipSuccess : hipErrorInvalidValue;
}
