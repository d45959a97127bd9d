// kernels/host.h -- host helpers the launchers of several kernel families share, and the
// launchers one family's file exports to another's.  Private to kernels.hip and csrc/kernels/.
#pragma once

#include "kernels.h"

namespace gg {

inline int blocks_for(long long n, int bs = kBlock, int cap = 65535)
{
    long long b = (n + bs - 1) / bs;
    if (b < 1) b = 1;
    if (b > cap) b = cap;
    return (int)b;
}

// compute units of the current device (0 when the query fails)
inline int device_cus()
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
    return cus;
}
// blocks of `kernel` that can be resident at once: CUs x blocks per CU, 0 when any query
// fails.  Uncached: a caller that needs it per launch keeps the result in a static.
inline int resident_blocks(const void *kernel, int threads, size_t dyn_lds = 0)
{
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, dyn_lds) != hipSuccess) return 0;
    return device_cus() * per;
}
template <class... A>
int resident_blocks(void (*kernel)(A...), int threads, size_t dyn_lds = 0)
{
    return resident_blocks(reinterpret_cast<const void *>(kernel), threads, dyn_lds);
}

// kernels.hip: the level-scheduled triangle T (DevTri::LEVEL) as one dataflow launch, or a
// launch per level
void launch_trsv_levels(Gate g, DevTri &T, const double *b, double *x, int *err, hipStream_t st);
// kernels/trsv_wave.hip: one triangle without its tail (launch_trsv adds the tail's steps)
void launch_trsv_one(Gate g, DevTri &T, const double *b, double *x, int *err, hipStream_t st);

}  // namespace gg
