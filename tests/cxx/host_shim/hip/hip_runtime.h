// Host stand-in for <hip/hip_runtime.h>, for compiling csrc/tsraster.h as plain C++ (tests/cxx/raster_rows_host.cpp): one "thread" at a time, so the
// atomics are plain read-modify-writes.  Only what tsraster.h uses.
#pragma once
#include <algorithm>
#define __device__
#define __forceinline__ inline
using std::max;
using std::min;
static inline unsigned atomicOr(unsigned *p, unsigned v) { const unsigned o = *p; *p = o | v; return o; }
static inline unsigned long long atomicAdd(unsigned long long *p, unsigned long long v) { const unsigned long long o = *p; *p = o + v; return o; }
static inline long long clock64() { return 0; }
