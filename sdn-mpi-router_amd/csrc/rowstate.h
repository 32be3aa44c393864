// rowstate.h -- the row-state accessors shared by the fused what-if kernels
// (failure_loads.hip, whatif_loads.hip): one (scenario, destination) item's
// per-vertex words live in LDS, or above the LDS bound in a per-workgroup
// slice of the context scratch that other waves of the workgroup write.
#pragma once

#include "common.h"

// row-state words: plain LDS accesses, or agent-scope relaxed ones on scratch
// that other waves of the workgroup write
template <bool LDS, typename T>
__device__ __forceinline__ T fl_ld(const T *p)
{
    if (LDS) return *p;
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS, typename T>
__device__ __forceinline__ void fl_st(T *p, T v)
{
    if (LDS)
        *p = v;
    else
        __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ double fl_ld_f64(const double *p)
{
    if (LDS) return *p;
    // (also written by atomics performed in L2: read past L1)
    return __longlong_as_double((long long)__hip_atomic_load(
        reinterpret_cast<const unsigned long long *>(p), __ATOMIC_RELAXED,
        __HIP_MEMORY_SCOPE_AGENT));
}

template <bool LDS>
__device__ __forceinline__ void fl_st_f64(double *p, double v)
{
    if (LDS)
        *p = v;
    else
        __hip_atomic_store(reinterpret_cast<unsigned long long *>(p),
                           (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
struct FailDepth {
    typedef uint16_t T;
    static constexpr int kPending = 0xFFFF;
};
template <>
struct FailDepth<false> {
    typedef uint32_t T;
    static constexpr int kPending = 0x7FFFFFFF;
};
