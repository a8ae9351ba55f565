// Wave-level helpers shared by the one-wave-per-item kernels (the vecchia_*.hip units, train.hip,
// linkgp.hpp).  Everything here is forced inline: a kernel that uses one compiles to what it did with a copy of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

// sum over the 64 lanes of a wave: the total ends up in lane 0 (the other lanes hold partial sums)
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
// ... and in every lane
__device__ __forceinline__ double wave_sum_all(double v) { return __shfl(wave_sum(v), 0, 64); }

// lane l's value of v in every lane (v_readlane: l must be wave-uniform)
__device__ __forceinline__ double readlane_f64(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// f(integral_constant<I>) ... f(integral_constant<N - 1>): every index a compile-time constant, so that arrays indexed with it stay
// in registers (left to `#pragma unroll` the compiler keeps some of the loops and the arrays go to scratch memory)
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// 1 / d: hardware estimate + two Newton rounds
__device__ __forceinline__ double rcp_newton(double d) {
    double x = __builtin_amdgcn_rcp(d);
    double e = fma(-d, x, 1.0);
    x = fma(x, e, x);
    e = fma(-d, x, 1.0);
    return fma(x, e, x);
}

// (distance, index) order of the neighbour searches: ties in distance go to the smaller index
template <class I>
__device__ __forceinline__ bool pair_less(double d1, I i1, double d2, I i2) {
    return d1 < d2 || (d1 == d2 && i1 < i2);
}
