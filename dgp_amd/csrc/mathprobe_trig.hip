// The two cosine cases of dgpamd_debug_mathfn (mathprobe.hip).  They have a translation unit of their own because cos_reduced_impl
// hands arguments of 2^30 and beyond to the device library's cos and sin, and this file is built as pathfun.hip and pathfun_grad.hip
// are (Makefile: TRIG_OBJS), without the contraction of the library's own multiply-adds that its large-argument reduction does not
// survive.  The rest of the probe is built as the kernels of the rest of the library are.
#include "pathfun.hpp"

template <bool WITH_SIN>
__global__ __launch_bounds__(256) void mathprobe_trig_kernel(int64_t count, const double *__restrict__ a, double *__restrict__ out0,
                                                             double *__restrict__ out1) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    double r1 = 0.0;
    out0[i] = cos_reduced_impl<WITH_SIN>(a[i], &r1);
    if (out1) out1[i] = r1;
}

void mathprobe_launch_trig(dgpamd_ctx *ctx, bool with_sin, int64_t count, const double *a, double *out0, double *out1) {
    const dim3 grid((unsigned)((count + 255) / 256));
    if (with_sin)
        hipLaunchKernelGGL(mathprobe_trig_kernel<true>, grid, dim3(256), 0, ctx->stream, count, a, out0, out1);
    else
        hipLaunchKernelGGL(mathprobe_trig_kernel<false>, grid, dim3(256), 0, ctx->stream, count, a, out0, out1);
}
