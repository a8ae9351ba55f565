// The whitening fold of field calibration (DESIGN I.24), f64, for gfx950: T sites x K outputs with a T x T error covariance per
// output become the K' = T K independent pseudo-outputs that the box chains and the SMC move already take.
//
// Per chain q, output k and site t, with W_k = L_k^-1 the lower-triangular whitening matrix of output k:
//   ft[q, t K + k]    = sum_{s <= t} W[k, t, s] f[q, s, k]
//   Jt[q, t K + k, d] = sum_{s <= t} W[k, t, s] J[q, s, k, cols[d]]
// every sum from 0.0 in the order of s, a term whose W[k, t, s] is exactly 0 skipped and not multiplied: the values of a site that
// was not observed may be NaN and reach nothing.  W comes transposed, Wt[k, s, t] = W[k, t, s]: thread t owns output row t, so the
// lanes of a wave read consecutive doubles of it for every s.  Entries with s > t are never read.
// One workgroup per (chain, output), T rounded up to whole waves of threads.  The chain's column of T inputs is staged in LDS, up
// to BOXSITES_CHUNK of the 1 + Dt columns (f, then J's columns cols[0 .. Dt - 1]) at a time, 16 KiB; a thread keeps one
// accumulator per staged column in registers and reads the staged values at one address per wave (a broadcast).
// No atomics, no cross-lane operation: an element is one fixed sequence of operations on its own chain's inputs, whatever Q is
// and whatever shares the launch.  The file is compiled with -ffp-contract=off (csrc/Makefile): every product is rounded before
// it enters its sum, as in tests/boxsites_ref.py.
#include <math.h>

#include "common.hpp"

#define BOXSITES_CHUNK 8

struct BoxsitesArgs {
    int T, K, Dx, Dt;
    const int32_t *cols;
    const double *Wt, *f, *J;
    double *ft, *Jt;
};

__global__ __launch_bounds__(DGPAMD_BOXSITES_MAXT) void boxsites_fold_kernel(BoxsitesArgs a) {
    __shared__ double col[DGPAMD_BOXSITES_MAXT * BOXSITES_CHUNK];     // [s][c]: site s of staged column c
    const int T = a.T, K = a.K, Dx = a.Dx, Dt = a.Dt;
    const int t = threadIdx.x, k = blockIdx.y;
    const int64_t row0 = (int64_t)blockIdx.x * T;                      // the chain's first row of f and J
    const double *Wk = a.Wt + (int64_t)k * T * T;
    // column v of the 1 + Dt: v = 0 is f, v >= 1 is column cols[v - 1] of J
    for (int v0 = 0; v0 <= Dt; v0 += BOXSITES_CHUNK) {
        const int nc = min(BOXSITES_CHUNK, Dt + 1 - v0);
        for (int i = t; i < T * nc; i += blockDim.x) {
            const int s = i / nc, c = i - s * nc, v = v0 + c;
            const int64_t e = (row0 + s) * K + k;
            col[s * BOXSITES_CHUNK + c] = v == 0 ? a.f[e] : a.J[e * Dx + a.cols[v - 1]];
        }
        __syncthreads();
        if (t < T) {
            double acc[BOXSITES_CHUNK];
#pragma unroll
            for (int c = 0; c < BOXSITES_CHUNK; ++c) acc[c] = 0.0;
            for (int s = 0; s <= t; ++s) {
                const double w = Wk[(int64_t)s * T + t];
                if (w != 0.0) {
#pragma unroll
                    for (int c = 0; c < BOXSITES_CHUNK; ++c)
                        if (c < nc) acc[c] = acc[c] + w * col[s * BOXSITES_CHUNK + c];
                }
            }
            const int64_t e = (row0 + t) * K + k;
#pragma unroll
            for (int c = 0; c < BOXSITES_CHUNK; ++c) {
                if (c < nc) {
                    const int v = v0 + c;
                    if (v == 0)
                        a.ft[e] = acc[c];
                    else
                        a.Jt[e * Dt + (v - 1)] = acc[c];
                }
            }
        }
        __syncthreads();                              // the next chunk overwrites what this one read
    }
}

extern "C" int dgpamd_boxsites_fold(dgpamd_ctx *ctx, int64_t Q, int T, int K, int Dx, int Dt, const int32_t *cols,
                                    const int32_t *cols_h, const double *Wt, const double *f, const double *J, double *ft,
                                    double *Jt) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (Q < 1 || Q > 0x7fffffffLL) BAD_ARG(ctx, "need 1 <= Q < 2^31");
    if (T < 1 || T > DGPAMD_BOXSITES_MAXT) BAD_ARG(ctx, "need 1 <= T <= DGPAMD_BOXSITES_MAXT");
    if (K < 1 || K > 65535) BAD_ARG(ctx, "need 1 <= K <= 65535");
    if (Dx < 1) BAD_ARG(ctx, "need Dx >= 1");
    if (Dt < 0 || Dt > DGPAMD_MAXD || Dt > Dx) BAD_ARG(ctx, "need 0 <= Dt <= min(Dx, DGPAMD_MAXD)");
    int64_t count;                                    // the elements of J: every index of the kernel stays below it
    if (__builtin_mul_overflow(Q * T, (int64_t)K, &count) || __builtin_mul_overflow(count, (int64_t)Dx, &count) ||
        count > (int64_t)1 << 60)
        BAD_ARG(ctx, "Q T K Dx is too large");
    if (!Wt || !f || !ft) BAD_ARG(ctx, "null pointer");
    if (Dt > 0) {
        if (!cols || !cols_h || !J || !Jt) BAD_ARG(ctx, "null pointer");
        for (int d = 0; d < Dt; ++d) {                // (Dt <= 64 columns: a quadratic scan of cols_h is short)
            if (cols_h[d] < 0 || cols_h[d] >= Dx) BAD_ARG(ctx, "every column must lie in 0 .. Dx - 1");
            for (int i = 0; i < d; ++i)
                if (cols_h[i] == cols_h[d]) BAD_ARG(ctx, "a column is named twice");
        }
    }
    BoxsitesArgs a;
    a.T = T, a.K = K, a.Dx = Dx, a.Dt = Dt;
    a.cols = cols, a.Wt = Wt, a.f = f, a.J = J, a.ft = ft, a.Jt = Jt;
    hipLaunchKernelGGL(boxsites_fold_kernel, dim3((unsigned)Q, (unsigned)K), dim3((unsigned)((T + 63) / 64 * 64)), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
