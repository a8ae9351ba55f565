// Pick-freeze sums for the Sobol' indices of function-valued posterior draws (DESIGN I.16), f64, for gfx950.
//
// Layout: the values of P paths at M design rows with K outputs, (P, M, K), K fastest -- a layer of the walk as it leaves it.
// shift (P, K): every value enters as g = f - shift[p, k], one IEEE subtraction (the estimators do not depend on the shift; it
// takes the cancellation out of the sums of squares of a path with a large mean).
// A tile is 64 consecutive rows, one row per lane.  Per (tile, path, output) one wave forms one term per lane -- every product
// rounded once, never fused into the sum that follows it -- and adds the 64 terms by wave_sum's fixed tree; lanes past the end
// of a short tile hold +0.  dgpamd_sobol_add then adds the tiles' sums one after the other, in tile order, onto a running sum.
// No atomics anywhere: the bits of a sum depend on the values and on where the tiles start, not on the launch.
#include "common.hpp"
#include "wave.hpp"

#define SOBOL_TILE 64               // rows of a tile: the lanes of a wave
#define SOBOL_WAVES 4               // waves ((tile, path) pairs) of a workgroup

// PAIR false: partial[t, p, k, 0..3] = sum g_A, sum g_B, sum g_A^2, sum g_B^2.
// PAIR true:  partial[t, p, k, 0..1] = sum g_B (g_AB - g_A), sum (g_A - g_AB)^2.
template <bool PAIR>
__global__ __launch_bounds__(SOBOL_TILE *SOBOL_WAVES) void sobol_tiles_kernel(int64_t P, int64_t M, int K, int64_t ntiles,
                                                                              const double *fA, const double *fB, const double *fAB,
                                                                              const double *shift, double *partial) {
    constexpr int NC = PAIR ? 2 : 4;
    const int lane = threadIdx.x % SOBOL_TILE;
    const int64_t w = (int64_t)blockIdx.x * SOBOL_WAVES + threadIdx.x / SOBOL_TILE;   // wave-uniform: (tile, path), path fastest
    if (w >= ntiles * P) return;
    const int64_t t = w / P, p = w % P;
    const int64_t row = t * SOBOL_TILE + lane;
    const bool live = row < M;
    const int64_t at = (p * M + (live ? row : 0)) * K;      // (a lane past the end reads row 0 of its path and drops it)
    double *out = partial + (t * P + p) * K * NC;
    for (int k = 0; k < K; ++k) {
        const double s = shift[p * K + k];
        const double a = fA[at + k] - s, b = fB[at + k] - s;
        if (PAIR) {
            const double ab = fAB[at + k] - s;
            const double u = wave_sum(live ? __dmul_rn(b, ab - a) : 0.0);
            const double d = a - ab;
            const double tt = wave_sum(live ? __dmul_rn(d, d) : 0.0);
            if (lane == 0) out[k * NC] = u, out[k * NC + 1] = tt;
        } else {
            const double s1 = wave_sum(live ? a : 0.0), s2 = wave_sum(live ? b : 0.0);
            const double q1 = wave_sum(live ? __dmul_rn(a, a) : 0.0), q2 = wave_sum(live ? __dmul_rn(b, b) : 0.0);
            if (lane == 0) out[k * NC] = s1, out[k * NC + 1] = s2, out[k * NC + 2] = q1, out[k * NC + 3] = q2;
        }
    }
}

// sums[c] = (((sums[c] + partial[0, c]) + partial[1, c]) + ...): one lane per c, the tiles in order.
__global__ __launch_bounds__(256) void sobol_add_kernel(int64_t ntiles, int64_t count, const double *partial, double *sums) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= count) return;
    double s = sums[c];
    for (int64_t t = 0; t < ntiles; ++t) s += partial[t * count + c];
    sums[c] = s;
}

extern "C" int dgpamd_sobol_tiles(dgpamd_ctx *ctx, int64_t P, int64_t M, int K, const double *fA, const double *fB, const double *fAB,
                                  const double *shift, double *partial) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (P < 1 || M < 1 || K < 1) BAD_ARG(ctx, "need P >= 1, M >= 1, K >= 1");
    if (!fA || !fB || !shift || !partial) BAD_ARG(ctx, "null pointer");
    const int64_t ntiles = (M + SOBOL_TILE - 1) / SOBOL_TILE;
    if (P > 0x7fffffffLL || ntiles > 0x7fffffffLL * SOBOL_WAVES / P) BAD_ARG(ctx, "tiles * P is beyond 2^33");
    const unsigned blocks = (unsigned)((ntiles * P + SOBOL_WAVES - 1) / SOBOL_WAVES);
    if (fAB)
        hipLaunchKernelGGL(sobol_tiles_kernel<true>, dim3(blocks), dim3(SOBOL_TILE * SOBOL_WAVES), 0, ctx->stream, P, M, K, ntiles, fA, fB,
                           fAB, shift, partial);
    else
        hipLaunchKernelGGL(sobol_tiles_kernel<false>, dim3(blocks), dim3(SOBOL_TILE * SOBOL_WAVES), 0, ctx->stream, P, M, K, ntiles, fA, fB,
                           fAB, shift, partial);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

extern "C" int dgpamd_sobol_add(dgpamd_ctx *ctx, int64_t ntiles, int64_t count, const double *partial, double *sums) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (ntiles < 1 || count < 1) BAD_ARG(ctx, "need ntiles >= 1, count >= 1");
    if (!partial || !sums) BAD_ARG(ctx, "null pointer");
    const int64_t nb = (count + 255) / 256;
    if (nb > 0x7fffffffLL) BAD_ARG(ctx, "count is beyond 2^39");
    hipLaunchKernelGGL(sobol_add_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, ntiles, count, partial, sums);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
