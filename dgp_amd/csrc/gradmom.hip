// Second moments of the input gradient of function-valued posterior draws (DESIGN I.18), f64, for gfx950: the sums behind
// C = E_x[grad f grad f^T] (active subspaces) and its diagonal (DGSM).
//
// Layout, as the layer walk leaves it: f (P, M, K) the values of P paths at M design rows with K outputs, J (P, M, K, Dx) their
// Jacobian with respect to x, Dx fastest, shift (P, K).  A tile is 64 consecutive rows.  Per (tile, path, output)
//   partial[t, p, k, :] = sum g, sum g^2 (g = f - shift, one IEEE subtraction, the square rounded once),
//                         sum J_d (d < Dx),  sum J_d J_e (d <= e, the upper triangle packed row-major)
// over the rows of the tile; rows past M contribute +0.  dgpamd_sobol_add adds the tiles in tile order (sobol.hip).
//
// One workgroup per (tile, path, output).  It stages the tile's 64 x Dx slab of J in LDS once, Dx padded with zeros to
// DP = 16 NBLK -- every thread asks for all its elements before it waits for the first, so a workgroup has its whole slab in
// flight at once -- and forms the tile's Gram matrix (Dx x 64) (64 x Dx) as 16 x 16 blocks of the upper triangle on
// v_mfma_f64_16x16x4: 16 k-steps per block, one wave per block, the blocks dealt to the waves so that each wave gets the same
// number (1, 3, 6, 10 blocks on 1, 3, 3, 5 waves).  Both operands of a block are k-major in the slab (row = design row), which is
// the fragment order of the instruction: nothing is transposed.  sum J_d comes from the same fragments: the A operand of step k0
// is J[k0 + (lane >> 4), 16 bi + (lane & 15)], so a lane adds its 16 operands as they pass (rows lane >> 4, + 4, ...: in the
// shadow of the MFMAs) and the four row classes are joined by two shuffles, (c0 + c2) + (c1 + c3); the wave that holds the
// diagonal block (bi, bi) writes the sums of its 16 columns.  sum g and sum g^2 go through wave_sum, one row per lane, while the
// slab is on its way.
// No atomics, and nothing a workgroup computes depends on the grid or on its neighbours: the bits of a tile's sums depend on the
// tile's values alone.  A zero column gives +0 in its sum and in every product entry it takes part in (the accumulators start at
// +0, and +0 + -0 = +0).  No product is followed by a sum outside the MFMA, so -ffp-contract has nothing to fuse here.
#include "common.hpp"
#include "wave.hpp"

#define GM_TILE 64      // rows of a tile
#define GM_MAXD 64      // widest Jacobian

// NBLK = ceil(Dx / 16) blocks along the padded width.
__host__ __device__ constexpr int gm_waves(int nblk) { return nblk == 1 ? 1 : nblk == 4 ? 5 : 3; }
// LDS leading dimension of the slab: ld mod 32 == 16, so that the rows k0, k0 + 1 (and k0 + 2, k0 + 3) of a fragment, 16 consecutive
// doubles each, fall into the two halves of the 64 banks: conflict-free ds_read_b64.
__host__ __device__ constexpr int gm_ld(int nblk) { return (16 * nblk) % 32 == 16 ? 16 * nblk : 16 * nblk + 16; }

template <int NBLK>
__global__ __launch_bounds__(64 * gm_waves(NBLK)) void gradmom_tiles_kernel(int64_t P, int64_t M, int K, int Dx, const double *f,
                                                                            const double *J, const double *shift, double *partial) {
    constexpr int W = gm_waves(NBLK), LD = gm_ld(NBLK), NT = 64 * W, DP = 16 * NBLK, PER = NBLK * (NBLK + 1) / 2 / W;
    constexpr int TRIPS = (GM_TILE * DP + NT - 1) / NT;     // elements of the padded slab per thread
    static_assert(PER * W == NBLK * (NBLK + 1) / 2, "every wave takes the same number of blocks");
    __shared__ double S[GM_TILE * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // (tile, path, output) from the workgroup's index, output fastest: 32-bit divisions (the grid is below 2^31)
    const unsigned u = blockIdx.x, tp = u / (unsigned)K, k = u - tp * (unsigned)K, tile = tp / (unsigned)P;
    const int64_t p = tp - tile * (unsigned)P, row0 = (int64_t)tile * GM_TILE;
    const int rows = (int)(M - row0 < GM_TILE ? M - row0 : GM_TILE);
    const int64_t ldj = (int64_t)K * Dx;                // doubles between two rows of one (path, output)
    const double *Jt = J + ((p * M + row0) * K + k) * Dx;
    double *out = partial + (int64_t)u * (2 + Dx + Dx * (Dx + 1) / 2);

    // A thread keeps one column d of the padded slab and takes the rows r0, r0 + RS, ...  The loads first, the value's in front
    // (its sums are taken while the slab is on its way); nothing is stored to memory before the slab has arrived, so that the wait
    // for the slab is a wait for loads alone.  A whole tile tests no row.
    constexpr int RS = NT / DP;
    static_assert(RS * DP == NT, "a thread keeps its column from trip to trip");
    const int d = tid % DP, r0 = tid / DP;
    const double *src = Jt + r0 * ldj + d;
    double fv = 0.0, s1 = 0.0, s2 = 0.0, v[TRIPS];
#pragma unroll
    for (int t = 0; t < TRIPS; ++t) v[t] = 0.0;
    if (wave == 0 && lane < rows) fv = f[(p * M + row0 + lane) * K + k];
    auto fetch = [&](auto whole) {
#pragma unroll
        for (int t = 0; t < TRIPS; ++t) {
            const int r = r0 + t * RS;
            if (decltype(whole)::value ? ((t + 1) * RS <= GM_TILE || r < GM_TILE) : r < rows) v[t] = src[t * RS * ldj];
        }
    };
    if (d < Dx) {
        if (rows == GM_TILE) fetch(std::true_type{});
        else fetch(std::false_type{});
    }
    if (wave == 0) {
        const double g = lane < rows ? fv - shift[p * K + k] : 0.0;
        s1 = wave_sum(g), s2 = wave_sum(__dmul_rn(g, g));
    }
#pragma unroll
    for (int t = 0; t < TRIPS; ++t)
        if ((t + 1) * RS <= GM_TILE || r0 + t * RS < GM_TILE) S[(r0 + t * RS) * LD + d] = v[t];
    __syncthreads();

    // fragment maps of v_mfma_f64_16x16x4 (tile.hpp): lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15];
    // its four results are D[(l >> 4) + 4 r][l & 15]
    const int m = lane & 15, kk = lane >> 4;
    double *tri = out + 2 + Dx;
    if (tid == 0) out[0] = s1, out[1] = s2;
#pragma unroll
    for (int s = 0; s < PER; ++s) {
        int bi = 0, bj = wave + s * W;                  // block wave + s W of the upper triangle, row-major -> (bi, bj), bi <= bj
        while (bj >= NBLK - bi) bj -= NBLK - bi, ++bi;
        bj += bi;
        const double *Sa = S + 16 * bi + m, *Sb = S + 16 * bj + m;
        d4 acc = {0.0, 0.0, 0.0, 0.0};
        double col = 0.0;
#pragma unroll
        for (int k0 = 0; k0 < GM_TILE; k0 += 4) {
            const double a = Sa[(k0 + kk) * LD];
            col += a;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Sb[(k0 + kk) * LD], acc, 0, 0, 0);
        }
        if (bi == bj) {                                 // (wave-uniform)
            col += __shfl_down(col, 32, 64);
            col += __shfl_down(col, 16, 64);
            if (lane < 16 && 16 * bi + lane < Dx) out[2 + 16 * bi + lane] = col;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * bi + kk + 4 * r, e = 16 * bj + m;
            if (d <= e && e < Dx) tri[d * Dx - d * (d - 1) / 2 + e - d] = acc[r];
        }
    }
}

extern "C" int dgpamd_gradmom_tiles(dgpamd_ctx *ctx, int64_t P, int64_t M, int K, int Dx, const double *f, const double *J,
                                    const double *shift, double *partial) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (P < 1 || M < 1 || K < 1) BAD_ARG(ctx, "need P >= 1, M >= 1, K >= 1");
    if (Dx < 1 || Dx > GM_MAXD) BAD_ARG(ctx, "need 1 <= Dx <= 64");
    if (!f || !J || !shift || !partial) BAD_ARG(ctx, "null pointer");
    const int64_t ntiles = (M + GM_TILE - 1) / GM_TILE;
    if (P > 0x7fffffffLL || ntiles > 0x7fffffffLL / P || ntiles * P > 0x7fffffffLL / K) BAD_ARG(ctx, "tiles * P * K is beyond 2^31");
    const dim3 grid((unsigned)(ntiles * P * K));
    switch ((Dx + 15) / 16) {
    case 1: hipLaunchKernelGGL(gradmom_tiles_kernel<1>, grid, dim3(64 * gm_waves(1)), 0, ctx->stream, P, M, K, Dx, f, J, shift, partial); break;
    case 2: hipLaunchKernelGGL(gradmom_tiles_kernel<2>, grid, dim3(64 * gm_waves(2)), 0, ctx->stream, P, M, K, Dx, f, J, shift, partial); break;
    case 3: hipLaunchKernelGGL(gradmom_tiles_kernel<3>, grid, dim3(64 * gm_waves(3)), 0, ctx->stream, P, M, K, Dx, f, J, shift, partial); break;
    default: hipLaunchKernelGGL(gradmom_tiles_kernel<4>, grid, dim3(64 * gm_waves(4)), 0, ctx->stream, P, M, K, Dx, f, J, shift, partial); break;
    }
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
