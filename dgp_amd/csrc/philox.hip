// Counter-based random streams on the device (DESIGN I.23), f64, for gfx950: dgpamd_philox_fill fills a contiguous
// (rounds, P, R, D) array with the numbers of the counter contract of philox.hpp.  A number is a pure function of
// (key, stream, round, p, r, e): nothing depends on how many paths, slots, rounds or calls run beside it.
//
// One lane covers one block of four elements of one slot: ten rounds of two 64 x 64 -> 128 bit products, then the kind's
// transform, then up to four 8-byte stores, guarded at a partial last block (D mod 4 != 0).  Neighbouring lanes write
// neighbouring 32 bytes.  No LDS, no atomics, no cross-lane operation; nothing is loaded from memory at all.  What bounds it:
// the integer products and, for the normal kind, the device library's log and sincospi (two of each per block); the stores
// are 8 bytes per number.  The grid is capped and strided, so any lane count the checks admit is a legal launch.
// The file is compiled with -ffp-contract=off: the transforms are the products and calls written below, nothing fused.
#include "common.hpp"
#include "philox.hpp"

#define PHILOX_THREADS 256
#define PHILOX_MAX_GROUPS (1 << 20)

struct PhiloxArgs {
    uint64_t k0, k1, stream, c2_first;
    int64_t lanes, PR, R;
    int D, nb, kind;
    double *out;
};

__global__ __launch_bounds__(PHILOX_THREADS) void philox_fill_kernel(PhiloxArgs a) {
    const int64_t stride = (int64_t)gridDim.x * PHILOX_THREADS;
    for (int64_t t = (int64_t)blockIdx.x * PHILOX_THREADS + threadIdx.x; t < a.lanes; t += stride) {
        const int64_t s = t / a.nb;                               // the slot's row of the output: (round P + p) R + r
        const int j = (int)(t - s * a.nb);                        // the block of four within the row
        const int64_t round = s / a.PR, pr = s - round * a.PR, p = pr / a.R, r = pr - p * a.R;
        uint64_t w[4];
        philox_slot_block(w, a.k0, a.k1, a.stream, a.c2_first + (uint64_t)round, (uint64_t)p, (uint64_t)r, (uint64_t)j);
        const int n = min(4, a.D - 4 * j);                        // 1 .. 4 elements of this block exist
        double *o = a.out + s * a.D + 4 * j;
        if (a.kind == DGPAMD_PHILOX_BITS) {
            for (int k = 0; k < n; ++k) ((uint64_t *)o)[k] = w[k];
        } else if (a.kind == DGPAMD_PHILOX_UNIFORM) {
            for (int k = 0; k < n; ++k) o[k] = philox_uniform(w[k]);
        } else if (a.kind == DGPAMD_PHILOX_LOG_UNIFORM) {
            for (int k = 0; k < n; ++k) o[k] = log(philox_uniform(w[k]));      // (log 0 = -inf)
        } else {
            // Box and Muller: words (0, 1) and (2, 3) give elements (0, 1) and (2, 3)
            for (int q = 0; 2 * q < n; ++q) {
                const double u1 = philox_uniform_open0(w[2 * q]), u2 = philox_uniform(w[2 * q + 1]);
                const double rho = sqrt(-2.0 * log(u1));
                double sn, cs;
                sincospi(2.0 * u2, &sn, &cs);
                o[2 * q] = rho * cs;
                if (2 * q + 1 < n) o[2 * q + 1] = rho * sn;
            }
        }
    }
}

extern "C" int dgpamd_philox_fill(dgpamd_ctx *ctx, int kind, uint64_t key0, uint64_t key1, uint64_t stream, uint64_t c2_first,
                                  int64_t rounds, int64_t P, int64_t R, int D, void *out) {
    if (!ctx) return DGPAMD_BAD_ARG;
    if (kind < 0 || kind >= DGPAMD_PHILOX_COUNT) BAD_ARG(ctx, "kind must be one of DGPAMD_PHILOX_*");
    if (rounds < 1 || P < 1 || R < 1) BAD_ARG(ctx, "need rounds >= 1, P >= 1 and R >= 1");
    if (D < 1 || D > DGPAMD_MAXD) BAD_ARG(ctx, "need 1 <= D <= DGPAMD_MAXD");
    if (P >= (1LL << 31) || R >= (1LL << 32)) BAD_ARG(ctx, "need P < 2^31 and R < 2^32");
    if (c2_first + (uint64_t)rounds < c2_first) BAD_ARG(ctx, "c2_first + rounds wraps");
    // (rounds, P and R are below 2^63, 2^31 and 2^32: the product of the last two fits, the one with rounds is checked)
    const int64_t PR = P * R;
    if (rounds > (1LL << 56) / PR) BAD_ARG(ctx, "rounds P R must not pass 2^56");
    if (!out) BAD_ARG(ctx, "null pointer");
    PhiloxArgs a;
    a.k0 = key0, a.k1 = key1, a.stream = stream, a.c2_first = c2_first;
    a.PR = PR, a.R = R, a.D = D, a.nb = (D + 3) / 4, a.kind = kind;
    a.lanes = rounds * PR * a.nb;
    a.out = (double *)out;
    const int64_t groups = (a.lanes + PHILOX_THREADS - 1) / PHILOX_THREADS;
    hipLaunchKernelGGL(philox_fill_kernel, dim3((unsigned)(groups < PHILOX_MAX_GROUPS ? groups : PHILOX_MAX_GROUPS)),
                       dim3(PHILOX_THREADS), 0, ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}
