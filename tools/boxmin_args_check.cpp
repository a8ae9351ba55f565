// Host-side argument checking of csrc/boxmin.hip under AddressSanitizer / UBSan, without a device: every call below returns
// before a launch (a bad argument), and the workspace formula is plain host arithmetic.  Build and run on a CPU (from the
// repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/boxmin_args_check.cpp -x hip dgp_amd/csrc/boxmin.hip -o build/boxmin_args_check && build/boxmin_args_check
#include <math.h>
#include <stdio.h>

#include "../dgp_amd/csrc/common.hpp"

static int failures = 0;
#define EXPECT(call, want)                                                                  \
    do {                                                                                    \
        const long long rc__ = (long long)(call);                                           \
        if (rc__ != (long long)(want)) {                                                    \
            printf("FAIL %s -> %lld, expected %lld (%s)\n", #call, rc__, (long long)(want), ctx->err); \
            ++failures;                                                                     \
        }                                                                                   \
    } while (0)

int main() {
    dgpamd_ctx *ctx = new dgpamd_ctx();
    ctx->stream = nullptr;
    ctx->err[0] = 0;
    double d[DGPAMD_MAXD + 1];                                  // stands for every device pointer: never dereferenced before a launch
    double lo[DGPAMD_MAXD + 1], hi[DGPAMD_MAXD + 1], nan_b[2] = {0.0, NAN}, up[2] = {1.0, 1.0}, down[2] = {1.0, 0.5};
    for (int i = 0; i <= DGPAMD_MAXD; ++i) d[i] = 0.0, lo[i] = -1.0, hi[i] = 1.0;
    int32_t n[1] = {0};
    // the workspace formula: x, g, d, 2 history pairs, rho, alpha, f, t as doubles and five int32, per problem
    EXPECT(dgpamd_boxmin_workspace(1, 1, 1), 8 * (3 + 2 + 2 + 2) + 20);
    EXPECT(dgpamd_boxmin_workspace(130, 5, 6), 130LL * (8 * (15 + 60 + 12 + 2) + 20));
    EXPECT(dgpamd_boxmin_workspace(800, 64, 16), 800LL * (8 * (192 + 2048 + 32 + 2) + 20));
    EXPECT(dgpamd_boxmin_workspace(0, 5, 6), 0);
    EXPECT(dgpamd_boxmin_workspace(4, 0, 6), 0);
    EXPECT(dgpamd_boxmin_workspace(4, DGPAMD_MAXD + 1, 6), 0);
    EXPECT(dgpamd_boxmin_workspace(4, 5, 0), 0);
    EXPECT(dgpamd_boxmin_workspace(4, 5, DGPAMD_BOXMIN_MAXHIST + 1), 0);
#define STEP(ctx_, Q, D, K, k, sign, f, J, lo_d, hi_d, lo_h, hi_h, hist, maxiter, max_eval, gtol, ftol, work, xt, x, fun, st, ni, ne, run) \
    dgpamd_boxmin_step(ctx_, Q, D, K, k, sign, f, J, lo_d, hi_d, lo_h, hi_h, hist, maxiter, max_eval, gtol, ftol, 1, work, xt, x, fun, st, ni, ne, run)
    // bad arguments: refused before any launch
    EXPECT(STEP(nullptr, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 0, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 0, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, DGPAMD_MAXD + 1, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 0, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 3, 3, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 3, -1, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 0.5, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, NAN, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 0, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 17, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 0, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 0, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, -1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, NAN, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, -1.0, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, NAN, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, up, down, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, nan_b, up, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, nan_b, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    // a null pointer in every position
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, nullptr, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, nullptr, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, nullptr, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, nullptr, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, nullptr, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, nullptr, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, nullptr, d, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, nullptr, d, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, nullptr, d, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, nullptr, n, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, nullptr, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, nullptr, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, nullptr, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 2, 1, 0, 1.0, d, d, d, d, lo, hi, 6, 100, 420, 1e-6, 1e-12, d, d, d, d, n, n, n, nullptr), DGPAMD_BAD_ARG);
    delete ctx;
    printf(failures ? "boxmin_args_check: %d FAILED\n" : "boxmin_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
