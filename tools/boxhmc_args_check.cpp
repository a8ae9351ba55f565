// Host-side argument checking of csrc/boxhmc.hip under AddressSanitizer / UBSan, without a device: every call below returns
// before a launch (a bad argument), and the workspace formula is plain host arithmetic.  Build and run on a CPU (from the
// repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/boxhmc_args_check.cpp -x hip dgp_amd/csrc/boxhmc.hip -o build/boxhmc_args_check && build/boxhmc_args_check
#include <math.h>
#include <stdio.h>
#include <string.h>

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

enum { D = 2, K = 3, NPAR = 2 * K + 5 * D };
// par: w (K), ybar (K), pv (D), pm (D), s (D), lo (D), hi (D)
static const double good[NPAR] = {1.0, 0.0, 2.0, 0.5, NAN, 0.5, 0.0, 4.0, 0.1, NAN, 1.0, 0.0, -1.0, 0.0, 1.0, 0.0};

// Every case runs with each combination of first and last, which the checks do not depend on (both together are accepted):
// the common return code, or -999 if the four differ.
static int step4(dgpamd_ctx *ctx, int64_t Q, int D_, int K_, const double *f, const double *J, const double *par, const double *par_h,
                 const double *z, const double *u, double h0, double hmin, double hmax, double up, double down, int slot, int nslots,
                 void *work, double *xt, double *h, double *logr, double *xs, double *lps, int32_t *status, int32_t *n_prop,
                 int32_t *n_acc) {
    int rc[4];
    for (int i = 0; i < 4; ++i)
        rc[i] = dgpamd_boxhmc_step(ctx, Q, D_, K_, f, J, par, par_h, z, u, h0, hmin, hmax, up, down, i & 1, i & 1, i >> 1, slot, nslots,
                                   work, xt, h, logr, xs, lps, status, n_prop, n_acc);
    return rc[0] == rc[1] && rc[1] == rc[2] && rc[2] == rc[3] ? rc[0] : -999;
}

int main() {
    dgpamd_ctx *ctx = new dgpamd_ctx();
    ctx->stream = nullptr;
    ctx->err[0] = 0;
    double d[8] = {0};                                          // stands for every device pointer: never dereferenced before a launch
    int32_t n[1] = {0};
    // the workspace formula: x, g, g', p, lp and H0 as doubles and one int32, per chain
    EXPECT(dgpamd_boxhmc_workspace(1, 1), 8 * (4 + 2) + 4);
    EXPECT(dgpamd_boxhmc_workspace(130, 5), 130LL * (8 * (20 + 2) + 4));
    EXPECT(dgpamd_boxhmc_workspace(800, 64), 800LL * (8 * (256 + 2) + 4));
    EXPECT(dgpamd_boxhmc_workspace(0, 5), 0);
    EXPECT(dgpamd_boxhmc_workspace(-3, 5), 0);
    EXPECT(dgpamd_boxhmc_workspace(1LL << 31, 5), 0);
    EXPECT(dgpamd_boxhmc_workspace(4, 0), 0);
    EXPECT(dgpamd_boxhmc_workspace(4, DGPAMD_MAXD + 1), 0);
// (the trailing arguments: work, x_trial, h, logr, xs, lps, status, n_prop, n_acc)
#define STEP(...) step4(__VA_ARGS__)
#define GOOD_TAIL d, d, d, d, d, d, n, n, n
    // sizes
    EXPECT(STEP(nullptr, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 0, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, 0, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, DGPAMD_MAXD + 1, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, 0, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    // the scalars: positive and finite, hmin <= hmax
    const double bad_scalar[4] = {0.0, -1.0, NAN, INFINITY};
    for (double b : bad_scalar) {
        EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, b, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
        EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, b, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
        EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, b, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
        EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, b, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
        EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, b, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    }
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1.0, 0.5, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    // a slot outside the sample buffer
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 4, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, -2, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 0, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, -1, -1, GOOD_TAIL), DGPAMD_BAD_ARG);
    // the host copy of par: a negative or NaN w, pv or s, lo > hi, a NaN bound (ybar and pm may hold anything)
    const struct { int at; double v; } bad_par[] = {{0, -1.0}, {2, NAN}, {2 * K, -4.0}, {2 * K + 1, NAN}, {2 * K + 2 * D, -1.0},
                                                    {2 * K + 2 * D + 1, NAN}, {2 * K + 3 * D, 2.0}, {2 * K + 3 * D + 1, NAN},
                                                    {2 * K + 4 * D, NAN}, {2 * K + 4 * D + 1, -1.0}};
    for (const auto &b : bad_par) {
        double par[NPAR];
        memcpy(par, good, sizeof par);
        par[b.at] = b.v;
        EXPECT(STEP(ctx, 4, D, K, d, d, d, par, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    }
    // a null pointer in every position
    EXPECT(STEP(ctx, 4, D, K, nullptr, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, nullptr, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, nullptr, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, nullptr, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, nullptr, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, nullptr, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, GOOD_TAIL), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, nullptr, d, d, d, d, d, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, nullptr, d, d, d, d, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, d, nullptr, d, d, d, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, d, d, nullptr, d, d, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, d, d, d, nullptr, d, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, d, d, d, d, nullptr, n, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, d, d, d, d, d, nullptr, n, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, d, d, d, d, d, n, nullptr, n), DGPAMD_BAD_ARG);
    EXPECT(STEP(ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, d, d, d, d, d, n, n, nullptr), DGPAMD_BAD_ARG);
    delete ctx;
    printf(failures ? "boxhmc_args_check: %d FAILED\n" : "boxhmc_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
