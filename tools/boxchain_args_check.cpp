// Host-side argument checking of csrc/boxmala.hip and csrc/boxhmc.hip (the checks are csrc/boxchain.hpp's, once for both) under
// AddressSanitizer / UBSan, without a device: every call below returns before a launch (a bad argument), and the workspace
// formulas are plain host arithmetic.  One table of refusals runs through both entry points.  Build and run on a CPU (from the
// repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/boxchain_args_check.cpp \
//         -x hip dgp_amd/csrc/boxmala.hip dgp_amd/csrc/boxhmc.hip -o build/boxchain_args_check && build/boxchain_args_check
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "../dgp_amd/csrc/common.hpp"

static int failures = 0;
static dgpamd_ctx *ctx;
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

// the arguments the two steps share; first, last and adapt are the adapters'
struct Call {
    dgpamd_ctx *ctx;
    int64_t Q;
    int D, K;
    const double *f, *J, *par, *par_h, *z, *logu;
    double h0, hmin, hmax, up, down;
    int slot, n_slots;
    void *work;
    double *x_trial, *h, *logr, *xs, *lps;
    int32_t *status, *n_prop, *n_acc;
};

static int mala(const Call &c) {
    return dgpamd_boxmala_step(c.ctx, c.Q, c.D, c.K, c.f, c.J, c.par, c.par_h, c.z, c.logu, c.h0, c.hmin, c.hmax, c.up, c.down, 1, 1,
                               c.slot, c.n_slots, c.work, c.x_trial, c.h, c.logr, c.xs, c.lps, c.status, c.n_prop, c.n_acc);
}

// each combination of first and last, which the checks do not depend on (both together are accepted): the common return code,
// or -999 if the four differ
static int hmc(const Call &c) {
    int rc[4];
    for (int i = 0; i < 4; ++i)
        rc[i] = dgpamd_boxhmc_step(c.ctx, c.Q, c.D, c.K, c.f, c.J, c.par, c.par_h, c.z, c.logu, c.h0, c.hmin, c.hmax, c.up, c.down,
                                   i & 1, i & 1, i >> 1, c.slot, c.n_slots, c.work, c.x_trial, c.h, c.logr, c.xs, c.lps, c.status,
                                   c.n_prop, c.n_acc);
    return rc[0] == rc[1] && rc[1] == rc[2] && rc[2] == rc[3] ? rc[0] : -999;
}

// both steps refuse the call, each under its own name and with this text
static void refused(const Call &c, const char *what, const char *text) {
    const struct { const char *name; int (*step)(const Call &); } steps[] = {{"dgpamd_boxmala_step", mala}, {"dgpamd_boxhmc_step", hmc}};
    for (const auto &s : steps) {
        char want[256];
        snprintf(want, sizeof want, "%s: %s", s.name, text);
        ctx->err[0] = 0;
        const int rc = s.step(c);
        if (rc != DGPAMD_BAD_ARG || (c.ctx && strcmp(ctx->err, want))) {
            printf("FAIL %s with %s -> %d \"%s\", expected %d \"%s\"\n", s.name, what, rc, ctx->err, DGPAMD_BAD_ARG, want);
            ++failures;
        }
    }
}
// a call that differs from an accepted one by `change`
#define REFUSED(change, text)     \
    do {                          \
        Call c = ok;              \
        change;                   \
        refused(c, #change, text); \
    } while (0)

int main() {
    ctx = new dgpamd_ctx();
    ctx->stream = nullptr;
    ctx->err[0] = 0;
    double d[8] = {0};                                          // stands for every device pointer: never dereferenced before a launch
    int32_t n[1] = {0};
    // the workspace formulas: x, g, g' and lp (boxhmc: and p and H0) as doubles and one int32, per chain
    EXPECT(dgpamd_boxmala_workspace(1, 1), 8 * (3 + 1) + 4);
    EXPECT(dgpamd_boxmala_workspace(130, 5), 130LL * (8 * (15 + 1) + 4));
    EXPECT(dgpamd_boxmala_workspace(800, 64), 800LL * (8 * (192 + 1) + 4));
    EXPECT(dgpamd_boxhmc_workspace(1, 1), 8 * (4 + 2) + 4);
    EXPECT(dgpamd_boxhmc_workspace(130, 5), 130LL * (8 * (20 + 2) + 4));
    EXPECT(dgpamd_boxhmc_workspace(800, 64), 800LL * (8 * (256 + 2) + 4));
    for (size_t (*workspace)(int64_t, int) : {dgpamd_boxmala_workspace, dgpamd_boxhmc_workspace}) {
        EXPECT(workspace(0, 5), 0);
        EXPECT(workspace(-3, 5), 0);
        EXPECT(workspace(1LL << 31, 5), 0);
        EXPECT(workspace(4, 0), 0);
        EXPECT(workspace(4, DGPAMD_MAXD + 1), 0);
    }
    const Call ok = {ctx, 4, D, K, d, d, d, good, d, d, 0.1, 1e-10, 1e2, 1.5, 0.5, 0, 4, d, d, d, d, d, d, n, n, n};
    // sizes
    REFUSED(c.ctx = nullptr, "");
    REFUSED(c.Q = 0, "need 1 <= Q < 2^31");
    REFUSED(c.Q = 1LL << 31, "need 1 <= Q < 2^31");
    REFUSED(c.D = 0, "need 1 <= D <= DGPAMD_MAXD");
    REFUSED(c.D = DGPAMD_MAXD + 1, "need 1 <= D <= DGPAMD_MAXD");
    REFUSED(c.K = 0, "need K >= 1");
    // the scalars: positive and finite, hmin <= hmax
    const char *scalar = "h0, hmin, hmax, up and down must be positive and finite";
    for (double b : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
        REFUSED(c.h0 = b, scalar);
        REFUSED(c.hmin = b, scalar);
        REFUSED(c.hmax = b, scalar);
        REFUSED(c.up = b, scalar);
        REFUSED(c.down = b, scalar);
    }
    REFUSED((c.hmin = 1.0, c.hmax = 0.5), "need hmin <= hmax");
    // a slot outside the sample buffer
    REFUSED(c.slot = 4, "need -1 <= slot < n_slots");
    REFUSED(c.slot = -2, "need -1 <= slot < n_slots");
    REFUSED(c.n_slots = 0, "need -1 <= slot < n_slots");
    REFUSED((c.slot = -1, c.n_slots = -1), "need -1 <= slot < n_slots");
    // the host copy of par: a negative or NaN w, pv or s, lo > hi, a NaN bound (ybar and pm may hold anything)
    const char *weight = "every weight w must be a number >= 0", *scales = "every pv and s must be a number >= 0";
    const char *bound = "every bound must be a number with lo <= hi";
    const struct { int at; double v; const char *text; } bad_par[] = {
        {0, -1.0, weight}, {2, NAN, weight}, {2 * K, -4.0, scales}, {2 * K + 1, NAN, scales}, {2 * K + 2 * D, -1.0, scales},
        {2 * K + 2 * D + 1, NAN, scales}, {2 * K + 3 * D, 2.0, bound}, {2 * K + 3 * D + 1, NAN, bound}, {2 * K + 4 * D, NAN, bound},
        {2 * K + 4 * D + 1, -1.0, bound}};
    for (const auto &b : bad_par) {
        double par[NPAR];
        memcpy(par, good, sizeof par);
        par[b.at] = b.v;
        REFUSED(c.par_h = par, b.text);
    }
    // a null pointer in every position
    REFUSED(c.f = nullptr, "null pointer");
    REFUSED(c.J = nullptr, "null pointer");
    REFUSED(c.par = nullptr, "null pointer");
    REFUSED(c.par_h = nullptr, "null pointer");
    REFUSED(c.z = nullptr, "null pointer");
    REFUSED(c.logu = nullptr, "null pointer");
    REFUSED(c.work = nullptr, "null pointer");
    REFUSED(c.x_trial = nullptr, "null pointer");
    REFUSED(c.h = nullptr, "null pointer");
    REFUSED(c.logr = nullptr, "null pointer");
    REFUSED(c.xs = nullptr, "null pointer");
    REFUSED(c.lps = nullptr, "null pointer");
    REFUSED(c.status = nullptr, "null pointer");
    REFUSED(c.n_prop = nullptr, "null pointer");
    REFUSED(c.n_acc = nullptr, "null pointer");
    delete ctx;
    printf(failures ? "boxchain_args_check: %d FAILED\n" : "boxchain_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
