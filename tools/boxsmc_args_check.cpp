// Host-side argument checking of csrc/boxsmc.hip under AddressSanitizer / UBSan, without a device: every call below returns
// before a launch (a bad argument), and the workspace formula is plain host arithmetic.  The checks that dgpamd_boxsmc_move
// shares with the chains are csrc/boxchain.hpp's (tools/boxchain_args_check.cpp runs their table); here: that they are reached
// under this entry point's name, and the cases of its own and of dgpamd_boxsmc_temper.  Build and run on a CPU (from the
// repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/boxsmc_args_check.cpp \
//         -x hip dgp_amd/csrc/boxsmc.hip -o build/boxsmc_args_check && build/boxsmc_args_check
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

struct Move {
    dgpamd_ctx *ctx;
    int64_t P, R;
    int D, K;
    const double *f, *J, *par, *par_h, *beta, *z, *logu;
    double hmin, hmax, up, down;
    void *work;
    double *x_trial, *x, *ll, *lprior, *h, *logr;
    int32_t *status, *n_prop, *n_acc;
};
struct Temper {
    dgpamd_ctx *ctx;
    int64_t P, R;
    int D;
    double ess_frac;
    const double *ll, *x, *u;
    double *beta, *dbeta, *log_evidence, *stage_ess;
    int32_t *status, *anc;
    double *x_trial;
    int32_t *running;
};

// each combination of first and last, which the checks do not depend on: the common return code, or -999 if the four differ
static int move(const Move &c) {
    int rc[4];
    for (int i = 0; i < 4; ++i)
        rc[i] = dgpamd_boxsmc_move(c.ctx, c.P, c.R, c.D, c.K, c.f, c.J, c.par, c.par_h, c.beta, c.z, c.logu, c.hmin, c.hmax, c.up,
                                   c.down, i & 1, i & 1, i >> 1, c.work, c.x_trial, c.x, c.ll, c.lprior, c.h, c.logr, c.status,
                                   c.n_prop, c.n_acc);
    return rc[0] == rc[1] && rc[1] == rc[2] && rc[2] == rc[3] ? rc[0] : -999;
}
static int temper(const Temper &c) {
    return dgpamd_boxsmc_temper(c.ctx, c.P, c.R, c.D, c.ess_frac, c.ll, c.x, c.u, c.beta, c.dbeta, c.log_evidence, c.stage_ess,
                                c.status, c.anc, c.x_trial, c.running);
}

static void refused(int rc, const char *name, const char *what, const char *text, bool has_ctx) {
    char want[256];
    snprintf(want, sizeof want, "%s: %s", name, text);
    if (rc != DGPAMD_BAD_ARG || (has_ctx && strcmp(ctx->err, want))) {
        printf("FAIL %s with %s -> %d \"%s\", expected %d \"%s\"\n", name, what, rc, ctx->err, DGPAMD_BAD_ARG, want);
        ++failures;
    }
}
// a call that differs from an accepted one by `change`
#define MOVE_REFUSED(change, text)                                             \
    do {                                                                       \
        Move c = ok;                                                           \
        change;                                                                \
        ctx->err[0] = 0;                                                       \
        refused(move(c), "dgpamd_boxsmc_move", #change, text, c.ctx != nullptr); \
    } while (0)
#define TEMPER_REFUSED(change, text)                                               \
    do {                                                                           \
        Temper c = tok;                                                            \
        change;                                                                    \
        ctx->err[0] = 0;                                                           \
        refused(temper(c), "dgpamd_boxsmc_temper", #change, text, c.ctx != nullptr); \
    } while (0)

int main() {
    ctx = new dgpamd_ctx();
    ctx->stream = nullptr;
    ctx->err[0] = 0;
    double d[8] = {0};                                          // stands for every device pointer: never dereferenced before a launch
    int32_t n[1] = {0};
    // the workspace formula: g and g' as doubles and one int32, per particle
    EXPECT(dgpamd_boxsmc_workspace(1, 1, 1), 16 + 4);
    EXPECT(dgpamd_boxsmc_workspace(26, 5, 5), 130LL * (16 * 5 + 4));
    EXPECT(dgpamd_boxsmc_workspace(100, DGPAMD_BOXSMC_MAXR, 64), 100LL * DGPAMD_BOXSMC_MAXR * (16 * 64 + 4));
    EXPECT(dgpamd_boxsmc_workspace(0, 5, 5), 0);
    EXPECT(dgpamd_boxsmc_workspace(-3, 5, 5), 0);
    EXPECT(dgpamd_boxsmc_workspace(4, 0, 5), 0);
    EXPECT(dgpamd_boxsmc_workspace(4, DGPAMD_BOXSMC_MAXR + 1, 5), 0);
    EXPECT(dgpamd_boxsmc_workspace(1LL << 31, 1, 5), 0);
    EXPECT(dgpamd_boxsmc_workspace(1LL << 18, DGPAMD_BOXSMC_MAXR, 5), 0);     // P R = 2^31
    EXPECT(dgpamd_boxsmc_workspace(1LL << 62, 8, 5), 0);                      // (P R would overflow)
    EXPECT(dgpamd_boxsmc_workspace(4, 5, 0), 0);
    EXPECT(dgpamd_boxsmc_workspace(4, 5, DGPAMD_MAXD + 1), 0);

    const Move ok = {ctx, 2, 3, D, K, d, d, d, good, d, d, d, 1e-10, 1e2, 1.5, 0.5, d, d, d, d, d, d, d, n, n, n};
    const char *sizes = "need P >= 1, 1 <= R <= DGPAMD_BOXSMC_MAXR and P R < 2^31";
    MOVE_REFUSED(c.ctx = nullptr, "");
    MOVE_REFUSED(c.P = 0, sizes);
    MOVE_REFUSED(c.R = 0, sizes);
    MOVE_REFUSED(c.R = DGPAMD_BOXSMC_MAXR + 1, sizes);
    MOVE_REFUSED((c.P = 1LL << 18, c.R = DGPAMD_BOXSMC_MAXR), sizes);
    MOVE_REFUSED((c.P = 1LL << 62, c.R = 8), sizes);
    MOVE_REFUSED(c.beta = nullptr, "null pointer");
    MOVE_REFUSED(c.x = nullptr, "null pointer");
    MOVE_REFUSED(c.ll = nullptr, "null pointer");
    MOVE_REFUSED(c.lprior = nullptr, "null pointer");
    // the chains' checks, reached under this name
    MOVE_REFUSED(c.D = 0, "need 1 <= D <= DGPAMD_MAXD");
    MOVE_REFUSED(c.D = DGPAMD_MAXD + 1, "need 1 <= D <= DGPAMD_MAXD");
    MOVE_REFUSED(c.K = 0, "need K >= 1");
    const char *scalar = "h0, hmin, hmax, up and down must be positive and finite";
    for (double b : {0.0, -1.0, (double)NAN, (double)INFINITY}) {
        MOVE_REFUSED(c.hmin = b, scalar);
        MOVE_REFUSED(c.hmax = b, scalar);
        MOVE_REFUSED(c.up = b, scalar);
        MOVE_REFUSED(c.down = b, scalar);
    }
    MOVE_REFUSED((c.hmin = 1.0, c.hmax = 0.5), "need hmin <= hmax");
    double par[NPAR];
    memcpy(par, good, sizeof par);
    par[0] = -1.0;
    MOVE_REFUSED(c.par_h = par, "every weight w must be a number >= 0");
    memcpy(par, good, sizeof par);
    par[2 * K + 3 * D] = 2.0;
    MOVE_REFUSED(c.par_h = par, "every bound must be a number with lo <= hi");
    MOVE_REFUSED(c.f = nullptr, "null pointer");
    MOVE_REFUSED(c.J = nullptr, "null pointer");
    MOVE_REFUSED(c.par = nullptr, "null pointer");
    MOVE_REFUSED(c.par_h = nullptr, "null pointer");
    MOVE_REFUSED(c.z = nullptr, "null pointer");
    MOVE_REFUSED(c.logu = nullptr, "null pointer");
    MOVE_REFUSED(c.work = nullptr, "null pointer");
    MOVE_REFUSED(c.x_trial = nullptr, "null pointer");
    MOVE_REFUSED(c.h = nullptr, "null pointer");
    MOVE_REFUSED(c.logr = nullptr, "null pointer");
    MOVE_REFUSED(c.status = nullptr, "null pointer");
    MOVE_REFUSED(c.n_prop = nullptr, "null pointer");
    MOVE_REFUSED(c.n_acc = nullptr, "null pointer");

    const Temper tok = {ctx, 2, 3, D, 0.5, d, d, d, d, d, d, d, n, n, d, n};
    const char *tsizes = "need P >= 1, 1 <= R <= DGPAMD_BOXSMC_MAXR, P R < 2^31 and 1 <= D <= DGPAMD_MAXD";
    TEMPER_REFUSED(c.ctx = nullptr, "");
    TEMPER_REFUSED(c.P = 0, tsizes);
    TEMPER_REFUSED(c.R = 0, tsizes);
    TEMPER_REFUSED(c.R = DGPAMD_BOXSMC_MAXR + 1, tsizes);
    TEMPER_REFUSED((c.P = 1LL << 18, c.R = DGPAMD_BOXSMC_MAXR), tsizes);
    TEMPER_REFUSED(c.D = 0, tsizes);
    TEMPER_REFUSED(c.D = DGPAMD_MAXD + 1, tsizes);
    for (double b : {0.0, 1.0, -0.5, 1.5, (double)NAN, (double)INFINITY})
        TEMPER_REFUSED(c.ess_frac = b, "need 0 < ess_frac < 1");
    TEMPER_REFUSED(c.ll = nullptr, "null pointer");
    TEMPER_REFUSED(c.x = nullptr, "null pointer");
    TEMPER_REFUSED(c.u = nullptr, "null pointer");
    TEMPER_REFUSED(c.beta = nullptr, "null pointer");
    TEMPER_REFUSED(c.dbeta = nullptr, "null pointer");
    TEMPER_REFUSED(c.log_evidence = nullptr, "null pointer");
    TEMPER_REFUSED(c.stage_ess = nullptr, "null pointer");
    TEMPER_REFUSED(c.status = nullptr, "null pointer");
    TEMPER_REFUSED(c.anc = nullptr, "null pointer");
    TEMPER_REFUSED(c.x_trial = nullptr, "null pointer");
    TEMPER_REFUSED(c.running = nullptr, "null pointer");
    delete ctx;
    printf(failures ? "boxsmc_args_check: %d FAILED\n" : "boxsmc_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
