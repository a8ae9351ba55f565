// Host-side argument checking of csrc/boxsus.hip under AddressSanitizer / UBSan, without a device: every call below returns
// before a launch (a bad argument).  The two entry points need no workspace (the state is named tensors of the caller's), so
// there is no formula to check beside the sizes; what is checked instead is that the host copy of par is read inside its
// 4 D doubles (the arrays below end where par ends, so a read past it is the sanitizer's).  Build and run on a CPU (from the
// repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/boxsus_args_check.cpp \
//         -x hip dgp_amd/csrc/boxsus.hip -o build/boxsus_args_check && build/boxsus_args_check
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../dgp_amd/csrc/common.hpp"

static int failures = 0;
static dgpamd_ctx *ctx;

enum { D = 2, K = 3, NPAR = 4 * D };
// par: pv (D), pm (D), lo (D), hi (D); a flat column's pm is not read
static const double good[NPAR] = {0.5, 0.0, 0.1, NAN, -1.0, 0.0, 1.0, 0.0};

struct Move {
    dgpamd_ctx *ctx;
    int64_t P, R;
    int D, K, output;
    double sign, threshold;
    const double *f, *par, *par_h, *level, *lam, *sd, *z, *logu;
    double *x_trial, *x, *score;
    int32_t *moved, *status, *n_prop, *n_acc;
};
struct Level {
    dgpamd_ctx *ctx;
    int64_t P, R;
    int D, n_s;
    double min_prob;
    const double *score, *x;
    double *prob, *level;
    int32_t *nsurv, *done, *status, *anc;
    double *x_trial, *sd;
    int32_t *running;
};

// each combination of first and last, which the checks do not depend on: the common return code, or -999 if the four differ
static int move(const Move &c) {
    int rc[4];
    for (int i = 0; i < 4; ++i)
        rc[i] = dgpamd_boxsus_move(c.ctx, c.P, c.R, c.D, c.K, c.output, c.sign, c.threshold, c.f, c.par, c.par_h, c.level, c.lam, c.sd,
                                   c.z, c.logu, i & 1, i >> 1, c.x_trial, c.x, c.score, c.moved, c.status, c.n_prop, c.n_acc);
    return rc[0] == rc[1] && rc[1] == rc[2] && rc[2] == rc[3] ? rc[0] : -999;
}
static int level(const Level &c) {
    return dgpamd_boxsus_level(c.ctx, c.P, c.R, c.D, c.n_s, c.min_prob, c.score, c.x, c.prob, c.level, c.nsurv, c.done, c.status,
                               c.anc, c.x_trial, c.sd, c.running);
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
        refused(move(c), "dgpamd_boxsus_move", #change, text, c.ctx != nullptr); \
    } while (0)
#define LEVEL_REFUSED(change, text)                                              \
    do {                                                                         \
        Level c = lok;                                                           \
        change;                                                                  \
        ctx->err[0] = 0;                                                         \
        refused(level(c), "dgpamd_boxsus_level", #change, text, c.ctx != nullptr); \
    } while (0)

int main() {
    ctx = new dgpamd_ctx();
    ctx->stream = nullptr;
    ctx->err[0] = 0;
    double d[8] = {0};                                          // stands for every device pointer: never dereferenced before a launch
    int32_t n[1] = {0};
    static_assert(DGPAMD_BOXSUS_OK == 0 && DGPAMD_BOXSUS_NAN == 1 && DGPAMD_BOXSUS_MAX_STAGES == 2 && DGPAMD_BOXSUS_BELOW_MIN == 3 &&
                      DGPAMD_BOXSUS_COUNT == 4 && DGPAMD_BOXSUS_MAXR == 8192,
                  "the numbers that ops.py and tests/boxsus_ref.py restate");
    // the host copy of par on the heap, exactly 4 D doubles: a read past it is reported
    std::vector<double> heap(good, good + NPAR);

    const Move ok = {ctx, 2, 3, D, K, 1, 1.0, 0.25, d, d, heap.data(), d, d, d, d, d, d, d, d, n, n, n, n};
    const char *sizes = "need P >= 1, 1 <= R <= DGPAMD_BOXSUS_MAXR, P R < 2^31 and 1 <= D <= DGPAMD_MAXD";
    MOVE_REFUSED(c.ctx = nullptr, "");
    MOVE_REFUSED(c.P = 0, sizes);
    MOVE_REFUSED(c.P = -3, sizes);
    MOVE_REFUSED(c.R = 0, sizes);
    MOVE_REFUSED(c.R = DGPAMD_BOXSUS_MAXR + 1, sizes);
    MOVE_REFUSED((c.P = 1LL << 18, c.R = DGPAMD_BOXSUS_MAXR), sizes);              // P R = 2^31
    MOVE_REFUSED((c.P = 1LL << 62, c.R = 8), sizes);                               // (P R would overflow)
    MOVE_REFUSED(c.D = 0, sizes);
    MOVE_REFUSED(c.D = DGPAMD_MAXD + 1, sizes);
    const char *outputs = "need K >= 1 and 0 <= output < K";
    MOVE_REFUSED(c.K = 0, outputs);
    MOVE_REFUSED(c.output = -1, outputs);
    MOVE_REFUSED(c.output = K, outputs);
    for (double b : {0.0, 0.5, -2.0, (double)NAN, (double)INFINITY}) MOVE_REFUSED(c.sign = b, "sign must be +1 or -1");
    for (double b : {(double)NAN, (double)INFINITY, -(double)INFINITY}) MOVE_REFUSED(c.threshold = b, "threshold must be finite");
    std::vector<double> par(good, good + NPAR);
    par[0] = -1.0;
    MOVE_REFUSED(c.par_h = par.data(), "every pv must be a number >= 0");
    par[0] = NAN;
    MOVE_REFUSED(c.par_h = par.data(), "every pv must be a number >= 0");
    par.assign(good, good + NPAR);
    par[2 * D + 1] = 2.0;                                                          // lo_1 > hi_1
    MOVE_REFUSED(c.par_h = par.data(), "every bound must be a number with lo <= hi");
    par.assign(good, good + NPAR);
    par[3 * D] = NAN;
    MOVE_REFUSED(c.par_h = par.data(), "every bound must be a number with lo <= hi");
    MOVE_REFUSED(c.f = nullptr, "null pointer");
    MOVE_REFUSED(c.par = nullptr, "null pointer");
    MOVE_REFUSED(c.par_h = nullptr, "null pointer");
    MOVE_REFUSED(c.level = nullptr, "null pointer");
    MOVE_REFUSED(c.lam = nullptr, "null pointer");
    MOVE_REFUSED(c.sd = nullptr, "null pointer");
    MOVE_REFUSED(c.z = nullptr, "null pointer");
    MOVE_REFUSED(c.logu = nullptr, "null pointer");
    MOVE_REFUSED(c.x_trial = nullptr, "null pointer");
    MOVE_REFUSED(c.x = nullptr, "null pointer");
    MOVE_REFUSED(c.score = nullptr, "null pointer");
    MOVE_REFUSED(c.moved = nullptr, "null pointer");
    MOVE_REFUSED(c.status = nullptr, "null pointer");
    MOVE_REFUSED(c.n_prop = nullptr, "null pointer");
    MOVE_REFUSED(c.n_acc = nullptr, "null pointer");

    const Level lok = {ctx, 2, 3, D, 1, 1e-12, d, d, d, d, n, n, n, n, d, d, n};
    LEVEL_REFUSED(c.ctx = nullptr, "");
    LEVEL_REFUSED(c.P = 0, sizes);
    LEVEL_REFUSED(c.R = 0, sizes);
    LEVEL_REFUSED(c.R = DGPAMD_BOXSUS_MAXR + 1, sizes);
    LEVEL_REFUSED((c.P = 1LL << 18, c.R = DGPAMD_BOXSUS_MAXR), sizes);
    LEVEL_REFUSED(c.D = 0, sizes);
    LEVEL_REFUSED(c.D = DGPAMD_MAXD + 1, sizes);
    const char *ranks = "need 1 <= n_s < R";
    LEVEL_REFUSED(c.n_s = 0, ranks);
    LEVEL_REFUSED(c.n_s = -1, ranks);
    LEVEL_REFUSED(c.n_s = 3, ranks);
    LEVEL_REFUSED((c.R = 1, c.n_s = 1), ranks);                                    // one particle has no level to take
    LEVEL_REFUSED((c.R = DGPAMD_BOXSUS_MAXR, c.n_s = DGPAMD_BOXSUS_MAXR), ranks);
    for (double b : {1.0, -0.5, 1.5, (double)NAN, (double)INFINITY}) LEVEL_REFUSED(c.min_prob = b, "need 0 <= min_prob < 1");
    LEVEL_REFUSED(c.score = nullptr, "null pointer");
    LEVEL_REFUSED(c.x = nullptr, "null pointer");
    LEVEL_REFUSED(c.prob = nullptr, "null pointer");
    LEVEL_REFUSED(c.level = nullptr, "null pointer");
    LEVEL_REFUSED(c.nsurv = nullptr, "null pointer");
    LEVEL_REFUSED(c.done = nullptr, "null pointer");
    LEVEL_REFUSED(c.status = nullptr, "null pointer");
    LEVEL_REFUSED(c.anc = nullptr, "null pointer");
    LEVEL_REFUSED(c.x_trial = nullptr, "null pointer");
    LEVEL_REFUSED(c.sd = nullptr, "null pointer");
    LEVEL_REFUSED(c.running = nullptr, "null pointer");
    delete ctx;
    printf(failures ? "boxsus_args_check: %d FAILED\n" : "boxsus_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
