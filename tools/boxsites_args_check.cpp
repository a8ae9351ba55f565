// Host-side argument checking of csrc/boxsites.hip under AddressSanitizer / UBSan, without a device: every call below returns
// before a launch (a bad argument).  Build and run on a CPU (from the repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined tools/boxsites_args_check.cpp \
//         -x hip dgp_amd/csrc/boxsites.hip -o build/boxsites_args_check && build/boxsites_args_check
#include <stdio.h>
#include <string.h>

#include "../dgp_amd/csrc/common.hpp"

static int failures = 0;
static dgpamd_ctx *ctx;

struct Call {
    dgpamd_ctx *ctx;
    int64_t Q;
    int T, K, Dx, Dt;
    const int32_t *cols, *cols_h;
    const double *Wt, *f, *J;
    double *ft, *Jt;
};

static void refused(const Call &c, const char *what, const char *text) {
    char want[256];
    snprintf(want, sizeof want, "dgpamd_boxsites_fold: %s", text);
    ctx->err[0] = 0;
    const int rc = dgpamd_boxsites_fold(c.ctx, c.Q, c.T, c.K, c.Dx, c.Dt, c.cols, c.cols_h, c.Wt, c.f, c.J, c.ft, c.Jt);
    if (rc != DGPAMD_BAD_ARG || (c.ctx && strcmp(ctx->err, want))) {
        printf("FAIL %s -> %d \"%s\", expected %d \"%s\"\n", what, rc, ctx->err, DGPAMD_BAD_ARG, want);
        ++failures;
    }
}
// a call that differs from an accepted one by `change`
#define REFUSED(change, text)      \
    do {                           \
        Call c = ok;               \
        change;                    \
        refused(c, #change, text); \
    } while (0)

int main() {
    ctx = new dgpamd_ctx();
    ctx->stream = nullptr;
    ctx->err[0] = 0;
    double d[8] = {0};                                          // stands for every device pointer: never dereferenced before a launch
    int32_t dc[1] = {0};
    static int32_t good[DGPAMD_MAXD + 1];
    for (int i = 0; i <= DGPAMD_MAXD; ++i) good[i] = DGPAMD_MAXD - i;      // distinct, not increasing
    const Call ok = {ctx, 4, 5, 3, 70, 3, dc, good, d, d, d, d, d};
    // sizes
    REFUSED(c.ctx = nullptr, "");
    REFUSED(c.Q = 0, "need 1 <= Q < 2^31");
    REFUSED(c.Q = -1, "need 1 <= Q < 2^31");
    REFUSED(c.Q = 1LL << 31, "need 1 <= Q < 2^31");
    REFUSED(c.T = 0, "need 1 <= T <= DGPAMD_BOXSITES_MAXT");
    REFUSED(c.T = DGPAMD_BOXSITES_MAXT + 1, "need 1 <= T <= DGPAMD_BOXSITES_MAXT");
    REFUSED(c.K = 0, "need 1 <= K <= 65535");
    REFUSED(c.K = 65536, "need 1 <= K <= 65535");
    REFUSED(c.Dx = 0, "need Dx >= 1");
    REFUSED(c.Dt = -1, "need 0 <= Dt <= min(Dx, DGPAMD_MAXD)");
    REFUSED(c.Dt = DGPAMD_MAXD + 1, "need 0 <= Dt <= min(Dx, DGPAMD_MAXD)");
    REFUSED((c.Dx = 2, c.Dt = 3), "need 0 <= Dt <= min(Dx, DGPAMD_MAXD)");
    REFUSED((c.Q = 0x7fffffffLL, c.T = 256, c.K = 8, c.Dx = 1 << 20), "Q T K Dx is too large");       // 2^62: no wrap
    REFUSED((c.Q = 0x7fffffffLL, c.T = 256, c.K = 65535, c.Dx = 0x7fffffff), "Q T K Dx is too large");
    // the host copy of cols: out of range, named twice (the last column of a full set included)
    const char *range = "every column must lie in 0 .. Dx - 1", *twice = "a column is named twice";
    {
        int32_t bad[3] = {0, 70, 1};
        REFUSED(c.cols_h = bad, range);
        bad[1] = -1;
        REFUSED(c.cols_h = bad, range);
        bad[1] = 0;
        REFUSED(c.cols_h = bad, twice);
        bad[1] = 2, bad[2] = 2;
        REFUSED(c.cols_h = bad, twice);
        int32_t full[DGPAMD_MAXD];
        for (int i = 0; i < DGPAMD_MAXD; ++i) full[i] = i;
        full[DGPAMD_MAXD - 1] = 0;
        REFUSED((c.Dt = DGPAMD_MAXD, c.cols_h = full), twice);
        REFUSED((c.Dt = DGPAMD_MAXD, c.Dx = DGPAMD_MAXD, c.cols_h = good), range);       // good[0] = 64 = Dx
    }
    // a null pointer in every position; with Dt = 0 the Jacobian's four are not read, the others still are
    REFUSED(c.cols = nullptr, "null pointer");
    REFUSED(c.cols_h = nullptr, "null pointer");
    REFUSED(c.Wt = nullptr, "null pointer");
    REFUSED(c.f = nullptr, "null pointer");
    REFUSED(c.J = nullptr, "null pointer");
    REFUSED(c.ft = nullptr, "null pointer");
    REFUSED(c.Jt = nullptr, "null pointer");
    REFUSED((c.Dt = 0, c.cols = nullptr, c.cols_h = nullptr, c.J = nullptr, c.Jt = nullptr, c.Wt = nullptr), "null pointer");
    REFUSED((c.Dt = 0, c.f = nullptr), "null pointer");
    REFUSED((c.Dt = 0, c.ft = nullptr), "null pointer");
    delete ctx;
    printf(failures ? "boxsites_args_check: %d FAILED\n" : "boxsites_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
