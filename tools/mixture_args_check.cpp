// Host-side argument checking of csrc/mixture.hip under AddressSanitizer / UBSan, without a device: every call below returns
// before a launch (count = 0, or a bad argument).  Build and run on a CPU (from the repository root):
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         tools/mixture_args_check.cpp -x hip dgp_amd/csrc/mixture.hip -o build/mixture_args_check && build/mixture_args_check
#include <math.h>
#include <stdio.h>

#include "../dgp_amd/csrc/common.hpp"

static int failures = 0;
#define EXPECT(call, want)                                                                  \
    do {                                                                                    \
        const int rc__ = (call);                                                            \
        if (rc__ != (want)) {                                                               \
            printf("FAIL %s -> %d, expected %d (%s)\n", #call, rc__, (want), ctx->err);     \
            ++failures;                                                                     \
        }                                                                                   \
    } while (0)

int main() {
    dgpamd_ctx *ctx = new dgpamd_ctx();
    ctx->stream = nullptr;
    double one[1] = {0.5}, z[1] = {0.0}, bad_p[2] = {0.5, 1.0}, nan_p[1] = {NAN}, zz[2] = {0.0, 0.0};
    double many[DGPAMD_MIX_MAXT + 1];
    for (int t = 0; t <= DGPAMD_MIX_MAXT; ++t) many[t] = 0.5;
    int32_t info = 0;
    // count = 0: nothing to do, whatever the pointers
    EXPECT(dgpamd_mixture_eval(ctx, DGPAMD_MIX_CDF, 3, 0, 2, nullptr, nullptr, nullptr, 2, nullptr), DGPAMD_OK);
    EXPECT(dgpamd_mixture_eval(ctx, DGPAMD_MIX_LOGPDF, 3, 0, 2, nullptr, nullptr, nullptr, 0, nullptr), DGPAMD_OK);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 0, 1, nullptr, nullptr, one, z, 0, nullptr, nullptr), DGPAMD_OK);
    EXPECT(dgpamd_mixture_quantile(ctx, 200, 0, 1, nullptr, nullptr, one, z, 2, nullptr, nullptr), DGPAMD_OK);
    EXPECT(dgpamd_mixture_crps(ctx, 3, 0, nullptr, nullptr, nullptr, 0, nullptr), DGPAMD_OK);
    // bad arguments: refused before any launch
    EXPECT(dgpamd_mixture_eval(nullptr, DGPAMD_MIX_CDF, 3, 0, 2, nullptr, nullptr, nullptr, 2, nullptr), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_eval(ctx, 7, 3, 4, 2, one, one, one, 2, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_eval(ctx, DGPAMD_MIX_SF, 0, 4, 2, one, one, one, 2, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_eval(ctx, DGPAMD_MIX_SF, 3, 4, 0, one, one, one, 0, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_eval(ctx, DGPAMD_MIX_SF, 3, -1, 2, one, one, one, 2, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_eval(ctx, DGPAMD_MIX_SF, 3, 4, 2, one, one, one, 1, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_eval(ctx, DGPAMD_MIX_SF, 3, 4, 2, nullptr, one, one, 2, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 0, 4, 1, one, one, one, z, 0, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 4, 0, one, one, one, z, 0, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 4, 2, one, one, bad_p, zz, 0, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 4, 1, one, one, nan_p, z, 0, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 4, 1, one, one, one, nan_p, 0, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 4, 1, one, one, nullptr, z, 0, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 4, DGPAMD_MIX_MAXT + 1, one, one, many, many, 0, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 4, 1, one, one, one, z, 3, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 200, 4, 1, one, one, one, z, 1, one, &info), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_quantile(ctx, 3, 4, 1, one, one, one, z, 0, one, nullptr), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_crps(ctx, 0, 4, one, one, one, 0, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_crps(ctx, 3, -2, one, one, one, 0, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_crps(ctx, 3, 4, one, one, one, -1, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_crps(ctx, 161, 4, one, one, one, 1, one), DGPAMD_BAD_ARG);
    EXPECT(dgpamd_mixture_crps(ctx, 3, 4, one, one, nullptr, 0, one), DGPAMD_BAD_ARG);
    delete ctx;
    printf(failures ? "mixture_args_check: %d FAILED\n" : "mixture_args_check: ok\n", failures);
    return failures ? 1 : 0;
}
