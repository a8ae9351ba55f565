// What the Vecchia translation units share on the host side: the kernel parameters, the argument blocks of the prediction
// kernels (csrc/vecchia_gp.hip: the LDS kernels and the host entries; csrc/vecchia_pred.hip, csrc/vecchia_pred_link_*.hip: the
// register-resident kernels -- translation units of their own: their fully unrolled eliminations take minutes to compile) and
// the launch of a per-KIND kernel.  The device side of the conditioning block is csrc/vblock.hpp.
#pragma once
#include "common.hpp"

struct VParams {
    int kind, D, nlen;
    double inv_len[DGPAMD_MAXD];
    double nugget;
};

static inline int fill_vparams(dgpamd_ctx *ctx, VParams &p, int kind, int D, const double *length_h, int nlen, double nugget) {
    if (kind != DGPAMD_SEXP && kind != DGPAMD_MATERN25) BAD_ARG(ctx, "kind must be 0 or 1");
    if (D <= 0 || D > DGPAMD_MAXD || !length_h || (nlen != 1 && nlen != D)) BAD_ARG(ctx, "bad D / nlen / length");
    p.kind = kind; p.D = D; p.nlen = nlen; p.nugget = nugget;
    for (int d = 0; d < D; ++d) p.inv_len[d] = 1.0 / length_h[nlen == 1 ? 0 : d];
    return DGPAMD_OK;
}

// Debugging aid (DGPAMD_POISON_LDS=1): fill the LDS of every CU with NaNs before a launch, so that a read of LDS the
// kernel has not written shows up in the results whatever ran on the device before (csrc/vecchia_rows.hip)
int maybe_poison_lds(dgpamd_ctx *ctx, const double *any_device_ptr);

// One launch of a kernel that exists once per correlation KIND: the instantiation for `kind`, its LDS opt-in, the poison
// launch of the debugging aid, the launch itself and its check
template <class ARGS>
static inline int launch_by_kind(dgpamd_ctx *ctx, int kind, void (*sexp)(ARGS), void (*matern)(ARGS), dim3 grid, dim3 block,
                                 size_t shm, const ARGS &a, const double *any_device_ptr) {
    void (*fn)(ARGS) = kind == DGPAMD_SEXP ? sexp : matern;
    int rc = set_lds(ctx, (const void *)fn, shm);
    if (rc) return rc;
    rc = maybe_poison_lds(ctx, any_device_ptr);
    if (rc) return rc;
    void *args[] = {const_cast<ARGS *>(&a)};
    HIP_TRY(ctx, hipLaunchKernel((const void *)fn, grid, block, args, shm, ctx->stream));
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

struct VGpArgs {
    VParams vp;
    int64_t M, n;
    int pm;
    const double *x, *w, *y, *nugget_diag;
    const int64_t *NN;
    double scale;
    double *mean, *var;
};

struct VLinkArgs {
    int kind, Dw, Dz, pm;
    int64_t M, n;
    const double *m, *v, *z, *w1, *wg, *y, *nugget_diag;
    const int64_t *NN;
    double len[DGPAMD_MAXD];
    double scale, nugget;
    double *mean, *var;
};

#define VG_BC 51   // neighbours the register-resident gp kernel holds (pm <= VG_BC, D <= 16)
#define VL_BC 50   // neighbours the register-resident link_gp kernel holds (pm <= VL_BC, Dw <= 8, Dz <= 8; both kernels)
void launch_vecchia_gp_reg(dgpamd_ctx *ctx, const VGpArgs &a);
void launch_vecchia_linkgp_sexp_reg(dgpamd_ctx *ctx, const VLinkArgs &a);
void launch_vecchia_linkgp_matern_reg(dgpamd_ctx *ctx, const VLinkArgs &a);
