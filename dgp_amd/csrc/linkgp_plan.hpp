// The plan of one linked-GP prediction call: which form of the pair kernel serves it, its test points per workgroup, the
// chunk of test points per launch, the launch's dynamic LDS and the records a chunk needs.  linkgp_run launches by it, each
// form's file reads its variant from it, and dgpamd_linkgp_workspace sizes the records with it: the choice is made here, once.
// Plain C++17 (host arithmetic only): a host program includes it without HIP (tools/linkgp_plan_check.cpp).
#pragma once
#include "linkgp.hpp"

enum LinkForm {
    LINK_DIRECT,         // linkgp_J_kernel: the reference's direct form; every leave-one-out call (its weights change per test point)
    LINK_SEXP_MFMA,      // linkgp_Jsexp_kernel: SExp, the first form
    LINK_SEXP_RECORDS,   // sexp_records_kernel + linkgp_Jsexp2_kernel: SExp up to Dw = 14
    LINK_MATERN_SEP      // matern_records_kernel (+ global_factor_kernel) + linkgp_Jsep_kernel
};

// The DGPAMD_* switches the plan reads, at their built-in values.  (common.hpp's Tuning carries the same names.)
struct LinkSwitches {
    int64_t jsep_tch = 0, jsexp_tch = 0, pair_chunk = 0, sexp_form1 = 0, sexp_poly = 0, jsep_pipe = 2, jsep_log = 0, jsep_noclass = 0, jsep_diag = 0;
};

struct LinkPlan {
    LinkForm form;
    int nb, ntiles;            // 64-blocks of training points; lower tiles of C
    int tc;                    // test points per workgroup of the form's pair kernel
    int64_t Mc;                // test points per launch (a positive multiple of TCH, <= MC_MAX)
    size_t lds;                // dynamic LDS of the pair kernel; past LDS_CU_BYTES the call is refused before any launch
    int KPA;                   // LINK_SEXP_RECORDS: doubles per record (k-steps x 4)
    int64_t partial_doubles;   // the partial sums in front of the records: ntiles x (the call's test points, to a multiple of TCH, <= MC_MAX)
    int64_t gfac_off;          // doubles of a chunk's records in front of its per-point global terms (LinkArgs::gfac - recs)
    int64_t rec_doubles;       // doubles of records (gfac included) one chunk needs behind the partial sums; 0: a form without records
    bool loo, poly, plog;      // leave-one-out; Jsexp2: the table-free exponential; Jsep: the step log
    int pipe, no_order_classes;   // Jsep: DGPAMD_JSEP_PIPE; DGPAMD_JSEP_NOCLASS | DGPAMD_JSEP_DIAG
    bool refused() const { return lds > LDS_CU_BYTES; }
};

// Test points per launch of the record-based pair kernels (Matern: linkgp_Jsep_kernel, `per_wg` = TCH; SExp: linkgp_Jsexp2_kernel,
// TCH2).  A launch is ntiles x (points / per_wg) workgroups on the chip's 512 workgroup slots, and its last, ragged round leaves
// slots idle: at n = 2000 with 256 points per launch that was 8.25 rounds and 10 % of the kernel's time (tools/gpu_pair_steplog.py:
// slot occupancy 0.32 over the last tenth of the launch).  >= 32 rounds per launch bound that loss by 1-2 %; the records of a launch
// (Matern: points x Dw x npad x 240 B) are kept under 4 GiB, and a launch never holds fewer than MC_SEP points.
static inline int64_t pair_chunk(int64_t nb, int64_t Mc, int per_wg, int64_t rec_doubles_per_point) {
    const int64_t ntiles = nb * (nb + 1) / 2;
    int64_t want = ((32 * 512 + ntiles - 1) / ntiles) * per_wg;
    const int64_t cap = (((int64_t)4 << 30) / (rec_doubles_per_point * (int64_t)sizeof(double))) / per_wg * per_wg;
    if (want > cap) want = cap;
    if (want < MC_SEP) want = MC_SEP;
    return Mc < want ? Mc : want;
}
// doubles of records per test point: Matern (Dw x npad records of REC + the global factor), SExp second form (npad x (KPA <= 16) + ss)
static inline int64_t matern_rec_doubles(int64_t nb, int Dw) { return (int64_t)(Dw * REC + 1) * nb * 64; }
static inline int64_t sexp_rec_doubles(int64_t nb, int Dw) { return (int64_t)(((Dw + 2 + 3) & ~3) + 1) * nb * 64; }

// Test points per workgroup of linkgp_Jsexp2_kernel: a workgroup's set-up (the tile's weights and base exponents) is amortised over them -- 256 where a launch of
// MC_MAX points still has 32 rounds of workgroups (n = 5000: 28.5 -> 27.4 ms per 2048 points), 128 below (n = 2000: 256 would leave 8 rounds and cost 6 %).
static inline int sexp_tch2(int64_t nb) { return nb * (nb + 1) / 2 * (MC_MAX / 256) >= 32 * 512 ? 256 : TCH2; }

// `Switches`: LinkSwitches or common.hpp's Tuning.  direct_flag: dgpamd_set_linkgp_direct.  tasklog: dgpamd_debug_tasklog's buffer is set.
template <class Switches>
static inline LinkPlan linkgp_plan(const Switches &tn, int kind, int64_t n, int64_t M, int Dw, int Dz, bool loo, bool direct_flag, bool tasklog = false) {
    LinkPlan p;
    p.nb = (int)((n + 63) / 64);
    p.ntiles = p.nb * (p.nb + 1) / 2;
    p.loo = loo;
    p.poly = tn.sexp_poly != 0;   // (comparison run: the table-free exponential)
    p.pipe = (int)tn.jsep_pipe;
    p.plog = tasklog && tn.jsep_log;
    p.no_order_classes = (tn.jsep_noclass ? 1 : 0) | (int)tn.jsep_diag;
    p.KPA = (Dw + 2 + 3) & ~3;
    const int64_t nb = p.nb;
    const bool sexp = kind == DGPAMD_SEXP;
    const bool direct = direct_flag || loo;   // the leave-one-out weights change per test point: direct kernels
    const bool sep = !sexp && !direct;
    const bool sx2 = sexp && !direct && Dw + 2 <= 16;
    // The chunk.  Records of one chunk: Mc*Dw*npad*240 B (Matern), Mc*npad*(Dw+3..6)*8 B (SExp).  Under a DGPAMD_JSEP_TCH / _JSEXP_TCH override the
    // chunk stays within what the built-in points per workgroup give: dgpamd_linkgp_workspace sizes records by the plan of the built-in switches.
    int64_t Mc = ((M + TCH - 1) / TCH) * TCH;
    if (Mc > MC_MAX) Mc = MC_MAX;
    p.partial_doubles = (int64_t)p.ntiles * Mc;
    int tch = tn.jsep_tch ? (int)tn.jsep_tch : TCHS;   // (DGPAMD_JSEP_TCH: comparison runs)
    if (sx2) tch = tn.jsexp_tch ? (int)tn.jsexp_tch : sexp_tch2(nb);
    if (sep || sx2) {
        const int64_t per_point = sep ? matern_rec_doubles(nb, Dw) : sexp_rec_doubles(nb, Dw);
        const int64_t sized = pair_chunk(nb, Mc, sep ? TCHS : sexp_tch2(nb), per_point);
        Mc = pair_chunk(nb, Mc, tch, per_point);
        if (Mc > sized) Mc = sized;
        const int64_t c = tn.pair_chunk;   // (DGPAMD_PAIR_CHUNK, comparison runs: the fixed 256 points per launch of the earlier builds)
        if (c >= TCH && c < Mc) Mc = c / TCH * TCH;
        p.rec_doubles = Mc * per_point;
    } else {
        p.rec_doubles = 0;
    }
    p.Mc = Mc;
    p.gfac_off = Mc * nb * 64 * (sx2 ? (int64_t)p.KPA     // (SExp second form: [Mc][npad][KPA] records, then the ss values)
                                     : (int64_t)Dw * REC);
    // The form.  SExp: the second form up to Dw = 14; the first form (MFMA) above, while it fits in a CU's LDS (to Dw = 39..48, by Dz);
    // past that the direct kernel (99 KB at Dw = 64).
    const size_t lds_mfma = JSexpLds(Dw, Dz).bytes();
    if (sep)
        p.form = LINK_MATERN_SEP;
    else if (sx2 && !tn.sexp_form1)
        p.form = LINK_SEXP_RECORDS;
    else if (sexp && !direct && lds_mfma <= LDS_CU_BYTES)
        p.form = LINK_SEXP_MFMA;
    else
        p.form = LINK_DIRECT;
    switch (p.form) {
        case LINK_MATERN_SEP:
            p.tc = tch;
            p.lds = JSepLds(Dw, Dz, tch).bytes(tn.jsep_log != 0);
            break;
        case LINK_SEXP_RECORDS:
            p.tc = tch;
            p.lds = JSexp2Lds(Dw, tch).bytes();
            break;
        case LINK_SEXP_MFMA:
            p.tc = TCH;
            p.lds = lds_mfma;
            break;
        case LINK_DIRECT:
            // Matern leave-one-out from Dw + Dz = 63 on: past a CU's LDS at TCH test points per workgroup; half of them fit
            p.tc = TCH;
            p.lds = JDirectLds(kind, Dw, Dz, TCH, loo).bytes();
            if (loo && !sexp && p.lds > LDS_CU_BYTES) {
                p.tc = TCH / 2;
                p.lds = JDirectLds(kind, Dw, Dz, p.tc, loo).bytes();
            }
            break;
    }
    return p;
}

// dgpamd_linkgp_workspace: the partial sums plus the records of one launch, the larger of the Matern and the SExp plan's (the call's
// kind is not known there).  No context, no switch: the plans of the built-in switches, and linkgp_plan never puts more points into
// a launch than those do.
static inline size_t linkgp_workspace_bytes(int64_t n, int64_t M, int Dw) {
    const LinkPlan ps = linkgp_plan(LinkSwitches(), DGPAMD_SEXP, n, M, Dw, 0, false, false);
    const LinkPlan pm = linkgp_plan(LinkSwitches(), DGPAMD_MATERN25, n, M, Dw, 0, false, false);
    return (size_t)(pm.partial_doubles + (ps.rec_doubles > pm.rec_doubles ? ps.rec_doubles : pm.rec_doubles)) * sizeof(double);
}

#ifdef __HIPCC__
// One chunk of `mc` test points through the plan's form: set_lds on the kernel of the plan's variant, then its launch (and the
// launches of its records).  The library is built without relocatable device code: each lives in the file of its kernels.
int linkgp_launch_direct(dgpamd_ctx *ctx, const LinkArgs &a, const LinkPlan &p, int64_t mc);         // linkgp_direct.hip
int linkgp_launch_sexp_mfma(dgpamd_ctx *ctx, const LinkArgs &a, const LinkPlan &p, int64_t mc);      // linkgp_sexp.hip
int linkgp_launch_sexp_records(dgpamd_ctx *ctx, const LinkArgs &a, const LinkPlan &p, int64_t mc);   // linkgp_sexp.hip
int linkgp_launch_matern_sep(dgpamd_ctx *ctx, LinkArgs a, const LinkPlan &p, int64_t mc);            // linkgp_matern.hip (sets the chunk's debug fields in its copy)
#endif
