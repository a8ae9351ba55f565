// The plan of the linked-GP predictor (csrc/linkgp_plan.hpp, with the LDS layouts of csrc/linkgp.hpp) over a grid of calls, under
// AddressSanitizer / UBSan, without a device and without HIP: the plan is plain host arithmetic.  For every point: the launch's LDS
// fits a CU or the call is refused, as the byte formulas the dispatch used to carry (restated below, independently of the layouts)
// say; the chunk is a positive multiple of TCH within MC_MAX; the records of a chunk fit the workspace; the form is the one the
// comments promise.  Build and run on a CPU (from the repository root):
//   c++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/linkgp_plan_check.cpp -o build/linkgp_plan_check
//   build/linkgp_plan_check
#include <stdio.h>

#include "../dgp_amd/csrc/linkgp_plan.hpp"

static int failures = 0;
static long long points = 0;
#define CHECK(cond)                                                                                                             \
    do {                                                                                                                        \
        if (!(cond) && ++failures <= 20)                                                                                        \
            printf("FAIL %s: kind %d n %lld M %lld Dw %d Dz %d loo %d direct %d jsep_tch %lld jsexp_tch %lld pair_chunk %lld\n", \
                   #cond, kind, (long long)n, (long long)M, Dw, Dz, loo, direct, (long long)sw.jsep_tch, (long long)sw.jsexp_tch, \
                   (long long)sw.pair_chunk);                                                                                   \
    } while (0)

// the dynamic LDS of each pair kernel as the dispatch computed it before the layouts existed
static size_t old_j_lds(int kind, int Dw, int Dz, int tc, bool loo) {
    size_t s = ((size_t)2 * (Dw + Dz) * 64 + (size_t)tc * (2 * Dw + Dz) + tc * 4) * sizeof(double);
    if (kind == DGPAMD_MATERN25) s += 64 * 65 * sizeof(double);
    if (loo) s += ((size_t)2 * tc * 64 + 128 + 2 * tc) * sizeof(double);
    return s;
}
static size_t old_sexp_lds(int Dw, int Dz) {
    const int KP = (Dw + 3) & ~3, LDU = KP + 2;
    return ((size_t)2 * (Dw + Dz) * 64 + (size_t)KP * 80 + (size_t)32 * (2 * Dw + Dz) + 32 * 4 + 2 * 64 * LDU + 4 * 64 + Dz) * sizeof(double);
}
static size_t old_sexp2_lds(int Dw, int tch) { return ((size_t)2 * Dw * 64 + tch * 4 + 256) * sizeof(double); }
static size_t old_sep_lds(int Dw, int Dz, int tch, bool log) {
    return ((size_t)2 * (Dw + Dz) * 64 + (size_t)tch * Dz + tch * 4 + 2 * 128 * 30) * sizeof(double) + (size_t)Dw * 4 * sizeof(int) +
           (log ? 16 + 48 * 8 * sizeof(long long) : 0);
}

static void check(const LinkSwitches &sw, int kind, int64_t n, int64_t M, int Dw, int Dz, bool loo, bool direct) {
    ++points;
    const LinkPlan p = linkgp_plan(sw, kind, n, M, Dw, Dz, loo, direct);
    const bool sexp = kind == DGPAMD_SEXP, plain = !loo && !direct;
    // the form
    LinkForm want = LINK_DIRECT;
    if (plain && !sexp) want = LINK_MATERN_SEP;
    if (plain && sexp) want = Dw <= 14 ? LINK_SEXP_RECORDS : (old_sexp_lds(Dw, Dz) <= LDS_CU_BYTES ? LINK_SEXP_MFMA : LINK_DIRECT);
    CHECK(p.form == want);
    if (plain && sexp && Dz == 0) CHECK((p.form == LINK_SEXP_MFMA) == (Dw >= 15 && Dw <= 48));   // "to Dw = 39..48, by Dz": 48 without global inputs
    if (plain && sexp && Dz == 24) CHECK((p.form == LINK_SEXP_MFMA) == (Dw >= 15 && Dw <= 39));  // ... 39 with 24 of them
    // the points per workgroup and the LDS: what the old formulas give, within a CU or refused
    size_t lds = 0;
    int tc = TCH;
    switch (want) {
        case LINK_DIRECT:
            if (loo && !sexp && old_j_lds(kind, Dw, Dz, TCH, loo) > LDS_CU_BYTES) tc = TCH / 2;
            if (loo && !sexp && Dz == 0) CHECK((p.tc == TCH / 2) == (Dw >= 63));   // "Matern leave-one-out from Dw + Dz = 63 on"
            lds = old_j_lds(kind, Dw, Dz, tc, loo);
            break;
        case LINK_SEXP_MFMA: lds = old_sexp_lds(Dw, Dz); break;
        case LINK_SEXP_RECORDS:
            tc = sw.jsexp_tch ? (int)sw.jsexp_tch : sexp_tch2(p.nb);
            lds = old_sexp2_lds(Dw, tc);
            break;
        case LINK_MATERN_SEP:
            tc = sw.jsep_tch ? (int)sw.jsep_tch : TCHS;
            lds = old_sep_lds(Dw, Dz, tc, sw.jsep_log != 0);
            break;
    }
    CHECK(p.tc == tc);
    CHECK(p.lds == lds);
    CHECK(p.refused() == (lds > LDS_CU_BYTES));
    if (sw.jsep_tch == 0 && sw.jsexp_tch == 0) CHECK(!p.refused());   // (the built-in geometry always fits)
    // the chunk
    CHECK(p.Mc > 0 && p.Mc % TCH == 0 && p.Mc <= MC_MAX);
    CHECK(p.nb == (n + 63) / 64 && p.ntiles == p.nb * (p.nb + 1) / 2);
    CHECK(p.partial_doubles >= (int64_t)p.ntiles * p.Mc);
    // the workspace covers the partial sums and one chunk's records, the per-point global terms behind them
    CHECK((size_t)(p.partial_doubles + p.rec_doubles) * sizeof(double) <= linkgp_workspace_bytes(n, M, Dw));
    if (want == LINK_SEXP_RECORDS) CHECK(p.KPA % 4 == 0 && p.KPA >= Dw + 2 && p.KPA <= 4 * SX_KS && p.gfac_off == p.Mc * p.nb * 64 * p.KPA && p.gfac_off + p.Mc * p.nb * 64 == p.rec_doubles);
    if (want == LINK_MATERN_SEP) CHECK(p.gfac_off == p.Mc * p.nb * 64 * Dw * REC && p.gfac_off + p.Mc * p.nb * 64 == p.rec_doubles);
}
#undef CHECK

int main() {
    const int64_t ns[] = {1, 64, 65, 2000, 5000}, Ms[] = {1, 31, 300, 2048, 16384};
    const int Dws[] = {1, 14, 15, 39, 48, 49, 62, 63, 64}, Dzs[] = {0, 1, 24};   // (62, 63: the edge of the Matern leave-one-out's half chunk)
    const int64_t over[] = {0, 16, 64, 256, 416};
    for (int kind = DGPAMD_SEXP; kind <= DGPAMD_MATERN25; ++kind)
        for (int64_t n : ns)
            for (int64_t M : Ms)
                for (int Dw : Dws)
                    for (int Dz : Dzs)
                        for (int flags = 0; flags < 4 && Dw + Dz <= DGPAMD_MAXD; ++flags) {
                            LinkSwitches sw;
                            for (int64_t o : over) {   // each override alone, as context.hip lets it through
                                sw = LinkSwitches();
                                sw.jsep_tch = (o >= 8 && o <= 256 && o % 8 == 0) ? o : 0;
                                check(sw, kind, n, M, Dw, Dz, flags & 1, flags >> 1);
                                sw = LinkSwitches();
                                sw.jsexp_tch = (o >= 64 && o <= 256 && (o & (o - 1)) == 0) ? o : 0;
                                check(sw, kind, n, M, Dw, Dz, flags & 1, flags >> 1);
                                sw = LinkSwitches();
                                sw.pair_chunk = o;
                                check(sw, kind, n, M, Dw, Dz, flags & 1, flags >> 1);
                            }
                            sw = LinkSwitches();   // the other switches the plan reads
                            sw.sexp_form1 = sw.jsep_log = 1;
                            const LinkPlan p = linkgp_plan(sw, kind, n, M, Dw, Dz, flags & 1, flags >> 1);
                            if (p.form == LINK_SEXP_RECORDS || p.refused() || p.Mc <= 0 || p.Mc % TCH || p.Mc > MC_MAX ||
                                (size_t)(p.partial_doubles + p.rec_doubles) * sizeof(double) > linkgp_workspace_bytes(n, M, Dw)) {
                                printf("FAIL form1 / log: kind %d n %lld M %lld Dw %d Dz %d flags %d\n", kind, (long long)n, (long long)M, Dw, Dz, flags);
                                ++failures;
                            }
                        }
    // the chunk sizes tests/test_cabi_symbols.py states
    const LinkPlan bench = linkgp_plan(LinkSwitches(), DGPAMD_MATERN25, 2000, 16384, 5, 0, false, false);
    const LinkPlan cfg3 = linkgp_plan(LinkSwitches(), DGPAMD_MATERN25, 5000, 100000, 10, 0, false, false);
    printf("points per launch: n = 2000, Dw = 5: %lld; n = 5000, Dw = 10: %lld\n", (long long)bench.Mc, (long long)cfg3.Mc);
    if (bench.Mc != 1024 || cfg3.Mc != 256) ++failures;
    printf(failures ? "linkgp_plan_check: %lld plans, %d FAILED\n" : "linkgp_plan_check: %lld plans, ok\n", points, failures);
    return failures ? 1 : 0;
}
