// The register-resident Vecchia row kernels (conditioning sets of at most VR_MAXB points) with what they share with the LDS row
// kernel of csrc/vecchia_rows.hip: the modes, the argument block, the derivative coefficient.  54 fully unrolled kernels, minutes
// to compile: they are instantiated per correlation kind in a translation unit of their own (csrc/vecchia_row4_sexp.hip,
// csrc/vecchia_row4_matern.hip define VROW4_KIND before including this); everybody else sees launch_vrow4 declared.
#pragma once
#include "common.hpp"
#include "diagfac.hpp"   // (rsqrt_sqrt)
#include "vecchia_pred.hpp"
#include "wave.hpp"

#include <math.h>

template <int KIND>
__device__ __forceinline__ double dcoef_v(double df) {
    if (KIND == DGPAMD_SEXP) return 2.0 * df * df;
    double r = fabs(df);
    double e1 = fma(r, SQRT5, 1.0), e2 = (5.0 / 3.0) * r * r;
    const double den = e1 + e2;   // >= 1: hardware reciprocal + two Newton rounds instead of the ~30-instruction division
    double x = __builtin_amdgcn_rcp(den);
    x = fma(x, fma(-den, x, 1.0), x);
    x = fma(x, fma(-den, x, 1.0), x);
    return e2 * e1 * x;
}

// ---------------------------------------------------------------------------
// a19-a21  per-row kernels on the ordered data
// ---------------------------------------------------------------------------
enum { V_LLIK = 0, V_NLLIK = 1, V_LMAT = 2 };

struct VRowArgs {
    VParams vp;
    int64_t n;
    int m;            // NNarray has m+1 columns
    const double *X, *y, *nugget_diag;
    const int64_t *NN;
    int nugget_est, P;
    double *partial;  // [batch][n][2 + 2P] (LLIK: [batch][n][2])
    double *Lmat;     // [n][m+1]
    int64_t x_stride; // doubles between the input sets of a batch (blockIdx.y); LLIK only
    const int32_t *pred;   // null, or a device word: the launch does nothing when it is non-zero (dgpamd_ess_queue)
    long long *trace = nullptr;   // diagnostics (dgpamd_debug_trace): shader-clock stamps of the first 64 row blocks' phases, 16 words each
};
#define VR4_STAMP(slot)                                                                                               \
    do {                                                                                                              \
        if (a.trace && rowblk < 64 && by == 0 && threadIdx.x == 0) a.trace[rowblk * 16 + (slot)] = (long long)__builtin_amdgcn_s_memtime(); \
    } while (0)

// ---------------------------------------------------------------------------
// The same three per-row computations for conditioning sets of at most 31 points (m <= 30: the default m = 25), held in
// REGISTERS: FOUR rows of the likelihood per wave, one 16-lane DPP row each.  Lane t of a group owns rows t and 16 + t of
// the (m+2) x (m+1) block (the right-hand side rides as row m+1).  Column j of the factor is normalised in place and
// every trailing entry takes  a[r][c] -= l[r] * l[c]  in ONE v_fmac_f64_dpp whose first operand is read from lane
// c mod 16 of the group (row_newbcast) -- no LDS round trips, no shuffles and no barriers inside the factorisation.
// (The LDS version above spends its time on three barriers and a dependent LDS read-modify-write chain per column with
// 40 % of the lanes idle; a version with 32-wide ds_bpermute shuffles was bound by the LDS pipe: 2.9x slower than this.)
// The block itself is assembled with its m(m+1)/2 entries spread evenly over the group and handed over through LDS
// once.  Sets shorter than the compiled size (the first m rows; sizes between the compiled ones) are padded IN FRONT
// with identity rows, so that "self" is always the last slot and the loop bounds are compile-time constants.
// ---------------------------------------------------------------------------
#define VR_MAXB 31

__device__ __forceinline__ void tri_decode_small(int t, int &r, int &c) {   // t < 2^16: float is plenty
    int b = (int)((sqrtf(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
    while ((b + 1) * (b + 2) / 2 <= t) ++b;
    while (b * (b + 1) / 2 > t) --b;
    r = b;
    c = t - b * (b + 1) / 2;
}

__device__ __forceinline__ double hsum16(double v) {   // sum over the 16 lanes of a group, in every lane of it
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) v += __shfl_xor(v, off, 16);
    return v;
}

// the same with four DPP rotations of the 16-lane row (every lane pairs the same values: identical sums in all lanes)
__device__ __forceinline__ double row_allreduce_sum(double v) {
#define ROR_ADD(CTRL)                                                                                 \
    {                                                                                                 \
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, false);      \
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, false);      \
        v += __hiloint2double(hi, lo);                                                                \
    }
    ROR_ADD(0x128) ROR_ADD(0x124) ROR_ADD(0x122) ROR_ADD(0x121)
#undef ROR_ADD
    return v;
}

// value of lane C of the caller's 16-lane group.  s_nop 4: a DPP source written by the previous VALU needs two wait states
// and an EXEC written by the previous SALU (the end of a divergent region: the compiler cannot see into the asm) five.
template <int C>
__device__ __forceinline__ double group_bcast(const double &v) {
    double out;
    asm volatile("s_nop 4\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(out) : "v"(v), "i"(C));
    return out;
}
// acc += (lane C's src) * mul
template <int C>
__device__ __forceinline__ void fmac_bcast(double &acc, const double &src, const double &mul) {
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(mul), "i"(C));
}

// Row stride of the scaled inputs in LDS: the dimensions padded with zeros to a multiple of eight (the pair loop reads whole chunks of
// eight: no index clamps, no selects -- two of the four VALU instructions per pair and dimension), + 2: rows stay 16-byte aligned
// (ds_read_b128) and the sixteen rows a group reads at once fall on disjoint bank quadruples (stride 10: banks 0, 20, 40, 60, 16, ...;
// stride 18: 0, 36, 8, 44, ...).
#define VR4_DP(D) ((((D) + 7) & ~7) + 2)
static size_t vrow4_lds(int BS, int D, bool grad, bool solves) {
    const size_t asz = (size_t)(BS + 1) * (BS + 2) / 2 + (grad ? (size_t)BS * (BS - 1) / 2 : 0);
    return 4 * (asz + (size_t)BS * VR4_DP(D) + (solves ? 2 * 32 : 0)) * sizeof(double);   // (llik: 19.9 KB at m = 25, d = 8: 8 waves per CU)
}

// four rows (row block rb) of input set `by`: the body of vecchia_row4_kernel
template <int KIND, int MODE, int BS>
__device__ __forceinline__ void vrow4_body(const VRowArgs &a, double *lds, const int64_t rowblk, const int by) {
    constexpr int rows = BS + 1;                      // block rows, then the right-hand side as row BS
    constexpr int T2 = BS * (BS - 1) / 2;
    constexpr int asz = rows * (rows + 1) / 2 + (MODE == V_NLLIK ? T2 : 0);
    constexpr int NBB = BS > 16 ? BS : 16;            // columns kept for the second row of a lane
#define AT(r, c) ((r) * ((r) + 1) / 2 + (c))
    const int mp1 = a.m + 1, D = a.vp.D, DP = VR4_DP(D);
    const int lane = threadIdx.x, g = lane >> 4, t = lane & 15;
    double *A = lds + (size_t)g * asz;                                   // packed lower triangle (+ K itself for the gradient)
    double *Kp = A + rows * (rows + 1) / 2;
    double *xs = lds + (size_t)4 * asz + (size_t)g * BS * DP;             // [BS][D] scaled inputs
    double *V = lds + (size_t)4 * asz + (size_t)4 * BS * DP + (size_t)g * 64;   // [2][32] u, alpha
    const int64_t i = rowblk * 4 + g;
    const bool live = i < a.n;
    const double *X = a.X + (MODE == V_LLIK ? (int64_t)by * a.x_stride : 0);
    double *partial = a.partial;
    if (MODE == V_LLIK) partial += (int64_t)by * a.n * 2;

    // conditioning set: the valid entries of the row come first; slot R <- entry b-1-(R-pad)  (ascending, self last).
    // One load of the row, the reversal by shuffle; then every slot fetches its own point (inputs, output, nugget
    // weight) with all loads in flight together: two memory latencies in all before the arithmetic starts.
    VR4_STAMP(0);
    const int nn0 = (live && t < mp1) ? (int)a.NN[i * mp1 + t] : -1;
    const int nn1 = (live && 16 + t < mp1) ? (int)a.NN[i * mp1 + 16 + t] : -1;
    const unsigned m0 = (unsigned)(__ballot(nn0 >= 0) >> (16 * g)) & 0xffffu, m1 = (unsigned)(__ballot(nn1 >= 0) >> (16 * g)) & 0xffffu;
    const int b = __popc(m0) + __popc(m1);
    const int pad = BS - b;
    int my[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int R = 16 * h + t, src = b - 1 - (R - pad);
        const int g0 = __shfl(nn0, src & 15, 16), g1 = __shfl(nn1, src & 15, 16);
        my[h] = (R >= pad && R < BS) ? ((src & 16) ? g1 : g0) : -1;
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int R = 16 * h + t;
        double yv = 0.0, ndv = 1.0;
        if (MODE != V_LMAT && my[h] >= 0) {
            yv = a.y[my[h]];
            ndv = a.nugget_diag[my[h]];
        }
        const double *xrow = X + (int64_t)(my[h] >= 0 ? my[h] : 0) * D;
        for (int d0 = 0; d0 < D; d0 += 8) {
            double x8[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) x8[q] = (my[h] >= 0 && d0 + q < D) ? xrow[d0 + q] : 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (R < BS) xs[R * DP + d0 + q] = d0 + q < D ? x8[q] * a.vp.inv_len[d0 + q] : 0.0;   // (zeros past D: see VR4_DP)
        }
        if (R < BS) {
            A[AT(R, R)] = my[h] >= 0 ? 1.0 + a.vp.nugget * ndv : 1.0;
            if (MODE != V_LMAT) A[AT(BS, R)] = yv;
        }
    }
    VR4_STAMP(1);
    __syncthreads();
    VR4_STAMP(2);
    // Strictly lower entries in 2 x 2 tiles: rows (2i, 2i + 1) against columns (2j, 2j + 1), j <= i, one tile per lane and pass -- FOUR
    // points read from LDS for four entries.  (Two entries per lane and pass took four points as well: with the selects gone the
    // pair loop ran at the LDS's bandwidth, 2 KB per wave, pass and dimension.)  The diagonal tiles hold one entry below the
    // diagonal; their other three results, and those of the phantom row / column of an odd block size, are not stored.
    {
        constexpr int NP = (BS + 1) / 2, NT = NP * (NP + 1) / 2;
        const bool iso = MODE == V_NLLIK && a.vp.nlen == 1;
        // tile e = the strictly-lower pair (i + 1, j) of an (NP + 1) x (NP + 1) matrix, j <= i: decoded once, then advanced by sixteen
        // entries per pass with integer arithmetic (a table in memory cost a dependent load per pass: ~1000 cycles of a 12 000-cycle loop)
        int trow, tcol;
        tri_decode_small(t, trow, tcol);
        ++trow;
        for (int e = t; e < NT; e += 16) {
            const int ti = trow - 1, tj = tcol;
            tcol += 16;
            while (tcol >= trow) {
                tcol -= trow;
                ++trow;
            }
            const int r0 = 2 * ti, r1 = 2 * ti + 1, c0 = 2 * tj, c1 = 2 * tj + 1;
            const double *pr0 = xs + r0 * DP, *pr1 = xs + (r1 < BS ? r1 : BS - 1) * DP;
            const double *pc0 = xs + c0 * DP, *pc1 = xs + (c1 < BS ? c1 : BS - 1) * DP;
            double sa[4] = {0.0, 0.0, 0.0, 0.0}, pa[4] = {1.0, 1.0, 1.0, 1.0}, cfa[4] = {0.0, 0.0, 0.0, 0.0};   // (r0,c0) (r0,c1) (r1,c0) (r1,c1)
            for (int d0 = 0; d0 < D; d0 += 8) {
                double2 x0[4], x1[4], y0[4], y1[4];
#pragma unroll
                for (int h = 0; h < 4; ++h) {   // (16-byte reads; the columns past D hold zeros: 0 - 0, neutral for both kernels)
                    x0[h] = reinterpret_cast<const double2 *>(pr0 + d0)[h];
                    x1[h] = reinterpret_cast<const double2 *>(pr1 + d0)[h];
                    y0[h] = reinterpret_cast<const double2 *>(pc0 + d0)[h];
                    y1[h] = reinterpret_cast<const double2 *>(pc1 + d0)[h];
                }
#pragma unroll
                for (int h = 0; h < 8; ++h) {
                    const double u0 = (h & 1) ? x0[h >> 1].y : x0[h >> 1].x, u1 = (h & 1) ? x1[h >> 1].y : x1[h >> 1].x;
                    const double v0 = (h & 1) ? y0[h >> 1].y : y0[h >> 1].x, v1 = (h & 1) ? y1[h >> 1].y : y1[h >> 1].x;
                    const double f[4] = {u0 - v0, u0 - v1, u1 - v0, u1 - v1};
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        if (KIND == DGPAMD_SEXP) {
                            corr_accum_sexp(f[w], sa[w]);
                        } else if (!iso) {
                            corr_accum_matern(f[w], pa[w], sa[w]);
                        } else {
                            // one shared lengthscale: dK/dlog(l) = K sum_d n_d / g_d with g_d = 1 + sqrt5 r + 5/3 r^2 the dimension's
                            // factor of K and n_d = (5/3 r^2)(1 + sqrt5 r).  The sum is carried as a fraction over the running product
                            // of the g_d -- which K needs anyway -- so that NO reciprocal is taken: N <- N g_d + n_d G, G <- G g_d, and
                            // at the end dK = exp(-sqrt5 s) N  (K = G exp(-sqrt5 s), the G cancels).  A reciprocal per pair and
                            // dimension (quarter-rate seed + two Newton rounds) was a third of this loop's issue cycles.
                            const double r = fabs(f[w]);
                            const double gk = fma(r, fma(r, 5.0 / 3.0, SQRT5), 1.0);   // (corr_accum_matern's factor: K holds the same bits in every mode)
                            const double nd = ((5.0 / 3.0) * r * r) * fma(r, SQRT5, 1.0);
                            cfa[w] = fma(nd, pa[w], cfa[w] * gk);
                            pa[w] *= gk;
                            sa[w] += r;
                        }
                    }
                }
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int r = (w & 2) ? r1 : r0, c = (w & 1) ? c1 : c0;
                if (iso && KIND == DGPAMD_SEXP) cfa[w] = 2.0 * sa[w];   // dcoef = 2 df^2
                // exp_negated: the exponential from full-rate instructions only (the library's exp spends half of its issue cycles on
                // three quarter-rate ones); the three modes of this kernel -- I-step sums, M-step sums + gradients, sparse-factor rows
                // -- share it
                // (the squared-exponential instance gains 3-4 % from the pinned form; in the Matern instances it costs as much, SGPR pressure)
                //  and the sparse-factor mode of the squared exponential loses 4 %)
                const double ex = KIND == DGPAMD_SEXP ? (MODE == V_LMAT ? exp_negated(sa[w]) : exp_negated_v3(sa[w])) : exp_negated(SQRT5 * sa[w]);
                double kv = (KIND == DGPAMD_SEXP) ? ex : pa[w] * ex;
                if (c < pad) kv = 0.0;   // pads come first
                if (r < BS && c < r) {
                    const int el = r * (r - 1) / 2 + c;
                    A[el + r] = kv;   // AT(r, c) = r (r - 1) / 2 + c + r
                    // kept for the derivative sums: dK itself with one shared lengthscale (Matern: the numerator of the fraction
                    // above times the exponential), else the correlation
                    if (MODE == V_NLLIK)
                        Kp[el] = !iso ? kv : (KIND == DGPAMD_SEXP ? cfa[w] * kv : (c < pad ? 0.0 : cfa[w] * ex));
                }
            }
        }
    }
    VR4_STAMP(3);
    __syncthreads();
    VR4_STAMP(4);

    double ra[16], rb[NBB];   // rows t and 16 + t
    constexpr int LROWS = MODE == V_LMAT ? BS : BS + 1;   // (no right-hand-side row in the sparse-factor mode: nothing wrote it)
#pragma unroll
    for (int c = 0; c < 16; ++c) ra[c] = (c <= t && c < BS && t < LROWS) ? A[AT(t, c)] : 0.0;
#pragma unroll
    for (int c = 0; c < NBB; ++c) rb[c] = (c < BS && 16 + t < LROWS && c <= 16 + t) ? A[AT(16 + t, c < BS ? c : 0)] : 0.0;

    double sd_last = 1.0, w_last = 0.0;
    VR4_STAMP(5);
    static_for<0, BS>([&](auto J) {
        constexpr int j = J;
        double d = j < 16 ? group_bcast<(j & 15)>(ra[j & 15]) : group_bcast<(j & 15)>(rb[j < NBB ? j : 0]);
        if (!(d > 0.0)) d = 1.0;
        double inv, sd;
        rsqrt_sqrt(d, inv, sd);
        double la = 0.0, lb, nla = 0.0, nlb;
        if constexpr (j < 16) {
            la = ra[j] * inv;   // (lane j: d * inv = the diagonal of the factor)
            ra[j] = la;
            nla = -la;
        }
        lb = rb[j] * inv;
        rb[j] = lb;
        nlb = -lb;
        asm volatile("s_nop 4" : "+v"(nla), "+v"(nlb));   // (DPP sources just written; see group_bcast)
        static_for<0, BS>([&](auto Cc) {
            constexpr int c = Cc;
            if constexpr (c > j) {
                if constexpr (c < 16) {
                    fmac_bcast<(c & 15)>(ra[c & 15], nla, la);
                    if constexpr (BS >= 16) fmac_bcast<(c & 15)>(rb[c], nla, lb);
                } else {
                    fmac_bcast<(c & 15)>(rb[c], nlb, lb);
                }
            }
        });
        if constexpr (j == BS - 1) {
            sd_last = sd;
            w_last = BS < 16 ? la : lb;   // (in the right-hand-side row's lane: (L^-1 y)_last)
        }
    });
    constexpr int WL = BS & 15;   // lane of the right-hand-side row BS (second row of the lane when BS >= 16)
    VR4_STAMP(6);

    if (MODE == V_LLIK) {
        if (t == WL && live) {
            partial[i * 2] = w_last * w_last;            // vecchia.py:177
            partial[i * 2 + 1] = 2.0 * log(sd_last);     // vecchia.py:178
        }
        return;
    }
    // x <- L^-T x for e_last (u) and for w (alpha), in registers.  As soon as x_r is known the lane that owns row r adds
    // L[r][c] x_r to its partial sums of the columns c < r; when column c's turn comes the sum over the group's 16 lanes
    // (four DPP rotations) closes it.  No LDS, no barrier; pads decouple (identity rows in front).
    {
        // (entries above the diagonal are by-products of the factorisation, possibly not finite: they meet zeros below)
#pragma unroll
        for (int c = 0; c < 16; ++c) ra[c] = c <= t ? ra[c] : 0.0;
#pragma unroll
        for (int c = 0; c < NBB; ++c) rb[c] = c <= 16 + t ? rb[c] : 0.0;
        double accu[BS], acca[MODE == V_NLLIK ? BS : 1];
#pragma unroll
        for (int c = 0; c < BS; ++c) accu[c] = 0.0;
#pragma unroll
        for (int c = 0; c < (MODE == V_NLLIK ? BS : 1); ++c) acca[c] = 0.0;
        double u0 = 0.0, u1 = 0.0, a0 = 0.0, a1 = 0.0;   // x of rows t and 16 + t
        static_for<0, BS>([&](auto RR) {
            constexpr int r = BS - 1 - RR, owner = r & 15;
            constexpr bool sb = r >= 16;
            double diag;
            if constexpr (sb) diag = group_bcast<owner>(rb[r]); else diag = group_bcast<owner>(ra[r & 15]);
            double inv = __builtin_amdgcn_rcp(diag);
            inv = fma(inv, fma(-diag, inv, 1.0), inv);
            inv = fma(inv, fma(-diag, inv, 1.0), inv);
            const double ur = ((r == BS - 1 ? 1.0 : 0.0) - row_allreduce_sum(accu[r])) * inv;
            const double um = (t == owner) ? ur : 0.0;
            if constexpr (sb) u1 += um; else u0 += um;
            double am = 0.0;
            if constexpr (MODE == V_NLLIK) {
                double wr;
                if constexpr (BS < 16) wr = group_bcast<WL>(ra[r & 15]); else wr = group_bcast<WL>(rb[r]);
                const double ar = (wr - row_allreduce_sum(acca[r])) * inv;
                am = (t == owner) ? ar : 0.0;
                if constexpr (sb) a1 += am; else a0 += am;
            }
            static_for<0, r>([&](auto Cc) {
                constexpr int c = Cc;
                double lrc;
                if constexpr (sb) lrc = rb[c]; else lrc = ra[c & 15];
                accu[c] = fma(lrc, um, accu[c]);
                if constexpr (MODE == V_NLLIK) acca[c] = fma(lrc, am, acca[c]);
            });
        });
        VR4_STAMP(7);
        V[t] = u0;
        if (MODE == V_NLLIK) V[32 + t] = a0;
        if (16 + t < BS) {
            V[16 + t] = u1;
            if (MODE == V_NLLIK) V[48 + t] = a1;
        }
    }
    __syncthreads();
    if (MODE == V_LMAT) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int R = 16 * h + t;
            if (R < mp1 && live) a.Lmat[i * mp1 + R] = V[BS - 1 - R];   // reversed, self first; pads give the trailing zeros
        }
        return;
    }
    // vecchia.py:216-219 restated: t_last = u^T dK u ; s = alpha^T dK u
    const int P = a.P, npl = (a.vp.nlen == 1) ? 1 : D;
    const double wl = __shfl(w_last, WL, 16);
    double *out = partial + i * (2 + 2 * P);
    if (t == 0 && live) {
        out[0] = wl * wl;
        out[1] = 2.0 * log(sd_last);
    }
    const double *u = V, *al = V + 32;
    int gr0, gc0;   // the lane's first strictly-lower entry (r, c); advanced by sixteen entries per pass (see the pair loop)
    tri_decode_small(t, gr0, gc0);
    ++gr0;
    for (int k = 0; k < npl; ++k) {
        double tl = 0.0, sm = 0.0;
        int gr = gr0, gc = gc0;
        // (a fixed number of passes, the entries past the end clamped and weighted with zero, unrolled seven at a time: the five
        //  LDS reads of a pass depend on its (r, c) and, issued pass by pass, each pass waited ~450 cycles for them -- 10 000 of
        //  the 47 000 cycles of a wave)
        constexpr int NPASS = (T2 + 15) / 16;
#pragma unroll 7
        for (int p = 0; p < NPASS; ++p) {
            const int e = t + 16 * p;
            const bool in = e < T2;
            const int r = in ? gr : 1, c = in ? gc : 0, ec = in ? e : 0;
            gc += 16;
            while (gc >= gr) {
                gc -= gr;
                ++gr;
            }
            double dk = a.vp.nlen == 1 ? Kp[ec] : dcoef_v<KIND>(xs[r * DP + k] - xs[c * DP + k]) * Kp[ec];
            dk = in ? dk : 0.0;
            tl = fma(2.0 * dk, u[r] * u[c], tl);
            sm = fma(dk, al[r] * u[c] + al[c] * u[r], sm);
        }
        tl = row_allreduce_sum(tl);
        sm = row_allreduce_sum(sm);
        if (t == 0 && live) {
            out[2 + k] = 2.0 * sm * wl - tl * wl * wl;
            out[2 + P + k] = tl;
        }
    }
    VR4_STAMP(8);
    if (a.nugget_est) {   // dK/dlog eta = diag(nugget * nugget_diag)   vecchia.py:329-332
        double tl = 0.0, sm = 0.0;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int R = 16 * h + t;
            if (R < BS && my[h] >= 0) {
                const double dk = a.vp.nugget * a.nugget_diag[my[h]];
                tl = fma(dk, u[R] * u[R], tl);
                sm = fma(dk, al[R] * u[R], sm);
            }
        }
        tl = row_allreduce_sum(tl);
        sm = row_allreduce_sum(sm);
        if (t == 0 && live) {
            out[2 + npl] = 2.0 * sm * wl - tl * wl * wl;
            out[2 + P + npl] = tl;
        }
    }
#undef AT
}

// A workgroup (one wave) walks row blocks rb = blockIdx.x, blockIdx.x + gridDim.x, ...: the grid is capped (launch_vrow4_nb)
// so that a launch the device-side ESS queue has predicated away costs a few thousand workgroup dispatches, not
// n / 4 x batch of them (at n = 50 000 the no-op launches of an I-step added up to 9 ms: ~7 ns per dispatched workgroup).
template <int KIND, int MODE, int BS>
__global__ __launch_bounds__(64) void vecchia_row4_kernel(VRowArgs a) {
    extern __shared__ double lds[];
    if (a.pred && *a.pred) return;
    const int64_t nrb = (a.n + 3) / 4;
    for (int64_t q = blockIdx.x; q < nrb; q += gridDim.x) {
        vrow4_body<KIND, MODE, BS>(a, lds, q, (int)blockIdx.y);
        __syncthreads();   // (the next row block reuses the LDS)
    }
}

#define VR4_GRID 2048   // row-block workgroups per input set (each walks n / 4 / 2048 row blocks)
template <int KIND, int MODE, int BS>
static int launch_vrow4_nb(dgpamd_ctx *ctx, VRowArgs &a, int batch) {
    const size_t shm = vrow4_lds(BS, a.vp.D, MODE == V_NLLIK, MODE != V_LLIK);
    int rc = set_lds(ctx, (const void *)vecchia_row4_kernel<KIND, MODE, BS>, shm);
    if (rc) return rc;
    const int64_t nrb = (a.n + 3) / 4;
    // the cap applies to the launches a device-side queue may predicate away (ctx->pred set); the others keep one
    // workgroup per row block, which the hardware balances better (llik x6 688 vs 721 us, nllik 333 vs 380 us at n = 50 000)
    const int64_t cap = a.pred ? VR4_GRID : nrb;
    a.trace = ctx->trace;
    hipLaunchKernelGGL((vecchia_row4_kernel<KIND, MODE, BS>), dim3((unsigned)(nrb < cap ? nrb : cap), (unsigned)batch), dim3(64), shm,
                       ctx->stream, a);
    LAUNCH_CHECK(ctx);
    return DGPAMD_OK;
}

template <int KIND, int MODE>
int launch_vrow4(dgpamd_ctx *ctx, VRowArgs &a, int batch) {
    const int nb = a.m + 1;   // compiled sizes: every fourth, and 26 (the default m = 25) exactly
    if (nb <= 4) return launch_vrow4_nb<KIND, MODE, 4>(ctx, a, batch);
    if (nb <= 8) return launch_vrow4_nb<KIND, MODE, 8>(ctx, a, batch);
    if (nb <= 12) return launch_vrow4_nb<KIND, MODE, 12>(ctx, a, batch);
    if (nb <= 16) return launch_vrow4_nb<KIND, MODE, 16>(ctx, a, batch);
    if (nb <= 20) return launch_vrow4_nb<KIND, MODE, 20>(ctx, a, batch);
    if (nb <= 24) return launch_vrow4_nb<KIND, MODE, 24>(ctx, a, batch);
    if (nb <= 26) return launch_vrow4_nb<KIND, MODE, 26>(ctx, a, batch);
    if (nb <= 28) return launch_vrow4_nb<KIND, MODE, 28>(ctx, a, batch);
    return launch_vrow4_nb<KIND, MODE, VR_MAXB>(ctx, a, batch);
}

#define VROW4_ALL_MODES(PREFIX, KIND)                                              \
    PREFIX template int launch_vrow4<KIND, V_LLIK>(dgpamd_ctx *, VRowArgs &, int);  \
    PREFIX template int launch_vrow4<KIND, V_NLLIK>(dgpamd_ctx *, VRowArgs &, int); \
    PREFIX template int launch_vrow4<KIND, V_LMAT>(dgpamd_ctx *, VRowArgs &, int);
#ifdef VROW4_KIND
VROW4_ALL_MODES(, VROW4_KIND)
#else
VROW4_ALL_MODES(extern, DGPAMD_SEXP)
VROW4_ALL_MODES(extern, DGPAMD_MATERN25)
#endif
