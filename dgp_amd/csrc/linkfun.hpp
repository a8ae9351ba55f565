// Closed forms of E[k(x,Z)] and E[k(x,Z)k(x',Z)] for the Matern-2.5 kernel under Z ~ N(m, v):
// the per-dimension factors of the linked-GP I and J (functions.py:453-494, vecchia.py:915-988).
//
// The factors follow the INTEGRAL, not the reference's float64 expression: that one forms exp(+10 v/l^2 ..) (1 + erf(-t)) and moment
// polynomials in raw coordinates, loses every digit from v/l^2 ~ 4 on and is NaN from ~100 (tests/linkfun_ref.py has the figures).
// Here every point is normalised first, x <- (x - m)/l, w = v/l^2, and the integral is taken region by region:
//   * beyond both points (z = x + s, s > 0) the integrand is a quartic in s WITH POSITIVE COEFFICIENTS times
//     exp(-x^2/2w - s (2 sqrt5 + x/w) - s^2/2w), so the region is exp(..) / sqrt(pi) sum_k q_k H_k with H_k = s2^k g_k(t),
//     g_k(t) = int_0^inf u^k exp(-u^2 - 2tu) du, t = (x + 2 sqrt5 w)/s2, s2 = sqrt(2w): positive terms, no cancellation at any w.
//     matern_tail_moments evaluates the g_k in whichever direction of their recurrence is stable;
//   * between the points the reference's polynomials stay, in normalised coordinates, and the erf difference is taken as a
//     difference of erfc where both arguments lie on one side.
// tests/test_gpu_linkfn.py holds each function to the exact value through dgpamd_debug_linkfn.
#pragma once
#include "common.hpp"

#include <math.h>

#define LINK_SQRTPI 1.7724538509055160273
#define LINK_RSQRTPI 0.56418958354775628695
#define LINK_B2 (5.0 / 3.0)
#define LINK_T_FORWARD 2.5   // below it the forward recurrence of the tail moments loses < 3e-13
#define LINK_MILLER_N 48     // start of the backward recurrence above it
#define LINK_EXP_CLAMP 600.0 // of the bare exp(+-sqrt5 x) of a record: exact within 268 lengthscales of m, finite beyond

__device__ __forceinline__ double matern_point(double d, double l) {
    double a = fabs(d);
    return (1.0 + SQRT5 * a / l + 5.0 * d * d / (3.0 * l * l)) * exp(-SQRT5 * a / l);
}

// H[k] = s2^k g_k(t), k = 0..4, t = X / s2, for t > 0 (returns true), and exp(-t^2) H[k] for t <= 0 (returns false: the caller
// folds exp(t^2) into its prefactor's exponent, which that leaves non-positive).
//   t <= 0       : H0 = sqrt(pi)/2 erfc(t), H1 = s2 exp(-t^2)/2 - X H0, H[k+1] = k w H[k-1] - X H[k]: every term positive.
//   0 < t < 2.5  : the same forward recurrence from erfcx; it loses (2t)^2k / k! and stays below 3e-13.
//   t >= 2.5     : the g_k are the recurrence's minimal solution, so it runs backwards from k = 48 (Miller) in the scaled unknowns
//                  y_k = g_k (2t)^k / k!:  y[k-1] = y[k] + 2 (k + 1) y[k+1] / (2t)^2, positive terms again, normalised by H0.
static __device__ bool matern_tail_moments(double X, double w, double s2, double *H) {
    const double t = X / s2;
    const bool fold = t > 0.0;
    const double H0 = 0.5 * LINK_SQRTPI * (fold ? erfcx(t) : erfc(t));
    H[0] = H0;
    if (t >= LINK_T_FORWARD) {
        const double u = 0.5 / t, u2 = u * u;
        double yn = 0.0, y = 1.0, y1 = 0.0, y2 = 0.0, y3 = 0.0, y4 = 0.0;   // y[k+1], y[k]
#pragma unroll
        for (int k = LINK_MILLER_N; k >= 1; --k) {
            const double ym = y + (2.0 * (k + 1)) * u2 * yn;
            yn = y;
            y = ym;
            if (k == 4) y4 = yn;
            if (k == 3) y3 = yn;
            if (k == 2) y2 = yn;
            if (k == 1) y1 = yn;
        }
        const double r = w / X;   // s2 / (2t)
        double c = H0 / y;
        c *= r; H[1] = c * y1;
        c *= r; H[2] = 2.0 * c * y2;
        c *= r; H[3] = 6.0 * c * y3;
        c *= r; H[4] = 24.0 * c * y4;
    } else {
        H[1] = 0.5 * s2 * (fold ? 1.0 : exp(-t * t)) - X * H0;
        H[2] = w * H[0] - X * H[1];
        H[3] = 2.0 * w * H[1] - X * H[2];
        H[4] = 3.0 * w * H[2] - X * H[3];
    }
    return fold;
}

// (a0 + a1 s + a2 s^2)(1 + sqrt5 s + 5/3 s^2) . H
static __device__ __forceinline__ double matern_polyB_dot(double a0, double a1, double a2, const double *H) {
    return a0 * H[0] + (a0 * SQRT5 + a1) * H[1] + (a0 * LINK_B2 + a1 * SQRT5 + a2) * H[2] + (a1 * LINK_B2 + a2 * SQRT5) * H[3] +
           (a2 * LINK_B2) * H[4];
}

// int over z beyond x of k(x - z) N(z; 0, w)  (normalised; the region below is the same with -x)
static __device__ double matern_tail_I(double x, double w, double s2) {
    double H[5];
    const bool fold = matern_tail_moments(x + SQRT5 * w, w, s2, H);
    const double e = exp(fold ? -0.5 * x * x / w : SQRT5 * x + 2.5 * w);
    return e * LINK_RSQRTPI * (H[0] + SQRT5 * H[1] + LINK_B2 * H[2]);
}

// The three entry points are not inlined: each translation unit then compiles the same body on its own, whatever surrounds the call,
// so the multiply-adds the compiler fuses are the same everywhere and a kernel's factor equals dgpamd_debug_linkfn's bit for bit
// (tests/test_gpu_linkfn.py reads single entries out of the kernels to check it).  A call costs ~1% of the body.

// one dimension of IJ_matern's I
static __device__ __noinline__ double matern_I_dim(double xk, double zm, double zv, double l) {
    if (zv == 0.0) return matern_point(zm - xk, l);
    const double d = (xk - zm) / l, w = zv / (l * l), s2 = sqrt(2.0 * w);
    return matern_tail_I(d, w, s2) + matern_tail_I(-d, w, s2);
}

// int over z beyond both points of k k N: x the point next to the region (mirrored for the region below), dl >= 0 the other
// one's distance from it
static __device__ double matern_tail_J(double dl, double x, double w, double s2) {
    double H[5];
    const bool fold = matern_tail_moments(x + 2.0 * SQRT5 * w, w, s2, H);
    const double e = exp(-SQRT5 * dl + (fold ? -0.5 * x * x / w : 2.0 * SQRT5 * x + 10.0 * w));
    return e * LINK_RSQRTPI * matern_polyB_dot(1.0 + dl * (SQRT5 + LINK_B2 * dl), SQRT5 + 2.0 * LINK_B2 * dl, LINK_B2, H);
}

// erf(tb) - erf(ta), ta <= tb, without cancelling the 1s
static __device__ __forceinline__ double matern_erf_difference(double ta, double tb) {
    return ta > 0.0 ? erfc(ta) - erfc(tb) : (tb < 0.0 ? erfc(-tb) - erfc(-ta) : erf(tb) - erf(ta));
}

// the off-diagonal J factor
static __device__ __noinline__ double matern_Jd(double X1, double X2, double z_m, double z_v, double l) {
    const double x1 = (fmin(X1, X2) - z_m) / l, x2 = (fmax(X1, X2) - z_m) / l;
    const double w = z_v / (l * l), sv = sqrt(0.5 * w / M_PI), s2 = sqrt(2.0 * w);
    const double P1 = matern_tail_J(x2 - x1, x2, w, s2), P3 = matern_tail_J(x2 - x1, -x1, w, s2);
    // between the points: vecchia.py:936-947 with m = 0, l = 1 (the moments of N(0, w) are 0, w, 0, 3 w^2)
    const double x1s = x1 * x1, x2s = x2 * x2, x12 = x1 * x2, xs = x1 + x2;
    const double E0 = 9.0 + 25.0 * x1s * x2s + 3.0 * SQRT5 * (3.0 - 5.0 * x12) * (x2 - x1) + 15.0 * (x1s + x2s - 3.0 * x12);
    const double E1 = 5.0 * (3.0 * SQRT5 * (x2s - x1s) + 3.0 * xs - 10.0 * x12 * xs);
    const double E2 = 5.0 * (5.0 * x1s + 5.0 * x2s - 3.0 - 3.0 * SQRT5 * (x2 - x1) + 20.0 * x12);
    const double E3 = -50.0 * xs;
    const double U = (E0 + w * E2 + 3.0 * w * w * 25.0) / 9.0;
    const double V2 = (E1 + x1 * E2 + (2.0 * w + x1s) * E3 + (x1s * x1 + 3.0 * w * x1) * 25.0) / 9.0;
    const double V3 = (E1 + x2 * E2 + (2.0 * w + x2s) * E3 + (x2s * x2 + 3.0 * w * x2) * 25.0) / 9.0;
    const double P2 = exp(-SQRT5 * (x2 - x1)) * (0.5 * U * matern_erf_difference(x1 / s2, x2 / s2) + V2 * sv * exp(-0.5 * x1s / w) -
                                                 V3 * sv * exp(-0.5 * x2s / w));
    return P1 + P2 + P3;
}

// the diagonal J factor: no region between the points
static __device__ __noinline__ double matern_Jd0(double x1, double z_m, double z_v, double l) {
    const double x = (x1 - z_m) / l, w = z_v / (l * l), s2 = sqrt(2.0 * w);
    return matern_tail_J(0.0, x, w, s2) + matern_tail_J(0.0, -x, w, s2);
}


// ---------------------------------------------------------------------------------------------------
// Separable form of the same factor:
//     Jd(x1,x2) = sum_{c<12} S_c(lo) T_c(hi) + (f2(hi) - f2(lo)) * sum_{a<3} S_{6+a}(lo) T_{12+a}(hi)
// with lo = min, hi = max.  In normalised coordinates:
//     c = 0..2   region above both:  S = exp(sqrt5 lo) lo^a, T = the coefficient of lo^a in that region's tail (matern_tail_T)
//     c = 3..5   region below both:  T = exp(-sqrt5 hi) hi^a, S_{3+a}(lo) = (-1)^a T_a(-lo) by symmetry
//     c = 6..11, 12..14  between the points.  erf((x-m)/sqrt(2v)) = f2 -+ erfc(|t|) with f2 = +-1 the SIDE of m the point lies on:
//                the pair kernels' f2 difference is then exactly 0 or +-2, and the erfc parts ride in T[6..8] (the larger point's)
//                and S[9..11] (the smaller point's, re-expanded by powers of hi), so no 1 - 1 is ever formed.
// The exponentials are split so that every factor of every product is bounded within LINK_EXP_CLAMP / sqrt5 lengthscales of m
// and finite everywhere: no record holds inf.
// ---------------------------------------------------------------------------------------------------
struct MaternDimConst {   // per (test point, dimension)
    double m, l, w, sv, s2;   // w = v / l^2
};

static __device__ __forceinline__ void matern_dim_const(double m, double v, double l, MaternDimConst &k) {
    k.m = m; k.l = l;
    k.w = v / (l * l);
    k.sv = sqrt(0.5 * k.w / M_PI);
    k.s2 = sqrt(2.0 * k.w);
}

// T[0..2] of the normalised point x in the larger-point role.  With z = x + s the other point's factor is
// 1 + sqrt5 (sg - lo) + 5/3 (sg - lo)^2, sg = s + x, by powers of lo.
static __device__ void matern_tail_T(double x, double w, double s2, double *T) {
    double H[5];
    const bool fold = matern_tail_moments(x + 2.0 * SQRT5 * w, w, s2, H);
    const double e = exp(fmin(fold ? -SQRT5 * x - 0.5 * x * x / w : SQRT5 * x + 10.0 * w, LINK_EXP_CLAMP)) * LINK_RSQRTPI;
    T[0] = e * matern_polyB_dot(1.0 + x * (SQRT5 + LINK_B2 * x), SQRT5 + 2.0 * LINK_B2 * x, LINK_B2, H);
    T[1] = e * matern_polyB_dot(-SQRT5 - 2.0 * LINK_B2 * x, -2.0 * LINK_B2, 0.0, H);
    T[2] = e * (LINK_B2 * (H[0] + SQRT5 * H[1] + LINK_B2 * H[2]));
}

// The parts of the region between the points that one point carries: U4[a], V[a] (a < 3) by powers of the other point
// (sg = +1: this point is the smaller one; -1: the larger), the side sgn of m it lies on and erfcx(|t|).
static __device__ __forceinline__ void matern_middle(double x, double w, double s2, double sg, double *U4, double *V, double &sgn,
                                                     double &cx) {
    const double p0[3] = {9.0 + x * (-sg * 9.0 * SQRT5 + 15.0 * x), sg * 9.0 * SQRT5 + x * (-45.0 + sg * 15.0 * SQRT5 * x),
                          15.0 + x * (-sg * 15.0 * SQRT5 + 25.0 * x)};
    const double p1[3] = {x * (15.0 - sg * 15.0 * SQRT5 * x), 15.0 - 50.0 * x * x, sg * 15.0 * SQRT5 - 50.0 * x};
    const double p2[3] = {-15.0 + x * (sg * 15.0 * SQRT5 + 25.0 * x), -sg * 15.0 * SQRT5 + 100.0 * x, 25.0};
    const double p3[3] = {-50.0 * x, -50.0, 0.0};
    const double p4[3] = {25.0, 0.0, 0.0};
    const double b2 = x, b3 = 2.0 * w + x * x, b4 = x * x * x + 3.0 * w * x;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        U4[a] = (p0[a] + w * p2[a] + 3.0 * w * w * p4[a]) / 9.0;
        V[a] = (p1[a] + b2 * p2[a] + b3 * p3[a] + b4 * p4[a]) / 9.0;
    }
    const double t = x / s2;
    sgn = t >= 0.0 ? 1.0 : -1.0;
    cx = erfcx(fabs(t));
}

// S-role (the point is the SMALLER one): out[0..11], f2
static __device__ __forceinline__ void matern_role_S(double X, const MaternDimConst &k, double *out, double &f2) {
    const double x = (X - k.m) / k.l, w = k.w;
    const double eP = exp(fmin(SQRT5 * x, LINK_EXP_CLAMP)), e2 = exp(SQRT5 * x - 0.5 * x * x / w);
    double U4[3], V42[3], T[3], sgn, cx;
    matern_middle(x, w, k.s2, 1.0, U4, V42, sgn, cx);
    matern_tail_T(-x, w, k.s2, T);
    f2 = sgn;
    double xa = 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[a] = eP * xa;
        out[3 + a] = a == 1 ? -T[a] : T[a];
        out[6 + a] = eP * xa;
        out[9 + a] = e2 * (k.sv * V42[a] + sgn * 0.5 * cx * U4[a]);
        xa *= x;
    }
}

// T-role (the point is the LARGER one): out[0..14]
static __device__ __forceinline__ void matern_role_T(double X, const MaternDimConst &k, double *out) {
    const double x = (X - k.m) / k.l, w = k.w;
    const double eM = exp(fmin(-SQRT5 * x, LINK_EXP_CLAMP)), e2 = exp(-SQRT5 * x - 0.5 * x * x / w);
    double U4[3], V43[3], T[3], sgn, cx;
    matern_middle(x, w, k.s2, -1.0, U4, V43, sgn, cx);
    matern_tail_T(x, w, k.s2, T);
    double xa = 1.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        out[a] = T[a];
        out[3 + a] = eM * xa;
        out[6 + a] = e2 * (-k.sv * V43[a] - sgn * 0.5 * cx * U4[a]);
        out[9 + a] = eM * xa;
        out[12 + a] = eM * (0.5 * U4[a]);
        xa *= x;
    }
}
