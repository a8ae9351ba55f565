"""The host reference of the dense factorisation (tests/chol_ref.py) checked on its own, without a GPU: the extended
arithmetic against mpmath at 60 digits, the +-1 probe estimate against the full Frobenius norm, longdouble against
double-double at the largest size either is used at, LAPACK itself inside the bounds the device is held to
(tests/test_gpu_chol_residuals.py), and failing() against LAPACK's info."""
import numpy as np
import pytest

import chol_ref as R

FAMILIES = ('well', 'matern', 'sexp')
ARITH_TOL = 1.0 / 64   # units of u: the arithmetic's own error in every measure


def second_lapack(K, y):
    """An independent second run in the device's place: numpy's Cholesky, triangular solves, S = T T^T, T = L^-T."""
    from scipy.linalg import solve_triangular
    n = K.shape[0]
    L = np.linalg.cholesky(K)
    w = solve_triangular(L, y, lower=True)
    T = solve_triangular(L, np.eye(n), lower=True).T
    S = T @ T.T   # (dpotri's own route, and the device's; an LU inverse has no small right residual at cond 1e8)
    alpha = solve_triangular(L, w, lower=True, trans='T')
    return L, w, T, S, alpha


def all_measures(K, y, out, ar=None, probe=None):
    L, w, T, S, alpha = out
    n = K.shape[0]
    tr, tl = R.eps_T(L, R.mask_T(T, n), ar, probe)
    return dict(eps_L=R.eps_L(K, L, ar, probe), eps_w=R.eps_w(L, w, y, ar), eps_T_right=tr, eps_T_left=tl,
                eps_S=R.eps_S(K, S, ar, probe), eps_alpha=R.eps_alpha(K, alpha, y, ar))


@pytest.mark.parametrize('n', [7, 40])
@pytest.mark.parametrize('name', FAMILIES)
def test_extended_arithmetic_against_mpmath(n, name):
    """Every measure in longdouble and in double-double, full and through the probes, stands within u / 64 of the same measure
    in mpmath at 60 digits."""
    K, y = R.family(name, n)
    out = second_lapack(K, y)
    for probe in (False, True):
        exact = all_measures(K, y, out, R.MPMATH, probe)
        for ar in (R.LONGDOUBLE, R.DOUBLEDOUBLE):
            if ar is R.LONGDOUBLE and not R.HAVE_LD:
                continue
            got = all_measures(K, y, out, ar, probe)
            for k, v in exact.items():
                assert abs(got[k] - v) <= ARITH_TOL, (ar.name, probe, k, got[k], v)


def test_exact_dot_and_corner():
    import mpmath
    rng = np.random.default_rng(4)
    w = rng.normal(size=130) * 10.0**rng.integers(-8, 8, size=130)
    with mpmath.workdps(60):
        ref = mpmath.fsum(mpmath.mpf(float(x))**2 for x in w)
        assert R.exact_dot(w, w) == float(ref)
    ww = float(np.dot(w, w))
    got, bnd = R.corner(-ww, w)
    assert bnd == 132.0 and got <= bnd
    assert R.corner(-ww * (1 + 200 * R.U), w)[0] > bnd


@pytest.mark.parametrize('name', FAMILIES)
def test_probe_estimate_within_its_sampling_spread(name):
    """||R V||_F^2 / 8 estimates ||R||_F^2 without bias; for +-1 probes its variance is 2 (||R^T R||_F^2 - sum_i (R^T R)_ii^2) / 8.
    The seeded probes stand within four standard deviations of the full norm."""
    n = 128
    K, y = R.family(name, n)
    L = np.linalg.cholesky(K)
    ar = R.arith_for(n)
    Rm = np.asarray(ar.diff(ar.prod([K]), ar.prod([L, np.ascontiguousarray(L.T)])), dtype=np.float64) / R.U
    G = Rm.T @ Rm
    full2 = float(np.trace(G))
    sd = np.sqrt(2.0 * ((G * G).sum() - (np.diagonal(G)**2).sum()) / R.NPROBE)
    est2 = (R.eps_L(K, L, probe=True) * R.fro(K))**2
    assert abs(est2 - full2) <= 4.0 * sd, (est2, full2, sd)
    assert abs(np.sqrt(full2) / R.fro(K) - R.eps_L(K, L, probe=False)) <= 1e-6


@pytest.mark.skipif(not R.HAVE_LD, reason='numpy.longdouble is a double here: every product is double-double already')
@pytest.mark.parametrize('name', FAMILIES)
def test_longdouble_against_double_double_at_320(name):
    K, y = R.family(name, 320)
    L = R.lapack_values(320, name)['L']
    a, b = R.eps_L(K, L, R.LONGDOUBLE, False), R.eps_L(K, L, R.DOUBLEDOUBLE, False)
    assert abs(a - b) <= ARITH_TOL, (a, b)


@pytest.mark.parametrize('n', [1, 2, 17, 63, 64, 65, 128, 129, 320, 449, 511])
def test_lapack_itself_is_within_the_bounds(n):
    """The bound the device is held to -- 4 x max(LAPACK's value, 1 u) per measure, the corner's a-priori (n + 2) u -- with a
    second, independent LAPACK run in the device's place: the inputs chosen do not make it unreachable."""
    for name in FAMILIES:
        K, y = R.family(name, n)
        ref = R.lapack_values(n, name)
        out = second_lapack(K, y)
        got = all_measures(K, y, out)
        tr, tl = R.lapack_eps_T(out[0])
        want = dict(eps_L=ref['eps_L'], eps_w=ref['eps_w'], eps_T_right=tr, eps_T_left=tl, eps_S=ref['eps_S'], eps_alpha=ref['eps_alpha'])
        for k, v in got.items():
            assert v <= R.bound(want[k]), (n, name, k, v, want[k])
        w = out[1]
        c, bnd = R.corner(-float(np.dot(w, w)), w)
        assert c <= bnd
        if name == 'well':
            assert ref['eps_logdet'] <= R.bound(0.0)
            assert R.eps_logdet(2 * np.log(np.diagonal(out[0])).sum(), ref['logdet_ref'], n) <= R.bound(ref['eps_logdet'])


def test_what_sets_the_device_apart_from_lapack_in_a_host_model():
    """The two attributions of DESIGN.md (accuracy of the factorisation) in chol_ref.blocked_model, which differs from LAPACK in
    one switch at a time.  With a triangular solve and 64-blocks summed from zero it is LAPACK to within the factor 4 that covers
    summation order.  The explicit inverse of the diagonal block's factor alone takes eps_L of sexp at n = 128 past 4 x LAPACK
    (the device: 21.5 u; LAPACK: 2.2 u) and stays inside the kappa_2(L_kk) growth that bound_eps_L admits; one rounding per
    product alone takes eps_L of `well` at n = 449 to what the device measured while its trailing updates accumulated every
    product onto the tile (5.3 u; LAPACK: 1.3 u; 3.4 u since they sum half tiles from zero) and does nothing of the kind to
    a kernel matrix."""
    K, y = R.family('sexp', 128)
    ref = R.lapack_values(128, 'sexp')
    assert R.eps_L(K, R.blocked_model(K, False, 64)) <= R.bound(ref['eps_L'])
    inv = R.eps_L(K, R.blocked_model(K, True, 64))
    assert R.bound(ref['eps_L']) < inv <= R.bound_eps_L('sexp', ref['eps_L'], ref['L'])
    assert R.eps_L(K, R.blocked_model(K, False, 1)) <= R.bound(ref['eps_L'])
    K, y = R.family('well', 449)
    ref = R.lapack_values(449, 'well')
    assert R.eps_L(K, R.blocked_model(K, False, 64)) <= 1.5 * ref['eps_L']
    assert R.eps_L(K, R.blocked_model(K, True, 64)) <= 1.5 * ref['eps_L']
    one = R.eps_L(K, R.blocked_model(K, False, 1))
    assert 3.0 * ref['eps_L'] < one < 6.0 * ref['eps_L'], (one, ref['eps_L'])


def test_logdet_reference_against_mpmath():
    import mpmath
    K, y = R.family('well', 24)
    with mpmath.workdps(60):
        ref = mpmath.log(mpmath.det(mpmath.matrix(K.tolist())))
        got = R.logdet_ref(K)
        hi = float(got)
        got = mpmath.mpf(hi) + mpmath.mpf(float(got - R.LD(hi)))   # (the longdouble in two doubles, exactly)
        assert abs(got - ref) <= R.U / 64 * (24 + abs(ref))      # u / 64 of eps_logdet's unit


POSITIONS = {130: (1, 2, 16, 17, 63, 64, 65, 80, 128, 129, 130), 128: (64, 65, 128), 1: (1,)}


@pytest.mark.parametrize('n', sorted(POSITIONS))
def test_failing_matrices_fail_where_they_say(n):
    """LAPACK reports minor p for 'neg' and 'zero' at every position the GPU tests use; the NaN kinds (for which the LAPACK at
    hand is no reference: it compares `<= 0`) carry the NaN where the docstring says and leave the leading (p-1) x (p-1) block
    positive definite."""
    from scipy.linalg.lapack import dpotrf
    K, y = R.family('well', n)
    for p in POSITIONS[n]:
        for kind in ('neg', 'zero'):
            assert dpotrf(R.failing(K, p, kind), lower=1)[1] == p, (n, p, kind)
        for kind in ('nan_diag', 'nan_row'):
            if kind == 'nan_row' and p < 2:
                continue
            A = R.failing(K, p, kind)
            assert np.isnan(A).sum() == (1 if kind == 'nan_diag' else 2) and np.isnan(A[p - 1, :p]).any()
            if p > 1:
                assert dpotrf(A[:p - 1, :p - 1], lower=1)[1] == 0
    for first, second in ((20, 70), (70, 100)):
        if n >= second:
            A = R.failing(R.failing(K, second, 'neg'), first, 'neg')
            assert dpotrf(A, lower=1)[1] == first
            assert dpotrf(R.failing(K, second, 'neg'), lower=1)[1] == second
