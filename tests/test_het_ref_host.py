"""tests/het_ref.py, the extended-precision reference of the heteroskedastic posterior draws, checked without a GPU: against the
float64 oracle and the reference's recorded draws, through an identity that trusts neither restatement, for the conditions on
the inputs that the measured tolerances of tests/test_gpu_hetero_posterior.py rest on, and for the sensitivity of the very
comparison functions the GPU tests apply (a float64 restatement with a deliberately wrong block must be rejected by each)."""
import numpy as np
import pytest

import het_ref as H
from conftest import case
from oracle import dgp_oracle as O

pytestmark = pytest.mark.skipif(not H.HAVE_LONGDOUBLE, reason='numpy.longdouble is no wider than float64 on this platform')

VCASES = [(n, D, m, name) for (n, D, m) in H.VECCHIA_CASES for name in H.NAMES]
DCASES = [(n, name) for n in H.DENSE_N for name in H.NAMES]


def vid(c):
    return '-'.join(str(v) for v in c)


# ------------------------------------------------------------------ the reference against what exists
@pytest.mark.parametrize('n,D,m,name', VCASES, ids=[vid(c) for c in VCASES])
def test_vecchia_reference_against_the_oracle_and_input_conditions(n, D, m, name):
    """O.U_matrix_rows / O.post_het_vecch against het_ref.rows / draw_vecchia: the oracle's error E_ref must be a rounding error
    (inside the rigorous forward bound of its own algorithm, and below 1e-9, the tolerance the oracle is held to against the
    recorded draws), and every block's kappa_2 is at most 1e6."""
    c, R, f, e_rows, e_draw = H.vecchia_reference(n, D, m, name)
    assert R.idx.shape == (n, min(m, n) + 1) and np.all(R.idx[:, -1] == np.arange(n) + n) and np.all(R.idx[:, -2] == np.arange(n))
    assert R.cond.max() <= H.KAPPA_MAX, R.cond.max()
    outer = H.rigorous_rows_bound(R)
    print('case %s: kappa %.2e  E_ref rows %.2e t %.2e draw %.2e  rigorous %.2e' % (vid((n, D, m, name)), R.cond.max(), *e_rows, e_draw, outer))
    assert max(e_rows) <= min(outer, 1e-9), (e_rows, outer)
    assert e_draw <= 1e-9, e_draw
    # the layout: slot 0 the own latent, then latents only, each an earlier row; zero padding
    slot = np.arange(R.NNl.shape[1])[None, :]
    used = slot <= R.lat[:, :-1].sum(1)[:, None]
    assert np.all(R.NNl[:, 0] == np.arange(n)) and np.all((R.NNl < np.arange(n)[:, None])[used & (slot > 0)])
    assert np.all(R.NNl[~used] == 0) and np.all(R.Lrows[~used] == 0) and np.all(R.Lrows[:, 0] > 0)


@pytest.mark.parametrize('n,name', DCASES, ids=[vid(c) for c in DCASES])
def test_dense_reference_against_the_oracle_and_input_conditions(n, name):
    """O.post_het1 / O.post_het2 against het_ref.draw_dense, and kappa_2(K) <= 1e6."""
    c = H.dense_case(n, name)
    K = O.k_matrix(c.X, c.length, c.nugget, name)
    kappa = np.linalg.cond(K)
    assert kappa <= H.KAPPA_MAX, kappa
    for rep in (False, True):
        f, e = H.dense_reference(c, K, rep)
        print('dense %s rep=%d: kappa %.2e  E_ref %.2e' % (vid((n, name)), rep, kappa, e))
        assert f.shape == (n,) and e <= 1e-9, e


def test_site_terms_are_posterior_terms():
    c = H.dense_case(130, 'sexp')
    g, y = H.site_terms(c.gamma_obs, c.y_obs, c.mask, c.n)
    Gi = 1.0 / c.gamma_obs
    g64 = 1.0 / np.bincount(c.mask, weights=Gi, minlength=c.n)
    np.testing.assert_allclose(np.asarray(g, float), g64, rtol=1e-14)
    np.testing.assert_allclose(np.asarray(y, float), g64 * np.bincount(c.mask, weights=Gi * c.y_obs, minlength=c.n), rtol=1e-13)
    assert np.bincount(c.mask).min() == 1 and np.bincount(c.mask).max() == 3


def test_reference_against_the_recorded_dense_draws(golden):
    """g13_hetero at the tolerances tests/test_oracle_golden.py holds the oracle to."""
    g = golden('g13_hetero')
    f1 = H.draw_dense(g['a_v'], 1.0, g['a_Gamma'], g['a_y'], g['a_z1'])
    np.testing.assert_allclose(np.asarray(f1, float), g['a_f1'], rtol=1e-9, atol=1e-11)
    ge, ye = H.site_terms(g['a_Gamma2'], g['a_y2'], g['a_mask'], g['a_v'].shape[0])
    f2 = H.draw_dense(g['a_v'], 1.0, ge, ye, g['a_z2'])
    np.testing.assert_allclose(np.asarray(f2, float), g['a_f2'], rtol=1e-9, atol=1e-11)


def test_reference_against_the_recorded_vecchia_draws(golden):
    """g15_hetero_vecchia, without and with replicates, at the tolerance of tests/test_oracle_golden.py."""
    g = golden('g15_hetero_vecchia')
    for k in range(2):
        d = case(g, 'c%d_' % k)
        X, ord_, n = d['X'], d['ord'], len(d['X'])
        y = d['lik_output'].ravel()
        gam = np.exp(d['lik_input'][:, 1])
        ge, ye = H.site_terms(gam, y, d['rep'] if bool(d['has_rep']) else None, n)
        f = H.draw_vecchia(X[ord_], d['impNN'], d['scale'][0], d['length'], str(d['name']), ge[ord_], ye[ord_], d['z'])
        np.testing.assert_allclose(np.asarray(f, float)[np.argsort(ord_)], d['f'], rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize('name', H.NAMES)
def test_vecchia_with_every_point_in_the_block_is_the_dense_posterior_mean(name):
    """With m >= n every latent is conditioned on all the others, so the sparse factor is exact and the draw at z = 0 is the
    dense posterior mean v (v + Gamma)^-1 y, up to the 1e-10 on the blocks' diagonals (measured 6e-10 and 1.4e-9 relative at
    n = 20): neither restatement is trusted for this, float64 and longdouble both."""
    c = H.vecchia_case(20, 2, 50, name)
    v = c.scale * O.corr_matrix(c.X, c.length, name)
    mean = v @ np.linalg.solve(v + np.diag(c.gamma), c.y)
    g2 = np.concatenate((c.gamma, c.gamma))
    f64 = O.post_het_vecch(c.X, c.impNN, c.scale, c.length, name, g2, c.y, np.zeros(c.n))
    fld = H.draw_vecchia(c.X, c.impNN, c.scale, c.length, name, c.gamma, c.y, np.zeros(c.n))
    mld = H.draw_dense(H.corr(c.X, c.X, c.length, name), c.scale, c.gamma, c.y, np.zeros((c.n, 2)))
    tol = 1e-8 * np.abs(mean).max()
    assert np.abs(f64 - mean).max() <= tol and np.abs(np.asarray(fld - mld, float)).max() <= tol
    assert np.abs(np.asarray(fld, float) - mean).max() <= tol


def test_sparse_residual_and_dot_terms():
    c, R, f, _, _ = H.vecchia_reference(130, 2, 2, 'sexp')
    res, mag = H.sparse_residual(R.Lrows, R.NNl, f, np.asarray(c.z, H.LD) - R.t)
    assert np.all(res <= 4 * 2.0 ** -63 * mag)
    x = f.copy()
    x[50] *= 1 + 1e-12
    res, mag = H.sparse_residual(R.Lrows, R.NNl, x, np.asarray(c.z, H.LD) - R.t)
    assert res[50] > 1e3 * H.U * mag[50]
    s, a = H.dot_terms(np.array([[1.0, -1.0, 2.0 ** -60]]), np.ones(3))
    assert float(s[0]) == 2.0 ** -60 and a[0] > 2 and a.dtype == H.LD   # (a sum float64 would lose)


# ------------------------------------------------------------------ checker sensitivity
WRONG = ['no_jitter', 'gamma_on_latents', 'gamma_one_off', 'flag_flipped', 't_over_latents']


def f64_rows(c, wrong=None):
    """(Lrows, NNl, t) in float64 like O.U_matrix_rows + the device's row layout, optionally from a deliberately wrong block:
    no_jitter: the 1e-10 left out; gamma_on_latents: row n // 2 puts gamma on its latent entries; gamma_one_off: gamma[idx + 1];
    flag_flipped: entry 0 of row n // 2 changes sides in the layout; t_over_latents: t summed over the latent entries."""
    n = c.n
    idx_all = c.impNN[:, ::-1]
    X2 = np.vstack((c.X, c.X))
    g2 = np.concatenate((c.gamma, c.gamma))
    U = np.zeros(idx_all.shape)
    for i in range(n):
        idx = idx_all[i]
        b = len(idx)
        obs = idx < n
        gi = g2[(idx + 1) % (2 * n)] if wrong == 'gamma_one_off' else g2[idx]
        if wrong == 'gamma_on_latents' and i == n // 2:
            obs = ~obs
        Ki = c.scale * O.corr_matrix(X2[idx], c.length, c.name)
        Ki[np.arange(b), np.arange(b)] = c.scale * 1.0 + gi * obs + (0.0 if wrong == 'no_jitter' else 1e-10)
        e = np.zeros(b)
        e[-1] = 1.0
        U[i] = np.linalg.solve(np.linalg.cholesky(Ki).T, e)
    lat = idx_all >= n
    if wrong == 'flag_flipped':
        lat = lat.copy()
        lat[n // 2, 0] = ~lat[n // 2, 0]
    Lrows, NNl, t = H.assemble(idx_all, U, n, c.y, lat=lat)
    if wrong == 't_over_latents':
        t = (np.where(lat, U, 0) * c.y[idx_all % n]).sum(1)
    return Lrows, NNl, t


@pytest.mark.parametrize('n,D,m,name', VCASES, ids=[vid(c) for c in VCASES])
def test_the_row_check_passes_the_oracle_and_rejects_every_wrong_block(n, D, m, name):
    """rows_accepted, the GPU test's comparison of dgpamd_vecchia_het_rows: a second float64 restatement (numpy.linalg.solve in
    place of scipy's triangular solve: other roundings) passes at the margin the device gets, each wrong block is rejected."""
    c, R, f, e_rows, e_draw = H.vecchia_reference(n, D, m, name)
    ok, eL, et = H.rows_accepted(*f64_rows(c), R, c.y, e_rows)
    assert ok, (eL, et, e_rows)
    for wrong in WRONG:
        ok, eL, et = H.rows_accepted(*f64_rows(c, wrong), R, c.y, e_rows)
        print('%s %s: eL %.2e et %.2e against tolerances %.2e %.2e' % (vid((n, D, m, name)), wrong, eL, et, H.tolerance(e_rows[0]), H.tolerance(e_rows[1])))
        assert not ok, wrong


@pytest.mark.parametrize('n,D,m,name', VCASES, ids=[vid(c) for c in VCASES])
def test_the_draw_check_passes_the_oracle_and_rejects_wrong_draws(n, D, m, name):
    """accept(draw_error(..)), the GPU test's comparison of Engine.vecchia_post_het and of the imputer's glue: the draw from the
    float64 rows passes; the draws with gamma one index off, with t over the latent entries, and with two entries of the
    ordering swapped where the glue reorders (gamma, y) are rejected."""
    c, R, f, e_rows, e_draw = H.vecchia_reference(n, D, m, name)

    def draw(Lrows, NNl, t):
        return O.forward_solve_sp(Lrows, NNl, c.z - t)
    assert H.accept(H.draw_error(draw(*f64_rows(c)), f), e_draw)
    for wrong in ('gamma_one_off', 't_over_latents'):
        assert not H.accept(H.draw_error(draw(*f64_rows(c, wrong)), f), e_draw), wrong
    ord_ = np.arange(n)
    ord_[[n // 3, n // 3 + 1]] = ord_[[n // 3 + 1, n // 3]]
    g2 = np.concatenate((c.gamma[ord_], c.gamma[ord_]))
    fs = O.post_het_vecch(c.X, c.impNN, c.scale, c.length, name, g2, c.y[ord_], c.z)
    assert not H.accept(H.draw_error(fs, f), e_draw)
    # ... and where it maps the result back: two rows of f exchanged
    assert not H.accept(H.draw_error(np.asarray(f, float)[ord_], f), e_draw)


@pytest.mark.parametrize('n,name', [(64, 'sexp'), (130, 'matern2.5')])
def test_the_dense_draw_check_rejects_a_wrong_system(n, name):
    """accept(draw_error(..)) on the dense draw: the oracle passes; gamma / scale left undivided, the right-hand side row one
    short, and w dropped are rejected."""
    c = H.dense_case(n, name)
    K = O.k_matrix(c.X, c.length, c.nugget, name)
    f, e = H.dense_reference(c, K)
    assert H.accept(H.draw_error(O.post_het1(c.scale * K, c.gamma, c.y, c.sd), f), e)
    assert not H.accept(H.draw_error(O.post_het1(c.scale * K, c.gamma * c.scale, c.y, c.sd), f), e)
    y1 = c.y.copy()
    y1[-1] = 0.0
    assert not H.accept(H.draw_error(O.post_het1(c.scale * K, c.gamma, y1, c.sd), f), e)
    sd1 = c.sd.copy()
    sd1[:, 1] = 0.0
    assert not H.accept(H.draw_error(O.post_het1(c.scale * K, c.gamma, c.y, sd1), f), e)
    assert not H.accept(np.nan, e)
