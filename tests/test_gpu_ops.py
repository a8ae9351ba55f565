"""Parity of every C-ABI operator (HIP, through ctypes) against the oracle and the
golden vectors recorded from the reference.  Needs an MI355X: -m gpu.

Tolerances (f64): 1e-10 relative on kernel matrices and likelihood scalars;
1e-8 where a Cholesky at n >= 1000 or the Jd-based Matern J is involved;
variances that are differences of O(scale) terms carry an absolute tolerance
of 1e-7*scale (cond(R) ~ 1e6 at nugget 1e-6); index arrays are bit-exact."""
import contextlib
import os

import numpy as np
import pytest

from conftest import case
from far_ref import FAR_LENGTH, FAR_NUGGET, FAR_SCALE, check_zeros, far_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def integral_oracle():
    """The oracle with its three Matern-2.5 linked factors on the integral (linkfun_ref.oracle_on_the_integral; everything else of the
    oracle untouched): the reference of the Matern linked predictions whose inputs reach v/l^2 >~ 0.3.  There the reference's float64
    expression -- which the golden files record and test_oracle_golden.py pins the unpatched oracle to -- is off by more than these
    tests' tolerances (6e-4 at v/l^2 = 1, variances of 1e3 from 4 on), while csrc/linkfun.hpp follows the integral
    (tests/test_gpu_linkfn.py); tests/test_linkfun_host.py holds the substituted factors to the exact values."""
    import linkfun_ref
    from oracle import dgp_oracle as O
    return linkfun_ref.oracle_on_the_integral(O)


@contextlib.contextmanager
def engine_under(**switches):
    """A fresh Engine created with DGPAMD_<name> = value in the environment for every keyword (None: unset), closed afterwards.  A context keeps the
    switches it was created under, so the environment is put back as soon as the engine exists; the engine must report every value it was given
    (a misspelt name raises here instead of comparing a kernel with itself).  It shares the thread's stream with the module's `eng`: tensors of either
    serve both."""
    from dgp_amd.ops import Engine
    names = {k: 'DGPAMD_' + k for k in switches}
    before = {k: os.environ.get(names[k]) for k in switches}
    try:
        for k, v in switches.items():
            os.environ.pop(names[k], None)
            if v is not None:
                os.environ[names[k]] = str(v)
        e = Engine(0)
    finally:
        for k, v in before.items():
            os.environ.pop(names[k], None)
            if v is not None:
                os.environ[names[k]] = v
    try:
        for k, v in switches.items():
            assert v is None or e.tuning(k) == int(v), (k, v, e.tuning(k))
        yield e
        e.sync()
    finally:
        e.close()


def test_a_context_keeps_the_switches_it_was_created_under(eng, monkeypatch):
    """The C library reads its DGPAMD_* switches once, in dgpamd_create (csrc/context.hip: one table): an engine made before the environment
    changes does not see the change, one made after it does and goes on doing so when the variables are gone again.  Values are reported as
    parsed -- clamped (MEGA_NEAR 0..6), the default where a value is not accepted (JSEP_TCH: 8..256 in steps of 8) -- and an unknown name raises.
    Nothing is launched."""
    from dgp_amd.ops import Engine, DgpAmdError
    names = ('VECCHIA_LDS', 'JSEP_TCH', 'MEGA_NEAR')
    for k in names:
        monkeypatch.delenv('DGPAMD_' + k, raising=False)
    first = Engine(0)
    for k, v in zip(names, ('1', '64', '9')):
        monkeypatch.setenv('DGPAMD_' + k, v)
    second = Engine(0)
    monkeypatch.setenv('DGPAMD_JSEP_TCH', '7')
    third = Engine(0)
    for k in names:
        monkeypatch.delenv('DGPAMD_' + k)
    try:
        assert [first.tuning(k) for k in names] == [0, 0, 3]
        assert [second.tuning(k) for k in names] == [1, 64, 6]
        assert third.tuning('JSEP_TCH') == 0 and third.tuning('DGPAMD_JSEP_TCH') == 0
        assert second.tuning('DGPAMD_MEGA_NEAR') == 6   # (with or without the prefix)
        with pytest.raises(DgpAmdError):
            second.tuning('VECCHIA_LSD')
    finally:
        for e in (first, second, third):
            e.close()


def close(a, b, rtol=1e-10, atol=1e-13):
    np.testing.assert_allclose(np.asarray(a, float), np.asarray(b, float), rtol=rtol, atol=atol)


def npy(t):
    return t.detach().cpu().numpy()


def split(eng, X, nl):
    """device tensors (Xloc, Xglob) of X = [local | global]"""
    Xl = eng.tensor(X[:, :nl])
    Xg = eng.tensor(X[:, nl:]) if X.shape[1] > nl else None
    return Xl, Xg


# ---------------------------------------------------------------- a1/a2/a5/a8
@pytest.mark.parametrize('fixture', ['g1_kernel_llik', 'g19_kernel_llik_n130'])
def test_kmatrix_golden(eng, golden, fixture):
    g = golden(fixture)
    for c in range(int(g['n_cases'])):
        d = case(g, 'c%d_' % c)
        nl = 3
        Xl, Xg = split(eng, d['X'], nl)
        W = eng.tensor(d['W_diag']) if 'W_diag' in d else None
        K = eng.kmatrix(str(d['name']), Xl, None, Xg, d['length'], d['nugget'][0], W=W)
        eng.sync()
        close(npy(K), d['K'], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
@pytest.mark.parametrize('full', [True, False])
def test_kmatrix_at_the_maximum_dimension(eng, name, full):
    """D = DGPAMD_MAXD = 64 inputs (40 gathered local columns + 24 global ones): the symmetric form stages 2 x 64 x 64 inputs and
    the mirror's transposition buffer in 73.9 KB of dynamic LDS -- more than a launch gets without asking -- and
    the augmented form 65.5 KB; n = 150 (three row tiles, ragged edge), against the oracle (kernel_class.py:304-359)."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(64)
    n, Dl, Dg = 150, 40, 24
    X = rng.uniform(size=(n, 50))
    cols = rng.permutation(50)[:Dl]
    G = rng.uniform(size=(n, Dg))
    length = rng.uniform(3.0, 6.0, size=Dl + Dg)
    Kref = O.k_matrix(np.concatenate((X[:, cols], G), 1), length, 1e-5, name)
    if full:
        K = npy(eng.kmatrix(name, eng.tensor(X), cols, eng.tensor(G), length, 1e-5))
        close(K, Kref, rtol=1e-12, atol=1e-15)
    else:
        y = rng.normal(size=n)
        A = npy(eng.kmatrix(name, eng.tensor(X), cols, eng.tensor(G), length, 1e-5, full=False, Y=eng.tensor(y)))
        close(np.tril(A[:n, :n]), np.tril(Kref), rtol=1e-12, atol=1e-15)
        close(A[n, :n], y, rtol=0, atol=0)


def close_or_zero(a, ref, rtol, atol):
    """|a| <= 1e-300 where the reference is exactly 0 (far_ref.check_zeros); the sibling test's tolerance everywhere else."""
    a, ref = np.asarray(a, float), np.asarray(ref, float)
    nz = check_zeros(a, ref)
    close(a[nz], ref[nz], rtol=rtol, atol=atol)


@pytest.mark.parametrize('s', [1.0, 1e4])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
@pytest.mark.parametrize('full', [True, False])
def test_kmatrix_beyond_the_exponent_range(eng, name, full, s):
    """Exponents from 4.5e5 to beyond 2^63 (far_inputs): K is the oracle's (1 + nugget) I, n = 65 (two tiles)."""
    from oracle import dgp_oracle as O
    n = 65
    X = far_inputs(n, s)
    Kref = O.k_matrix(X, FAR_LENGTH, FAR_NUGGET, name)
    assert np.count_nonzero(Kref) == n
    if full:
        K = npy(eng.kmatrix(name, eng.tensor(X), None, None, FAR_LENGTH, FAR_NUGGET))
        close_or_zero(K, Kref, rtol=1e-12, atol=1e-15)
    else:
        y = np.random.default_rng(1).normal(size=n)
        A = npy(eng.kmatrix(name, eng.tensor(X), None, None, FAR_LENGTH, FAR_NUGGET, full=False, Y=eng.tensor(y)))
        K = A[:n, :n]
        close_or_zero(np.tril(K), np.tril(Kref), rtol=1e-12, atol=1e-15)
        close(A[n, :n], y, rtol=0, atol=0)
    assert np.all(np.diag(K) == 1.0 + FAR_NUGGET)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_kmatrix_keeps_a_nan_input_in_its_row_and_column(eng, name):
    """A NaN in one input row: NaN in that row and column of K and nowhere else, as in the oracle (whose diagonal is set, not
    computed) -- the exponentials' guard for huge arguments must not turn a NaN argument into a number."""
    from oracle import dgp_oracle as O
    n = 65
    X = far_inputs(n, 1.0)
    X[7, 1] = np.nan
    with np.errstate(invalid='ignore'):
        Kref = O.k_matrix(X, FAR_LENGTH, FAR_NUGGET, name)
    K = npy(eng.kmatrix(name, eng.tensor(X), None, None, FAR_LENGTH, FAR_NUGGET))
    assert np.isnan(Kref).sum() == 2 * (n - 1)
    assert np.array_equal(np.isnan(K), np.isnan(Kref))
    ok = ~np.isnan(Kref)
    close_or_zero(K[ok], Kref[ok], rtol=1e-12, atol=1e-15)


@pytest.mark.parametrize('s', [1.0, 1e4])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_loglik_beyond_the_exponent_range(eng, name, s):
    """log_likelihood on far_inputs (K = (1 + nugget) I in the oracle) at test_loglik_batched_vs_oracle's tolerance."""
    from oracle import dgp_oracle as O
    n = 65
    X = far_inputs(n, s)
    y = np.random.default_rng(2).normal(size=n)
    ll, info = eng.loglik(name, eng.tensor(X), None, None, FAR_LENGTH, FAR_NUGGET, FAR_SCALE, eng.tensor(y))
    eng.sync()
    assert not npy(info).any()
    close(npy(ll).reshape(-1)[0], O.log_likelihood(X, y, FAR_LENGTH, FAR_SCALE, FAR_NUGGET, name), rtol=1e-10)


def test_kmatrix_rejects_views_it_would_write_wrongly(eng):
    """Engine.kmatrix takes the row stride of a caller's `out` (rows on 128-byte lines: bench.py); a transposed or too narrow
    view must be refused, not written in another layout."""
    X = eng.tensor(np.random.default_rng(0).uniform(size=(70, 2)))
    buf = eng.empty(70, 96)
    K = eng.kmatrix('sexp', X, None, None, [1.0], 1e-6, out=buf[:, :70])
    assert K.shape == (70, 70) and float(K[3, 3]) == 1.0 + 1e-6
    with pytest.raises(ValueError):
        eng.kmatrix('sexp', X, None, None, [1.0], 1e-6, out=eng.empty(70, 70).t())
    with pytest.raises(ValueError):
        eng.kmatrix('sexp', X, None, None, [1.0], 1e-6, out=eng.empty(70, 64))


def test_sexp_link_gp_with_exponents_beyond_the_tables_old_range(eng, lengthscale=1e-3):
    """linkgp_Jsexp2_kernel's table exponential took k = round(-256 x / ln 2) from the low word of the magic-number sum: from
    x = 5.8e6 on the word wrapped and the underflow clamp was passed by.  Lengthscales of 1e-3 against inputs of
    order one put most pair exponents between 1e6 and 1e8: every such J entry is exactly zero in the reference's arithmetic
    (functions.py:432-451) and must be here -- the prediction is then mean 0, variance scale (1 + nugget - sum_i Rinv_ii J_ii)."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(8)
    n, M, Dw = 200, 40, 3
    W = rng.normal(size=(n, Dw)) * 2.0
    y = rng.normal(size=n)
    length, scale, nugget = np.array([lengthscale]), 1.1, 1e-6
    st = O.compute_stats(W, y, length, nugget, 'sexp', Dw)
    m, v = rng.normal(size=(M, Dw)) * 2.0, rng.uniform(1e-8, 1e-6, size=(M, Dw))
    m[:4] = W[:4] + 1e-4            # a few test points next to training points: non-trivial J_ii, everything else underflows
    mo, vo = O.link_gp_predict(m, v, None, W, None, st['Rinv'], st['Rinv_y'], scale, length, nugget, 'sexp')
    lm, lv = eng.linkgp_predict('sexp', eng.tensor(m), eng.tensor(v), None, eng.tensor(W), None, length, eng.tensor(st['Rinv']), n,
                                eng.tensor(st['Rinv_y']), scale, nugget)
    lm, lv = npy(lm), npy(lv)
    assert np.all(np.isfinite(lm)) and np.all(np.isfinite(lv))
    close(lm, mo, rtol=1e-9, atol=1e-12)
    close(lv, vo, rtol=1e-9, atol=1e-12)


def test_sexp_link_gp_with_exponents_beyond_the_exponent_range(eng):
    """The same at a lengthscale of 1e-5: pair exponents between 1e10 and 1e12, past 2^39 ln 2 / 256 = 1.4886e9 where the table
    exponential's integer part leaves the 39 bits its exponent is cut from."""
    test_sexp_link_gp_with_exponents_beyond_the_tables_old_range(eng, lengthscale=1e-5)


def gpu_nll_grad(eng, d):
    """kernel.llik (kernel_class.py:403-449) assembled from the HIP pieces, host arithmetic as in dgp_amd.kernel."""
    from dgp_amd.kernel_class import kernel as K
    name = str(d['name'])
    prior = str(d['prior'])
    prior = None if prior == 'none' else prior
    nl = 3
    k = K(length=d['length'].copy(), scale=d['scale'][0], nugget=d['nugget'][0], name=name, prior_name=prior,
          prior_coef=None, nugget_est=bool(d['flags'][2]), scale_est=bool(d['flags'][4]), engine=eng)
    if prior is not None:
        k.prior_coef = d['prior_coef'].copy()   # stored coefficients
    k.input = d['X'][:, :nl].copy()
    k.global_input = d['X'][:, nl:].copy() if d['X'].shape[1] > nl else None
    k.output = d['y'].copy()
    if 'cl' in d:
        k.cl = d['cl'] if len(d['cl']) > 1 else d['cl'][0]
    if bool(d['flags'][3]):
        k.rep = np.zeros(int(d['n_rep']), dtype=int)   # only len(rep) enters llik
        k.W_diag = d['W_diag'].copy()
        k.sum_residual = d['sum_residual'].copy()
    return k


@pytest.mark.parametrize('fixture', ['g1_kernel_llik', 'g19_kernel_llik_n130'])
def test_llik_and_loglik_golden(eng, golden, fixture):
    """kernel.llik / log_likelihood_func against the reference's recorded values: 112 configurations at n = 12..21 and
    four at n = 130 (three 64-wide tiles: panel and bulk tasks, flag hand-offs of the factorisation + fused inverse)."""
    g = golden(fixture)
    for c in range(int(g['n_cases'])):
        d = case(g, 'c%d_' % c)
        k = gpu_nll_grad(eng, d)
        if 'loglik' in d:
            close(k.log_likelihood_func(), d['loglik'][0], rtol=1e-9)
        nll, grad = k.llik(d['x'].copy())
        close(nll, d['nll'], rtol=1e-9)
        close(grad, d['grad'], rtol=1e-7, atol=1e-8)
        close(k.scale, d['scale_after'], rtol=1e-9)
        Kf, fod = k.k_matrix(fod_eval=True)   # (fod is assembled in host numpy: API only, not on the hot path)
        # fod after llik(x): parameters moved to exp(x); compare against the oracle at those parameters
        from oracle import dgp_oracle as O
        X = d['X']
        _, fod_ref = O.k_matrix_fod(X, k.length, k.nugget[0], str(d['name']), bool(d['flags'][2]), d.get('W_diag'))
        close(fod, fod_ref, rtol=1e-10, atol=1e-14)


def test_wellconditioned_fixture_at_1e10(eng, golden):
    """g24 (nugget 1e-3, n = 150: three 64-wide tiles, cond(K) ~ 1e5), recorded from the reference: here the device results
    must agree to 1e-10 -- objective, gradient (K assembly, one-sweep factorisation + inverse, in-flight derivative
    reductions), ESS target, R^-1 y, gp and link_gp predictions (1e-8 on the link_gp variance: the Jd-based Matern J,
    SURVEY 8(c)).  The fixtures at the default nugget 1e-6 need looser bounds (cond ~ 1e7), which by themselves cannot tell a
    1e-7 kernel bug from conditioning."""
    from dgp_amd.kernel_class import kernel as K
    g = golden('g24_wellcond')
    for c in range(int(g['n_cases'])):
        d = case(g, 'c%d_' % c)
        name, nl = str(d['name']), int(d['n_local'])
        k = K(length=d['length'].copy(), scale=d['scale'][0], nugget=d['nugget'][0], name=name, prior_name='ga', prior_coef=None,
              nugget_est=bool(d['flags'][2]), scale_est=bool(d['flags'][4]), engine=eng)
        k.prior_coef = d['prior_coef'].copy()
        k.input = d['X'][:, :nl].copy()
        k.global_input = d['X'][:, nl:].copy() if d['X'].shape[1] > nl else None
        k.connect = np.arange(d['X'].shape[1] - nl) if k.global_input is not None else None
        k.output = d['y'].copy()
        close(k.log_likelihood_func(), d['loglik'][0], rtol=1e-10)
        k.compute_stats()
        close(npy(k.Rinv_y) if hasattr(k.Rinv_y, 'detach') else k.Rinv_y, d['Rinv_y'], rtol=1e-10, atol=1e-10 * np.abs(d['Rinv_y']).max())
        z = d['z'] if 'z' in d else None
        m, v = k.gp_prediction(d['x'], z)
        close(m, d['gp_m'], rtol=1e-10, atol=1e-12)
        close(v, d['gp_v'], rtol=1e-10, atol=1e-10 * d['scale'][0])   # (a difference of O(scale) terms)
        lm, lv = k.linkgp_prediction(d['lm_in'], d['lv_in'], z)
        close(lm, d['link_m'], rtol=1e-10, atol=1e-12)
        close(lv, d['link_v'], rtol=1e-8, atol=1e-10 * d['scale'][0])
        nll, grad = k.llik(d['x_opt'].copy())
        close(nll, d['nll'], rtol=1e-10)
        close(grad, d['grad'], rtol=1e-10, atol=1e-10 * np.abs(d['grad']).max())
        close(k.scale, d['scale_after'], rtol=1e-10)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
@pytest.mark.parametrize('n', [65, 500, 1984, 2000])
def test_potrf_potri_sizes(eng, name, n):
    """Factor / inverse / alpha / logdet / quad against LAPACK at sizes around the tile edges and the bench size."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(n)
    D = 4
    X = rng.uniform(size=(n, D))
    y = rng.normal(size=n)
    length = np.array([0.8])
    Kref = O.k_matrix(X, length, 1e-4, name)
    Xl = eng.tensor(X)
    A = eng.kmatrix(name, Xl, None, None, length, 1e-4, full=False, Y=eng.tensor(y))
    logdet, info = eng.potrf(n, A)
    work = eng.potrf_workspace(n, 1)
    quad = eng.aug_quad(n, A, 1, 1)
    eng.sync()
    Np = eng.padded_dim(n)
    L = np.tril(npy(A)[:n, :n])
    Lref = np.linalg.cholesky(Kref)
    assert int(npy(info)[0]) == 0
    close(L, Lref, rtol=1e-8, atol=1e-10)
    w = np.linalg.solve(Lref, y)
    close(npy(quad)[0, 0, 0], w @ w, rtol=1e-8)
    close(npy(logdet)[0], 2 * np.log(np.diag(Lref)).sum(), rtol=1e-10, atol=1e-9)
    Ainv = eng.empty(Np, Np)
    eng.potri(n, A, Ainv, 1, work)
    eng.sync()
    Kinv = np.linalg.inv(Kref)
    Ai = npy(Ainv)
    sc = np.abs(Kinv).max()
    close(Ai[:n, :n], Kinv, rtol=1e-7, atol=1e-8 * sc)
    close(Ai[:n, :n], Ai[:n, :n].T, rtol=0, atol=0)   # symmetric by construction
    alpha = Kinv @ y
    close(-Ai[n, :n], alpha, rtol=1e-7, atol=1e-8 * np.abs(alpha).max())


# (five or more matrices: the deeper task table -- 8 / 12 panels per visit, more than the block count at the small sizes --
#  and two to eight XCD groups, even and uneven)
@pytest.mark.parametrize('n,B', [(10, 2), (64, 1), (65, 1), (200, 3), (333, 5), (1000, 2), (2000, 1), (1984, 1),
                                 (300, 16), (520, 7), (700, 6), (1300, 5), (200, 12), (900, 8)])
def test_potrf_inv_one_sweep(eng, n, B):
    """dgpamd_potrf_inv: factor, L^-T, K^-1 (lower tiles) and -alpha from ONE sweep, against LAPACK."""
    import torch
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(n + B)
    Np = eng.padded_dim(n)
    A = eng.empty(B, Np, Np)
    T = torch.full((B, Np, Np), float('nan'), dtype=torch.float64, device=A.device)   # needs no initialisation
    S = torch.full((B, Np, Np), float('nan'), dtype=torch.float64, device=A.device)
    Ks, ys = [], []
    for b in range(B):
        X = rng.uniform(size=(n, 3))
        y = rng.normal(size=n)
        name = 'sexp' if b % 2 else 'matern2.5'
        Ks.append(O.k_matrix(X, np.array([0.6]), 1e-4, name))
        ys.append(y)
        eng.kmatrix(name, eng.tensor(X), None, None, np.array([0.6]), 1e-4, out=A[b], full=False, Y=eng.tensor(y))
    logdet, info = eng.potrf_inv(n, A, T, S, batch=B)
    eng.sync()
    assert not npy(info).any()
    for b in range(B):
        Lref = np.linalg.cholesky(Ks[b])
        Kinv = np.linalg.inv(Ks[b])
        sc = np.abs(Kinv).max()
        close(np.tril(npy(A[b])[:n, :n]), Lref, rtol=1e-8, atol=1e-10)
        close(npy(logdet)[b], 2 * np.log(np.diag(Lref)).sum(), rtol=1e-10, atol=1e-9)
        Linv = np.linalg.inv(Lref)
        Tb = npy(T[b])[:n, :n]
        # T is block upper triangular: compare where it is defined (tile row <= tile column)
        tr, tc = np.arange(n)[:, None] // 64, np.arange(n)[None, :] // 64
        close(np.where(tr <= tc, Tb, 0.0), np.where(tr <= tc, Linv.T, 0.0), rtol=1e-7, atol=1e-8 * np.abs(Linv).max())
        Sb = npy(S[b])
        close(np.where(tr >= tc, Sb[:n, :n], 0.0), np.where(tr >= tc, Kinv, 0.0), rtol=1e-7, atol=1e-8 * sc)
        alpha = Kinv @ ys[b]
        close(-Sb[n, :n], alpha, rtol=1e-7, atol=1e-8 * np.abs(alpha).max())
        close(-npy(A[b])[n, n], ys[b] @ alpha, rtol=1e-8)


def test_potrf_reports_not_pd(eng):
    import torch
    n = 100
    Np = eng.padded_dim(n)
    M = np.eye(Np)
    M[70, 70] = -1.0
    A = eng.tensor(M)
    logdet, info = eng.potrf(n, A)
    eng.sync()
    assert int(npy(info)[0]) == 71   # LAPACK convention: leading minor of order 71


def test_loglik_batched_vs_oracle(eng):
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(3)
    n, B = 300, 5
    F = rng.normal(size=(n, 3))
    NU = rng.normal(size=(n, 3))
    G = rng.uniform(size=(n, 2))
    y = rng.normal(size=n)
    th = rng.uniform(-3, 3, size=B)
    FP = eng.ess_propose(eng.tensor(F), eng.tensor(NU), th)
    eng.sync()
    for b in range(B):
        close(npy(FP)[b], O.update_f(F, NU, th[b]), rtol=1e-14, atol=1e-15)
    length = np.array([1.2, 0.7, 0.9, 1.1])
    colmap = [2, 0]
    ll, info = eng.loglik('matern2.5', FP, colmap, eng.tensor(G), length, 1e-5, 1.3, eng.tensor(y), batch=B)
    eng.sync()
    assert not npy(info).any()
    for b in range(B):
        Xb = np.concatenate((O.update_f(F, NU, th[b])[:, colmap], G), 1)
        close(npy(ll)[b], O.log_likelihood(Xb, y, length, 1.3, 1e-5, 'matern2.5'), rtol=1e-10)


def test_llik_batch_vs_oracle(eng):
    """dgpamd_llik_batch (one call per lock-step M-step round): nodes with different kernels, inputs, lengthscale
    layouts and nugget_est, full batch and a sub-batch, against the oracle's nll/gradient ingredients."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(11)
    n = 333
    Xa, Xb, G = rng.uniform(size=(n, 2)), rng.uniform(size=(n, 3)), rng.uniform(size=(n, 2))
    ys = [rng.normal(size=n) for _ in range(3)]
    cfg = [dict(kind='sexp', Xl=Xa, Xg=None, length=np.array([0.7]), nugget=1e-4, nugget_est=False, y=ys[0]),
           dict(kind='matern2.5', Xl=Xb, Xg=G, length=np.array([0.9, 1.3, 0.6, 1.1, 0.8]), nugget=2e-3, nugget_est=True, y=ys[1]),
           dict(kind='matern2.5', Xl=Xa, Xg=G, length=np.array([1.2]), nugget=1e-5, nugget_est=True, y=ys[2])]
    plan = eng.llik_plan(n, [dict(kind=c['kind'], Xloc=eng.tensor(c['Xl']), Xglob=None if c['Xg'] is None else eng.tensor(c['Xg']),
                                  nlen=len(c['length']), nugget_est=c['nugget_est'], W=None, y=eng.tensor(c['y'])) for c in cfg])

    def reference(c):
        X = c['Xl'] if c['Xg'] is None else np.concatenate((c['Xl'], c['Xg']), 1)
        K, fod = O.k_matrix_fod(X, c['length'], c['nugget'], c['kind'], c['nugget_est'], None)
        Kinv = np.linalg.inv(K)
        a = Kinv @ c['y']
        return (np.linalg.slogdet(K)[1], c['y'] @ a, np.array([np.sum(Kinv * d) for d in fod]),
                np.array([a @ d @ a for d in fod]))

    for idx in ([0, 1, 2], [2, 0], [1]):
        for b in idx:
            plan.set(b, cfg[b]['length'], cfg[b]['nugget'])
        out = plan.run(idx)
        for b in idx:
            ld, q, tr, qq = reference(cfg[b])
            P = len(tr)
            h = out[b]
            assert len(h) == 3 + 2 * P and h[-1] == 0
            close(h[0], ld, rtol=1e-10, atol=1e-9)
            close(h[1], q, rtol=1e-8)
            close(h[2:2 + P], tr, rtol=1e-7, atol=1e-8 * np.abs(tr).max())
            close(h[2 + P:2 + 2 * P], qq, rtol=1e-7, atol=1e-8 * np.abs(qq).max())
    # the same call in two halves (dgpamd_llik_batch_launch / _wait) with other blocking calls of the engine in between: the same bits
    for b in (0, 1, 2):
        plan.set(b, cfg[b]['length'], cfg[b]['nugget'])
    whole = plan.run([0, 1, 2])
    token = plan.launch([0, 1, 2])
    probe = eng.tensor(np.arange(5000.0))
    assert np.array_equal(eng.fetch(probe), np.arange(5000.0))       # (a fetch through the engine's own pinned staging buffer while the evaluation is in flight)
    with pytest.raises(Exception):
        plan.launch([0])                                             # one evaluation in flight per engine
    halves = plan.wait(token)
    for b in (0, 1, 2):
        assert np.array_equal(whole[b], halves[b])
    with pytest.raises(Exception):
        plan.wait(token)                                             # nothing in flight any more
    # a non-positive-definite node is reported through its info word, the others are unaffected
    plan.set(0, cfg[0]['length'], -2.0)
    out = plan.run([0, 1])
    assert out[0][-1] > 0 and out[1][-1] == 0
    close(out[1][0], reference(cfg[1])[0], rtol=1e-10, atol=1e-9)


def test_trmv_is_fmvn(eng, golden):
    g = golden('g4_fmvn')
    # cov = scale*K: factor K = cov/scale on device, nu = sqrt(scale) L z  (functions.py:113-121)
    cov, z = g['cov'], g['z']
    n = len(z)
    Np = eng.padded_dim(n)
    A = np.zeros((Np, Np))
    A[:n, :n] = cov / 1.3
    Ad = eng.tensor(A)
    eng.potrf(n, Ad)
    nu = eng.trmv_lower(n, Ad, [1.3], eng.tensor(z))
    eng.sync()
    close(npy(nu)[0], g['sample'], rtol=1e-9, atol=1e-12)


# ---------------------------------------------------------------- a10-a14
@pytest.mark.parametrize('direct', [False, True])
def test_gp_and_linkgp_golden(eng, golden, direct):
    """direct=True: the Matern J factor in the reference's own expression order; False: its separable form."""
    eng.set_linkgp_direct(direct)
    g = golden('g7_predict')
    for c in range(int(g['n_cases'])):
        d = case(g, 'c%d_' % c)
        name = str(d['name'])
        nl = int(d['n_local'])
        X = d['X']
        n = len(X)
        x = d['x'] if 'z' not in d else np.concatenate((d['x'], d['z']), 1)
        Rinv = eng.tensor(d['Rinv'])
        ry = eng.tensor(d['Rinv_y'])
        m, v = eng.gp_predict(name, eng.tensor(x), eng.tensor(X), d['length'], Rinv, n, ry, d['scale'][0], d['nugget'][0])
        eng.sync()
        close(npy(m), d['gp_m'], rtol=1e-9, atol=1e-11)
        close(npy(v), d['gp_v'], rtol=1e-7, atol=1e-9)
        z = eng.tensor(d['z']) if 'z' in d else None
        Wg = eng.tensor(X[:, nl:]) if 'z' in d else None
        lm, lv = eng.linkgp_predict(name, eng.tensor(d['lm_in']), eng.tensor(d['lv_in']), z, eng.tensor(X[:, :nl]), Wg,
                                    d['length'], Rinv, n, ry, d['scale'][0], d['nugget'][0])
        eng.sync()
        ref_m, ref_v = d['link_m'], d['link_v']
        if name == 'matern2.5':   # (the recorded values are the reference's expression: the same inputs through the oracle on the integral)
            from oracle import dgp_oracle as O
            with integral_oracle():
                ref_m, ref_v = O.link_gp_predict(d['lm_in'], d['lv_in'], d.get('z'), X[:, :nl], X[:, nl:] if 'z' in d else None, d['Rinv'],
                                                 d['Rinv_y'], d['scale'], d['length'], d['nugget'], name)
        close(npy(lm), ref_m, rtol=1e-8, atol=1e-10)
        close(npy(lv), ref_v, rtol=1e-6, atol=1e-8)
    eng.set_linkgp_direct(False)


@pytest.mark.parametrize('n,M,Dw,Dz', [(130, 40, 4, 1), (200, 37, 2, 0), (64, 5, 5, 3), (257, 19, 1, 2), (70, 300, 3, 2)])   # (M = 300: two record chunks)
def test_linkgp_separable_equals_direct(eng, n, M, Dw, Dz):
    """Same inputs through both evaluations of the Matern J factor, incl. tiny and zero input variances, with and
    without deterministic global inputs, sizes on and off the 64-point tile edge."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(21)
    X = rng.uniform(size=(n, Dw + Dz))
    y = rng.normal(size=n)
    length = rng.uniform(0.3, 1.5, size=Dw + Dz)
    nug = 1e-4 if Dw + Dz >= 5 else 1e-2   # (few input dimensions: keep R well conditioned, the two forms differ by rounding x cond)
    st = O.compute_stats(X, y, length, nug, 'matern2.5', Dw)
    mm = rng.uniform(-0.2, 1.2, size=(M, Dw))
    vv = 10.0 ** rng.uniform(-6, 0, size=(M, Dw))
    vv[0] = 0.0
    vv[1, Dw - 1] = 0.0
    z = rng.uniform(size=(M, Dz)) if Dz else None
    args = (eng.tensor(mm), eng.tensor(vv), eng.tensor(z) if Dz else None, eng.tensor(X[:, :Dw]),
            eng.tensor(X[:, Dw:]) if Dz else None, length, eng.tensor(st['Rinv']), n, eng.tensor(st['Rinv_y']), 1.3, nug)
    eng.set_linkgp_direct(True)
    m1, v1 = eng.linkgp_predict('matern2.5', *args)
    m1, v1 = npy(m1), npy(v1)
    eng.set_linkgp_direct(False)
    m2, v2 = eng.linkgp_predict('matern2.5', *args)
    close(npy(m2), m1, rtol=1e-12, atol=1e-14)
    close(npy(v2), v1, rtol=1e-6, atol=1e-8)
    with integral_oracle():
        lmr, lvr = O.link_gp_predict(mm, vv, z, X[:, :Dw], X[:, Dw:] if Dz else None, st['Rinv'], st['Rinv_y'], 1.3, length, nug, 'matern2.5')
    close(m1, lmr, rtol=1e-8, atol=1e-10)
    close(v1, lvr, rtol=1e-6, atol=1e-8)
    close(npy(v2), lvr, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_gp_linkgp_larger_vs_oracle(eng, name):
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(8)
    n, M, Dw, Dz = 150, 70, 3, 2
    X = rng.uniform(size=(n, Dw + Dz))
    y = rng.normal(size=n)
    length = rng.uniform(0.6, 1.4, size=Dw + Dz)
    st = O.compute_stats(X, y, length, 1e-3, name, Dw)
    x = rng.uniform(size=(M, Dw + Dz))
    mr, vr = O.gp_predict(x, X, st['Rinv'], st['Rinv_y'], 1.4, length, 1e-3, name)
    Rinv, ry = eng.tensor(st['Rinv']), eng.tensor(st['Rinv_y'])
    m, v = eng.gp_predict(name, eng.tensor(x), eng.tensor(X), length, Rinv, n, ry, 1.4, 1e-3)
    eng.sync()
    close(npy(m), mr, rtol=1e-9, atol=1e-11)
    close(npy(v), vr, rtol=1e-7, atol=1e-9)
    mm = rng.uniform(size=(M, Dw))
    vv = rng.uniform(0.001, 0.2, size=(M, Dw))
    vv[3] = 0.0
    z = rng.uniform(size=(M, Dz))
    with integral_oracle():
        lmr, lvr = O.link_gp_predict(mm, vv, z, X[:, :Dw], X[:, Dw:], st['Rinv'], st['Rinv_y'], 1.4, length, 1e-3, name)
    lm, lv = eng.linkgp_predict(name, eng.tensor(mm), eng.tensor(vv), eng.tensor(z), eng.tensor(X[:, :Dw]),
                                eng.tensor(X[:, Dw:]), length, Rinv, n, ry, 1.4, 1e-3)
    eng.sync()
    close(npy(lm), lmr, rtol=1e-8, atol=1e-10)
    close(npy(lv), lvr, rtol=1e-6, atol=1e-8)


def test_moments(eng):
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(5)
    mus, vs = rng.normal(size=(4, 50, 2)), rng.uniform(size=(4, 50, 2))
    s1, s2 = eng.zeros(50, 2), eng.zeros(50, 2)
    for a, b in zip(mus, vs):
        eng.moments_accumulate(eng.tensor(a), eng.tensor(b), s1, s2)
    eng.moments_finalize(4, s1, s2)
    eng.sync()
    mu, var = O.aggregate_moments(mus, vs)
    close(npy(s1), mu, rtol=1e-13)
    close(npy(s2), var, rtol=1e-11, atol=1e-13)


# ---------------------------------------------------------------- a17-a23
def test_vecchia_nn_bit_exact(eng, golden):
    import torch
    g = golden('g8_vecchia')
    NN = eng.nn_ordered(eng.tensor(g['nn_x']), int(g['nn_m']))
    PN = eng.nn_query(eng.tensor(g['pq']), eng.tensor(g['nn_x']), 12)
    eng.sync()
    assert NN.dtype == torch.int64
    np.testing.assert_array_equal(npy(NN), g['NNarray'])
    np.testing.assert_array_equal(npy(PN), g['pred_nn'])
    # m == n shortcut of get_pred_nn (vecchia.py:23-26)
    from oracle import dgp_oracle as O
    q = g['pq'][:5]
    np.testing.assert_array_equal(npy(eng.nn_query(eng.tensor(q), eng.tensor(g['nn_x'][:7]), 50)), O.pred_nn(q, g['nn_x'][:7], 50))


def test_vecchia_kernels_golden(eng, golden):
    g = golden('g8_vecchia')
    for c in range(int(g['n_cases'])):
        d = case(g, 'v%d_' % c)
        name = str(d['name'])
        X, y, NN = d['X'], d['y'], d['NN']
        n = len(X)
        sc, ng, ln = float(d['scale']), float(d['nugget']), d['length']
        nugget_est, scale_est = bool(d['flags'][0]), bool(d['flags'][1])
        dX, dy, dNN, ones = eng.tensor(X), eng.tensor(y[:, 0]), eng.tensor(NN, dtype=__import__('torch').int64), eng.tensor(np.ones(n))
        np.testing.assert_array_equal(npy(eng.nn_ordered(eng.tensor(X / ln), 6)), NN)
        out = npy(eng.vecchia_llik(name, dX, dy, dNN, ln, ng, ones))
        close(-0.5 * (out[1] + out[0] / sc), d['llik'][0], rtol=1e-9)
        o, P = eng.vecchia_nllik(name, dX, dy, dNN, ln, ng, ones, nugget_est)
        o = npy(o)
        quad, logdet, dquad, dlogdet = o[0], o[1], o[2:2 + P], o[2 + P:]
        if scale_est:
            s2 = quad / n
            nll = 0.5 * (logdet + n * np.log(s2))
        else:
            s2 = sc
            nll = 0.5 * (logdet + quad / sc)
        close(nll, d['nll'][0], rtol=1e-9)
        close(0.5 * (dlogdet - dquad / s2), d['grad'], rtol=1e-7, atol=1e-8)
        close(s2, d['scale_out'][0], rtol=1e-9)
        Lm = eng.vecchia_lmatrix(name, dX, dNN, ln, ng)
        close(npy(Lm), d['Lmat'], rtol=1e-8, atol=1e-8 * np.abs(d['Lmat']).max())
        xs = eng.vecchia_spsolve(eng.tensor(d['Lmat']), dNN, 1 / np.sqrt(sc), eng.tensor(d['b']))
        close(npy(xs), d['spsolve'], rtol=1e-9, atol=1e-11)
        pNN = eng.tensor(d['pNN'], dtype=__import__('torch').int64)
        gm, gv = eng.vecchia_gp(name, eng.tensor(d['xq']), dX, pNN, dy, sc, ln, ng, ones)
        close(npy(gm), d['gpv_m'], rtol=1e-8, atol=1e-10)
        close(npy(gv), d['gpv_v'], rtol=1e-7, atol=1e-10)
        lm, lv = eng.vecchia_linkgp(name, eng.tensor(d['lm_in']), eng.tensor(d['lv_in']), eng.tensor(d['lz_in']),
                                    eng.tensor(X[:, :2]), eng.tensor(X[:, 2:]), pNN, dy, sc, ln, ng, ones)
        ref_m, ref_v = d['lgv_m'], d['lgv_v']
        if name == 'matern2.5':   # (as in test_gp_and_linkgp_golden)
            from oracle import dgp_oracle as O
            with integral_oracle():
                ref_m, ref_v = O.link_gp_vecch(d['lm_in'], d['lv_in'], d['lz_in'], X[:, :2], X[:, 2:], d['pNN'], y, sc, ln, ng, np.ones(n), name)
        close(npy(lm), ref_m, rtol=1e-7, atol=1e-9)
        close(npy(lv), ref_v, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_vecchia_row_kernels_register_and_lds_versions_agree(eng, name):
    """Conditioning sets of up to 31 points take the register-resident two-rows-per-wave kernel, larger ones (and
    DGPAMD_VECCHIA_LDS=1) the LDS kernel the golden vectors were first pinned on: same sums, gradients and sparse-factor
    rows to rounding over ragged first rows, odd n, isotropic / ARD lengthscales, nugget weights, and a batch of inputs."""
    import torch
    rng = np.random.default_rng(31)
    with contextlib.ExitStack() as stack:   # (POISON_LDS: NaNs in every CU's LDS before each row launch: nothing unwritten may be read)
        engines = {lds: stack.enter_context(engine_under(POISON_LDS=1, VECCHIA_LDS=lds)) for lds in ('0', '1')}
        for n, D, m, ard, nugget_est in [(301, 3, 6, False, True), (777, 8, 25, False, False), (500, 5, 30, True, True), (64, 1, 12, False, True),
                                         (40, 2, 30, True, False), (260, 2, 8, False, False), (130, 2, 3, False, True), (200, 12, 17, True, True),
                                         (333, 4, 21, False, True), (150, 3, 27, False, False)]:
            X = rng.uniform(size=(n, D))
            y = np.sin(3 * X[:, 0]) + 0.1 * rng.normal(size=n)
            ln = rng.uniform(0.4, 1.2, size=D) if ard else np.array([0.7])
            w = rng.uniform(0.5, 2.0, size=n)
            dX, dy, dw = eng.tensor(X), eng.tensor(y), eng.tensor(w)
            NN = eng.nn_ordered(eng.tensor(X / ln), m)
            XB = eng.tensor(np.stack([X, X + 0.01 * rng.normal(size=X.shape), rng.uniform(size=X.shape)]))
            got = {}
            for lds, e in engines.items():
                o, P = e.vecchia_nllik(name, dX, dy, NN, ln, 1e-3, dw, nugget_est)
                got[lds] = (npy(e.vecchia_llik(name, dX, dy, NN, ln, 1e-3, dw)), npy(o), npy(e.vecchia_lmatrix(name, dX, NN, ln, 1e-3)),
                            npy(e.vecchia_llik_batch(name, XB, dy, NN, ln, 1e-3, dw)))
            for a, b in zip(got['0'], got['1']):
                close(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max())
            close(got['0'][3][0], got['0'][0], rtol=1e-14)       # batch member 0 is the single evaluation
            for j in range(3):                                   # and every member equals its own single evaluation
                close(got['0'][3][j], npy(engines['0'].vecchia_llik(name, XB[j], dy, NN, ln, 1e-3, dw)), rtol=1e-14)


@pytest.mark.parametrize('s', [1.0, 1e4])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_vecchia_row_kernels_beyond_the_exponent_range(eng, name, s):
    """vecchia_llik, vecchia_nllik and vecchia_lmatrix on far_inputs (n = 130, m = 10, neighbour arrays from the oracle): every
    conditioning block is (1 + nugget) I in the oracle's arithmetic.  test_vecchia_kernels_golden's tolerances; sparse-factor
    entries and gradient components that are exactly 0 there may be 1e-300 here at the most."""
    import torch
    from oracle import dgp_oracle as O
    n, m = 130, 10
    X = far_inputs(n, s)
    y = np.random.default_rng(4).normal(size=n)
    ones = np.ones(n)
    NN = O.nn_ordered(X / FAR_LENGTH, m)
    dX, dy, dNN, d1 = eng.tensor(X), eng.tensor(y), eng.tensor(NN, dtype=torch.int64), eng.tensor(ones)
    out = npy(eng.vecchia_llik(name, dX, dy, dNN, FAR_LENGTH, FAR_NUGGET, d1))
    close(-0.5 * (out[1] + out[0] / FAR_SCALE), O.vecchia_llik(X, y, NN, FAR_SCALE, FAR_LENGTH, FAR_NUGGET, ones, name), rtol=1e-9)
    o, P = eng.vecchia_nllik(name, dX, dy, dNN, FAR_LENGTH, FAR_NUGGET, d1, True)
    o = npy(o)
    quad, logdet, dquad, dlogdet = o[0], o[1], o[2:2 + P], o[2 + P:]
    nll, grad, _ = O.vecchia_nllik(X, y, NN, FAR_SCALE, FAR_LENGTH, FAR_NUGGET, ones, name, False, True, n, 0.0)
    close(0.5 * (logdet + quad / FAR_SCALE), nll, rtol=1e-9)
    assert grad[0] == 0.0 and grad[1] != 0.0
    close_or_zero(0.5 * (dlogdet - dquad / FAR_SCALE), grad, rtol=1e-7, atol=1e-8)
    Lref = O.L_matrix(X, NN, FAR_LENGTH, FAR_NUGGET, name)
    assert np.count_nonzero(Lref) == n
    close_or_zero(npy(eng.vecchia_lmatrix(name, dX, dNN, FAR_LENGTH, FAR_NUGGET)), Lref, rtol=1e-8, atol=1e-8 * np.abs(Lref).max())


@pytest.mark.parametrize('s', [1.0, 1e4])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_vecchia_predictions_beyond_the_exponent_range(eng, name, s):
    """vecchia_gp and vecchia_linkgp (sexp against the oracle; matern2.5 against the exact factors of tests/linkfun_ref.py, the reference's
    expression being not finite here) on far_inputs, register and LDS kernels: M = 8 test points, four ON training points (mean y_i up to the nugget) and four
    between them (prior mean 0, variance scale (1 + nugget)), n = 130, 10 neighbours from the oracle.
    test_vecchia_kernels_golden's tolerances; means that are exactly 0 in the oracle may be 1e-300 here at the most."""
    import torch
    from oracle import dgp_oracle as O
    n, pm = 130, 10
    X = far_inputs(n, s)
    y = np.random.default_rng(6).normal(size=n)
    ones = np.ones(n)
    xq = np.concatenate((X[[0, 5, 64, 129]], far_inputs(4, s) + 0.25 * s))
    vq = np.full(xq.shape, 1e-12)
    pNN = O.pred_nn(xq / FAR_LENGTH, X / FAR_LENGTH, pm)
    gm, gv = O.gp_vecch(xq, X, pNN, y, FAR_SCALE, FAR_LENGTH, FAR_NUGGET, ones, name)
    assert np.count_nonzero(gm) == 4
    with np.errstate(all='ignore'):
        lm, lv = O.link_gp_vecch(xq, vq, None, X, None, pNN, y, FAR_SCALE, FAR_LENGTH, FAR_NUGGET, ones, name)
    if name == 'sexp':
        assert np.count_nonzero(lm) == 4
    else:   # (why vecchia_linkgp is not compared for the Matern kind: the reference itself is not finite on these inputs)
        assert not (np.all(np.isfinite(lm)) and np.all(np.isfinite(lv))), (lm, lv)
    with contextlib.ExitStack() as stack:
        for lds in ('0', '1'):
            e = stack.enter_context(engine_under(POISON_LDS=1, VECCHIA_LDS=lds))
            t = e.tensor
            dNN = t(pNN, dtype=torch.int64)
            m_, v_ = e.vecchia_gp(name, t(xq), t(X), dNN, t(y), FAR_SCALE, FAR_LENGTH, FAR_NUGGET, t(ones))
            close_or_zero(npy(m_), gm, rtol=1e-8, atol=1e-10)
            close(npy(v_), gv, rtol=1e-7, atol=1e-10)
            if name == 'sexp':
                m_, v_ = e.vecchia_linkgp(name, t(xq), t(vq), None, t(X), None, dNN, t(y), FAR_SCALE, FAR_LENGTH, FAR_NUGGET, t(ones))
                close_or_zero(npy(m_), lm, rtol=1e-7, atol=1e-9)
                close(npy(v_), lv, rtol=1e-6, atol=1e-8)
            else:   # the Matern factors follow the integral (tests/linkfun_ref.py): finite here, and compared with its exact values
                import linkfun_ref
                far = linkfun_ref.load_e2e()
                I2, J2 = (float(linkfun_ref.join(*far[k]) ** 2) for k in ('far_I', 'far_J0'))   # two dimensions; every other factor is 0
                ry = y[[0, 5, 64, 129]] / (1.0 + FAR_NUGGET)
                em = np.concatenate((I2 * ry, np.zeros(4)))                # on a training point: y_i up to the nugget; between: the prior
                ev = np.concatenate((np.abs(ry * ry * J2 - (I2 * ry) ** 2 + FAR_SCALE * (1.0 + FAR_NUGGET - J2 / (1.0 + FAR_NUGGET))),
                                     np.full(4, FAR_SCALE * (1.0 + FAR_NUGGET))))
                m_, v_ = e.vecchia_linkgp(name, t(xq), t(vq), None, t(X), None, dNN, t(y), FAR_SCALE, FAR_LENGTH, FAR_NUGGET, t(ones))
                close_or_zero(npy(m_), em, rtol=1e-7, atol=1e-9)
                close(npy(v_), ev, rtol=1e-6, atol=1e-8)


def test_nn_streaming_topk_equals_store_once_kernel(eng):
    """Candidate sets of 4096 points and more in up to 16 dimensions take the streaming top-k kernels (register-resident
    sorted lists, candidates staged once per 64 queries); DGPAMD_NN_STORE_ONCE=1 forces the store-once histogram kernel
    the bit-exact golden comparison was first made with (=2 the streaming ones).  Same neighbour arrays, element for element: ordered (vecchia.py:
    98-109) and query form (:20-37), ties between duplicated points broken by index, fewer candidates than neighbours in
    the first rows, query counts that do not fill the last block of 64."""
    rng = np.random.default_rng(17)
    # (2: streaming at every size; by default it starts where it pays: n >= 12 000)
    with engine_under(NN_STORE_ONCE=2) as e2, engine_under(NN_STORE_ONCE=1) as e1:
        for n, D, m in [(4500, 3, 25), (6001, 8, 25), (5000, 1, 15), (4200, 12, 50), (9000, 2, 60), (4100, 5, 31)]:
            x = rng.uniform(size=(n, D))
            x[rng.integers(0, n, 300)] = x[rng.integers(0, n, 300)]       # duplicated points: equal distances
            q = np.concatenate((rng.uniform(size=(333, D)), x[:40]))
            dx, dq = eng.tensor(x), eng.tensor(q)
            got = {}
            for flag, e in (('2', e2), ('1', e1)):
                got[flag] = (npy(e.nn_ordered(dx, m)), npy(e.nn_query(dq, dx, m)))
            np.testing.assert_array_equal(got['2'][0], got['1'][0])
            np.testing.assert_array_equal(got['2'][1], got['1'][1])
            a = got['2'][0]
            assert a.shape == (n, m + 1) and np.array_equal(a[:, 0], np.arange(n)) and np.all(a[:5, 6:] == -1)


@pytest.mark.parametrize('B', [24, 32, 64])
def test_one_launch_factorisation_with_many_matrices(eng, B):
    """24-64 matrices per call (DGPAMD_MAXB = 64): the one-launch kernel's critical-lane workers are capped per XCD so that workers
    which take bulk work first remain (uncapped, 12 x 64 of them would be every worker of the launch, each running ahead in the critical
    queue and waiting for bulk results nobody computes).  Factors, inverses and log-determinants equal the per-block-step kernel's, bit for bit."""
    import torch
    n = 300
    Np = eng.padded_dim(n)
    r = np.random.default_rng(B)
    X, G, y = eng.tensor(r.uniform(size=(B, n, 4))), eng.tensor(r.uniform(size=(n, 3))), eng.tensor(r.normal(size=n))
    work = eng.potrf_workspace(n, B)
    out = {}
    try:
        for mode in (0, 1):
            eng.set_potrf_mode(mode)
            A, T, S = eng.empty(B, Np, Np), eng.empty(B, Np, Np), eng.empty(B, Np, Np)
            eng.kmatrix('matern2.5', X, None, G, [0.7], 1e-5, out=A, full=False, Y=y, batch=B)
            ld, info = eng.potrf(n, A, batch=B, work=work)
            L = torch.tril(A[:, :n + 1, :n]).clone()
            eng.kmatrix('matern2.5', X, None, G, [0.7], 1e-5, out=A, full=False, Y=y, batch=B)
            ld2, info2 = eng.potrf_inv(n, A, T, S, batch=B, work=work)
            out[mode] = (L, torch.tril(S[:, :n + 1, :n]).clone(), ld.clone(), ld2.clone(), int(info.abs().sum()) + int(info2.abs().sum()))
    finally:
        eng.set_potrf_mode(1)
    assert out[0][4] == 0 and out[1][4] == 0
    for a, b in zip(out[0][:4], out[1][:4]):
        assert torch.equal(a, b)


def test_nn_query_filter_then_select_equals_streaming_topk(eng):
    """From 30 000 queries against 20 000 points on the query search (vecchia.py:20-40) takes the filter-then-select kernels of round 5
    (a sampled upper bound of every query's K-th nearest distance, a register-light scan that notes the candidates at or below it, the
    K nearest of the notes; csrc/vecchia_nn.hip nn_tau / nn_collect / nn_pick); DGPAMD_NN_FILTER=0 keeps the streaming top-k kernel.  Same
    neighbour arrays element for element -- uniform points, a cluster the strided sample all but misses (wide bounds, the exact
    slow path), exactly tied distances on a grid, all candidates equal, a query count that does not fill the last block -- and, on a
    sample of queries, the brute-force (distance, index) order."""
    rng = np.random.default_rng(23)
    cases = [('uniform', rng.uniform(size=(30011, 6)), rng.uniform(size=(20050, 6)), 50),
             ('uniform, 16 dims, 64 neighbours', rng.uniform(size=(30001, 16)), rng.uniform(size=(20000, 16)), 64)]
    xc = np.concatenate([rng.normal(size=(300, 3)) * 1e-3, rng.uniform(size=(20700, 3)) * 30.0])
    rng.shuffle(xc)
    cases.append(('cluster', np.concatenate([rng.normal(size=(15000, 3)) * 1e-3, rng.uniform(size=(15040, 3)) * 30.0]), xc, 40))
    g = np.stack(np.meshgrid(np.arange(150.), np.arange(140.)), -1).reshape(-1, 2)
    cases.append(('grid', g[rng.integers(0, len(g), 30100)], g, 31))
    cases.append(('equal', rng.uniform(size=(30000, 2)), np.ones((20000, 2)), 33))
    with engine_under(NN_FILTER=1) as e1, engine_under(NN_FILTER=0) as e0:
        for name, q, x, m in cases:
            dq, dx = eng.tensor(q), eng.tensor(x)
            got = {'1': npy(e1.nn_query(dq, dx, m)), '0': npy(e0.nn_query(dq, dx, m))}
            np.testing.assert_array_equal(got['1'], got['0'], err_msg=name)
            for i in rng.integers(0, len(q), 12):   # ... and both against brute force
                dist = ((x - q[i]) ** 2).sum(1)
                want = np.lexsort((np.arange(len(x)), dist))[:m]
                # (numpy sums the squares in another order: compare the sets through their distances)
                np.testing.assert_allclose(np.sort(dist[got['1'][i]]), np.sort(dist[want]), rtol=0, atol=1e-12 * max(1.0, dist.max()), err_msg=name)


def test_vecchia_spsolve_long_chain(eng):
    """Rows span many 1024-row windows and deep in-window dependency chains."""
    from oracle import dgp_oracle as O
    import torch
    rng = np.random.default_rng(12)
    n, m = 3000, 5
    x = np.sort(rng.uniform(size=(n, 1)), axis=0)   # ordered 1-D points: every row depends on its predecessor
    NN = O.nn_ordered(x, m)
    L = rng.uniform(0.5, 1.5, size=(n, m + 1))
    b = rng.normal(size=n)
    ref = O.forward_solve_sp(L, NN, b)
    out = eng.vecchia_spsolve(eng.tensor(L), eng.tensor(NN, dtype=torch.int64), 1.0, eng.tensor(b))
    close(npy(out), ref, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('n', [1, 2, 3, 63, 64, 127, 128, 129, 192, 257, 320, 449, 511])
def test_potrf_and_inv_edge_sizes(eng, n):
    """Sizes around the 64-wide block edges (also n = 64 j: a last block that carries only the right-hand side), three
    matrices per call, both entry points, against LAPACK."""
    import torch
    rng = np.random.default_rng(1000 + n)
    B = 3
    Np = eng.padded_dim(n)
    A1, A2 = eng.empty(B, Np, Np), eng.empty(B, Np, Np)
    T = torch.full((B, Np, Np), float('nan'), dtype=torch.float64, device=A1.device)
    S = torch.full((B, Np, Np), float('nan'), dtype=torch.float64, device=A1.device)
    Ks, ys = [], []
    for b in range(B):
        X = rng.uniform(size=(n, 2))
        G = rng.normal(size=(n, n + 3))
        K = G @ G.T / (n + 3) + 0.5 * np.eye(n)          # well conditioned, not a kernel matrix
        y = rng.normal(size=n)
        Ks.append(K)
        ys.append(y)
        M = np.zeros((Np, Np))
        M[:n, :n] = K
        M[n, :n] = y
        A1[b] = eng.tensor(M)
        A2[b] = eng.tensor(M)
    ld1, info1 = eng.potrf(n, A1, batch=B)
    ld2, info2 = eng.potrf_inv(n, A2, T, S, batch=B)
    eng.sync()
    assert not npy(info1).any() and not npy(info2).any()
    tr, tc = np.arange(n)[:, None] // 64, np.arange(n)[None, :] // 64
    for b in range(B):
        L = np.linalg.cholesky(Ks[b])
        Kinv = np.linalg.inv(Ks[b])
        alpha = Kinv @ ys[b]
        for A, ld in ((A1, ld1), (A2, ld2)):
            close(np.tril(npy(A[b])[:n, :n]), L, rtol=1e-9, atol=1e-11)
            close(npy(ld)[b], 2 * np.log(np.diag(L)).sum(), rtol=1e-11, atol=1e-10)
            close(-npy(A[b])[n, n], ys[b] @ alpha, rtol=1e-9)
        close(np.where(tr >= tc, npy(S[b])[:n, :n], 0.0), np.where(tr >= tc, Kinv, 0.0), rtol=1e-8, atol=1e-10)
        close(-npy(S[b])[n, :n], alpha, rtol=1e-8, atol=1e-10)
        close(np.where(tr <= tc, npy(T[b])[:n, :n], 0.0), np.where(tr <= tc, np.linalg.inv(L).T, 0.0), rtol=1e-8, atol=1e-10)


def test_ess_update_resumes_when_uniforms_run_out(eng):
    """dgpamd_ess_update hands back (status 1) when the supplied uniforms are used up; continuing with the next
    uniforms must reach the accepted proposal, log-likelihood and uniform count of a single call that had them all,
    and of the sequential loop (imputation.py:81-119) done by hand with the oracle."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(5)
    n, M = 150, 2
    F0, NU = rng.normal(size=(n, M)), rng.normal(size=(n, M))
    G = rng.uniform(size=(n, 1))
    length, nugget, scale = np.array([1.1, 0.8, 0.9]), 1e-4, 1.4
    # y drawn from the GP at the current latent: the current state is a good one, most proposals are rejected
    y = O.fmvn(scale * O.k_matrix(np.concatenate((F0, G), 1), length, nugget, 'sexp'), rng.standard_normal(n))
    us = rng.uniform(size=40)

    def ll_of(Fp):
        return O.log_likelihood(np.concatenate((Fp, G), 1), y, length, scale, nugget, 'sexp')
    cur = ll_of(F0)
    theta0 = 2 * np.pi * 0.37

    def sequential(log_y):
        theta, lo, hi, used = theta0, theta0 - 2 * np.pi, theta0, 0
        while True:
            Fp = O.update_f(F0, NU, theta)
            l = ll_of(Fp)
            if l > log_y:
                return Fp, l, used
            if theta < 0:
                lo = theta
            else:
                hi = theta
            theta = lo + (hi - lo) * us[used]
            used += 1
    for frac in (0.999, 0.99, 0.9, 0.5):     # a slice demanding enough for several shrinks before acceptance
        log_y = cur + np.log(frac)
        Fp, l, used = sequential(log_y)
        if used >= 3:
            break
    assert 3 <= used < 30

    def run(chunks):
        plan = eng.ess_plan(n, M, 'sexp', np.arange(M, dtype=np.int32), eng.tensor(G), length, nugget, None, eng.tensor(y), 3)
        Fd, NUd = eng.tensor(F0.copy()), eng.tensor(NU)
        th, l_, h_, pend, pos, props = theta0, theta0 - 2 * np.pi, theta0, False, 0, 0
        while True:
            status, u, p, nb, ll_acc, info, th, l_, h_, pend = plan.run(Fd, NUd, scale, log_y, th, l_, h_, pend,
                                                                      us[pos:pos + chunks], 2)
            pos += u
            props += p
            assert status in (0, 1) and info == 0
            if status == 0:
                eng.sync()
                return npy(Fd), ll_acc, pos, props
    Fa, lla, useda, propsa = run(40)
    Fb, llb, usedb, propsb = run(1)       # one uniform per call: resumes after every shrink
    assert useda == usedb == used and propsa >= used + 1
    close(Fa, Fp, rtol=1e-12, atol=1e-13)
    close(Fb, Fp, rtol=1e-12, atol=1e-13)
    close(lla, l, rtol=1e-9)
    close(llb, l, rtol=1e-9)


def test_nn_large_candidate_sets(eng):
    """The store-once neighbour search (>= 4096 candidates) against numpy: bit-exact in (distance, index) order on integer
    coordinates (all distances exact, many ties), set-equal with equal neighbour distances on clustered real data,
    all-equal points, ordered (Vecchia) variant."""
    rng = np.random.default_rng(11)
    grid = np.stack(np.meshgrid(np.arange(90.), np.arange(70.)), -1).reshape(-1, 2)[rng.permutation(6300)]
    q = grid[rng.integers(0, len(grid), 50)] + np.array([0.0, 0.5])
    got = npy(eng.nn_query(eng.tensor(q), eng.tensor(grid), 40))
    d = ((q[:, None, :] - grid[None]) ** 2).sum(-1)
    want = np.lexsort((np.broadcast_to(np.arange(len(grid)), d.shape), d), axis=1)[:, :40]
    assert np.array_equal(got, want)
    od = npy(eng.nn_ordered(eng.tensor(grid), 15))
    for i in (0, 3, 15, 16, 4095, 4096, 5000, 6299):
        di = ((grid[:i + 1] - grid[i]) ** 2).sum(1)
        w = np.sort(np.lexsort((np.arange(i + 1), di))[:16])[::-1]
        assert np.array_equal(od[i][:len(w)], w) and np.all(od[i][len(w):] == -1)
    x = np.concatenate([rng.normal(size=(3000, 3)) * 1e-3, rng.uniform(size=(3000, 3)) * 100.0])
    q = x[rng.integers(0, len(x), 30)] + 1e-4
    got = npy(eng.nn_query(eng.tensor(q), eng.tensor(x), 25))
    d = ((q[:, None, :] - x[None]) ** 2).sum(-1)
    want = np.argsort(d, 1)[:, :25]
    for a, b, dq in zip(got, want, d):
        assert np.allclose(np.sort(dq[a]), np.sort(dq[b]), rtol=1e-12, atol=0)
    same = np.ones((5000, 2))
    assert np.array_equal(npy(eng.nn_query(eng.tensor(same[:3]), eng.tensor(same), 7)), np.tile(np.arange(7), (3, 1)))


def test_vecchia_spsolve_batch_equals_single(eng):
    """dgpamd_vecchia_spsolve_batch (one workgroup per chain) against the single-chain solve, bit for bit, and against
    the oracle's forward_solve_sp: 3 matrices x 4 right-hand sides, n larger than one 1024-row window."""
    from oracle import dgp_oracle as O
    import torch
    rng = np.random.default_rng(17)
    n, m, nmat, nrhs = 2500, 9, 3, 4
    Ls, NNs, scs = [], [], [0.7, 1.0, 1.9]
    for j in range(nmat):
        X = rng.uniform(size=(n, 2))
        length = np.array([0.3 + 0.1 * j, 0.5])
        NN = eng.nn_ordered(eng.tensor(X / length), m)
        Ls.append(eng.vecchia_lmatrix('matern2.5' if j else 'sexp', eng.tensor(X), NN, length, 1e-3))
        NNs.append(NN)
    b = eng.tensor(rng.normal(size=(nmat, nrhs, n)))
    xb = npy(eng.vecchia_spsolve_batch(torch.stack(Ls), torch.stack(NNs), scs, b))
    for j in range(nmat):
        for r in range(nrhs):
            x1 = npy(eng.vecchia_spsolve(Ls[j], NNs[j], scs[j], b[j, r].contiguous()))
            assert np.array_equal(xb[j, r], x1)
        ref = O.forward_solve_sp(npy(Ls[j]) * scs[j], npy(NNs[j]), npy(b[j, 0]))
        close(xb[j, 0], ref, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('n,m,nrhs', [(2500, 9, 4), (700, 25, 13), (40, 40, 1), (5000, 33, 2)])
def test_vecchia_spsolve_level_schedule(eng, n, m, nrhs):
    """The level-scheduled sparse forward substitution (dgpamd_vecchia_levels + dgpamd_vecchia_spsolve_levels: rows whose
    dependencies are solved run side by side) against the row-by-row kernel and the oracle's forward_solve_sp
    (vecchia.py:112-120): same solution to rounding (a row's sum is a 32-lane butterfly instead of left to right); the
    schedule is a permutation of the rows in which every row comes after all rows it depends on, level by level; more
    right-hand sides than one workgroup takes (13 > 12), conditioning sets wider than the 32 lanes of a row (m = 33, 40)."""
    from oracle import dgp_oracle as O
    import torch
    rng = np.random.default_rng(n + m)
    nmat = 2
    Ls, NNs, scs = [], [], [0.8, 1.7]
    for j in range(nmat):
        X = rng.uniform(size=(n, 3))
        length = np.array([0.4 + 0.2 * j, 0.6, 0.9])
        NN = eng.nn_ordered(eng.tensor(X / length), m)
        Ls.append(eng.vecchia_lmatrix('matern2.5' if j else 'sexp', eng.tensor(X), NN, length, 1e-3))
        NNs.append(NN)
    Lm, NNa = torch.stack(Ls), torch.stack(NNs)
    b = eng.tensor(rng.normal(size=(nmat, nrhs, n)))
    sched = eng.vecchia_levels(NNa)
    xl = npy(eng.vecchia_spsolve_levels(Lm, NNa, scs, b, sched))
    xb = npy(eng.vecchia_spsolve_batch(Lm, NNa, scs, b))
    close(xl, xb, rtol=1e-10, atol=1e-12)
    close(xl[1, 0], O.forward_solve_sp(npy(Ls[1]) * scs[1], npy(NNs[1]), npy(b[1, 0])), rtol=1e-10, atol=1e-12)
    # the schedule itself
    w = 4 * n + 3
    sc = npy(sched).reshape(nmat, w)
    for j in range(nmat):
        lev, order, ptr, nlev = sc[j, :n], sc[j, n:2 * n], sc[j, 2 * n:3 * n + 1], sc[j, 4 * n + 2]
        NNh = npy(NNs[j])
        assert sorted(order.tolist()) == list(range(n))
        assert ptr[0] == 0 and ptr[nlev] == n and np.all(np.diff(ptr[:nlev + 1]) > 0)
        dep = np.where(NNh[:, 1:] >= 0, lev[np.maximum(NNh[:, 1:], 0)], -1).max(1) if NNh.shape[1] > 1 else np.full(n, -1)
        assert np.array_equal(lev, dep + 1)                      # level = 1 + highest level among the dependencies
        assert np.array_equal(np.sort(lev[order]), lev[order])   # rows in level order


def test_linkgp_sexp_mfma_equals_direct_across_chunks(eng):
    """SExp link_gp: the MFMA pair kernel (dot-product form of the exponent) against the direct evaluation, M = 2100
    test points (two workspace chunks), incl. zero input variances; a slice against the oracle."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(5)
    n, M, Dw, Dz = 70, 2100, 3, 1
    X = rng.uniform(size=(n, Dw + Dz))
    y = rng.normal(size=n)
    length = rng.uniform(0.3, 1.2, size=Dw + Dz)
    st = O.compute_stats(X, y, length, 1e-3, 'sexp', Dw)
    mm = rng.uniform(-0.3, 1.3, size=(M, Dw))
    vv = 10.0 ** rng.uniform(-5, 0, size=(M, Dw))
    vv[::17] = 0.0
    z = rng.uniform(size=(M, Dz))
    args = (eng.tensor(mm), eng.tensor(vv), eng.tensor(z), eng.tensor(X[:, :Dw]), eng.tensor(X[:, Dw:]), length,
            eng.tensor(st['Rinv']), n, eng.tensor(st['Rinv_y']), 1.7, 1e-3)
    eng.set_linkgp_direct(True)
    m1, v1 = eng.linkgp_predict('sexp', *args)
    m1, v1 = npy(m1), npy(v1)
    eng.set_linkgp_direct(False)
    m2, v2 = eng.linkgp_predict('sexp', *args)
    close(npy(m2), m1, rtol=1e-12, atol=1e-14)
    close(npy(v2), v1, rtol=1e-6, atol=1e-9)     # (variance = difference of O(1e3) terms through R^-1)
    sl = slice(2040, 2060)
    lmr, lvr = O.link_gp_predict(mm[sl], vv[sl], z[sl], X[:, :Dw], X[:, Dw:], st['Rinv'], st['Rinv_y'], 1.7, length, 1e-3, 'sexp')
    close(npy(m2)[sl], lmr, rtol=1e-8, atol=1e-10)
    close(npy(v2)[sl], lvr, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('kind,n,M,Dw,Dz', [('matern2.5', 130, 4500, 3, 1), ('matern2.5', 700, 1100, 5, 0), ('sexp', 130, 4500, 3, 1)])
def test_linkgp_launch_geometry_does_not_change_a_bit(eng, kind, n, M, Dw, Dz):
    """Round 5: the record-based pair kernels take as many test points per launch as make >= 32 rounds of workgroups (csrc/linkgp_plan.hpp
    pair_chunk; 256 before), the Matern kernel's records of a step are requested between its column tiles instead of behind the
    step's barrier, with scalar addresses.  None of that touches a pair's arithmetic: the earlier geometry (DGPAMD_PAIR_CHUNK=256,
    DGPAMD_JSEP_PIPE=0), other points per workgroup (DGPAMD_JSEP_TCH, DGPAMD_JSEXP_TCH) and a chunk that is no multiple of the workgroup's points
    give the same bits -- M spans several launches, the last one ragged -- and a slice equals the oracle (functions.py:453-494)."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(41)
    X = rng.uniform(size=(n, Dw + Dz))
    y = rng.normal(size=n)
    length = rng.uniform(0.4, 1.2, size=Dw + Dz)
    st = O.compute_stats(X, y, length, 1e-3, kind, Dw)
    mm = rng.uniform(-0.2, 1.2, size=(M, Dw))
    vv = 10.0 ** rng.uniform(-5, 0, size=(M, Dw))
    vv[::19] = 0.0
    z = rng.uniform(size=(M, Dz)) if Dz else None
    args = (eng.tensor(mm), eng.tensor(vv), eng.tensor(z) if Dz else None, eng.tensor(X[:, :Dw]), eng.tensor(X[:, Dw:]) if Dz else None, length,
            eng.tensor(st['Rinv']), n, eng.tensor(st['Rinv_y']), 1.4, 1e-3)
    unset = dict(PAIR_CHUNK=None, JSEP_PIPE=None, JSEP_TCH=None, JSEXP_TCH=None)
    with engine_under(**unset) as e:
        assert [e.tuning(k) for k in ('PAIR_CHUNK', 'JSEP_PIPE', 'JSEP_TCH', 'JSEXP_TCH')] == [0, 2, 0, 0]   # (0: the built-in geometry)
        m0, v0 = (npy(t) for t in e.linkgp_predict(kind, *args))
    for env in ({'PAIR_CHUNK': '256', 'JSEP_PIPE': '0'}, {'JSEP_TCH': '16'}, {'JSEP_TCH': '64', 'PAIR_CHUNK': '416'},
                {'PAIR_CHUNK': '96', 'JSEP_PIPE': '0', 'JSEP_TCH': '8'}, {'JSEXP_TCH': '256'}, {'JSEXP_TCH': '64', 'PAIR_CHUNK': '160'}):
        with engine_under(**dict(unset, **env)) as e:
            m1, v1 = (npy(t) for t in e.linkgp_predict(kind, *args))
        np.testing.assert_array_equal(m1, m0, err_msg=str(env))
        np.testing.assert_array_equal(v1, v0, err_msg=str(env))
    sl = slice(M - 12, M)
    with integral_oracle():
        lmr, lvr = O.link_gp_predict(mm[sl], vv[sl], None if z is None else z[sl], X[:, :Dw], X[:, Dw:] if Dz else None, st['Rinv'], st['Rinv_y'], 1.4, length, 1e-3, kind)
    close(m0[sl], lmr, rtol=1e-8, atol=1e-10)
    close(v0[sl], lvr, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('name,n,Dz', [('sexp', 70, 1), ('matern2.5', 131, 2), ('matern2.5', 64, 0)])
def test_linkgp_loo_equals_oracle_refit(eng, name, n, Dz):
    """dgpamd_linkgp_loo: test point t conditioned on all training points but drop[t] (arbitrary indices, as the
    nearest latent of a deeper layer need not be the point itself) against the oracle's link_gp with the statistics
    refitted on the n-1 remaining points."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(12)
    M, Dw = 40, 2
    X = rng.uniform(size=(n, Dw + Dz))
    y = rng.normal(size=n)
    length = rng.uniform(0.4, 1.2, size=Dw + Dz)
    nug = 1e-2
    st = O.compute_stats(X, y, length, nug, name, Dw)
    mm = rng.uniform(-0.2, 1.2, size=(M, Dw))
    vv = 10.0 ** rng.uniform(-5, -1, size=(M, Dw))
    vv[3] = 0.0
    z = rng.uniform(size=(M, Dz)) if Dz else None
    drop = rng.integers(0, n, size=M).astype(np.int32)
    drop[0], drop[1] = 0, n - 1
    m1, v1 = eng.linkgp_predict(name, eng.tensor(mm), eng.tensor(vv), eng.tensor(z) if Dz else None, eng.tensor(X[:, :Dw]),
                                eng.tensor(X[:, Dw:]) if Dz else None, length, eng.tensor(st['Rinv']), n,
                                eng.tensor(st['Rinv_y']), 1.3, nug, drop=eng.tensor(drop, dtype=__import__("torch").int32))
    m1, v1 = npy(m1), npy(v1)
    for t in range(M):
        keep = np.delete(np.arange(n), drop[t])
        s2 = O.compute_stats(X[keep], y[keep], length, nug, name, Dw)
        mr, vr = O.link_gp_predict(mm[t:t + 1], vv[t:t + 1], z[t:t + 1] if Dz else None, X[keep, :Dw],
                                   X[keep, Dw:] if Dz else None, s2['Rinv'], s2['Rinv_y'], 1.3, length, nug, name)
        close(m1[t], mr[0], rtol=1e-8, atol=1e-10)
        close(v1[t], vr[0], rtol=1e-6, atol=1e-9)


@pytest.mark.gpu
def test_loglik_finish_matches_loglik(eng):
    """dgpamd_loglik_finish on buffers factored as members of another batched call == dgpamd_loglik of the same matrices
    (bit for bit: the imputer folds the first slice threshold of an I-step into the prior factorisation this way)."""
    import torch
    rng = np.random.default_rng(11)
    n, B = 333, 3
    Np = eng.padded_dim(n)
    X = eng.tensor(rng.uniform(size=(B, n, 4)))
    G = eng.tensor(rng.uniform(size=(n, 2)))
    y = eng.tensor(rng.normal(size=n))
    ll_ref, info = eng.loglik('matern2.5', X, None, G, [0.8], 1e-5, 1.7, y, batch=B)
    A = eng.empty(B + 2, Np, Np)
    for b in range(B):
        eng.kmatrix('matern2.5', X[b], None, G, [0.8], 1e-5, out=A[b + 2], full=False, Y=y)
    for b in range(2):   # two unrelated matrices ahead of them in the same call (no y row)
        eng.kmatrix('sexp', X[b], None, G, [0.5], 1e-4, out=A[b], full=False)
    logdet, info2 = eng.potrf(n, A, batch=B + 2)
    ll = torch.cat([eng.loglik_finish(n, A[b + 2], logdet[b + 2:b + 3], 1.7) for b in range(B)])
    eng.sync()
    assert not npy(info).any() and not npy(info2).any()
    assert np.array_equal(npy(ll), npy(ll_ref))


@pytest.mark.gpu
def test_one_launch_factorisation_random_shapes_repeatable(eng):
    """Random sizes / batch sizes / with and without the inverse through the one-launch kernel, several launches each on the
    same buffers: info == 0 and a bitwise identical log-determinant every time (a stale tile read or a lost hand-off between
    the kernel's workgroups would show here); the short version of tools/gpu_mega_stress.py."""
    rng = np.random.default_rng(5)
    for _ in range(40):
        n = int(rng.choice([64, 65, 130, 333, 640, 1000, 1280]))
        B = int(rng.choice([1, 2, 3, 5, 6, 8, 12, 16]))
        inv = bool(rng.integers(2))
        Np = eng.padded_dim(n)
        X = eng.tensor(rng.uniform(size=(B, n, 3)))
        y = eng.tensor(rng.normal(size=n))
        A, T, S = eng.empty(B, Np, Np), eng.empty(B, Np, Np), eng.empty(B, Np, Np)
        work = eng.potrf_workspace(n, B)
        ref = None
        for rep in range(4):
            eng.kmatrix('matern2.5', X, None, None, [0.6], 1e-5, out=A, full=False, Y=y, batch=B)
            ld, info = eng.potrf_inv(n, A, T, S, batch=B, work=work) if inv else eng.potrf(n, A, batch=B, work=work)
            ldh, ih = eng.fetch(ld), eng.fetch(info)
            assert not ih.any(), (n, B, inv, ih)
            if ref is None:
                ref = ldh.copy()
            assert np.array_equal(ldh, ref), (n, B, inv, rep)


def test_one_workspace_shared_by_batch_sizes_and_modes(eng):
    """The scenario of the hazard round 2 parked (per-step graphs of two batch sizes replayed on one workspace
    after a one-launch call gave a wrong `info` once): ONE workspace shared by factorisations of different batch sizes --
    whose layouts alias: the info / log-determinant words of a 4-matrix call lie where a 12-matrix call keeps diagonal-
    block inverses -- under both modes (per-step graphs, one launch; round 2's third mode, chosen per call, is gone), queued back to back with NO
    synchronisation; afterwards every call must report info = 0 and, per batch size, bit-identical log-determinants.
    (Not reproduced in round 3 in 30 runs of the original sequence, tools/gpu_iter_split.py, nor by this stress;
    the words are now written and read with device-scope accesses, so that no stale per-XCD L2 line of an earlier layout
    can serve them.)"""
    import torch
    n, Bmax = 700, 12
    Np = eng.padded_dim(n)
    rng = np.random.default_rng(0)
    X = eng.tensor(rng.uniform(size=(Bmax, n, 4)))
    y = eng.tensor(rng.normal(size=n))
    A = eng.empty(Bmax, Np, Np)
    work = eng.potrf_workspace(n, Bmax)
    seq = [(1, 12), (0, 4), (0, 12), (1, 3), (0, 6), (1, 12), (1, 4), (0, 4), (1, 12), (0, 12), (1, 9), (0, 3)]
    ref = {}
    try:
        for r in range(12):
            outs = []
            for mode, B in seq:
                eng.set_potrf_mode(mode)
                eng.kmatrix('matern2.5', X[:B], None, None, [1.0], 1e-4, out=A[:B], full=False, Y=y, batch=B)
                outs.append((mode, B) + tuple(eng.potrf(n, A[:B], batch=B, work=work)))
            torch.cuda.synchronize()
            for mode, B, ld, info in outs:
                assert not npy(info).any(), (r, mode, B, npy(info))
                assert np.array_equal(npy(ld), ref.setdefault(B, npy(ld))), (r, mode, B)
    finally:
        eng.set_potrf_mode(1)


@pytest.mark.parametrize('kind', ['Poisson', 'NegBin', 'ZIP', 'ZINB', 'logit', 'probit', 'softmax', 'robustmax'])
@pytest.mark.parametrize('replicates', [False, True])
def test_lik_loglik_vs_host_protocol(eng, kind, replicates):
    """dgpamd_lik_loglik == the host plugin protocol's llik() (the reference's likelihood_class.py llik methods as restated in
    dgp_amd/likelihood_class.py and pinned by g17 / g18) for every candidate block, with and without a replicate map, on
    ordinary latents and on the wild ones a slice-sampling proposal can reach (|f| up to 30: the probit tail series, exp
    overflow guards of logaddexp); candidate blocks the sampler must reject (NaN) come back as NaN."""
    import torch
    from dgp_amd import Poisson, NegBin, ZIP, ZINB, Categorical
    rng = np.random.default_rng(31)
    n, M, B = 700, 5, 4
    FP = rng.normal(size=(B, n, M))
    FP[1] *= 6.0
    FP[2, :50] = rng.uniform(-30, 30, size=(50, M))
    nobs = 950 if replicates else n
    rep = np.concatenate((np.arange(n), rng.integers(0, n, nobs - n))) if replicates else None
    if kind in ('Poisson', 'NegBin', 'ZIP', 'ZINB'):
        y = rng.poisson(3.0, size=nobs).astype(float)
        y[rng.uniform(size=nobs) < 0.2] = 0.0
        node = {'Poisson': Poisson, 'NegBin': NegBin, 'ZIP': ZIP, 'ZINB': ZINB}[kind]()
        cols = {'Poisson': [3], 'NegBin': [0, 2], 'ZIP': [4, 1], 'ZINB': [1, 2, 3]}[kind]
        K = 0
    elif kind in ('logit', 'probit'):
        y = rng.integers(0, 2, nobs).astype(float)
        node, cols, K = Categorical(num_classes=2, link=kind), [2], 2
    else:
        y = rng.integers(0, 4, nobs).astype(float)
        node, cols, K = Categorical(num_classes=4, link=kind), [4, 0, 1, 3], 4
    lik = dict(kind=kind, y=eng.tensor(y), rep=None if rep is None else torch.as_tensor(rep, device='cuda'), classes=K, par=1e-3)
    got = eng.lik_loglik(lik, np.asarray(cols, dtype=np.int32), eng.tensor(FP)).cpu().numpy()
    node.output = y[:, None]
    want = np.empty(B)
    for b in range(B):
        node.input = (FP[b][rep] if replicates else FP[b])[:, cols]
        want[b] = float(np.sum(node.llik()))
    assert np.all(np.isfinite(want))
    atol = np.full(B, 1e-9)
    if kind in ('NegBin', 'ZINB'):
        # eps x the size of the terms that are actually added: y log(size), lgamma(y + 1), y a and (y + size) logaddexp(0, a) --
        # not gammaln(size), of order size log(size) (0.25 per observation at size = e^30), which neither side computes
        # where it would cancel (tests/test_gpu_lik.py holds each side to exact values)
        from scipy.special import gammaln
        for b in range(B):
            f = (FP[b][rep] if replicates else FP[b])[:, cols]
            size, a = np.exp(-f[:, 1]), f[:, 0] + f[:, 1]
            atol[b] += 8e-16 * np.sum(y * np.abs(f[:, 1]) + gammaln(y + 1.0) + y * np.abs(a) + (y + size) * np.logaddexp(0.0, a))
    assert np.all(np.abs(got - want) <= 2e-13 * np.abs(want) + atol), (got, want, atol)
    bad = FP.copy()
    bad[0, 7, cols[0]] = np.nan
    got = eng.lik_loglik(lik, np.asarray(cols, dtype=np.int32), eng.tensor(bad)).cpu().numpy()
    assert np.isnan(got[0]) or (kind == 'robustmax') and np.all(np.isfinite(got[1:]))


@pytest.mark.parametrize('n,M,Dw,Dz', [(400, 70, 3, 2), (650, 40, 5, 0), (130, 33, 1, 1), (1000, 20, 2, 0)])
def test_linkgp_order_classes_equal_any_order(eng, n, M, Dw, Dz):
    """The Matern pair kernel's order classes (one record product where a wave's rows all lie on one side of the tile's
    columns in a dimension): the training points grouped by cells (Engine.linkgp_cells -> ops.cell_order) give the
    predictions of the caller's order -- the same sums over all pairs, functions.py:453-494 -- to rounding, the class-free run
    (DGPAMD_JSEP_NOCLASS) and the direct formula included; inputs with zero variances, ties between coordinates (the
    class bounds are <= / >), sizes off the tile edge; the leave-one-out call takes `pos` as its drop list."""
    import torch
    from oracle import dgp_oracle as O
    from dgp_amd.ops import cell_order
    rng = np.random.default_rng(77)
    X = rng.uniform(size=(n, Dw + Dz))
    X[: n // 3, 0] = np.round(X[: n // 3, 0], 1)   # ties
    y = rng.normal(size=n)
    length = rng.uniform(0.4, 1.3, size=Dw + Dz)
    nug = 1e-2
    st = O.compute_stats(X, y, length, nug, 'matern2.5', Dw)
    mm = rng.uniform(-0.2, 1.2, size=(M, Dw))
    vv = 10.0 ** rng.uniform(-5, 0, size=(M, Dw))
    vv[0] = 0.0
    z = rng.uniform(size=(M, Dz)) if Dz else None
    Rinv, ry = eng.tensor(st['Rinv']), eng.tensor(st['Rinv_y'])
    W, Wg = X[:, :Dw], (eng.tensor(X[:, Dw:]) if Dz else None)
    dm, dv, dz = eng.tensor(mm), eng.tensor(vv), (eng.tensor(z) if Dz else None)
    m0, v0 = (npy(t) for t in eng.linkgp_predict('matern2.5', dm, dv, dz, eng.tensor(W), Wg, length, Rinv, n, ry, 1.3, nug))
    cells = eng.linkgp_cells('matern2.5', W, Wg, Rinv, ry)
    p = cell_order(W)
    assert sorted(p.tolist()) == list(range(n)) and np.array_equal(npy(cells['W']), W[p])
    assert np.array_equal(npy(cells['pos'])[p], np.arange(n))
    m1, v1 = (npy(t) for t in eng.linkgp_predict('matern2.5', dm, dv, dz, cells['W'], cells['Wg'], length, cells['Rinv'], n,
                                                 cells['ry'], 1.3, nug))
    close(m1, m0, rtol=1e-9, atol=1e-11)   # (sums of terms up to 1e3 times their total, taken in another order)
    close(v1, v0, rtol=1e-6, atol=1e-8)
    with engine_under(JSEP_NOCLASS=1) as e:
        m2, v2 = (npy(t) for t in e.linkgp_predict('matern2.5', dm, dv, dz, cells['W'], cells['Wg'], length, cells['Rinv'], n,
                                                   cells['ry'], 1.3, nug))
    close(m2, m1, rtol=1e-13, atol=1e-14)   # (the mean does not pass through the pair kernel)
    close(v2, v1, rtol=1e-6, atol=1e-8)
    with integral_oracle():
        lmr, lvr = O.link_gp_predict(mm, vv, z, W, X[:, Dw:] if Dz else None, st['Rinv'], st['Rinv_y'], 1.3, length, nug, 'matern2.5')
    close(m1, lmr, rtol=1e-8, atol=1e-10)
    close(v1, lvr, rtol=1e-5, atol=1e-7)   # (random outputs, test points outside the data: variances of 10 x scale from sums 1e4 times larger)
    # leave-one-out: test row t drops training point t % n, in either order
    Ml = min(M, n)
    d0 = torch.arange(Ml, device='cuda', dtype=torch.int32)
    a0 = eng.linkgp_predict('matern2.5', dm[:Ml], dv[:Ml], None if dz is None else dz[:Ml], eng.tensor(W), Wg, length, Rinv, n, ry, 1.3, nug, drop=d0)
    a1 = eng.linkgp_predict('matern2.5', dm[:Ml], dv[:Ml], None if dz is None else dz[:Ml], cells['W'], cells['Wg'], length, cells['Rinv'], n,
                            cells['ry'], 1.3, nug, drop=cells['pos'][:Ml].contiguous())
    close(npy(a1[0]), npy(a0[0]), rtol=1e-8, atol=1e-10)
    close(npy(a1[1]), npy(a0[1]), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
@pytest.mark.parametrize('D,pm', [(3, 10), (8, 50), (12, 51), (8, 25)])
def test_vecchia_gp_register_kernel_equals_lds_kernel(eng, name, D, pm):
    """gp_vecch (vecchia.py:635-654) through the register-resident kernel (one row of the conditioning block per lane,
    readlane broadcasts, no LDS) and through the one-wave-per-point LDS kernel it replaces (DGPAMD_VECCHIA_LDS=1): the same
    means and variances; conditioning sets shorter than pm (trailing -1 entries), a test-point count off the four-per-
    workgroup grid, replicate weights on the nugget, anisotropic lengthscales; a few points against the oracle."""
    import torch
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(5 + D)
    n, M = 1500, 1001
    X = rng.uniform(size=(n, D))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=n)
    xq = rng.uniform(size=(M, D))
    length = rng.uniform(0.5, 1.5, size=D)
    nd = rng.uniform(0.5, 2.0, size=n)
    dX, dq = eng.tensor(X), eng.tensor(xq)
    NN = eng.nn_query(eng.tensor(xq / length), eng.tensor(X / length), pm).clone()
    short = rng.integers(0, M, 40)
    for i, t in enumerate(short):   # shorter sets: the valid entries come first
        NN[t, max(1, pm - 1 - i % pm):] = -1
    args = (name, dq, dX, NN, eng.tensor(y), 1.7, length, 1e-3, eng.tensor(nd))
    m1, v1 = (npy(t) for t in eng.vecchia_gp(*args))
    with engine_under(VECCHIA_LDS=1, POISON_LDS=1) as e:   # (every CU's LDS filled with NaNs before the LDS kernel's launch)
        m0, v0 = (npy(t) for t in e.vecchia_gp(*args))
    assert np.all(np.isfinite(m1)) and np.all(v1 > 0)
    close(m1, m0, rtol=1e-9, atol=1e-11)
    close(v1, v0, rtol=1e-8, atol=1e-11)
    NNh = npy(NN).astype(int)
    pick = np.array(list(short[:4]) + [0, 1, M - 1])
    mo, vo = O.gp_vecch(xq[pick], X, NNh[pick], y, 1.7, length, 1e-3, nd, name)
    close(m1[pick], mo, rtol=1e-8, atol=1e-10)
    close(v1[pick], vo, rtol=1e-7, atol=1e-10)


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
@pytest.mark.parametrize('Dw,Dz,pm', [(8, 8, 50), (3, 0, 20), (5, 2, 50), (8, 0, 37)])
def test_vecchia_linkgp_register_kernel_equals_lds_kernel(eng, Dw, Dz, pm, kind):
    """link_gp_vecch (vecchia.py:758-796, IJ_nb :838-907; both kernels) through the register-resident kernels
    (in-place Gauss-Jordan on one row per lane: K | N, J, y and I take the same row operations; the Matern J factors from
    per-lane separable records broadcast with v_readlane; no LDS) and through the LDS kernel they replace: the same means and
    variances, with and without deterministic global inputs, conditioning sets shorter than pm, zero input variances, ties
    between coordinates, a test-point count off the four-per-workgroup grid; a few points against the oracle."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(11 + Dw + Dz)
    n, M = 1200, 403
    W = rng.normal(size=(n, Dw))
    W[:300, 0] = np.round(W[:300, 0], 1)          # ties between coordinates (the Matern records' orientation select)
    Wg = rng.uniform(size=(n, Dz)) if Dz else None
    y = np.sin(W.sum(1)) + 0.1 * rng.normal(size=n)
    mm = rng.normal(size=(M, Dw))
    vv = 10.0 ** rng.uniform(-4, -0.5, size=(M, Dw))
    vv[0] = 0.0
    vv[1, Dw - 1] = 0.0
    z = rng.uniform(size=(M, Dz)) if Dz else None
    length = rng.uniform(0.8, 2.0, size=Dw + Dz)
    nd = rng.uniform(0.5, 2.0, size=n)
    Xall = W if not Dz else np.concatenate((W, Wg), 1)
    xq = mm if not Dz else np.concatenate((mm, z), 1)
    NN = eng.nn_query(eng.tensor(xq / length), eng.tensor(Xall / length), pm).clone()
    short = rng.integers(0, M, 30)
    for i, t in enumerate(short):
        NN[t, max(2, pm - 1 - i % pm):] = -1
    args = (kind, eng.tensor(mm), eng.tensor(vv), eng.tensor(z) if Dz else None, eng.tensor(W), eng.tensor(Wg) if Dz else None, NN,
            eng.tensor(y), 1.4, length, 1e-3, eng.tensor(nd))
    m1, v1 = (npy(t) for t in eng.vecchia_linkgp(*args))
    with engine_under(VECCHIA_LDS=1, POISON_LDS=1) as e:   # (every CU's LDS filled with NaNs before the LDS kernel's launch)
        m0, v0 = (npy(t) for t in e.vecchia_linkgp(*args))
    assert np.all(np.isfinite(m1)) and np.all(np.isfinite(v1))
    close(m1, m0, rtol=1e-9, atol=1e-11)
    close(v1, v0, rtol=1e-7, atol=1e-10)
    NNh = npy(NN).astype(int)
    pick = np.array(list(short[:3]) + [0, 1, M - 1])
    mo, vo = O.link_gp_vecch(mm[pick], vv[pick], None if z is None else z[pick], W, Wg, NNh[pick], y, 1.4, length, 1e-3, nd, kind)
    close(m1[pick], mo, rtol=1e-8, atol=1e-10)
    close(v1[pick], vo, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize('Dw,Dz,pm', [(3, 2, 40), (8, 0, 50), (1, 1, 12), (3, 2, 60), (9, 0, 30)])   # (the last two: beyond the register kernel, LDS)
def test_vecchia_linkgp_matern_separable_records_vs_oracle(eng, Dw, Dz, pm):
    """link_gp_vecch with the Matern-2.5 kernel (vecchia.py:758-796, IJ_nb :838-907 -> Jd / Jd0 :915-988): the kernel
    evaluates every neighbour's separable record once per dimension and a pair as 30 multiply-adds and a select
    (csrc/linkfun.hpp) instead of the reference's closed form per pair -- against the oracle's per-pair Jd, with zero input
    variances (the product of two point correlations), short conditioning sets and ties between coordinates."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(17 + Dw)
    n, M = 700, 45
    W = rng.normal(size=(n, Dw))
    W[:200, 0] = np.round(W[:200, 0], 1)
    Wg = rng.uniform(size=(n, Dz)) if Dz else None
    y = np.sin(W.sum(1)) + 0.1 * rng.normal(size=n)
    mm = rng.normal(size=(M, Dw))
    vv = 10.0 ** rng.uniform(-4, -0.3, size=(M, Dw))
    vv[0] = 0.0
    vv[1, Dw - 1] = 0.0
    z = rng.uniform(size=(M, Dz)) if Dz else None
    length = rng.uniform(0.8, 2.0, size=Dw + Dz)
    nd = rng.uniform(0.5, 2.0, size=n)
    Xall = W if not Dz else np.concatenate((W, Wg), 1)
    xq = mm if not Dz else np.concatenate((mm, z), 1)
    NN = eng.nn_query(eng.tensor(xq / length), eng.tensor(Xall / length), pm).clone()
    NN[3, 5:] = -1
    NN[4, 1:] = -1
    lm, lv = (npy(t) for t in eng.vecchia_linkgp('matern2.5', eng.tensor(mm), eng.tensor(vv), eng.tensor(z) if Dz else None, eng.tensor(W),
                                                 eng.tensor(Wg) if Dz else None, NN, eng.tensor(y), 1.4, length, 1e-3, eng.tensor(nd)))
    mo, vo = O.link_gp_vecch(mm, vv, z, W, Wg, npy(NN).astype(int), y, 1.4, length, 1e-3, nd, 'matern2.5')
    close(lm, mo, rtol=1e-8, atol=1e-10)
    close(lv, vo, rtol=1e-6, atol=1e-9)


def test_mailboxes_deliver_results_without_draining_the_stream(eng):
    """dgpamd_post / dgpamd_collect (include/dgp_amd.h): a result posted to a mailbox arrives as fetch() would deliver it --
    small ones through the one-block publishing kernel, large ones through the copy path -- while work queued afterwards is
    still running; a mailbox holds one result at a time; discard() frees it."""
    import torch
    from dgp_amd.ops import DgpAmdError
    rng = np.random.default_rng(5)
    small = rng.normal(size=37)
    ints = rng.integers(-5, 5, size=(3, 7)).astype(np.int32)
    large = rng.normal(size=(3000, 9))                     # 216 KB: above the kernel path's limit
    ds, di, dl = eng.tensor(small), torch.as_tensor(ints, device=eng.device), eng.tensor(large)
    with eng.stream():
        t0 = eng.post(ds, 0)
        t1 = eng.post(di, 1)
        t2 = eng.post(dl * 2.0, 2)
        big = torch.empty(4096, 4096, dtype=torch.float64, device=eng.device)
        for _ in range(4):                                 # (work behind the posts: they must not wait for it)
            big.normal_()
        with pytest.raises(DgpAmdError):
            eng.post(ds, 0)                                # the mailbox is occupied
        assert np.array_equal(eng.collect(t2), large * 2.0)
        assert np.array_equal(eng.collect(t0), small)
        assert np.array_equal(eng.collect(t1), ints)
        with pytest.raises(DgpAmdError):
            eng.collect(t0)                                # nothing posted any more
        for rep in range(50):                              # reuse: sequence words never repeat
            tok = eng.post(ds + rep, rep % eng.MAILBOXES)
            assert np.array_equal(eng.collect(tok), small + rep)
        tok = eng.post(ds, 3)
        eng.discard(tok)
        tok = eng.post(dl, 3)
        assert np.array_equal(eng.collect(tok), large)
    with pytest.raises(DgpAmdError):
        eng.post(ds, eng.MAILBOXES)
    assert np.array_equal(eng.fetch(ds), small) and np.array_equal(eng.fetch(dl), large)   # (fetch: the same two paths)


def test_one_launch_factorisation_when_processes_share_the_gpu(eng):
    """The one-launch factorisation with other processes' waves on its CUs (two ranks on one GPU; a busy neighbour): every result
    must equal the first run of the same inputs, bit for bit.  Round 4's chain stored the panel tile with 16-byte stores whose four
    data registers the compiler rewrote right behind each store (no wait state: the store's offset sits in an SGPR); with the memory
    pipeline under load from the other processes the store had not read all of its data yet, and a few factors per thousand launches
    came out wrong in the first double of the lanes read last -- never with the device to itself.  Three processes, small matrices
    (the chain dominates), 2500 launches each."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SIZES='100,150,190,200,260,333', LAUNCHES='2500')
    procs = [subprocess.Popen([sys.executable, os.path.join(root, 'tools', 'gpu_mega_stress.py')], env=dict(env, SEED=str(11 + p)),
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for p in range(3)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0 and 'all results consistent' in o, o[-1500:]
