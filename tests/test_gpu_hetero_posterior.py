"""The exact conditional-posterior draw of a Hetero likelihood's mean latent on the device, dense (Engine.post_het) and Vecchia
(Engine.vecchia_post_het: dgpamd_vecchia_het_rows + two sparse solves), its building blocks gemv and trmv_lower, the imputer's
glue around both and the error reports -- against tests/het_ref.py, the same operations in numpy.longdouble.  Needs an MI355X:
-m gpu.

Tolerances.  Rows, draws and dense draws: per case E_ref is the error of the float64 oracle against het_ref in the same norm,
computed here; the device must stay within max(32 E_ref, 64 * 2^-53) (het_ref.accept; tests/test_het_ref_host.py shows that a
subtly wrong block does not).  The sparse solve and the gemv / trmv_lower sums are held to derived componentwise bounds that do
not depend on conditioning.  Every test prints its figures before it asserts; profiles/hetero_posterior_parity.txt records them.

Shapes: blocks of 2 to 101 entries (one trip and two trips of the 64 lanes, LDS above the default from m = 100), m >= n,
D = 1 .. 12, n across the solver's 1024-row window; dense n on both sides of the 64-wide tile and at its multiples, where the
last block row of the factorisation holds the right-hand side alone."""
import numpy as np
import pytest

import het_ref as H
from test_gpu_ops import engine_under

pytestmark = pytest.mark.gpu

VCASES = [(n, D, m, name) for (n, D, m) in H.VECCHIA_CASES for name in H.NAMES]
U = H.U


def vid(c):
    return '-'.join(str(v) for v in c)


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


@pytest.fixture(scope='module', params=['plain', 'poisoned_lds'])
def veng(request, eng):
    """The engine of the Vecchia tests: the module's own, and one created under POISON_LDS=1 (NaNs in every CU's LDS before the
    row launch: nothing the kernel has not written may reach a result)."""
    if request.param == 'plain':
        yield eng
    else:
        with engine_under(POISON_LDS=1) as e:
            yield e


def npy(t):
    return t.detach().cpu().numpy()


def het_rows(e, c, gamma=None):
    """dgpamd_vecchia_het_rows as Engine.vecchia_post_het calls it: (Lrows, NNl, t, info) as numpy arrays."""
    import torch
    from dgp_amd.ops import lib, KIND, _dp, _hp, _f64
    n, mp1 = c.impNN.shape
    length = _f64(c.length)
    X, NN = e.tensor(c.X), e.tensor(c.impNN, dtype=torch.int64)
    g, y = e.tensor(c.gamma if gamma is None else gamma), e.tensor(c.y)
    Lrows, t = e.empty(n, mp1), e.empty(n)
    NNl = e.empty(n, mp1, dtype=torch.int64)
    info = e.empty(1, dtype=torch.int32)
    e._chk(e._enter() or lib.dgpamd_vecchia_het_rows(e.h, KIND[c.name], n, c.D, mp1 - 1, _dp(X), _dp(NN), _hp(length), len(length),
                                                     float(c.scale), _dp(g), _dp(y), _dp(Lrows), _dp(NNl), _dp(t), _dp(info)))
    return npy(Lrows), npy(NNl), npy(t), int(npy(info)[0])


def device_draw(e, c, z=None, gamma=None):
    import torch
    f = e.vecchia_post_het(c.name, e.tensor(c.X), e.tensor(c.impNN, dtype=torch.int64), c.scale, c.length,
                           e.tensor(c.gamma if gamma is None else gamma), e.tensor(c.y), e.tensor(c.z if z is None else z))
    return npy(f)


# ------------------------------------------------------------------ Vecchia (a) rows
@pytest.mark.parametrize('n,D,m,name', VCASES, ids=[vid(c) for c in VCASES])
def test_vecchia_rows_against_extended_precision(veng, n, D, m, name):
    """vecchia_het_rows_kernel: NNl equal to the reference's, padding slots included; every row of Lrows in the relative 2-norm
    and every t_i (relative to |u_obs|_2 |y_obs|_2 of its block) within max(32 E_ref, 64 * 2^-53), E_ref being O.U_matrix_rows'
    own error against the same reference; and inside the rigorous bound b (3 b + 17) 2^-53 kappa_2."""
    c, R, f, e_rows, e_draw = H.vecchia_reference(n, D, m, name)
    Lrows, NNl, t, info = het_rows(veng, c)
    assert info == 0
    assert np.array_equal(NNl, R.NNl)
    ok, eL, et = H.rows_accepted(Lrows, NNl, t, R, c.y, e_rows)
    print('PARITY rows %-22s kappa %.2e  oracle %.2e %.2e  device %.2e %.2e  ratio %.2f %.2f'
          % (vid((n, D, m, name)), R.cond.max(), e_rows[0], e_rows[1], eL, et, eL / max(e_rows[0], U), et / max(e_rows[1], U)))
    assert ok, (eL, et, e_rows, H.rigorous_rows_bound(R))


# ------------------------------------------------------------------ Vecchia (b) solve
@pytest.mark.parametrize('n,D,m,name', [(1100, 3, 25, 'sexp'), (1100, 3, 25, 'matern2.5'), (140, 2, 100, 'sexp'), (140, 2, 100, 'matern2.5')])
def test_sparse_solve_backward_error(veng, n, D, m, name):
    """dgpamd_vecchia_spsolve on the float64-rounded reference rows and a random right-hand side: the componentwise backward
    error of substitution, |L x - b| <= (m + 4) 2^-53 |L| |x| (Higham, Accuracy and Stability, Thm 8.5: one rounding per term of
    the fma chain, the subtraction, the division, and one unit each for a reciprocal and for the scale factor).  It does not
    depend on conditioning; a dropped or doubled term, a padded slot read as a dependency, or a row solved before its
    dependency was published in its 1024-row window breaks it by many decades."""
    import torch
    c, R, f, e_rows, e_draw = H.vecchia_reference(n, D, m, name)
    Lrows = np.asarray(R.Lrows, np.float64)
    rhs = np.random.default_rng(n + m).normal(size=n)
    x = npy(veng.vecchia_spsolve(veng.tensor(Lrows), veng.tensor(R.NNl, dtype=torch.int64), 1.0, veng.tensor(rhs)))
    res, mag = H.sparse_residual(Lrows, R.NNl, x, rhs)
    mdev = R.NNl.shape[1] - 1
    ratio = float((res / ((mdev + 4) * U * mag)).max())
    print('PARITY solve %-22s largest |L x - b| / ((m + 4) 2^-53 |L||x|) = %.3f' % (vid((n, D, m, name)), ratio))
    assert np.all(np.isfinite(x)) and ratio <= 1.0, ratio


# ------------------------------------------------------------------ Vecchia (c) the draw
@pytest.mark.parametrize('n,D,m,name', VCASES, ids=[vid(c) for c in VCASES])
def test_vecchia_draw_against_extended_precision(veng, n, D, m, name):
    """Engine.vecchia_post_het against het_ref.draw_vecchia in max |f - f_ref| / max |f_ref|, within max(32 E_ref, 64 * 2^-53)
    of O.post_het_vecch's own error."""
    c, R, f, e_rows, e_draw = H.vecchia_reference(n, D, m, name)
    err = H.draw_error(device_draw(veng, c), f)
    print('PARITY draw %-22s kappa %.2e  oracle %.2e  device %.2e  ratio %.2f' % (vid((n, D, m, name)), R.cond.max(), e_draw, err, err / max(e_draw, U)))
    assert H.accept(err, e_draw), (err, e_draw)


@pytest.mark.parametrize('name', H.NAMES)
def test_vecchia_draw_with_every_point_in_the_block_is_the_dense_mean(veng, name):
    """m >= n and z = 0: the draw is the dense posterior mean v (v + Gamma)^-1 y up to the 1e-10 on the blocks' diagonals (6e-10
    and 1.4e-9 relative between the two float64 forms on the host): 1e-8 max |f|."""
    c = H.vecchia_case(20, 2, 50, name)
    mean = np.asarray(H.draw_dense(H.corr(c.X, c.X, c.length, name), c.scale, c.gamma, c.y, np.zeros((c.n, 2))), float)
    f = device_draw(veng, c, z=np.zeros(c.n))
    print('PARITY m>=n %-10s |f - dense mean| / max|f| = %.2e' % (name, np.abs(f - mean).max() / np.abs(mean).max()))
    assert np.abs(f - mean).max() <= 1e-8 * np.abs(mean).max()


# ------------------------------------------------------------------ (d) the imputer's glue
def glue_model(eng, n, vecchia, rep, name, seed):
    """Two GP nodes (the first fed a global input) under a Hetero likelihood, latents and observations at fixed values."""
    from dgp_amd import kernel, Hetero
    rng = np.random.default_rng(seed)
    X, G = rng.uniform(size=(n, 2)), rng.uniform(size=(n, 1))
    nd0 = kernel(length=np.array([0.17, 0.22, 0.6]), scale=1.3, nugget=1e-4, name=name, input_dim=np.arange(2), connect=np.array([0]), engine=eng)
    nd1 = kernel(length=np.array([0.3]), scale=0.8, nugget=1e-4, name=name, input_dim=np.arange(2), engine=eng)
    nd0.input, nd0.global_input, nd1.input, nd1.global_input = X, G, X.copy(), None
    nd0.output, nd1.output = rng.normal(size=(n, 1)), rng.normal(-1.0, 0.7, size=(n, 1))
    nd0.D, nd1.D = 3, 2
    for nd in (nd0, nd1):
        nd.vecch = vecchia
        if vecchia:
            nd.m = 10
            nd.ord_nn(ord=rng.permutation(n), NNarray=np.zeros((n, 11), np.int64))
    mask = np.repeat(np.arange(n), rng.integers(1, 4, size=n)) if rep else None
    sites = np.arange(n) if mask is None else mask
    lik = Hetero(input_dim=np.array([0, 1]))
    lik.rep = mask
    lik.output = (np.sin(4 * X[sites, 0]) + np.exp(0.5 * nd1.output[sites, 0]) * rng.normal(size=len(sites)))[:, None]
    lik.input = np.concatenate((nd0.output, nd1.output), 1)[sites]
    return nd0, nd1, lik, mask, rng


@pytest.mark.parametrize('rep', [False, True], ids=['norep', 'rep'])
@pytest.mark.parametrize('name', H.NAMES)
def test_imputer_vecchia_glue(veng, name, rep):
    """imputer._exact_posterior, Vecchia branch, n = 150, m = 10: it reorders gamma, y and [input | global input] by nd.ord,
    aggregates replicates and maps the draw back through rev_ord.  Against het_ref.draw_vecchia assembled here from nd.ord,
    O.imp_nn_array and the host-side (gamma, y) reduction: F[ord[i], 0] = f_ord[i]; a permutation swapped on two rows fails
    (tests/test_het_ref_host.py)."""
    from dgp_amd.imputation import imputer, DrawStream
    from oracle import dgp_oracle as O
    n = 150
    nd0, nd1, lik, mask, rng = glue_model(veng, n, True, rep, name, 31 + rep)
    z = rng.normal(size=n)
    logvar, yobs, ord_ = nd1.output[:, 0].copy(), lik.output[:, 0].copy(), nd0.ord.copy()
    imp = imputer([[nd0, nd1], [lik]], draws=DrawStream(z=[z]), engine=veng)
    imp._attach()
    imp._exact_posterior(0, 0, lik)
    got = npy(imp.F[0])
    assert imp.draws._z == [] and np.array_equal(got[:, 1], logvar)
    Xo = np.concatenate((nd0.input, nd0.global_input), 1)[ord_]
    impNN = O.imp_nn_array(Xo / nd0.length, 10)
    assert np.array_equal(nd0.imp_NNarray, impNN)
    sites = np.arange(n) if mask is None else mask
    ge, ye = H.site_terms(np.exp(logvar[sites]), yobs, mask, n)
    f = H.draw_vecchia(Xo, impNN, nd0.scale[0], nd0.length, name, ge[ord_], ye[ord_], z)
    g64, y64 = np.asarray(ge, float)[ord_], np.asarray(ye, float)[ord_]
    e_ref = H.draw_error(O.post_het_vecch(Xo, impNN, nd0.scale[0], nd0.length, name, np.concatenate((g64, g64)), y64, z), f)
    err = H.draw_error(got[ord_, 0], f)
    print('PARITY glue vecchia %-10s rep=%d  oracle %.2e  device %.2e  ratio %.2f' % (name, rep, e_ref, err, err / max(e_ref, U)))
    assert H.accept(err, e_ref), (err, e_ref)


@pytest.mark.parametrize('rep', [False, True], ids=['norep', 'rep'])
@pytest.mark.parametrize('name', H.NAMES)
def test_imputer_dense_glue(eng, name, rep):
    """imputer._exact_posterior, dense branch, n = 130: K of [input | global input], Hetero.posterior_terms, post_het."""
    from dgp_amd.imputation import imputer, DrawStream
    from oracle import dgp_oracle as O
    n = 130
    nd0, nd1, lik, mask, rng = glue_model(eng, n, False, rep, name, 41 + rep)
    sd = rng.normal(size=(n, 2))
    logvar, yobs = nd1.output[:, 0].copy(), lik.output[:, 0].copy()
    imp = imputer([[nd0, nd1], [lik]], draws=DrawStream(z=[sd.reshape(-1)]), engine=eng)
    imp._attach()
    imp._exact_posterior(0, 0, lik)
    got = npy(imp.F[0])
    assert imp.draws._z == [] and np.array_equal(got[:, 1], logvar)
    K = npy(eng.kmatrix(name, eng.tensor(nd0.input), None, eng.tensor(nd0.global_input), nd0.length, nd0.nugget[0]))
    Ko = O.k_matrix(np.concatenate((nd0.input, nd0.global_input), 1), nd0.length, nd0.nugget[0], name)
    assert np.abs(K - Ko).max() <= 1e-12 and np.linalg.cond(Ko) <= H.KAPPA_MAX
    sites = np.arange(n) if mask is None else mask
    ge, ye = H.site_terms(np.exp(logvar[sites]), yobs, mask, n)
    f = H.draw_dense(K, nd0.scale[0], ge, ye, sd)
    e_ref = H.draw_error(O.post_het1(nd0.scale[0] * K, np.asarray(ge, float), np.asarray(ye, float), sd), f)
    err = H.draw_error(got[:, 0], f)
    print('PARITY glue dense   %-10s rep=%d  oracle %.2e  device %.2e  ratio %.2f' % (name, rep, e_ref, err, err / max(e_ref, U)))
    assert H.accept(err, e_ref), (err, e_ref)


# ------------------------------------------------------------------ dense
@pytest.mark.parametrize('n', H.DENSE_N)
@pytest.mark.parametrize('name', H.NAMES)
def test_dense_draw_against_extended_precision(eng, name, n):
    """Engine.post_het (potrf, trmv_lower, potrf_inv with the right-hand side in row n, -S[n, :n], gemv) with K from the device's
    own assembly, contiguous and as a view into a wider buffer whose other columns hold NaNs, against het_ref.draw_dense on the
    same K."""
    import torch
    c = H.dense_case(n, name)
    K = eng.kmatrix(name, eng.tensor(c.X), None, None, c.length, c.nugget, full=True)
    f, e_ref = H.dense_reference(c, npy(K))
    wide = eng.empty(n, n + 5)
    wide.fill_(float('nan'))
    Kw = wide[:, :n]
    Kw.copy_(K)
    assert Kw.stride(0) > n
    args = (c.scale, eng.tensor(c.gamma), eng.tensor(c.y), eng.tensor(c.sd))
    f1, f2 = npy(eng.post_het(K, *args)), npy(eng.post_het(Kw, *args))
    err = H.draw_error(f1, f)
    print('PARITY dense %-16s kappa %.2e  oracle %.2e  device %.2e  ratio %.2f' % (vid((n, name)), np.linalg.cond(npy(K)), e_ref, err, err / max(e_ref, U)))
    assert H.accept(err, e_ref), (err, e_ref)
    assert np.array_equal(f1, f2)
    assert torch.isnan(wide[:, n:]).all()


@pytest.mark.parametrize('name', H.NAMES)
def test_hetero_posterior_with_replicates(eng, name):
    """Hetero.posterior with a replicate mask at n = 130 (1-3 observations per site): posterior_terms' reduction, then post_het
    with v = scale K and scale 1."""
    from dgp_amd import Hetero
    c = H.dense_case(130, name)
    K = npy(eng.kmatrix(name, eng.tensor(c.X), None, None, c.length, c.nugget, full=True))
    v = c.scale * K
    h = Hetero()
    h.rep = c.mask.copy()
    h.input = np.stack((np.zeros(len(c.mask)), np.log(c.gamma_obs)), 1)
    h.output = c.y_obs[:, None].copy()
    got = h.posterior(np.array([0]), v, sd=c.sd.copy(), engine=eng)
    from oracle import dgp_oracle as O
    ge, ye = H.site_terms(np.exp(h.input[:, 1]), c.y_obs, c.mask, c.n)
    f = H.draw_dense(v, 1.0, ge, ye, c.sd)
    e_ref = H.draw_error(O.post_het2(v, np.exp(h.input[:, 1]), c.mask, c.y_obs, c.sd), f)
    err = H.draw_error(got, f)
    print('PARITY dense rep %-12s oracle %.2e  device %.2e  ratio %.2f' % (name, e_ref, err, err / max(e_ref, U)))
    assert H.accept(err, e_ref), (err, e_ref)


# ------------------------------------------------------------------ gemv and trmv_lower on their own
@pytest.mark.parametrize('cols', [1, 63, 64, 65, 200])
@pytest.mark.parametrize('rows', [1, 3, 4, 5, 130])
def test_gemv_against_long_double_sums(eng, rows, cols):
    """gemv_kernel (one wave per row, four rows per workgroup) with ld > cols and NaNs in the columns beyond: every row within
    (k + 2) 2^-53 sum_j |a_j x_j|, k = cols terms (an fma chain per lane and a 6-step tree: at most k roundings on any term)."""
    rng = np.random.default_rng(100 * rows + cols)
    A, x = rng.normal(size=(rows, cols)), rng.normal(size=cols)
    buf = eng.empty(rows, cols + 3)
    buf.fill_(float('nan'))
    buf[:, :cols] = eng.tensor(A)
    out = npy(eng.gemv(buf[:, :cols], eng.tensor(x)))
    s, a = H.dot_terms(A, x)
    ratio = float((np.abs(out - s) / ((cols + 2) * U * a)).max())
    print('PARITY gemv %dx%d: largest error / bound = %.3f' % (rows, cols, ratio))
    assert out.shape == (rows,) and ratio <= 1.0, ratio


@pytest.mark.parametrize('shared', [False, True])
@pytest.mark.parametrize('batch', [1, 3])
@pytest.mark.parametrize('n', [1, 64, 65, 130])
def test_trmv_lower_against_long_double_sums(eng, n, batch, shared):
    """trmv_lower_kernel: out[b][i] = sqrt(scale_b) sum_{j <= i} L_b[i][j] z[b][j] on padded buffers whose strict upper triangle
    holds NaNs, per-batch scales, one buffer for the whole batch (shared) or one each: within (k + 2) 2^-53 sqrt(scale)
    sum |l_ij z_j|, k = i + 1 terms (the chain and the tree as in gemv, the rounded square root and the product)."""
    rng = np.random.default_rng(1000 * n + 10 * batch + shared)
    Np = eng.padded_dim(n)
    nb = 1 if shared else batch
    L = np.full((nb, Np, Np), np.nan)
    L[:, np.tril_indices(Np)[0], np.tril_indices(Np)[1]] = rng.normal(size=(nb, Np * (Np + 1) // 2))
    z = rng.normal(size=(batch, n))
    scale = rng.uniform(0.5, 3.0, size=batch)
    out = npy(eng.trmv_lower(n, eng.tensor(L), scale, eng.tensor(z), batch=batch, shared=shared))
    assert out.shape == (batch, n)
    worst = 0.0
    for b in range(batch):
        Lb = np.tril(np.nan_to_num(L[0 if shared else b, :n, :n]))
        s, a = H.dot_terms(Lb, z[b])
        r = np.sqrt(H.LD(scale[b]))
        k = np.arange(n) + 1
        worst = max(worst, float((np.abs(out[b] - r * s) / ((k + 2) * U * r * a)).max()))
    print('PARITY trmv_lower n=%d batch=%d shared=%d: largest error / bound = %.3f' % (n, batch, shared, worst))
    assert worst <= 1.0, worst


# ------------------------------------------------------------------ error reports
@pytest.mark.parametrize('name', H.NAMES)
def test_vecchia_not_positive_definite_is_reported(veng, name):
    """A large negative gamma at one site p: every block that holds p as an observation has a negative pivot (lds_chol puts 1
    in its place and finishes; the first such row goes into the info word), Engine.vecchia_post_het raises
    numpy.linalg.LinAlgError naming one of those rows, and the next correct call on the same engine returns the bits it
    returned before."""
    import re
    c, R, f, e_rows, e_draw = H.vecchia_reference(130, 2, 2, name)
    before = device_draw(veng, c)
    p = 57
    bad = c.gamma.copy()
    bad[p] = -50.0
    holders = np.nonzero(((R.idx == p) & ~R.lat).any(1))[0]
    assert p in holders and len(holders) >= 1
    with pytest.raises(np.linalg.LinAlgError) as exc:
        device_draw(veng, c, gamma=bad)
    row = int(re.search(r'row (\d+)', str(exc.value)).group(1))
    assert row in holders, (row, holders)
    info = het_rows(veng, c, gamma=bad)[3]
    assert info - 1 in holders
    assert np.array_equal(device_draw(veng, c), before)


@pytest.mark.parametrize('n', [64, 130])
def test_dense_not_positive_definite_is_reported(eng, n):
    """The same gamma in Engine.post_het: what raise_not_pd raises for a positive status, numpy.linalg.LinAlgError, and the
    following correct call gives the bits of the call before."""
    c = H.dense_case(n, 'sexp')
    K = eng.kmatrix('sexp', eng.tensor(c.X), None, None, c.length, c.nugget, full=True)
    args = (eng.tensor(c.y), eng.tensor(c.sd))
    before = npy(eng.post_het(K, c.scale, eng.tensor(c.gamma), *args))
    bad = c.gamma.copy()
    bad[n // 3] = -50.0
    with pytest.raises(np.linalg.LinAlgError, match='leading minor'):
        eng.post_het(K, c.scale, eng.tensor(bad), *args)
    assert np.array_equal(npy(eng.post_het(K, c.scale, eng.tensor(c.gamma), *args)), before)
