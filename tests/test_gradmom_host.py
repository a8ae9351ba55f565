"""The host side of the active subspaces and derivative-based sensitivity measures (dgp_amd/sensitivity.py, DESIGN I.18): the
design, the result class on sums that the reference (tests/gradmom_ref.py) makes from analytic gradients, the refusals that
are decided before anything touches a device, the C entry, and the statistical check's margins on the numpy restatement.
No GPU."""
import ctypes
import inspect
import os
import warnings

import numpy as np
import pytest

import gradmom_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_signatures_of_the_entry_points():
    from dgp_amd import emulator, gp, pathfun, sensitivity
    conv = ['self', 'bounds', 'n_rows', 'sample_size', 'n_features', 'seed', 'qmc']
    for cls in (emulator, gp):
        sig = inspect.signature(cls.active_subspace)
        assert list(sig.parameters) == conv
        assert [sig.parameters[k].default for k in conv[2:]] == [4096, 20, 2048, None, False]
        assert sig.parameters['bounds'].default is inspect.Parameter.empty
    for cls in (pathfun.PathFunctions, pathfun.GpPaths):
        sig = inspect.signature(cls.active_subspace)
        assert list(sig.parameters) == ['self', 'X', 'bounds'] and sig.parameters['bounds'].default is None
    assert list(inspect.signature(sensitivity.uniform_design).parameters) == ['bounds', 'n_rows', 'seed', 'qmc']
    assert list(inspect.signature(sensitivity.gradient_moments).parameters) == ['e', 'value_and_jac', 'X', 'P', 'width']
    assert list(inspect.signature(sensitivity.ActiveSubspaceResult.__init__).parameters) == ['self', 'sums', 'n_rows', 'bounds', 'squeeze']
    from dgp_amd.ops import Engine
    assert list(inspect.signature(Engine.gradmom_tiles).parameters) == ['self', 'f', 'J', 'shift']


def test_uniform_design_shapes_bounds_and_seed():
    from dgp_amd.sensitivity import uniform_design
    bounds = np.array([[0.0, 1.0], [-3.0, 5.0], [2.0, 2.5]])
    X = uniform_design(bounds, 37, seed=3)
    assert X.shape == (37, 3) and X.dtype == np.float64
    assert np.all(X >= bounds[:, 0]) and np.all(X <= bounds[:, 1])
    u = np.random.default_rng(3).uniform(size=(37, 3))          # the documented draws
    assert np.array_equal(X, bounds[:, 0] + (bounds[:, 1] - bounds[:, 0]) * u)
    assert np.array_equal(X, uniform_design(bounds, 37, seed=3))
    assert not np.array_equal(X, uniform_design(bounds, 37, seed=4))


def test_uniform_design_qmc():
    from dgp_amd.sensitivity import uniform_design
    bounds = np.array([[0.0, 1.0], [-3.0, 5.0]])
    X = uniform_design(bounds, 64, seed=1, qmc=True)
    assert X.shape == (64, 2) and np.all(X >= bounds[:, 0]) and np.all(X <= bounds[:, 1])
    assert np.array_equal(X, uniform_design(bounds, 64, seed=1, qmc=True))
    # a scrambled Sobol' net of 2^6 points has 32 points in either half of every coordinate
    assert np.array_equal((X < bounds.mean(1)).sum(0), [32, 32])
    with pytest.raises(ValueError, match='power of two'):
        uniform_design(bounds, 100, qmc=True)


@pytest.mark.parametrize('bounds', [np.zeros(3), np.zeros((3, 3)), np.zeros((0, 2)), [[1.0, 0.0]], [[0.0, np.inf]]])
def test_uniform_design_refuses_bad_bounds(bounds):
    from dgp_amd.sensitivity import uniform_design
    with pytest.raises(ValueError, match='uniform_design'):
        uniform_design(bounds, 8)


def test_uniform_design_refuses_no_rows():
    from dgp_amd.sensitivity import uniform_design
    with pytest.raises(ValueError, match='n_rows'):
        uniform_design([[0.0, 1.0]], 0)


# ------------------------------------------------------------------------------------------------ the result class
A_LIN = np.array([[1.5, -2.0, 0.0, 0.25], [0.0, 3.0, -1.0, 0.5]])        # (K, Dx): output k is a_k . x + c_k
BOUNDS = np.array([[0.0, 1.0], [-1.0, 3.0], [2.0, 2.5], [-4.0, 4.0]])


def linear_case(P=3, M=150, seed=0):
    """f_pk(x) = (1 + p) a_k . x + c_k at M uniform rows of the box: values (P, M, K), gradients (P, M, K, Dx), the rows."""
    from dgp_amd.sensitivity import uniform_design
    X = uniform_design(BOUNDS, M, seed=seed)
    amp = 1.0 + np.arange(P)
    f = amp[:, None, None] * (X @ A_LIN.T)[None] + np.array([10.0, -3.0])
    G = np.broadcast_to(amp[:, None, None, None] * A_LIN[None, None], (P, M) + A_LIN.shape).copy()
    return X, f, G, amp


def test_linear_function_gives_a_rank_one_C():
    from dgp_amd.sensitivity import ActiveSubspaceResult
    X, f, G, amp = linear_case()
    P, M, (K, Dx) = len(amp), len(X), A_LIN.shape
    res = ActiveSubspaceResult(R.from_gradients(f, G), M, BOUNDS)
    assert res.C.shape == (K, P, Dx, Dx) and res.dgsm.shape == res.mean_grad.shape == (K, Dx, P)
    assert res.mean.shape == res.variance.shape == (K, P) and res.eigenvalues.shape == (K, P, Dx) and res.eigenvectors.shape == (K, P, Dx, Dx)
    scale = 0.5 * (BOUNDS[:, 1] - BOUNDS[:, 0])
    assert np.array_equal(res.scale, scale)
    for k in range(K):
        for p in range(P):
            a = amp[p] * A_LIN[k]
            np.testing.assert_allclose(res.C[k, p], np.outer(a, a), rtol=1e-13, atol=1e-13)
            assert np.array_equal(res.C[k, p], res.C[k, p].T)
            np.testing.assert_allclose(res.dgsm[k, :, p], a**2, rtol=1e-13)
            np.testing.assert_allclose(res.mean_grad[k, :, p], a, rtol=1e-13)
            sa = scale * a
            lam = res.eigenvalues[k, p]
            np.testing.assert_allclose(lam[0], sa @ sa, rtol=1e-13)
            assert np.all(np.abs(lam[1:]) <= 1e-13 * lam[0]) and np.all(np.diff(lam) <= 0.0)
            w = res.eigenvectors[k, p][:, 0]
            lead = sa / np.linalg.norm(sa)
            lead = lead * np.sign(lead[np.argmax(np.abs(lead))])       # the sign convention: largest-magnitude component positive
            np.testing.assert_allclose(w, lead, rtol=0, atol=1e-13)
            assert w[np.argmax(np.abs(w))] > 0.0
            np.testing.assert_allclose(res.mean[k, p], f[p, :, k].mean(), rtol=1e-13)
            np.testing.assert_allclose(res.variance[k, p], f[p, :, k].var(), rtol=1e-11)
    # exactly zero where the gradient is: column 2 of output 0, column 0 of output 1
    assert np.all(res.C[0][:, 2, :] == 0.0) and np.all(res.C[0][:, :, 2] == 0.0) and np.all(res.C[1][:, 0, :] == 0.0)


def test_every_eigenvector_is_oriented():
    from dgp_amd.sensitivity import ActiveSubspaceResult
    rng = np.random.default_rng(5)
    f, G = rng.normal(size=(4, 90, 2)), rng.normal(size=(4, 90, 2, 6))
    res = ActiveSubspaceResult(R.from_gradients(f, G), 90)
    V = res.eigenvectors
    top = np.take_along_axis(V, np.argmax(np.abs(V), -2)[..., None, :], -2)
    assert np.all(top > 0.0) and np.all(np.diff(res.eigenvalues, axis=-1) <= 0.0)
    ref = R.formulas(res.sums['sums'], res.sums['shift'], 90)
    # V diag(lambda) V^T is S C S, and without bounds S is the identity
    np.testing.assert_allclose(np.einsum('kpij,kpj,kplj->kpil', V, res.eigenvalues, V), ref['scaled'], rtol=0, atol=1e-12)
    assert np.array_equal(ref['scaled'], ref['C']) and np.array_equal(res.scale, np.ones(6))
    for name in ('C', 'dgsm', 'mean_grad', 'mean', 'variance'):
        assert np.array_equal(getattr(res, name), ref[name]), name


def test_activity_scores_and_total_bound():
    from dgp_amd.sensitivity import ActiveSubspaceResult
    rng = np.random.default_rng(6)
    f, G = rng.normal(size=(5, 120, 2)), rng.normal(size=(5, 120, 2, 4)) * [1.0, 0.1, 3.0, 0.0]
    res = ActiveSubspaceResult(R.from_gradients(f, G), 120, BOUNDS)
    ref = R.formulas(res.sums['sums'], res.sums['shift'], 120, BOUNDS)
    full = res.activity_scores(4)
    assert full.shape == (2, 4, 5)
    np.testing.assert_allclose(full, np.diagonal(ref['scaled'], axis1=-2, axis2=-1).transpose(0, 2, 1), rtol=1e-12, atol=1e-13)
    one = res.activity_scores(1)
    np.testing.assert_allclose(one, (res.eigenvalues[..., 0, None] * res.eigenvectors[..., 0]**2).transpose(0, 2, 1), rtol=1e-13)
    assert np.all(res.activity_scores(2) >= one - 1e-15)
    for k in (0, 5):
        with pytest.raises(ValueError, match='1 .. Dx'):
            res.activity_scores(k)
    # the bound computed directly: nu_i (b_i - a_i)^2 / (pi^2 V)
    tb = res.total_bound
    assert tb.shape == (2, 4, 5)
    width = BOUNDS[:, 1] - BOUNDS[:, 0]
    for k in range(2):
        for i in range(4):
            for p in range(5):
                want = res.dgsm[k, i, p] * width[i]**2 / (np.pi**2 * res.variance[k, p])
                assert abs(tb[k, i, p] - want) <= 1e-14 * want
    assert np.array_equal(tb, ref['total_bound']) and np.all(tb[:, 3] == 0.0)
    s = res.summary(level=0.8)
    assert sorted(s) == ['dgsm', 'eigenvalues', 'total_bound'] and sorted(s['dgsm']) == ['lower', 'mean', 'upper']
    assert s['dgsm']['mean'].shape == s['eigenvalues']['upper'].shape == s['total_bound']['lower'].shape == (2, 4)
    assert np.array_equal(s['dgsm']['mean'], np.nanmean(res.dgsm, -1))
    np.testing.assert_allclose(s['eigenvalues']['lower'], np.nanquantile(res.eigenvalues, 0.1, axis=1), rtol=1e-13)
    np.testing.assert_allclose(s['total_bound']['upper'], np.nanquantile(tb, 0.9, axis=-1), rtol=1e-13)
    with pytest.raises(ValueError, match='level'):
        res.summary(level=0.0)


def test_zero_variance_gives_nan_and_no_bounds_raises():
    from dgp_amd.sensitivity import ActiveSubspaceResult
    rng = np.random.default_rng(7)
    f, G = rng.normal(size=(2, 70, 1)), rng.normal(size=(2, 70, 1, 3))
    f[0] = 4.0                                                  # a constant draw: V == 0
    G[0] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        res = ActiveSubspaceResult(R.from_gradients(f, G), 70, BOUNDS[:3])
        tb = res.total_bound
        s = res.summary()
        one = ActiveSubspaceResult(R.from_gradients(f[:1], G[:1]), 70, BOUNDS[:3]).summary()
    assert res.variance[0, 0] == 0.0 and np.all(np.isnan(tb[0, :, 0])) and np.all(np.isfinite(tb[0, :, 1]))
    assert np.array_equal(s['total_bound']['mean'], tb[:, :, 1])            # the NaN draw is left out
    assert np.all(np.isnan(one['total_bound']['upper'])) and np.all(one['dgsm']['mean'] == 0.0)
    free = ActiveSubspaceResult(R.from_gradients(f, G), 70)
    with pytest.raises(ValueError, match='bounds'):
        free.total_bound
    assert sorted(free.summary()) == ['dgsm', 'eigenvalues']
    with pytest.raises(ValueError, match='rows'):
        ActiveSubspaceResult(R.from_gradients(f, G), 70, BOUNDS)            # four bounds, three columns
    with pytest.raises(ValueError, match='sums must be'):
        ActiveSubspaceResult({'sums': np.zeros((2, 1, 8)), 'shift': np.zeros((2, 1))}, 70)     # (7 is Dx = 2, 11 is Dx = 3)


def test_squeeze_drops_the_output_axis():
    from dgp_amd.sensitivity import ActiveSubspaceResult
    rng = np.random.default_rng(8)
    f, G = rng.normal(size=(6, 80, 1)), rng.normal(size=(6, 80, 1, 3))
    sums = R.from_gradients(f, G)
    full, one = ActiveSubspaceResult(sums, 80, BOUNDS[:3]), ActiveSubspaceResult(sums, 80, BOUNDS[:3], squeeze=True)
    assert one.C.shape == (6, 3, 3) and one.dgsm.shape == one.mean_grad.shape == one.total_bound.shape == (3, 6)
    assert one.mean.shape == one.variance.shape == (6,) and one.eigenvalues.shape == (6, 3) and one.eigenvectors.shape == (6, 3, 3)
    assert one.activity_scores(2).shape == (3, 6)
    for name in ('C', 'dgsm', 'mean_grad', 'mean', 'variance', 'eigenvalues', 'eigenvectors', 'total_bound'):
        assert np.array_equal(getattr(one, name), getattr(full, name)[0]), name
    assert np.array_equal(one.activity_scores(2), full.activity_scores(2)[0])
    s = one.summary()
    assert s['dgsm']['mean'].shape == s['eigenvalues']['mean'].shape == s['total_bound']['mean'].shape == (3,)
    W1, d1 = one.subspace(2)
    W2, d2 = full.subspace(2, output=0)
    assert np.array_equal(W1, W2) and np.array_equal(d1, d2)


def test_subspace_of_equal_and_of_different_draws():
    from dgp_amd.sensitivity import ActiveSubspaceResult
    rng = np.random.default_rng(9)
    f1, G1 = rng.normal(size=(1, 100, 2)), rng.normal(size=(1, 100, 2, 5)) * [3.0, 1.0, 0.3, 0.1, 0.03]
    same = ActiveSubspaceResult(R.from_gradients(np.repeat(f1, 4, 0), np.repeat(G1, 4, 0)), 100)
    for k in (1, 2, 5):
        for output in (0, 1):
            W, dist = same.subspace(k, output=output)
            assert W.shape == (5, k) and dist.shape == (4,) and np.all(dist <= 1e-12)
            np.testing.assert_allclose(W.T @ W, np.eye(k), rtol=0, atol=1e-13)
            np.testing.assert_allclose(W, same.eigenvectors[output, 0][:, :k], rtol=0, atol=1e-10)
    # draws with orthogonal gradients: each one's leading direction is at distance 1 from the other's
    G = np.zeros((2, 100, 1, 3))
    G[0, :, 0, 0], G[1, :, 0, 1] = 2.0, 1.0
    res = ActiveSubspaceResult(R.from_gradients(np.zeros((2, 100, 1)), G), 100)
    W, dist = res.subspace(1)
    assert np.array_equal(W[:, 0], [1.0, 0.0, 0.0])             # the mean of diag(4, 0, 0) and diag(0, 1, 0)
    np.testing.assert_allclose(dist, [0.0, 1.0], rtol=0, atol=1e-15)
    with pytest.raises(ValueError, match='1 .. Dx'):
        res.subspace(4)
    with pytest.raises(ValueError, match='output'):
        res.subspace(1, output=1)


# ------------------------------------------------------------------------------------------------ refusals
def _hollow(cls, **attrs):
    """An object of a paths class with the few attributes a refusal reads: a refusal comes before any device work."""
    obj = cls.__new__(cls)
    obj.__dict__.update(attrs)
    return obj


class _Node:
    def __init__(self, type, m=0):
        self.type, self.m = type, m


def test_active_subspace_refuses_before_any_device_work():
    from dgp_amd import pathfun
    X = np.zeros((8, 3))
    emu = _hollow(pathfun.PathFunctions, layers=[[_Node('gp')], [_Node('likelihood')]], nodes={})
    with pytest.raises(ValueError, match='has no derivative'):
        emu.active_subspace(X)
    for obj in (_hollow(pathfun.PathFunctions, layers=[[_Node('gp')]], nodes={(0, 0): _Node('gp', m=20)}),
                _hollow(pathfun.GpPaths, node=_Node('gp', m=20))):
        with pytest.raises(NotImplementedError, match='active_subspace: a draw made by local conditioning'):
            obj.active_subspace(X)
    for obj in (_hollow(pathfun.PathFunctions, layers=[[_Node('gp')]], nodes={(0, 0): _Node('gp')}),
                _hollow(pathfun.GpPaths, node=_Node('gp'))):
        with pytest.raises(Exception, match='2d-array'):
            obj.active_subspace(X[0])
        with pytest.raises(ValueError, match='at least 2 rows'):
            obj.active_subspace(X[:1])
        with pytest.raises(ValueError, match='1 to 64 columns'):
            obj.active_subspace(np.zeros((8, 65)))
        with pytest.raises(ValueError, match='bounds has 2 rows, X 3 columns'):
            obj.active_subspace(X, bounds=[[0.0, 1.0]] * 2)
        with pytest.raises(ValueError, match='low <= high'):
            obj.active_subspace(X, bounds=[[0.0, 1.0], [1.0, 0.0], [0.0, 1.0]])


def test_c_entry_is_declared_exported_and_refuses_before_any_launch():
    """include/dgp_amd.h declares dgpamd_gradmom_tiles, the library exports it and _lib.SIGNATURES carries it."""
    from dgp_amd import _lib
    from test_cabi_symbols import declared_functions
    assert 'dgpamd_gradmom_tiles' in declared_functions()
    lib = ctypes.CDLL(os.path.join(ROOT, 'dgp_amd', 'libdgp_amd.so'))
    assert hasattr(lib, 'dgpamd_gradmom_tiles') and 'dgpamd_gradmom_tiles' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['dgpamd_gradmom_tiles'][1]) == 9
    assert _lib.lib.dgpamd_gradmom_tiles(None, 1, 1, 1, 1, None, None, None, None) == _lib.BAD_ARG


def test_the_statistical_margins_clear_ten_standard_errors():
    """tests/test_gpu_gradmom_model.py's statistical check on the numpy restatement, without a device: the alignment of every
    draw's (and of the mean's) leading direction lies more than ten Monte-Carlo standard errors above the test's threshold,
    and total_bound exceeds the total index by more than ten for every input and draw."""
    import test_gpu_gradmom_model as T
    align, se_align, margin, se_margin = T.stat_restated()
    print('alignment %s (se %s); smallest margin / se %.3g' % (align, se_align, (margin / se_margin).min()))
    assert align.shape == (T.STAT_J + 1,) and margin.shape == (3, T.STAT_J)
    assert np.all(align - T.STAT_ALIGNMENT > 10.0 * se_align) and np.all(align <= 1.0 + 1e-15)
    assert np.all(margin > 10.0 * se_margin)


def test_reference_sums_on_known_numbers():
    """gradmom_ref on integers (every term and sum exact): the order of the entries, and the longdouble side on a cancelling
    sum that f64 loses."""
    f = np.arange(1.0, 7.0).reshape(1, 3, 2)                     # outputs (1, 3, 5) and (2, 4, 6)
    J = np.arange(1.0, 13.0).reshape(1, 3, 2, 2)                 # output 0: rows (1, 2), (5, 6), (9, 10)
    shift = np.array([[1.0, 1.0]])
    s = R.sums(f, J, shift)
    assert s.shape == (1, 2, 7) and s.dtype == np.float64
    # g = 0, 2, 4; sum J_0, sum J_1; then the products (0, 0), (0, 1), (1, 1)
    assert list(s[0, 0]) == [6.0, 20.0, 15.0, 18.0, 1.0 + 25.0 + 81.0, 2.0 + 30.0 + 90.0, 4.0 + 36.0 + 100.0]
    s3 = R.sums(f[:, :, :1], np.arange(1.0, 19.0).reshape(1, 3, 2, 3)[:, :, :1], shift[:, :1])
    # rows (1, 2, 3), (7, 8, 9), (13, 14, 15): the sums, then (0, 0) (0, 1) (0, 2) (1, 1) (1, 2) (2, 2)
    assert list(s3[0, 0]) == [6.0, 20.0, 21.0, 24.0, 27.0, 219.0, 240.0, 261.0, 264.0, 288.0, 315.0]
    long = R.sums(f, J, shift, np.longdouble)
    assert long.dtype == np.longdouble and np.array_equal(long, s)
    assert np.array_equal(R.magnitudes(f, -J, shift)[..., 4:], long[..., 4:]) and np.array_equal(R.magnitudes(f, -J, shift)[..., 2:4], long[..., 2:4])
    tiny = np.array([1.0, 2.0**-60, -1.0]).reshape(1, 3, 1, 1)      # f64 loses the middle term, 64 bits keep it
    z = np.zeros((1, 3, 1))
    assert np.finfo(np.longdouble).nmant < 63 or R.sums(z, tiny, np.zeros((1, 1)), np.longdouble)[0, 0, 2] == 2.0**-60
    assert R.worst_ratio(np.array([[[0.0, 0.0, 3.0, 3.0]]]), z, np.ones((1, 3, 1, 1)), np.zeros((1, 1))) == 0.0
    assert R.worst_ratio(np.array([[[0.0, 0.0, 3.0 + 2.0**-48, 3.0]]]), z, np.ones((1, 3, 1, 1)), np.zeros((1, 1))) > 1.0
    assert 0.0 < R.worst_ratio(np.array([[[0.0, 0.0, 3.0 + 2.0**-51, 3.0]]]), z, np.ones((1, 3, 1, 1)), np.zeros((1, 1))) < 1.0
