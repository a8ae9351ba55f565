"""The host side of the Sobol' indices (dgp_amd/sensitivity.py, DESIGN I.16): the designs, the formulas against an mpmath
evaluation, the refusals that are decided before anything touches a device, and the reference of the GPU tests against
itself.  No GPU."""
import ctypes
import os
import warnings
from fractions import Fraction

import numpy as np
import pytest

import sobol_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_saltelli_design_shapes_bounds_and_seed():
    from dgp_amd.sensitivity import saltelli_design
    bounds = np.array([[0.0, 1.0], [-3.0, 5.0], [2.0, 2.5]])
    A, B = saltelli_design(bounds, 37, seed=3)
    assert A.shape == B.shape == (37, 3) and A.dtype == np.float64
    for X in (A, B):
        assert np.all(X >= bounds[:, 0]) and np.all(X <= bounds[:, 1])
    # the documented draws: one uniform((n_base, 2 D)) block, its column halves
    u = np.random.default_rng(3).uniform(size=(37, 6))
    assert np.array_equal(A, bounds[:, 0] + (bounds[:, 1] - bounds[:, 0]) * u[:, :3])
    assert np.array_equal(B, bounds[:, 0] + (bounds[:, 1] - bounds[:, 0]) * u[:, 3:])
    A2, B2 = saltelli_design(bounds, 37, seed=3)
    assert np.array_equal(A, A2) and np.array_equal(B, B2)
    A3, _ = saltelli_design(bounds, 37, seed=4)
    assert not np.array_equal(A, A3)
    assert not np.array_equal(A, B)


def test_saltelli_design_qmc():
    from dgp_amd.sensitivity import saltelli_design
    bounds = np.array([[0.0, 1.0], [-3.0, 5.0]])
    A, B = saltelli_design(bounds, 64, seed=1, qmc=True)
    assert A.shape == B.shape == (64, 2)
    for X in (A, B):
        assert np.all(X >= bounds[:, 0]) and np.all(X <= bounds[:, 1])
    A2, B2 = saltelli_design(bounds, 64, seed=1, qmc=True)
    assert np.array_equal(A, A2) and np.array_equal(B, B2)
    # a scrambled Sobol' net of 2^6 points has 32 points in either half of every coordinate
    for X in (A, B):
        assert np.array_equal((X < bounds.mean(1)).sum(0), [32, 32])
    with pytest.raises(ValueError, match='power of two'):
        saltelli_design(bounds, 100, qmc=True)


@pytest.mark.parametrize('bounds', [np.zeros(3), np.zeros((3, 3)), np.zeros((0, 2)), [[1.0, 0.0]], [[0.0, np.inf]]])
def test_saltelli_design_refuses_bad_bounds(bounds):
    from dgp_amd.sensitivity import saltelli_design
    with pytest.raises(ValueError, match='saltelli_design'):
        saltelli_design(bounds, 8)


def test_saltelli_design_refuses_no_rows():
    from dgp_amd.sensitivity import saltelli_design
    with pytest.raises(ValueError, match='n_base'):
        saltelli_design([[0.0, 1.0]], 0)


def test_indices_from_sums_against_mpmath():
    """The three formula lines in 100-digit arithmetic from the same f64 sums.  Bound: V = a - m, a = (q1 + q2) / 2B with two
    roundings, m = ((s1 + s2) / 2B)^2 with three, one more for the difference: |error| <= 2^-53 (2 a + 3 m + |V|) =
    2^-53 (5 m + 3 |V|).  first and total divide twice more (2^-53 each) and carry V's relative error; 1.01 for the
    second-order terms."""
    import mpmath
    from dgp_amd.sensitivity import indices_from_sums
    rng = np.random.default_rng(0)
    D, P, K, B = 3, 5, 2, 300
    g = rng.normal(size=(2 + D, P, B, K)) + rng.normal(size=(P, 1, K))
    base = np.stack([g[0].sum(1), g[1].sum(1), (g[0]**2).sum(1), (g[1]**2).sum(1)], -1)
    pair = np.stack([np.stack([(g[1] * (g[2 + i] - g[0])).sum(1), ((g[0] - g[2 + i])**2).sum(1)], -1) for i in range(D)])
    first, total, V = indices_from_sums(base, pair, B)
    assert first.shape == total.shape == (D, P, K) and V.shape == (P, K)
    r = R.indices(base, pair, B)
    assert all(np.array_equal(a, c) for a, c in zip((first, total, V), r))
    u, worst = 2.0**-53, 0.0
    with mpmath.workdps(100):
        for p in range(P):
            for k in range(K):
                s1, s2, q1, q2 = (mpmath.mpf(float(v)) for v in base[p, k])
                m = ((s1 + s2) / (2 * B))**2
                Vx = (q1 + q2) / (2 * B) - m
                relV = u * (5 * m + 3 * abs(Vx)) / abs(Vx)
                worst = max(worst, float(abs(mpmath.mpf(float(V[p, k])) - Vx) / (1.01 * relV * abs(Vx))))
                for i in range(D):
                    for got, want in ((first[i, p, k], mpmath.mpf(float(pair[i, p, k, 0])) / B / Vx),
                                      (total[i, p, k], mpmath.mpf(float(pair[i, p, k, 1])) / (2 * B) / Vx)):
                        worst = max(worst, float(abs(mpmath.mpf(float(got)) - want) / (1.01 * (relV + 2 * u) * abs(want))))
    print('indices_from_sums: max error / bound = %.3g' % worst)
    assert worst <= 1.0


def test_zero_variance_gives_nan_without_a_warning():
    from dgp_amd.sensitivity import indices_from_sums, SobolResult
    base = np.zeros((2, 1, 4))
    base[1, 0] = [1.0, 2.0, 3.0, 4.0]
    pair = np.ones((3, 2, 1, 2))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        first, total, V = indices_from_sums(base, pair, 10)
        res = SobolResult({'base': base, 'pair': pair, 'shift': np.zeros((2, 1))}, 10)
        s = res.summary()
        one = SobolResult({'base': base[:1], 'pair': pair[:, :1], 'shift': np.zeros((1, 1))}, 10).summary()
    assert V[0, 0] == 0.0 and np.all(np.isnan(first[:, 0])) and np.all(np.isnan(total[:, 0]))
    assert np.all(np.isfinite(first[:, 1])) and np.all(np.isfinite(total[:, 1]))
    assert np.array_equal(s['first']['mean'], res.first[:, :, 1])        # the NaN draw is left out
    assert np.all(np.isnan(one['total']['upper']))


def test_result_layout_and_summary():
    from dgp_amd.sensitivity import SobolResult, indices_from_sums
    rng = np.random.default_rng(1)
    D, P, K, B = 3, 6, 2, 50
    base = np.abs(rng.normal(size=(P, K, 4))) * [1.0, 1.0, 40.0, 40.0]
    pair, shift = rng.normal(size=(D, P, K, 2)), rng.normal(size=(P, K))
    res = SobolResult({'base': base, 'pair': pair, 'shift': shift}, B)
    first, total, V = indices_from_sums(base, pair, B)
    assert res.n_base == B and res.first.shape == res.total.shape == (K, D, P) and res.variance.shape == res.mean.shape == (K, P)
    for k in range(K):
        for i in range(D):
            assert np.array_equal(res.first[k, i], first[i, :, k]) and np.array_equal(res.total[k, i], total[i, :, k])
        assert np.array_equal(res.variance[k], V[:, k])
        assert np.array_equal(res.mean[k], shift[:, k] + (base[:, k, 0] + base[:, k, 1]) / (2 * B))
    s = res.summary(level=0.8)
    assert sorted(s) == ['first', 'total'] and sorted(s['first']) == ['lower', 'mean', 'upper']
    assert np.array_equal(s['total']['mean'], np.nanmean(res.total, -1))
    np.testing.assert_allclose(s['first']['lower'], np.nanquantile(res.first, 0.1, axis=-1), rtol=1e-13)
    np.testing.assert_allclose(s['first']['upper'], np.nanquantile(res.first, 0.9, axis=-1), rtol=1e-13)
    assert np.all(s['total']['lower'] <= s['total']['upper'])
    with pytest.raises(ValueError, match='level'):
        res.summary(level=1.0)
    one = SobolResult({'base': base[:, :1], 'pair': pair[:, :, :1], 'shift': shift[:, :1]}, B, squeeze=True)
    assert one.first.shape == (D, P) and one.variance.shape == (P,) and np.array_equal(one.first, res.first[0])
    assert one.summary()['first']['mean'].shape == (D,)


def _hollow(cls, **attrs):
    """An object of a paths class with the few attributes a refusal reads: a refusal comes before any device work."""
    obj = cls.__new__(cls)
    obj.__dict__.update(attrs)
    return obj


class _Node:
    def __init__(self, type):
        self.type = type


@pytest.mark.parametrize('who', ['gp', 'emulator'])
def test_sobol_refuses_bad_designs(who):
    from dgp_amd import pathfun
    obj = _hollow(pathfun.GpPaths) if who == 'gp' else _hollow(pathfun.PathFunctions, layers=[[_Node('gp')]])
    A = np.zeros((8, 3))
    with pytest.raises(Exception, match='2d-array'):
        obj.sobol(A[0], A[0])
    with pytest.raises(Exception, match='2d-array'):
        obj.sobol(A, A[0])
    with pytest.raises(ValueError, match='one shape'):
        obj.sobol(A, A[:7])
    with pytest.raises(ValueError, match='one shape'):
        obj.sobol(A, A[:, :2])
    with pytest.raises(ValueError, match='n_base must be at least 2'):
        obj.sobol(A[:1], A[:1])


def test_sobol_refuses_sampled_nodes_before_it_looks_at_the_design():
    from dgp_amd import pathfun
    obj = _hollow(pathfun.PathFunctions, layers=[[_Node('gp'), _Node('gp')], [_Node('likelihood')]])
    with pytest.raises(ValueError, match='drawn afresh on every evaluation'):
        obj.sobol(None, None)


def test_row_blocks_in_tiles(monkeypatch):
    """_row_blocks with multiple=64: the step is _rows_per_call's rounded down to a multiple of 64, at least 64; without it the
    step is what it was."""
    from dgp_amd import pathfun
    x = np.arange(300.0).reshape(300, 1)
    for step, want in ((7, 64), (64, 64), (70, 64), (200, 192), (1000, 960)):
        monkeypatch.setattr(pathfun, '_rows_per_call', lambda e, P, width: step)
        blocks = list(pathfun._row_blocks(None, x, 6, 10, multiple=64))
        assert [m0 for m0, _ in blocks] == list(range(0, 300, want))
        assert np.array_equal(np.concatenate([b for _, b in blocks]), x)
        assert [m0 for m0, _ in pathfun._row_blocks(None, x, 6, 10)] == list(range(0, 300, step))


def test_c_entries_refuse_before_any_launch():
    from dgp_amd import _lib
    lib = ctypes.CDLL(os.path.join(ROOT, 'dgp_amd', 'libdgp_amd.so'))
    for name in ('dgpamd_sobol_tiles', 'dgpamd_sobol_add'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.lib.dgpamd_sobol_tiles(None, 1, 1, 1, None, None, None, None, None) == _lib.BAD_ARG
    assert _lib.lib.dgpamd_sobol_add(None, 1, 1, None, None) == _lib.BAD_ARG


def test_reference_sums_are_exact():
    """sobol_ref on numbers whose sums are known: integers (every term exact in f64) and a cancelling pair that a f64 sum loses."""
    P, M, K = 2, 5, 1
    fA = np.arange(1.0, 11.0).reshape(P, M, K)
    fB = fA[::-1].copy()
    fAB = fA + 1.0
    shift = np.zeros((P, K))
    s, m = R.exact_sums(fA, fB, None, shift)
    assert [int(v) for v in s[0, 0]] == [15, 40, 55, 330] and np.array_equal(s, m)
    s, m = R.exact_sums(fA, fB, fAB, shift)
    assert [int(v) for v in s[0, 0]] == [40, 5] and [int(v) for v in s[1, 0]] == [15, 5]
    big = np.array([1e30, 1.0, -1e30]).reshape(1, 3, 1)
    s, m = R.exact_sums(big, big, None, np.zeros((1, 1)))
    assert s[0, 0, 0] == 1 and m[0, 0, 0] == 2 * Fraction(1e30) + 1
    assert R.worst_ratio(np.array([1.0]), s[0, 0, :1], m[0, 0, :1], 1) == 0.0
    one = np.array([Fraction(1)], dtype=object)
    assert R.worst_ratio(np.array([1.0 + 2.0**-48]), one, one, 1) > 1.0 > R.worst_ratio(np.array([1.0 + 2.0**-52]), one, one, 1) > 0.0


def test_the_statistical_tolerance_is_the_restatement_s_deviation():
    """tests/test_gpu_sobol_model.py takes twice STAT_CPU_DEVIATION as its tolerance: the number is what the numpy
    restatement gives here, without a device."""
    import test_gpu_sobol_model as T
    dev = np.abs(T.stat_restated() - T.STAT_ANALYTIC)
    print('restated deviations from 1/5, 4/5, 0: %s' % dev)
    assert abs(dev.max() - T.STAT_CPU_DEVIATION) <= 1e-6
