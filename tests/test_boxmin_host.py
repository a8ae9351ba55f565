"""The numpy restatement of the box-constrained minimiser (tests/boxmin_ref.py, DESIGN I.17) against scipy's L-BFGS-B on the
objectives of tests/test_gpu_boxmin.py, and the host side of the C ABI (workspace formula, bad-argument returns, status
numbers) through ctypes, without a device."""
import ctypes
import os
import re

import numpy as np
import pytest

import boxmin_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GTOL = 1e-6


def scipy_lbfgsb(fun, x0, lo, hi, gtol=GTOL):
    return R.scipy_lbfgsb(fun, x0, lo, hi, gtol)


QUADRATICS = [(D, seed, outside, history) for D in (1, 2, 5, 64) for seed, outside in ((0, False), (1, True), (2, True))
              for history in (1, 6)]


@pytest.mark.parametrize('D,seed,outside,history', QUADRATICS)
def test_quadratics_end_at_kkt_points_next_to_scipys(D, seed, outside, history):
    """Both minimisers end with max |P(x - g) - x| <= gtol, and on a strongly convex quadratic two such points lie within
    2 sqrt(D) gtol / lambda_min of each other (each within sqrt(D) gtol / lambda_min of the minimiser: the distance that a
    projected-gradient residual of gtol allows at curvature lambda_min)."""
    fun, lo, hi, lam = R.quadratic(D, seed, outside)
    x0 = np.random.default_rng(100 + seed).uniform(lo, hi)
    # (history 1 on the condition number 100 at D = 64 needs some hundreds of steps: the limits are not what is tested)
    res = R.minimize(fun, x0, lo, hi, history=history, maxiter=5000, max_eval=100000, gtol=GTOL, ftol=0.0)
    ref = scipy_lbfgsb(fun, x0, lo, hi)
    print('D %d outside %s history %d: status %d, %d iterations, %d evaluations; |x - x_scipy| %.3g, bound %.3g' %
          (D, outside, history, res['status'], res['n_iter'], res['n_eval'], np.max(np.abs(res['x'] - ref)), 2 * np.sqrt(D) * GTOL / lam))
    assert res['status'] == R.GTOL
    assert R.kkt(res['x'], fun(res['x'])[1], lo, hi) <= GTOL
    assert R.kkt(ref, fun(ref)[1], lo, hi) <= GTOL
    assert np.all(res['x'] >= lo) and np.all(res['x'] <= hi)
    assert np.all(np.diff(res['accepted']) <= 0.0)
    assert np.max(np.abs(res['x'] - ref)) <= 2 * np.sqrt(D) * GTOL / lam
    if outside and D > 1:
        assert np.any((res['x'] == lo) | (res['x'] == hi))     # (a bound is active, and met exactly)


@pytest.mark.parametrize('hi,xstar', [(2.0, (1.0, 1.0)), (0.5, (0.5, 0.25))])
@pytest.mark.parametrize('history', [1, 6])
def test_rosenbrock_inside_and_on_the_boundary(hi, xstar, history):
    lo, hi = np.full(2, -2.0), np.full(2, hi)
    x0 = np.array([-1.2, 0.4])
    res = R.minimize(R.rosenbrock, x0, lo, hi, history=history, maxiter=20000, max_eval=200000, gtol=GTOL, ftol=0.0)
    ref = scipy_lbfgsb(R.rosenbrock, x0, lo, hi)
    print('rosenbrock hi %.1f history %d: status %d, %d iterations, %d evaluations; x %s scipy %s' %
          (hi[0], history, res['status'], res['n_iter'], res['n_eval'], res['x'], ref))
    assert res['status'] == R.GTOL
    assert R.kkt(res['x'], R.rosenbrock(res['x'])[1], lo, hi) <= GTOL
    assert R.kkt(ref, R.rosenbrock(ref)[1], lo, hi) <= GTOL
    assert np.all(np.diff(res['accepted']) <= 0.0)
    # (the Hessian at either solution has a smallest eigenvalue of about 0.4 on the free coordinates: 1e-4 is far outside
    #  what gtol = 1e-6 allows and far inside the distance to any other stationary point)
    assert np.max(np.abs(res['x'] - np.array(xstar))) <= 1e-4 and np.max(np.abs(ref - np.array(xstar))) <= 1e-4


@pytest.mark.parametrize('D', [1, 2, 5, 64])
def test_linear_objective_ends_on_the_corner(D):
    for seed in range(5):                                          # (the five problems of the device test)
        fun, lo, hi, c = R.linear(D, seed)
        res = R.minimize(fun, np.zeros(D), lo, hi, gtol=GTOL)
        assert res['status'] == R.GTOL
        assert np.array_equal(res['x'], np.where(c > 0, lo, hi))   # every coordinate EQUAL to a bound
        ref = scipy_lbfgsb(fun, np.zeros(D), lo, hi)
        assert np.array_equal(ref, res['x'])


def test_special_starts_and_limits():
    fun, lo, hi, _ = R.quadratic(3, 5, False)
    xs = scipy_lbfgsb(fun, np.zeros(3), lo, hi)
    flat = lambda x: (1.0, np.zeros(3))
    res = R.minimize(flat, np.zeros(3), lo, hi)                    # g = 0 at the start
    assert (res['status'], res['n_iter'], res['n_eval']) == (R.GTOL, 0, 1)
    res = R.minimize(lambda x: (np.nan, np.zeros(3)), np.zeros(3), lo, hi)
    assert (res['status'], res['n_iter'], res['n_eval']) == (R.NAN, 0, 1)
    res = R.minimize(lambda x: (0.0, np.array([0.0, np.inf, 0.0])), np.zeros(3), lo, hi)
    assert res['status'] == R.NAN
    calls = []

    def nan_after_start(x):
        calls.append(1)
        return fun(x) if len(calls) == 1 else (np.nan, np.full(3, np.nan))
    res = R.minimize(nan_after_start, np.full(3, 0.9), lo, hi)     # NaN at every trial: never accepted, never loops
    assert (res['status'], res['n_iter'], res['n_eval']) == (R.LINESEARCH, 0, 1 + R.HALVINGS + 1)
    assert np.array_equal(res['x'], np.full(3, 0.9))
    res = R.minimize(fun, np.full(3, 0.9), lo, hi, maxiter=2)
    assert (res['status'], res['n_iter']) == (R.MAXITER, 2)
    res = R.minimize(fun, np.full(3, 0.9), lo, hi, max_eval=3)
    assert (res['status'], res['n_eval']) == (R.MAXEVAL, 3)
    res = R.minimize(fun, np.full(3, 0.9), lo, hi, max_eval=1)       # the start alone: finished all the same
    assert (res['status'], res['n_iter'], res['n_eval']) == (R.MAXEVAL, 0, 1) and np.array_equal(res['x'], np.full(3, 0.9))
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[1] = hi2[1] = 0.25                                         # lo_i = hi_i in one coordinate
    res = R.minimize(fun, np.array([0.9, 0.25, -0.9]), lo2, hi2)
    assert res['status'] == R.GTOL and res['x'][1] == 0.25
    ref = scipy_lbfgsb(fun, np.array([0.9, 0.25, -0.9]), lo2, hi2)
    assert np.max(np.abs(res['x'] - ref)) <= 2 * np.sqrt(3) * GTOL
    assert np.max(np.abs(xs)) < 1.0                                # (the unconstrained case above was inside the box)


# ---------------------------------------------------------------------- the C ABI without a device
def _lib():
    from dgp_amd import _lib
    return _lib


def test_workspace_formula():
    L = _lib()
    for Q, D, h in ((1, 1, 1), (130, 5, 6), (800, 64, 16), (65, 2, 1)):
        assert L.lib.dgpamd_boxmin_workspace(Q, D, h) == R.workspace_bytes(Q, D, h)
    for Q, D, h in ((0, 5, 6), (4, 0, 6), (4, 65, 6), (4, 5, 0), (4, 5, 17), (-1, 5, 6)):
        assert L.lib.dgpamd_boxmin_workspace(Q, D, h) == 0
    from dgp_amd.ops import Engine
    assert Engine.boxmin_workspace(130, 5, 6) == R.workspace_bytes(130, 5, 6)
    with pytest.raises(ValueError):
        Engine.boxmin_workspace(4, 65, 6)


def test_step_refuses_a_null_context_first():
    """The other host-side checks are exercised by tools/boxmin_args_check.cpp under the sanitizers."""
    L = _lib()
    assert L.lib.dgpamd_boxmin_step(None, 1, 1, 1, 0, 1.0, *[None] * 6, 6, 100, 420, 1e-6, 1e-12, 1, *[None] * 8) == L.BAD_ARG


def test_status_numbers_match_header_and_restatement():
    from dgp_amd.ops import Engine
    src = open(os.path.join(ROOT, 'include', 'dgp_amd.h')).read()
    header = {k.lower(): int(v) for k, v in re.findall(r'#define\s+DGPAMD_BOXMIN_([A-Z0-9_]+)\s+(\d+)', src)}
    count, maxhist = header.pop('count'), header.pop('maxhist')
    assert header == Engine.BOXMIN == R.STATUS and sorted(header.values()) == list(range(count)) and maxhist == 16


def test_quality_seed():
    """tests/test_gpu_boxmin_model.py holds the device to the restatement on the draws of QUALITY_SEED within 1e-6 of each
    draw's spread over the candidate rows: on that seed the restatement and scipy's L-BFGS-B, from the same starts, agree on
    every draw's best value within the same margin (the two find the same optima, so the margin tests the device alone)."""
    import test_gpu_boxmin_model as M
    lo, hi = M.BOX[:, 0], M.BOX[:, 1]
    funs, x0, spread = M.quality_case()
    ref = M.quality_best(funs, x0, lambda f, s: R.minimize(f, s, lo, hi)['fun'])
    sci = M.quality_best(funs, x0, lambda f, s: f(R.scipy_lbfgsb(f, s, lo, hi))[0])
    print('restatement against scipy: largest |difference| / spread %.3g (1e-6)' % np.max(np.abs(ref - sci) / spread))
    assert len(ref) == M.QUALITY['J'] and np.all(spread > 0.1)
    assert np.all(np.abs(ref - sci) <= 1e-6 * spread)
