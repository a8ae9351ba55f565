"""dgpamd_boxmin_step on the device (csrc/boxmin.hip, DESIGN I.17) as an operator: the test computes every problem's objective
and gradient on the host, in numpy, at the kernel's own trial points, round by round, and uploads them inside (Q, K) / (Q, K, D)
arrays whose other columns hold NaN -- they are not read.  Held against the numpy restatement tests/boxmin_ref.py (status,
n_iter, n_eval equal; the largest difference of a trial point is printed, not asserted) and against scipy's L-BFGS-B.
Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import boxmin_ref as R

pytestmark = pytest.mark.gpu
GTOL = 1e-6


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def run(eng, funs, x0, lo, hi, K=1, k=0, sign=1.0, restate=True, nan_trials=(), **kw):
    """Drive Q problems to their end: funs[q](x) -> (value of the 'draw', gradient); the kernel minimises sign * value.
    Checks on the way: every emitted trial lies in the box, the counter equals the number of unfinished problems after every
    call, the accepted values never increase.  nan_trials: problems that return NaN at every trial after the start.
    Returns the results as host arrays, the restatement's machines (or None) and the largest |trial - restatement's trial|."""
    import torch
    kw = dict(dict(history=6, maxiter=100, max_eval=420, gtol=GTOL, ftol=1e-12), **kw)
    history = kw.pop('history')
    Q, D = x0.shape
    state = eng.boxmin_state(Q, D, history, lo, hi)
    xt = eng.tensor(x0)
    trial = x0.copy()
    machines = [R.Machine(x0[q], lo, hi, history=history, **kw) for q in range(Q)] if restate else None
    accepted = [[] for _ in range(Q)]
    n_iter_before = np.zeros(Q, dtype=np.int64)
    worst, rounds = 0.0, 0
    running = Q
    while running:
        assert rounds < kw['max_eval'], 'a problem outlived max_eval'
        f, J = np.full((Q, K), np.nan), np.full((Q, K, D), np.nan)
        for q in range(Q):
            if q in nan_trials and rounds > 0:
                continue
            f[q, k], J[q, k] = funs[q](trial[q])       # (the 'draw': the kernel minimises sign * its value)
        if machines:
            for q, m in enumerate(machines):
                if m.status == R.RUNNING:
                    if q in nan_trials and rounds > 0:
                        m.step(np.nan, np.full(D, np.nan))
                    else:
                        v, g = funs[q](m.trial)
                        m.step(sign * v, sign * g)
        eng.boxmin_step(state, eng.tensor(f), eng.tensor(J), xt, k=k, sign=sign, first=rounds == 0, **kw)
        rounds += 1
        new_trial, status, n_iter = npy(xt), npy(state['status']), npy(state['n_iter'])
        assert np.all(new_trial >= lo) and np.all(new_trial <= hi), 'a trial point left the box'
        running = int(npy(state['running'])[0])
        assert running == int(np.sum(status == R.RUNNING)), 'the counter is not the number of unfinished problems'
        for q in np.nonzero((n_iter > n_iter_before) | (rounds == 1))[0]:
            accepted[q].append(sign * f[q, k])
        n_iter_before = n_iter.copy()
        if machines:
            worst = max(worst, max(float(np.max(np.abs(new_trial[q] - m.trial))) for q, m in enumerate(machines)))
        trial = new_trial
    for q in range(Q):
        assert np.all(np.diff(accepted[q]) <= 0.0) or np.any(np.isnan(accepted[q])), 'an accepted value went up'
    out = {name: npy(state[name]) for name in ('x', 'fun', 'status', 'n_iter', 'n_eval')}
    assert np.array_equal(trial, out['x'])             # a finished problem leaves x_trial = x
    return out, machines, worst, rounds


def same_counts(out, machines, what):
    ref = np.array([[m.status, m.n_iter, m.n_eval] for m in machines])
    got = np.stack([out['status'], out['n_iter'], out['n_eval']], 1)
    assert np.array_equal(got, ref), (what, np.nonzero(np.any(got != ref, 1))[0][:5], got[np.any(got != ref, 1)][:5],
                                      ref[np.any(got != ref, 1)][:5])


def quadratics(Q, D):
    """Problem q: quadratic number q, with its centre outside the box for odd q; starts uniform in the box."""
    made = [R.quadratic(D, q, q % 2 == 1) for q in range(Q)]
    lo, hi = made[0][1], made[0][2]
    x0 = np.random.default_rng(Q * 100 + D).uniform(lo, hi, (Q, D))
    return [m[0] for m in made], x0, lo, hi, np.array([m[3] for m in made])


@pytest.mark.parametrize('Q,D,history,K', [(1, 1, 1, 1), (63, 2, 6, 3), (64, 5, 1, 1), (65, 5, 6, 3), (130, 2, 1, 3), (130, 1, 6, 1),
                                           (5, 64, 6, 3), (3, 64, 1, 1)])
def test_quadratics_against_the_restatement_and_scipy(eng, Q, D, history, K):
    """Condition number 100, the centre inside the box and outside it (bounds active).  Every problem ends with status GTOL at
    a point whose projected-gradient residual, evaluated here in numpy, is <= gtol, within 2 sqrt(D) gtol / lambda_min of
    scipy's; status, n_iter and n_eval are the restatement's."""
    funs, x0, lo, hi, lam = quadratics(Q, D)
    out, machines, worst, rounds = run(eng, funs, x0, lo, hi, K=K, k=K - 1, history=history, maxiter=5000, max_eval=100000, ftol=0.0)
    print('Q %d D %d history %d: %d rounds, %d..%d iterations; largest |trial - restatement| %.3g' %
          (Q, D, history, rounds, out['n_iter'].min(), out['n_iter'].max(), worst))
    assert np.all(out['status'] == R.GTOL)
    same_counts(out, machines, 'quadratics')
    gap = 0.0
    for q in range(Q):
        v, g = funs[q](out['x'][q])
        assert R.kkt(out['x'][q], g, lo, hi) <= GTOL
        assert out['fun'][q] == v
        xs = R.scipy_lbfgsb(funs[q], x0[q], lo, hi, GTOL)
        assert R.kkt(xs, funs[q](xs)[1], lo, hi) <= GTOL
        d = np.max(np.abs(out['x'][q] - xs)) / (2 * np.sqrt(D) * GTOL / lam[q])
        gap = max(gap, d)
    print('largest |x - x_scipy| / bound: %.3g' % gap)
    assert gap <= 1.0


@pytest.mark.parametrize('top,xstar', [(2.0, (1.0, 1.0)), (0.5, (0.5, 0.25))])
def test_rosenbrock_inside_and_on_the_boundary(eng, top, xstar):
    Q = 65
    lo, hi = np.full(2, -2.0), np.full(2, top)
    x0 = np.random.default_rng(7).uniform(lo, np.minimum(hi, 0.4), (Q, 2))     # (left of the valley's bend: one basin)
    out, _, _, rounds = run(eng, [R.rosenbrock] * Q, x0, lo, hi, restate=False, maxiter=20000, max_eval=200000, ftol=0.0)
    print('rosenbrock to %.1f: %d rounds, statuses %s' % (top, rounds, np.bincount(out['status'], minlength=7)))
    assert np.all(out['status'] == R.GTOL)
    for q in range(Q):
        assert R.kkt(out['x'][q], R.rosenbrock(out['x'][q])[1], lo, hi) <= GTOL
    # (the smallest curvature on the free coordinates is about 0.4 at either solution: gtol = 1e-6 allows far less than 1e-4)
    assert np.max(np.abs(out['x'] - np.array(xstar))) <= 1e-4
    if top == 0.5:
        assert np.all(out['x'][:, 0] == 0.5)


@pytest.mark.parametrize('D', [1, 2, 5, 64])
@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_linear_objective_ends_on_the_corner(eng, D, sign):
    made = [R.linear(D, q) for q in range(5)]
    lo, hi = made[0][1], made[0][2]
    # sign -1: the kernel maximises the 'draw' -c^T x, which is the same problem; fun is the draw's own value
    funs = [(lambda x, f=m[0]: (sign * f(x)[0], sign * f(x)[1])) for m in made]
    out, machines, worst, _ = run(eng, funs, np.zeros((5, D)), lo, hi, K=3, k=1, sign=sign)
    assert np.all(out['status'] == R.GTOL)
    for q, m in enumerate(made):
        assert np.array_equal(out['x'][q], np.where(m[3] > 0, lo, hi))         # every coordinate EQUAL to a bound
        assert out['fun'][q] == funs[q](out['x'][q])[0]
    for q, m in enumerate(machines):                                            # (the restatement minimised sign * draw)
        assert (m.status, m.n_iter, m.n_eval) == (out['status'][q], out['n_iter'][q], out['n_eval'][q])
    print('linear D %d: largest |trial - restatement| %.3g' % (D, worst))


def test_special_starts_and_limits(eng):
    fun, lo, hi, _ = R.quadratic(3, 5, False)
    start = np.full((4, 3), 0.9)
    flat = lambda x: (1.0, np.zeros(3))
    out, _, _, rounds = run(eng, [flat] * 4, start, lo, hi)                     # g = 0 at the start
    assert rounds == 1 and np.all(out['status'] == R.GTOL) and np.all(out['n_iter'] == 0) and np.all(out['n_eval'] == 1)
    assert np.array_equal(out['x'], start) and np.all(out['fun'] == 1.0)
    bad = lambda x: (np.nan, np.zeros(3))
    inf_g = lambda x: (0.0, np.array([0.0, np.inf, 0.0]))
    out, machines, _, rounds = run(eng, [fun, bad, inf_g, fun], start, lo, hi)  # NaN at the start: NAN after one call
    assert np.array_equal(out['status'][1:3], [R.NAN, R.NAN]) and np.array_equal(out['n_eval'][1:3], [1, 1])
    assert np.isnan(out['fun'][1]) and np.array_equal(out['x'][1:3], start[1:3])
    same_counts(out, machines, 'nan at the start')
    out, machines, _, _ = run(eng, [fun] * 4, start, lo, hi, maxiter=2)
    assert np.all(out['status'] == R.MAXITER) and np.all(out['n_iter'] == 2)
    same_counts(out, machines, 'maxiter')
    out, machines, _, rounds = run(eng, [fun] * 4, start, lo, hi, max_eval=3)
    assert np.all(out['status'] == R.MAXEVAL) and np.all(out['n_eval'] == 3) and rounds == 3
    same_counts(out, machines, 'max_eval')
    out, machines, _, rounds = run(eng, [fun] * 4, start, lo, hi, max_eval=1)   # the start alone: finished all the same
    assert rounds == 1 and np.all(out['status'] == R.MAXEVAL) and np.array_equal(out['x'], start)
    assert np.all(out['fun'] == fun(start[0])[0])
    same_counts(out, machines, 'max_eval = 1')
    lo2, hi2 = lo.copy(), hi.copy()
    lo2[1] = hi2[1] = 0.25                                                      # lo_i = hi_i in one coordinate
    x0 = np.array([[0.9, 0.25, -0.9], [-0.3, 0.25, 0.2]])
    out, machines, _, _ = run(eng, [fun] * 2, x0, lo2, hi2)
    assert np.all(out['status'] == R.GTOL) and np.all(out['x'][:, 1] == 0.25)
    same_counts(out, machines, 'a fixed coordinate')
    for q in range(2):
        assert R.kkt(out['x'][q], fun(out['x'][q])[1], lo2, hi2) <= GTOL


def test_nan_at_every_trial_stays_in_its_lane(eng):
    """One problem of a wave returns NaN at every trial after its start: it ends with LINESEARCH at its start after
    1 + 21 evaluations, and the 64 other problems end with the bits of a run without it."""
    funs, x0, lo, hi, _ = quadratics(65, 5)
    clean, _, _, _ = run(eng, funs, x0, lo, hi, restate=False)
    out, machines, _, _ = run(eng, funs, x0, lo, hi, nan_trials={17})
    assert (out['status'][17], out['n_iter'][17], out['n_eval'][17]) == (R.LINESEARCH, 0, 1 + R.HALVINGS + 1)
    assert np.array_equal(out['x'][17], x0[17]) and out['fun'][17] == funs[17](x0[17])[0]
    same_counts(out, machines, 'nan at every trial')
    others = np.arange(65) != 17
    for name in ('x', 'fun', 'status', 'n_iter', 'n_eval'):
        assert np.array_equal(out[name][others], clean[name][others]), name


def test_slices_of_the_problems_reproduce_the_whole_run(eng):
    """No cross-lane operation: problems [0:1], [1:65], [65:130] of a 130-problem run, each run on its own (other lanes, other
    workgroups, another Q in every address), give the same x, fun, status, n_iter."""
    funs, x0, lo, hi, _ = quadratics(130, 5)
    whole, _, _, _ = run(eng, funs, x0, lo, hi, K=3, k=2, restate=False)
    assert len(set(whole['n_iter'])) > 3                                        # (the problems do not finish together)
    for a, c in ((0, 1), (1, 65), (65, 130)):
        part, _, _, _ = run(eng, funs[a:c], x0[a:c], lo, hi, K=1, k=0, restate=False)
        for name in ('x', 'fun', 'status', 'n_iter', 'n_eval'):
            assert np.array_equal(part[name], whole[name][a:c]), (name, a, c)


def test_bad_arguments_are_refused(eng):
    from dgp_amd import _lib
    from dgp_amd.ops import DgpAmdError
    lo, hi = -np.ones(2), np.ones(2)
    state = eng.boxmin_state(4, 2, 6, lo, hi)
    f, J, xt = eng.zeros(4, 1), eng.zeros(4, 1, 2), eng.zeros(4, 2)
    eng.boxmin_step(state, f, J, xt, first=True)                                # (the arguments below are otherwise good)
    for kw in (dict(k=1), dict(k=-1), dict(sign=0.5), dict(sign=float('nan')), dict(maxiter=0), dict(max_eval=0),
               dict(gtol=-1.0), dict(gtol=float('nan')), dict(ftol=-1e-3), dict(ftol=float('nan'))):
        with pytest.raises(DgpAmdError):
            eng.boxmin_step(state, f, J, xt, first=True, **kw)
    for h in (0, 17):                                                           # (the front refuses it with the workspace formula)
        with pytest.raises(ValueError):
            eng.boxmin_step(dict(state, history=h), f, J, xt, first=True)
        ptr = [t.data_ptr() for t in (f, J, state['lo'], state['hi'])]
        res = [state[n].data_ptr() for n in ('work', 'x', 'x', 'fun', 'status', 'n_iter', 'n_eval', 'running')]
        with pytest.raises(DgpAmdError):
            eng._chk(_lib.lib.dgpamd_boxmin_step(eng.h, 4, 2, 1, 0, 1.0, *ptr, state['lo_h'].ctypes.data, state['hi_h'].ctypes.data,
                                                 h, 100, 420, 1e-6, 1e-12, 1, *res))
    for blo, bhi in ((np.array([0.0, 1.0]), np.array([1.0, 0.5])), (np.array([np.nan, 0.0]), hi), (lo, np.array([1.0, np.nan]))):
        with pytest.raises(DgpAmdError):
            eng.boxmin_step(dict(state, lo_h=blo, hi_h=bhi), f, J, xt, first=True)
    with pytest.raises(ValueError):
        eng.boxmin_state(4, 65, 6, -np.ones(65), np.ones(65))
    with pytest.raises(ValueError):
        eng.boxmin_state(4, 2, 6, lo, np.ones(3))
    with pytest.raises(ValueError):
        eng.boxmin_step(state, f, eng.zeros(4, 1, 3), xt, first=True)
    with pytest.raises(ValueError):
        eng.boxmin_step(state, f.float(), J, xt, first=True)
    with pytest.raises(ValueError):
        eng.boxmin_step(state, eng.zeros(4, 2)[:, :1], J, xt, first=True)       # (not contiguous)
    with pytest.raises(ValueError):
        eng.boxmin_step(state, eng.zeros(5, 1), eng.zeros(5, 1, 2), eng.zeros(5, 2), first=True)   # (another Q than the state's)
