"""Minimising function-valued posterior draws over a box, on the device (paths.minimize, emulator.thompson, gp.thompson;
DESIGN I.17).

Every draw of emulator.sample_functions / gp.sample_functions is a closed-form function of x with a closed-form gradient, so
its optimum over a box can be found by a gradient method.  The argmin of one fresh draw is a Thompson-sampling proposal for
Bayesian optimisation; the spread of argmin and min over many draws is the posterior of the minimiser and of the minimum.
P draws from R starts each are P R independent problems.  They advance in lock-step: a round evaluates every problem's trial
point through the layer walk at per-path rows (P, R, Dx), values and Jacobian, and dgpamd_boxmin_step (a projected L-BFGS,
one lane per problem) turns them into the next trial points.  Nothing but the count of running problems, every check_every
rounds, leaves the device until the end.  The starts are the best of n_candidates rows in the box, screened through the
shared-rows walk.
"""
import warnings

import numpy as np
import torch

from . import pathfun
from .ops import Engine

STATUS = Engine.BOXMIN


def check_bounds(bounds, Dx, what='minimize'):
    """bounds (Dx, 2) = [[low, high], ...] as (lo, hi); low == high fixes a column.  what: the caller named in a refusal."""
    bounds = np.asarray(bounds, dtype=np.float64)
    if bounds.ndim != 2 or bounds.shape[1] != 2 or bounds.shape[0] < 1:
        raise ValueError(what + ': bounds must be (Dx, 2), one [low, high] per input')
    if Dx is not None and bounds.shape[0] != Dx:
        raise ValueError(what + ': bounds has %d rows, the draws have %d inputs' % (bounds.shape[0], Dx))
    if not np.all(np.isfinite(bounds)) or np.any(bounds[:, 1] < bounds[:, 0]):
        raise ValueError(what + ': every bound must be finite with low <= high')
    if bounds.shape[0] > 64:
        raise ValueError(what + ': at most 64 inputs')
    return np.ascontiguousarray(bounds[:, 0]), np.ascontiguousarray(bounds[:, 1])


def candidates(lo, hi, n, seed=None, qmc=False, what='minimize'):
    """n rows in the box: np.random.default_rng(seed).uniform(size=(n, Dx)), or with qmc the first n points (a power of two)
    of scipy's scrambled Sobol' sequence, as sensitivity.saltelli_design takes its base samples."""
    n, D = int(n), len(lo)
    if n < 1:
        raise ValueError(what + ': n_candidates must be at least 1')
    if qmc:
        if n & (n - 1):
            raise ValueError(what + ': qmc=True needs n_candidates a power of two, got %d' % n)
        from scipy.stats import qmc as _qmc
        u = _qmc.Sobol(d=D, scramble=True, seed=seed).random_base2(n.bit_length() - 1)
    else:
        u = np.random.default_rng(seed).uniform(size=(n, D))
    return np.minimum(np.maximum(lo + (hi - lo) * u, lo), hi)


def best_candidates(e, values, cand, P, R, width, sign):
    """(P, R, Dx) host array: per path the R rows of cand (n, Dx) with the smallest sign * values, by a stable sort -- ties
    go to the lower row, and the blocks of rows do not change the choice.  values(xd (M, Dx)) -> (P, M) device tensor."""
    if R > len(cand):
        raise ValueError('minimize: n_starts = %d is more than n_candidates = %d' % (R, len(cand)))
    f = e.empty(P, len(cand))
    for m0, xb in pathfun._row_blocks(e, cand, P, width):
        f[:, m0:m0 + len(xb)] = values(e.tensor(xb))
    order = torch.sort(f if sign > 0 else -f, dim=1, stable=True)[1][:, :R].cpu().numpy()   # (NaN sorts last)
    return cand[order]


class PathOptimum:
    """The optima of P function-valued draws from R starts each.  x (P, Dx), fun (P,): each draw's best start (maximize: its
    largest value; fun is the draw's own value either way); start (P,) which one that was; success (P,): it ended at a
    Karush-Kuhn-Tucker point of the box, max |P(x - grad) - x| <= gtol (status 'gtol').  x_all (P, R, Dx), fun_all, status,
    n_iter, n_eval (P, R): every start; status holds the numbers of optimize.STATUS (= Engine.BOXMIN, DGPAMD_BOXMIN_*):
    gtol 1 converged; ftol 2 the decrease of an accepted step fell below ftol; maxiter 3; maxeval 4; linesearch 5 no lower
    point along the steepest-descent arc (x is the last accepted point); nan 6 the start's value or gradient was not finite.
    x0 (P, R, Dx): the starts.  rounds: the evaluations of the lock-step loop.  Column p of a result is path p of the draws' container (s * sample_size
    + j for an emulator)."""

    def __init__(self, x0, x_all, fun_all, status, n_iter, n_eval, sign, rounds):
        self.x0, self.x_all, self.fun_all, self.status, self.n_iter, self.n_eval, self.rounds = x0, x_all, fun_all, status, n_iter, n_eval, rounds
        key = np.where(np.isnan(fun_all), np.inf, sign * fun_all)
        self.start = np.argmin(key, 1)
        rows = np.arange(len(key))
        self.x, self.fun = x_all[rows, self.start], fun_all[rows, self.start]
        self.success = status[rows, self.start] == STATUS['gtol']

    def summary(self, level=0.95):
        """{'x': {'mean', 'lower', 'upper'} (Dx,), 'fun': {...} scalars}: the mean over the draws and the equal-tailed
        interval of probability `level` of the minimiser and of the minimum (draws without a finite optimum are left out)."""
        if not 0.0 < level < 1.0:
            raise ValueError('summary: level must lie in (0, 1)')
        tail = 0.5 * (1.0 - level)
        out = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)
            ok = np.isfinite(self.fun)
            for name, a in (('x', np.where(ok[:, None], self.x, np.nan)), ('fun', np.where(ok, self.fun, np.nan))):
                out[name] = {'mean': np.nanmean(a, 0), 'lower': np.nanquantile(a, tail, axis=0),
                             'upper': np.nanquantile(a, 1.0 - tail, axis=0)}
        return out


def minimize(e, P, K, Dx, values, value_and_jac, width, bounds, n_starts=8, n_candidates=2048, output=0, maximize=False, x0=None,
             seed=None, qmc=False, maxiter=100, gtol=1e-6, ftol=1e-12, history=6, check_every=8, max_eval=None):
    """The driver behind PathFunctions.minimize and GpPaths.minimize.  values(xd (M, Dx)) -> (P, M, K) device tensor, the
    draws at shared rows; value_and_jac(xt (P, R, Dx)) -> ((P, R, K), (P, R, K, Dx)) contiguous device tensors, every draw
    and its Jacobian at rows of its own; width: doubles per row and path of values (pathfun._row_blocks)."""
    lo, hi = check_bounds(bounds, Dx)
    output, maxiter, check_every = int(output), int(maxiter), max(1, int(check_every))
    if not 0 <= output < K:
        raise ValueError('minimize: output = %d, the draws have %d outputs' % (output, K))
    if maxiter < 1 or not gtol >= 0.0 or not ftol >= 0.0 or not 1 <= int(history) <= 16:
        raise ValueError('minimize: need maxiter >= 1, gtol >= 0, ftol >= 0 and 1 <= history <= 16')
    max_eval = 4 * maxiter + 20 if max_eval is None else int(max_eval)
    if max_eval < 1:
        raise ValueError('minimize: need max_eval >= 1')
    sign = -1.0 if maximize else 1.0
    if x0 is None:
        R = int(n_starts)
        if R < 1:
            raise ValueError('minimize: n_starts must be at least 1')
        cand = candidates(lo, hi, n_candidates, seed, qmc)
        x0 = best_candidates(e, lambda xd: values(xd)[:, :, output], cand, P, R, width, sign)
    else:
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.ndim == 2:
            x0 = np.broadcast_to(x0, (P,) + x0.shape)
        if x0.ndim != 3 or x0.shape[0] != P or x0.shape[1] < 1 or x0.shape[2] != Dx or np.any(np.isnan(x0)):
            raise ValueError('minimize: x0 must be (R, Dx) or (P, R, Dx) = (%d, R, %d) without NaN' % (P, Dx))
        x0 = np.minimum(np.maximum(x0, lo), hi)     # (a start outside the box begins at its projection)
        R = x0.shape[1]
    xt = e.tensor(np.ascontiguousarray(x0))
    state = e.boxmin_state(P * R, Dx, history, lo, hi)
    rounds = 0
    while rounds < max_eval:
        f, J = value_and_jac(xt)
        e.boxmin_step(state, f, J, xt, k=output, sign=sign, maxiter=maxiter, max_eval=max_eval, gtol=gtol, ftol=ftol,
                      first=rounds == 0)
        rounds += 1
        if rounds % check_every == 0 and int(state['running'].cpu()[0]) == 0:
            break
    # (a problem still running after max_eval rounds has had max_eval evaluations: the step has ended it with 'maxeval')
    host = {k: state[k].cpu().numpy() for k in ('x', 'fun', 'status', 'n_iter', 'n_eval')}
    return PathOptimum(np.array(x0), host['x'].reshape(P, R, Dx), host['fun'].reshape(P, R), host['status'].reshape(P, R),
                       host['n_iter'].reshape(P, R), host['n_eval'].reshape(P, R), sign, rounds)


def thompson_rows(res, batch_size, N, J):
    """X_new (batch_size, Dx) of emulator.thompson: row b is the optimum of path (b mod N) J + b div N, so that a batch spreads
    over the imputations first."""
    b = np.arange(int(batch_size))
    return res.x[(b % N) * J + b // N].copy()
