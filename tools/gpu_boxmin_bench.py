"""Minimising function-valued draws at the bench's model shape (profiles/boxmin_bench.txt; DESIGN I.17): n = 2000, d = 5 Matern
nodes -> one Matern node with `connect`, briefly trained; emulator(N=10); sample_size = 10 (100 paths), F = 2048; the box
[min X, max X]^5; R = 8 starts per path, fixed (the 8 best of 2048 candidates, screened once and passed as x0 to both arms).
  (a) paths.minimize(bounds, x0=x0): all 800 problems in lock-step on the device;
  (b) what a user writes without it: scipy L-BFGS-B per (path, start) on paths.value_and_grad at one row, keeping one column.
      Timed on the first 4 paths x 8 starts and SCALED by P / 4 (each call evaluates all P paths at the row whichever column is
      kept, so the cost per problem does not depend on how many paths are optimised).
Arms alternate; three rounds after a warm-up of each; medians.  Also: per-path best values of (a) against (b) on the paths (b)
ran; the share of (a) inside dgpamd_boxmin_step by device events around every call of one more run; rounds and evaluations per
problem; the time of the candidate screen.
Usage: python tools/gpu_boxmin_bench.py [file that also receives the lines]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None


def say(line):
    print(line, flush=True)
    if LOG:
        LOG.write(line + '\n')
        LOG.flush()


def timed(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def host_minimize(pf, bounds, x0, paths):
    """Best value per path of `paths`, the way a user writes it today."""
    from scipy.optimize import minimize
    best, calls = np.full(len(paths), np.inf), 0
    for i, p in enumerate(paths):
        def fun(x):
            v, g = pf.value_and_grad(x[None])
            return float(v[0][0, p]), g[0][0, :, p].copy()
        for s in x0[p]:
            r = minimize(fun, s, jac=True, method='L-BFGS-B', bounds=bounds, options=dict(gtol=1e-6, ftol=1e-12, maxiter=100))
            best[i] = min(best[i], r.fun)
            calls += r.nfev
    return best, calls


def main():
    import bench
    from dgp_amd import emulator, optimize
    n, d, N, J, F, R, NC, SUB = 2000, 5, 10, 10, 2048, 8, 2048, 4
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    pf = emu.sample_functions(sample_size=J, n_features=F)
    P = N * J
    bounds = np.stack((X.min(0), X.max(0)), 1)
    pf.minimize(bounds, n_starts=R, n_candidates=NC, seed=3, max_eval=1)                 # (warm)
    screen, t_screen = timed(lambda: pf.minimize(bounds, n_starts=R, n_candidates=NC, seed=3, max_eval=1))
    x0 = screen.x0
    cand = optimize.candidates(bounds[:, 0], bounds[:, 1], NC, 3)
    fc = pf(cand)[0]
    spread = fc.max(0) - fc.min(0)
    sub = list(range(SUB))
    legs = [('(a) paths.minimize, %d problems' % (P * R), lambda: pf.minimize(bounds, x0=x0)),
            ('(b) scipy per (path, start), %d paths' % SUB, lambda: host_minimize(pf, bounds, x0, sub))]
    res, (best_b, calls_b) = legs[0][1](), legs[1][1]()            # warm both
    say('n = %d, d = %d, %d paths, F = %d, %d starts per path (%d problems), box = the range of X' % (n, d, P, F, R, P * R))
    say('candidate screen (%d rows, all paths, one round of the loop included): %.1f ms' % (NC, t_screen))
    say('(a): %d rounds; per problem %.1f iterations (max %d), %.1f evaluations (max %d); statuses %s'
        % (res.rounds, res.n_iter.mean(), res.n_iter.max(), res.n_eval.mean(), res.n_eval.max(),
           {int(k): int(c) for k, c in zip(*np.unique(res.status, return_counts=True))}))
    diff = np.abs(res.fun[sub] - best_b) / spread[sub]
    say('per-path best of (a) against (b) on the %d paths of (b), same starts: %d of %d equal within 1e-6 of the spread; worst '
        'difference %.3g of the spread ((a) - (b) worst %.3g); (b) used %d evaluations'
        % (SUB, int((diff <= 1e-6).sum()), SUB, diff.max(), np.max(res.fun[sub] - best_b), calls_b))
    ms = np.zeros((3, 2))
    for rnd in range(3):
        for a, (name, f) in enumerate(legs):
            _, ms[rnd, a] = timed(f)
            say('round %d: %-44s %10.1f ms' % (rnd + 1, name, ms[rnd, a]))
    med = np.median(ms, 0)
    scaled = med[1] * P / SUB
    say('medians: (a) %.1f ms; (b) %.1f ms on %d paths, scaled by %d / %d: %.1f ms; (a) / (b) = %.4f'
        % (med[0], med[1], SUB, P, SUB, scaled, med[0] / scaled))
    spans = []
    step = e.boxmin_step

    def wrapped(*args, **kw):
        ev0, ev1 = e.event(), e.event()
        e.record(ev0)
        out = step(*args, **kw)
        e.record(ev1)
        spans.append((ev0, ev1))
        return out
    e.boxmin_step = wrapped
    _, whole = timed(legs[0][1])
    del e.boxmin_step
    inside = sum(e.elapsed_ms(a, c) for a, c in spans)
    say('(a) with events: %.1f ms; %d calls of boxmin_step: %.3f ms, %.2f %% of (a) (the rest: the walk at (P, R, Dx) rows)'
        % (whole, len(spans), inside, 100.0 * inside / whole))
    say('not measured: hardware counters, other D, history or check_every than the defaults, qmc starts')


if __name__ == '__main__':
    main()
