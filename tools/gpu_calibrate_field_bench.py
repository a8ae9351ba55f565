"""Field calibration at the bench's model shape (profiles/calibrate_field_bench.txt; DESIGN I.24): the model, draws, box and
starts of tools/gpu_calibrate_bench.py (n = 2000, d = 5, 100 paths, F = 2048, R = 4 chains per path); columns 0 and 1 of the
input are controls at T sites spread over their range, columns 2 .. 4 are calibrated; y is the mean of the draws at the sites with
the calibration columns at the middle of the box, obs_sd a tenth of the draws' spread, obs_cov a squared-exponential covariance
of that size over the sites.
Arms, alternating in one session, three rounds after a warm-up of each, medians, per round of the lock-step loop:
  (0) paths.calibrate without controls (the unchanged path: the parent's reference);
  (T) with T = 1, 8, 64 sites.
Then, for every T, one more run with device events around every call of Engine.boxsites_fold and of Engine.boxmala_step: their
shares of a round (the rest is the walk at Q T per-path rows and the indexed copy of the calibration columns).
Usage: python tools/gpu_calibrate_field_bench.py [file that also receives the lines]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from gpu_calibrate_bench import say, timed      # noqa: E402  (its LOG is opened from the same argument)

WARMUP, SAMPLES = 10, 20
SITES = (1, 8, 64)


def main():
    import bench
    from dgp_amd import emulator, optimize
    n, d, N, J, F, R, NC = 2000, 5, 10, 10, 2048, 4, 2048
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    pf = emu.sample_functions(sample_size=J, n_features=F)
    P = N * J
    bounds = np.stack((X.min(0), X.max(0)), 1)
    mid = bounds.mean(1)
    fc = pf(optimize.candidates(bounds[:, 0], bounds[:, 1], NC, 3))[0]
    sd = 0.1 * float(np.median(fc.max(0) - fc.min(0)))
    kw = dict(n_chains=R, n_samples=SAMPLES, warmup=WARMUP, seed=3)
    rounds = 1 + WARMUP + SAMPLES
    cc, th = [0, 1], [2, 3, 4]
    x0 = np.random.default_rng(5).uniform(bounds[:, 0], bounds[:, 1], (R, d))
    legs = [('(0) no controls, %d chains' % (P * R), lambda: pf.calibrate(float(pf(mid[None])[0].mean()), sd, bounds, x0=x0, **kw))]
    field = {}
    for T in SITES:
        u = np.random.default_rng(T).uniform(size=(T, 2))
        controls = bounds[cc, 0] + u * (bounds[cc, 1] - bounds[cc, 0])
        rows = np.tile(mid, (T, 1))
        rows[:, cc] = controls
        y = pf(rows)[0].mean(1)[:, None]
        dist = np.sum(((controls[:, None] - controls[None]) / (bounds[cc, 1] - bounds[cc, 0])) ** 2, -1)
        fkw = dict(controls=controls, control_columns=cc, obs_cov=sd * sd * np.exp(-dist / (2.0 * 0.3 ** 2)))
        field[T] = lambda y=y, fkw=fkw: pf.calibrate(y, sd, bounds[th], x0=x0[:, th], **kw, **fkw)
        legs.append(('(%d) %d sites, K\' = %d' % (T, T, T), field[T]))
    say('n = %d, d = %d, %d paths, F = %d, %d chains per path (%d chains), %d rounds per run, obs_sd = %.4g; controls: columns %s'
        % (n, d, P, F, R, P * R, rounds, sd, cc))
    for name, f in legs:                                                         # warm every arm
        res = f()
        say('%s: warm; acceptance %.2f .. %.2f, statuses %s' % (name, res.accept_rate.min(), res.accept_rate.max(),
                                                               {int(k): int(c) for k, c in zip(*np.unique(res.status, return_counts=True))}))
    ms = np.zeros((3, len(legs)))
    for rnd in range(3):
        for a, (name, f) in enumerate(legs):
            _, ms[rnd, a] = timed(f)
            say('round %d: %-28s %10.1f ms, %.3f ms per round' % (rnd + 1, name, ms[rnd, a], ms[rnd, a] / rounds))
    med = np.median(ms, 0) / rounds
    say('medians per round: ' + '; '.join('%s %.3f ms' % (name.split(' ')[0], m) for (name, _), m in zip(legs, med)))
    say('a round with T sites against T rounds without controls: ' +
        '; '.join('T = %d: %.3f' % (T, med[1 + i] / (T * med[0])) for i, T in enumerate(SITES)))
    for i, T in enumerate(SITES):
        spans = {'boxsites_fold': [], 'boxmala_step': []}
        for name in spans:
            def wrapped(*args, _f=getattr(e, name), _s=spans[name], **kw2):
                ev0, ev1 = e.event(), e.event()
                e.record(ev0)
                out = _f(*args, **kw2)
                e.record(ev1)
                _s.append((ev0, ev1))
                return out
            setattr(e, name, wrapped)
        _, whole = timed(field[T])
        for name in spans:
            delattr(e, name)
        inside = {name: sum(e.elapsed_ms(a, c) for a, c in s) for name, s in spans.items()}
        lane = [s for s in spans['boxsites_fold']][-rounds:]                      # (the folds of the loop; the screen's come first)
        fold_loop = sum(e.elapsed_ms(a, c) for a, c in lane)
        say('T = %d with events: %.1f ms; %d folds %.3f ms (%.2f %% of the run; the loop\'s %d: %.3f ms, %.4f ms each); %d steps '
            '%.3f ms (%.2f %%, %.4f ms each); fold + step = %.2f %% of the run'
            % (T, whole, len(spans['boxsites_fold']), inside['boxsites_fold'], 100.0 * inside['boxsites_fold'] / whole, len(lane),
               fold_loop, fold_loop / max(len(lane), 1), len(spans['boxmala_step']), inside['boxmala_step'],
               100.0 * inside['boxmala_step'] / whole, inside['boxmala_step'] / max(len(spans['boxmala_step']), 1),
               100.0 * (inside['boxsites_fold'] + inside['boxmala_step']) / whole))
    say('not measured: hardware counters of the fold, HMC and SMC arms, other Dt or K, T between 64 and 256, the candidate screen')


if __name__ == '__main__':
    main()
