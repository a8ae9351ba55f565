"""Calibrating function-valued draws at the bench's model shape (profiles/calibrate_bench.txt; DESIGN I.19): n = 2000, d = 5
Matern nodes -> one Matern node with `connect`, briefly trained; emulator(N=10); sample_size = 10 (100 paths), F = 2048; the
box [min X, max X]^5; the observation is the mean of the draws at the middle of the box, obs_sd a tenth of the draws' spread
over 2048 rows; R = 4 chains per path from fixed starts (screened once and passed as x0 to both arms); WARMUP warm-up rounds
and SAMPLES samples, thin 1.
  (a) paths.calibrate(y, obs_sd, bounds, x0=x0): all 400 chains in lock-step on the device;
  (b) what a user writes without it: the same MALA (the same proposal, acceptance and warm-up gain, numpy's generator) per
      (path, chain) on paths.value_and_grad at one row, keeping one column.  Timed on the first 4 paths x 4 chains and SCALED
      by P / 4 (each call evaluates all P paths at the row whichever column is kept, so the cost per chain does not depend on
      how many paths are calibrated).
Arms alternate; three rounds after a warm-up of each; medians.  Also: the share of (a) inside dgpamd_boxmala_step by device
events around every call of one more run; the cost of drawing and uploading the random numbers; acceptance rates, steps, split
R-hat and ess of (a); the pooled mean of (a) against (b)'s on the paths (b) ran.
With --long: arm (a) alone at 500 + 500 (the defaults) and 500 + 2000 rounds, its time and diagnostics, appended to the file.
With --hmc (profiles/calibrate_hmc_bench.txt; DESIGN I.20): method='hmc' beside method='mala' on the same model, starts and
seed, at EQUAL numbers of walk evaluations -- the HMC arm's warm-up and sample iterations are the most whose trajectories fit
into MALA's warm-up and sampling rounds.  Timing: the two arms alternate at 100 + 100 rounds, three rounds after a warm-up of
each, medians, per walk evaluation; the step kernel's share of the HMC arm by device events.  Mixing: one run of each at
500 + 2000 rounds (the runs are deterministic): acceptance, adapted steps, split R-hat, ess per draw and ESS PER WALK
EVALUATION, and the ratio of the two methods' medians.
Usage: python tools/gpu_calibrate_bench.py [--long | --hmc] [file that also receives the lines]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LONG = '--long' in sys.argv[1:]
HMC = '--hmc' in sys.argv[1:]
FILES = [a for a in sys.argv[1:] if a not in ('--long', '--hmc')]
LOG = open(FILES[0], 'a' if LONG else 'w') if FILES else None
WARMUP, SAMPLES = 100, 100


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


def host_mala(pf, y, sd, bounds, x0, paths, seed=0):
    """Samples (len(paths), R, SAMPLES, Dx) of the same sampler, the way a user writes it today."""
    from dgp_amd import calibrate
    lo, hi = bounds[:, 0], bounds[:, 1]
    s, w = hi - lo, 1.0 / sd ** 2
    rng = np.random.default_rng(seed)
    out, calls = np.empty((len(paths), x0.shape[1], SAMPLES, len(lo))), 0
    for i, p in enumerate(paths):
        def target(x):
            v, g = pf.value_and_grad(x[None])
            r = y - float(v[0][0, p])
            return -0.5 * w * r * r, w * r * g[0][0, :, p]
        for c, start in enumerate(x0[p]):
            x, h = start.copy(), 0.1
            lp, g = target(x)
            calls += 1
            for rnd in range(WARMUP + SAMPLES):
                mean = x + 0.5 * h * h * s * s * g
                xp = mean + h * s * rng.standard_normal(len(x))
                acc = False
                if np.all(xp >= lo) and np.all(xp <= hi):
                    lpp, gp = target(xp)
                    calls += 1
                    back = xp + 0.5 * h * h * s * s * gp
                    lr = lpp - lp - 0.5 * np.sum(((x - back) / (h * s)) ** 2) + 0.5 * np.sum(((xp - mean) / (h * s)) ** 2)
                    acc = np.log(rng.random()) < lr
                    if acc:
                        x, lp, g = xp, lpp, gp
                if rnd < WARMUP:
                    up, down = calibrate.gain(rnd, 0.574)
                    h = min(max(h * (up if acc else down), calibrate.HMIN), calibrate.HMAX)
                else:
                    out[i, c, rnd - WARMUP] = x
    return out, calls


def hmc_counts(seed, warm_rounds, sample_rounds, n_leapfrog=8):
    """(warm-up iterations, sample iterations) of the HMC arm: the most whose trajectories fit into warm_rounds and then
    sample_rounds walk evaluations."""
    from dgp_amd import calibrate
    spent = np.cumsum(calibrate.trajectory_lengths(seed, warm_rounds + sample_rounds, n_leapfrog, True))
    warm = int(np.searchsorted(spent, warm_rounds, 'right'))
    return warm, int(np.searchsorted(spent, spent[warm - 1] + sample_rounds, 'right')) - warm


def diagnostics(name, res, ms=None):
    per_eval = res.ess / res.evaluations
    say('%s: %d walk evaluations, %d samples per chain%s; acceptance %.2f .. %.2f (median %.2f); steps %.3g .. %.3g (median %.3g)'
        % (name, res.evaluations, res.x.shape[2], '' if ms is None else ', %.1f ms' % ms, res.accept_rate.min(), res.accept_rate.max(),
           np.median(res.accept_rate), res.step.min(), res.step.max(), np.median(res.step)))
    say('%s: split R-hat median %.3f, max %.3f; ess per draw and input (of %d samples) median %.0f, min %.0f; ess per walk evaluation '
        'median %.4f, min %.4f' % (name, np.nanmedian(res.rhat), np.nanmax(res.rhat), res.x.shape[1] * res.x.shape[2],
                                   np.nanmedian(res.ess), np.nanmin(res.ess), np.nanmedian(per_eval), np.nanmin(per_eval)))
    return per_eval


def hmc_arm(pf, e, y, sd, bounds, x0, seed=3):
    """The --hmc report."""
    def mala(warm, samples):
        return pf.calibrate(y, sd, bounds, x0=x0, seed=seed, warmup=warm, n_samples=samples)

    def hmc(warm, samples):
        w, s = hmc_counts(seed, warm, samples)
        return pf.calibrate(y, sd, bounds, x0=x0, seed=seed, warmup=w, n_samples=s, method='hmc')
    legs = [('mala', lambda: mala(WARMUP, SAMPLES)), ('hmc', lambda: hmc(WARMUP, SAMPLES))]
    evals = [f().evaluations for _, f in legs]                    # warm both
    say('timing at %d + %d rounds: mala %d walk evaluations, hmc %d (%d + %d iterations of 1 .. 8 leapfrog steps)'
        % ((WARMUP, SAMPLES, evals[0], evals[1]) + hmc_counts(seed, WARMUP, SAMPLES)))
    ms = np.zeros((3, 2))
    for rnd in range(3):
        for a, (name, f) in enumerate(legs):
            _, ms[rnd, a] = timed(f)
            say('round %d: %-5s %10.1f ms, %.3f ms per walk evaluation' % (rnd + 1, name, ms[rnd, a], ms[rnd, a] / evals[a]))
    med = np.median(ms, 0)
    say('medians per walk evaluation: mala %.3f ms, hmc %.3f ms; hmc / mala = %.4f' % (med[0] / evals[0], med[1] / evals[1],
                                                                                     med[1] / evals[1] * evals[0] / med[0]))
    spans = []
    step = e.boxhmc_step

    def wrapped(*args, **kw):
        ev0, ev1 = e.event(), e.event()
        e.record(ev0)
        out = step(*args, **kw)
        e.record(ev1)
        spans.append((ev0, ev1))
        return out
    e.boxhmc_step = wrapped
    _, whole = timed(legs[1][1])
    del e.boxhmc_step
    inside = sum(e.elapsed_ms(a, c) for a, c in spans)
    say('hmc with events: %.1f ms; %d calls of boxhmc_step: %.3f ms, %.2f %% of the run (the rest: the walk at (P, R, Dx) rows)'
        % (whole, len(spans), inside, 100.0 * inside / whole))
    for warm, samples in ((500, 500), (500, 2000)):
        say('mixing at %d + %d rounds, hmc %d + %d iterations:' % ((warm, samples) + hmc_counts(seed, warm, samples)))
        a, ms_a = timed(lambda: mala(warm, samples))
        b, ms_b = timed(lambda: hmc(warm, samples))
        pa, pb = diagnostics('mala', a, ms_a), diagnostics('hmc ', b, ms_b)
        say('ess per walk evaluation, hmc / mala: of the medians %.3f, of the minima %.3f; per draw and input: median %.3f, '
            'quartiles %.3f .. %.3f, hmc ahead in %d of %d' % ((np.nanmedian(pb) / np.nanmedian(pa), np.nanmin(pb) / np.nanmin(pa),
                                                               np.nanmedian(pb / pa)) + tuple(np.nanquantile(pb / pa, [0.25, 0.75]))
                                                              + (int(np.sum(pb > pa)), pa.size)))
        say('pooled means: mala %s, hmc %s' % (np.round(a.summary()['mean'], 3), np.round(b.summary()['mean'], 3)))
    say('not measured: hardware counters, other n_leapfrog, jitter off, other D or chain counts, thin > 1, a prior')


def main():
    import bench
    from dgp_amd import calibrate, emulator, optimize
    n, d, N, J, F, R, NC, SUB = 2000, 5, 10, 10, 2048, 4, 2048, 4
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    pf = emu.sample_functions(sample_size=J, n_features=F)
    P = N * J
    bounds = np.stack((X.min(0), X.max(0)), 1)
    fc = pf(optimize.candidates(bounds[:, 0], bounds[:, 1], NC, 3))[0]
    y, sd = float(pf(bounds.mean(1)[None])[0].mean()), 0.1 * float(np.median(fc.max(0) - fc.min(0)))
    kw = dict(n_chains=R, n_samples=SAMPLES, warmup=WARMUP, seed=3)
    pf.calibrate(y, sd, bounds, n_candidates=NC, **dict(kw, n_samples=1, warmup=0))       # (warm)
    screen, t_screen = timed(lambda: pf.calibrate(y, sd, bounds, n_candidates=NC, **dict(kw, n_samples=1, warmup=0)))
    x0 = screen.x0
    if HMC:
        say('n = %d, d = %d, %d paths, F = %d, %d chains per path (%d chains), box = the range of X, y = %.4g, obs_sd = %.4g'
            % (n, d, P, F, R, P * R, y, sd))
        return hmc_arm(pf, e, y, sd, bounds, x0)
    if LONG:
        for warm, samples in ((500, 500), (500, 2000)):
            long, ms_long = timed(lambda: pf.calibrate(y, sd, bounds, x0=x0, **dict(kw, warmup=warm, n_samples=samples)))
            say('(a) alone, %d warm-up rounds + %d samples: %.1f ms; acceptance %.2f .. %.2f (median %.2f); steps %.3g .. %.3g; split '
                'R-hat median %.3f, max %.3f; ess per draw (of %d samples) median %.0f, min %.0f'
                % (warm, samples, ms_long, long.accept_rate.min(), long.accept_rate.max(), np.median(long.accept_rate),
                   long.step.min(), long.step.max(), np.nanmedian(long.rhat), np.nanmax(long.rhat), R * samples,
                   np.nanmedian(long.ess), np.nanmin(long.ess)))
        return
    sub = list(range(SUB))
    legs = [('(a) paths.calibrate, %d chains' % (P * R), lambda: pf.calibrate(y, sd, bounds, x0=x0, **kw)),
            ('(b) host MALA per (path, chain), %d paths' % SUB, lambda: host_mala(pf, y, sd, bounds, x0, sub))]
    res, (xs_b, calls_b) = legs[0][1](), legs[1][1]()              # warm both
    say('n = %d, d = %d, %d paths, F = %d, %d chains per path (%d chains), %d warm-up rounds + %d samples, box = the range of X, '
        'y = %.4g, obs_sd = %.4g' % (n, d, P, F, R, P * R, WARMUP, SAMPLES, y, sd))
    say('candidate screen (%d rows, all paths, two rounds of the loop included): %.1f ms' % (NC, t_screen))
    say('(a): %d rounds; acceptance after warm-up %.2f .. %.2f (median %.2f); steps %.3g .. %.3g; statuses %s'
        % (res.rounds, res.accept_rate.min(), res.accept_rate.max(), np.median(res.accept_rate), res.step.min(), res.step.max(),
           {int(k): int(c) for k, c in zip(*np.unique(res.status, return_counts=True))}))
    say('(a): split R-hat median %.3f, max %.3f; ess per draw (of %d samples) median %.0f, min %.0f'
        % (np.nanmedian(res.rhat), np.nanmax(res.rhat), R * SAMPLES, np.nanmedian(res.ess), np.nanmin(res.ess)))
    summ = res.summary()
    say('(a): pooled mean %s; spread of the per-draw means %s' % (np.round(summ['mean'], 3), np.round(summ['draw_sd'], 3)))
    say('pooled mean over the %d paths of (b): (a) %s, (b) %s (other random numbers: not the same chains); (b) used %d evaluations'
        % (SUB, np.round(res.x[sub].reshape(-1, d).mean(0), 3), np.round(xs_b.reshape(-1, d).mean(0), 3), calls_b))
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
    step = e.boxmala_step

    def wrapped(*args, **kw):
        ev0, ev1 = e.event(), e.event()
        e.record(ev0)
        out = step(*args, **kw)
        e.record(ev1)
        spans.append((ev0, ev1))
        return out
    e.boxmala_step = wrapped
    _, whole = timed(legs[0][1])
    del e.boxmala_step
    inside = sum(e.elapsed_ms(a, c) for a, c in spans)
    say('(a) with events: %.1f ms; %d calls of boxmala_step: %.3f ms, %.2f %% of (a) (the rest: the walk at (P, R, Dx) rows)'
        % (whole, len(spans), inside, 100.0 * inside / whole))
    total = 1 + WARMUP + SAMPLES
    (zb, ub), t_draw = timed(lambda: calibrate.Streams(3, P, R, d).block(total))
    _, t_up = timed(lambda: (e.tensor(zb), e.tensor(ub)))
    say('random numbers of one run (%d rounds, %.1f MB): drawn on the host in %.1f ms, uploaded in %.1f ms: %.2f %% of (a)'
        % (total, (zb.nbytes + ub.nbytes) / 1e6, t_draw, t_up, 100.0 * (t_draw + t_up) / med[0]))
    say('not measured: hardware counters, arm (b) at the default 500 + 500 rounds, other D or chain counts, thin > 1, qmc starts, a prior')


if __name__ == '__main__':
    main()
