"""Subset simulation at the bench's model shape (profiles/sus_bench.txt; DESIGN I.22): the model, draws and box of
tools/gpu_calibrate_bench.py (n = 2000, d = 5, emulator(N=10), sample_size = 10: 100 paths, F = 2048).
  (1) dgpamd_boxsus_level and dgpamd_boxsus_move at P = 64 draws with R = 1024 and R = 8192 particles, D = 5, next to one
      values-only walk evaluation of the 100 paths at about the same number of rows, the three arms alternating inside every
      repeat.  Device events, 20 repeats after 3 warm ones, medians.
  (2) paths.failure_probability at a threshold whose probability is about 1e-5 (found by the run itself: the pooled level that
      a first run reaches after five stages of 0.1) against plain Monte Carlo through paths(x) with the same number of
      evaluated rows: time, stages, cov(), the spread over 5 seeds, and the hits the plain estimate got.
  (3) with --rng ARMS (profiles/rng_bench.txt; DESIGN I.23) instead of (1) and (2): the end-to-end run of (2) and one
      paths.calibrate_smc run at R = 1024 (y and obs_sd of tools/gpu_smc_bench.py) under every arm of the comma-separated
      list, the arms alternating inside every seed, by device events around the whole call: 'none' calls without the rng
      keyword (any tree), 'numpy' and 'device' pass it.  --tree DIR imports bench and dgp_amd from another checkout (the
      parent commit with its own library, run as a process of its own between runs of this tree).  For 'device' also the
      fill kernels of one stage by device events, and for the numpy arms the host's share as (2) reports it.
Usage: python tools/gpu_sus_bench.py [file that also receives the lines] [--rng none,numpy,device] [--tree DIR]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def option(name):
    """The value behind `name` on the command line, taken out of it; None without it."""
    if name not in sys.argv:
        return None
    i = sys.argv.index(name)
    value = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    return value


ARMS, TREE = option('--rng'), option('--tree')
sys.path.insert(0, os.path.abspath(TREE) if TREE else ROOT)
LOG = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None
REPEATS, WARM, R2, SEEDS = 20, 3, 1024, 5


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


def alternating_ms(e, arms, repeats=REPEATS):
    """{name: (median, min, max)} of every arm's f() by device events: each repeat runs every arm once, in turn, after its
    before(); WARM warm repeats are dropped."""
    spans = {name: [] for name, _, _ in arms}
    for i in range(WARM + repeats):
        for name, f, before in arms:
            if before:
                before()
            a, c = e.event(), e.event()
            e.record(a)
            f()
            e.record(c)
            e.sync()
            spans[name].append(e.elapsed_ms(a, c))
    return {k: (float(np.median(v[WARM:])), float(np.min(v[WARM:])), float(np.max(v[WARM:]))) for k, v in spans.items()}


def kernels(e, pf, bounds):
    P, D = 64, bounds.shape[0]
    lo, hi = bounds[:, 0], bounds[:, 1]
    values = pf._lane_values(bounds, 'failure_probability')[4]
    for R in (1024, 8192):
        rng = np.random.default_rng(R)
        Q = P * R
        state = e.boxsus_state(P, R, D, lo, hi)
        state['x'].copy_(e.tensor(rng.uniform(lo[:, None], hi[:, None], (D, Q))))
        state['sd'].copy_(e.tensor(np.tile(0.3 * (hi - lo), (P, 1))))
        score = e.tensor(-3.0 + rng.normal(size=Q))
        xt = e.zeros(P, R, D)

        def reset():
            state['score'].copy_(score)
            state['done'].zero_()
            state['prob'].fill_(1.0)
        f = e.tensor(rng.normal(size=(P, R, 1)))
        z, logu = e.tensor(rng.normal(size=(P, R, D))), e.tensor(np.log(rng.uniform(size=(P, R, D))))
        xm = e.tensor(rng.uniform(lo, hi, (P, R, D)))
        e.boxsus_move(state, f, xm, z, logu, 0.0, first=True)
        Pw = pf.N * pf.sample_size
        Rw = -(-Q // Pw)
        xw = e.tensor(rng.uniform(lo, hi, (Pw, Rw, D)))
        n_s = max(1, R // 10)
        out = alternating_ms(e, [('level', lambda: e.boxsus_level(state, xt, n_s), reset),
                                 ('move', lambda: e.boxsus_move(state, f, xm, z, logu, 0.0), None),
                                 ('walk', lambda: values(xw), None)], repeats=REPEATS if R == 1024 else 8)
        say('P %d R %d D %d (Q = %d): level median %.3f ms (%.3f .. %.3f); move %.3f ms (%.3f .. %.3f); walk, values only, %d paths x '
            '%d rows %.2f ms (%.2f .. %.2f); (level + move) / walk = %.4f'
            % (P, R, D, Q, *out['level'], *out['move'], Pw, Rw, *out['walk'], (out['level'][0] + out['move'][0]) / out['walk'][0]))


def runs(e, pf, bounds):
    P, D = pf.N * pf.sample_size, bounds.shape[0]
    # the threshold: what a ladder of five levels of 0.1 reaches, the median over the draws
    v = pf(np.random.default_rng(1).uniform(bounds[:, 0], bounds[:, 1], (4096, D)))[0]
    beyond = float(v.max() + 10.0 * (v.max() - v.min()))                          # (no draw gets there: the ladder runs its five stages)
    probe = pf.failure_probability(beyond, bounds, n_particles=R2, max_stages=5, seed=1)
    t = beyond + float(np.median(probe.levels[:, -1]))
    sus = lambda seed: pf.failure_probability(t, bounds, n_particles=R2, seed=seed)
    res, _ = timed(lambda: sus(0))
    say('threshold %.6g: the median over the draws of the level that five stages of 0.1 reach' % t)
    results, ms = [], []
    for seed in range(SEEDS):
        r, t_ms = timed(lambda: sus(seed))
        results.append(r), ms.append(t_ms)
    lp = np.array([r.log_prob for r in results])                                  # (seeds, P)
    r = results[0]
    rows = (r.evaluations + 1) * R2
    say('failure_probability: %d paths x %d particles, %d stages, %d + 1 walk evaluations = %d rows per path; statuses %s; '
        'median time %.1f ms (%.1f .. %.1f)' % (P, R2, r.n_stages, r.evaluations, rows,
                                                {int(k): int(c) for k, c in zip(*np.unique(r.status, return_counts=True))},
                                                np.median(ms), min(ms), max(ms)))
    s = r.summary()
    say('summary of seed 0: mean %.3g, median %.3g, 95 %% interval over the draws %.3g .. %.3g, n_bounded %d, mc_cov %.3f'
        % (s['mean'], s['median'], s['lower'], s['upper'], s['n_bounded'], s['mc_cov']))
    ok = np.all([x.status == 0 for x in results], 0)
    say('spread over %d seeds of ln P^ per draw (ok draws: %d): median %.3f, largest %.3f; cov() median %.3f; acceptance per stage '
        '(median over the draws) %s; steps %.3g .. %.3g' % (SEEDS, ok.sum(), np.median(lp[:, ok].std(0, ddof=1)), lp[:, ok].std(0, ddof=1).max(),
                                                           np.nanmedian(r.cov()), np.round(np.nanmedian(r.accept_rate, 0), 2),
                                                           np.nanmin(r.step), np.nanmax(r.step)))
    # plain Monte Carlo through paths(x) with the same number of rows
    def plain(seed):
        x = np.random.default_rng(seed).uniform(bounds[:, 0], bounds[:, 1], (rows, D))
        return np.sum(pf(x)[0] >= t, 0)
    hits, t_mc = timed(lambda: plain(0))
    say('plain Monte Carlo, %d rows through paths(x): %.1f ms; hits per draw: %d draws with 0, %d with 1, %d with more; largest %d; '
        'pooled estimate %.3g against the mean of P^ %.3g' % (rows, t_mc, np.sum(hits == 0), np.sum(hits == 1), np.sum(hits > 1), hits.max(),
                                                               hits.sum() / (rows * P), s['mean']))
    from dgp_amd import reliability
    streams = reliability.SusStreams(0, P, R2, D)
    _, t_rng = timed(lambda: [streams.prior_uniforms()] + [streams.stage(5) for _ in range(r.n_stages)])
    say('the random numbers of a run, drawn on the host: %.1f ms, %.1f %% of it' % (t_rng, 100.0 * t_rng / np.median(ms)))


def event_ms(e, f):
    a, c = e.event(), e.event()
    e.record(a)
    out = f()
    e.record(c)
    e.sync()
    return out, e.elapsed_ms(a, c)


def spans(ms):
    return '%.1f ms (%.1f .. %.1f)' % (np.median(ms), min(ms), max(ms))


def rng_arms(e, pf, bounds, arms):
    """(3) of the module's docstring."""
    from dgp_amd import optimize
    P, D = pf.N * pf.sample_size, bounds.shape[0]
    kw = {arm: {} if arm == 'none' else dict(rng=arm) for arm in arms}
    v = pf(np.random.default_rng(1).uniform(bounds[:, 0], bounds[:, 1], (4096, D)))[0]
    beyond = float(v.max() + 10.0 * (v.max() - v.min()))
    probe = pf.failure_probability(beyond, bounds, n_particles=R2, max_stages=5, seed=1)
    t = beyond + float(np.median(probe.levels[:, -1]))
    say('threshold %.6g; arms %s, alternating inside every seed, device events around the whole call' % (t, ', '.join(arms)))
    ms, stages, means = {a: [] for a in arms}, {a: [] for a in arms}, {a: [] for a in arms}
    for seed in [0] + list(range(SEEDS)):                                         # (the first pass is warm-up and dropped)
        for arm in arms:
            r, t_ms = event_ms(e, lambda: pf.failure_probability(t, bounds, n_particles=R2, seed=seed, **kw[arm]))
            ms[arm].append(t_ms), stages[arm].append(r.n_stages), means[arm].append(r.summary()['mean'])
    for arm in arms:
        say('failure_probability, rng %s: %d paths x %d particles, %s over %d seeds; stages %s; mean of P^ per seed %s'
            % (arm, P, R2, spans(ms[arm][1:]), SEEDS, stages[arm][1:], ' '.join('%.3g' % m for m in means[arm][1:])))
    n_stages = int(np.median(stages[arms[0]][1:]))
    from dgp_amd import reliability
    if 'device' in arms:
        streams = reliability.DeviceSusStreams(e, 0, P, R2, D)
        fills = [event_ms(e, lambda: streams.stage(5))[1] for _ in range(WARM + REPEATS)][WARM:]
        _, t_prior = timed(lambda: streams.prior_uniforms().cpu())
        say('device streams: the two fills of one stage (5 rounds x %d x %d x %d normals and log-uniforms) %s; the prior uniforms, filled '
            'and fetched, %.2f ms; the fills of a run of %d stages %.2f ms'
            % (P, R2, D, '%.3f ms (%.3f .. %.3f)' % (np.median(fills), min(fills), max(fills)), t_prior, n_stages, n_stages * np.median(fills)))
    host = reliability.SusStreams(0, P, R2, D)
    _, t_rng = timed(lambda: [host.prior_uniforms()] + [host.stage(5) for _ in range(n_stages)])
    say('numpy streams: the random numbers of a run of %d stages, drawn on the host, %.1f ms' % (n_stages, t_rng))
    # one calibrate_smc run per arm at R = 1024, the observation of tools/gpu_smc_bench.py
    fc = pf(optimize.candidates(bounds[:, 0], bounds[:, 1], 2048, 3))[0]
    y, sd = float(pf(bounds.mean(1)[None])[0].mean()), 0.1 * float(np.median(fc.max(0) - fc.min(0)))
    ms, stages = {a: [] for a in arms}, {a: [] for a in arms}
    for rep in range(4):                                                          # (the first pass is warm-up and dropped)
        for arm in arms:
            r, t_ms = event_ms(e, lambda: pf.calibrate_smc(y, sd, bounds, n_particles=R2, seed=3, **kw[arm]))
            ms[arm].append(t_ms), stages[arm].append(r.n_stages)
    for arm in arms:
        say('calibrate_smc, rng %s: %d paths x %d particles, y = %.4g, obs_sd = %.4g, %s over 3 runs; stages %s'
            % (arm, P, R2, y, sd, spans(ms[arm][1:]), stages[arm][1:]))
    say('not measured: hardware counters, other shapes, calibrate with mala or hmc, more than these %d seeds' % SEEDS)


def main():
    import bench
    from dgp_amd import emulator
    n, d, N, J, F = 2000, 5, 10, 10, 2048
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    pf = emu.sample_functions(sample_size=J, n_features=F)
    bounds = np.stack((X.min(0), X.max(0)), 1)
    say('n = %d, d = %d, %d paths, F = %d, box = the range of X' % (n, d, N * J, F))
    if ARMS:
        return rng_arms(e, pf, bounds, ARMS.split(','))
    kernels(e, pf, bounds)
    runs(e, pf, bounds)
    say('not measured: hardware counters, other D, P or level_prob, n_moves other than 4, a prior, and the spread of the estimate '
        'at this scale beyond these %d seeds' % SEEDS)


if __name__ == '__main__':
    main()
