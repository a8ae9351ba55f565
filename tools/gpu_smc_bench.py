"""Tempered SMC at the bench's model shape (profiles/smc_bench.txt; DESIGN I.21): the model, draws, box, y and obs_sd of
tools/gpu_calibrate_bench.py (n = 2000, d = 5, emulator(N=10), sample_size = 10: 100 paths, F = 2048).
  (1) dgpamd_boxsmc_temper at P = 64 draws with R = 1024 and R = 8192 particles, D = 5, on ll = -5 + 30 N(0, 1) (beta lands
      inside: all 53 rounds of the bisection run) and on equal ll (the full step: one round), next to one
      dgpamd_boxsmc_move call at the same Q = P R and one walk evaluation (values and Jacobian) of the 100 paths at about the
      same number of rows.  Device events, 20 repeats after 3 warm ones, medians.
  (2) paths.calibrate_smc(n_particles=R2) against paths.calibrate(method='mala', n_chains=R2, x0=uniform starts) with
      warmup + n_samples = the SMC run's walk evaluations: stages, wall time (three alternating rounds after a warm-up of
      each, medians), and what of the SMC run is the host's random numbers; then again with obs_sd / 20, which takes several
      stages.
Usage: python tools/gpu_smc_bench.py [file that also receives the lines]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LOG = open(sys.argv[1], 'w') if len(sys.argv) > 1 else None
REPEATS, WARM, R2 = 20, 3, 256


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


def device_ms(e, f, before=None, repeats=REPEATS):
    """The median over `repeats` runs of f() by device events, after WARM warm runs; before() restores its inputs."""
    spans = []
    for i in range(WARM + repeats):
        if before:
            before()
        a, c = e.event(), e.event()
        e.record(a)
        f()
        e.record(c)
        e.sync()
        spans.append(e.elapsed_ms(a, c))
    return float(np.median(spans[WARM:])), float(np.min(spans[WARM:])), float(np.max(spans[WARM:]))


def kernels(e, pf, bounds):
    P, D = 64, bounds.shape[0]
    lo, hi = bounds[:, 0], bounds[:, 1]
    for R in (1024, 8192):
        rng = np.random.default_rng(R)
        Q = P * R
        state = e.boxsmc_state(P, R, D, np.ones(1), np.zeros(1), lo, hi, hi - lo)
        state['x'].copy_(e.tensor(rng.uniform(lo[:, None], hi[:, None], (D, Q))))
        xt, u = e.zeros(P, R, D), e.tensor(rng.uniform(size=P))
        for name, ll in (('spread 30', -5.0 + 30.0 * rng.normal(size=Q)), ('equal', np.full(Q, -5.0))):
            lld = e.tensor(ll)

            def reset():
                state['ll'].copy_(lld)
                state['beta'].zero_()
            med, low, high = device_ms(e, lambda: e.boxsmc_temper(state, xt, u, 0.5), reset)
            say('temper P %d R %d (%s ll; beta\' %.4g): median %.3f ms (%.3f .. %.3f)' % (P, R, name, float(state['beta'][0]), med, low, high))
        f, J = e.tensor(rng.normal(size=(P, R, 1))), e.tensor(rng.normal(size=(P, R, 1, D)))
        z, logu = e.tensor(rng.normal(size=(P, R, D))), e.tensor(np.log(rng.uniform(size=(P, R))))
        xt.copy_(e.tensor(rng.uniform(lo, hi, (P, R, D))))
        e.boxsmc_move(state, f, J, xt, z, logu, first=True)
        med, low, high = device_ms(e, lambda: e.boxsmc_move(state, f, J, xt, z, logu))
        say('move   P %d R %d (Q = %d, K = 1, D = %d): median %.3f ms (%.3f .. %.3f)' % (P, R, Q, D, med, low, high))
        Pw = pf.N * pf.sample_size
        Rw = -(-Q // Pw)
        _, _, _, _, _, value_and_jac, _ = pf._lane_problem(bounds, 'calibrate_smc')
        xw = e.tensor(rng.uniform(lo, hi, (Pw, Rw, D)))
        med, low, high = device_ms(e, lambda: value_and_jac(xw), repeats=5 if R == 1024 else 2)
        say('walk   %d paths x %d rows (Q = %d): median %.1f ms (%.1f .. %.1f)' % (Pw, Rw, Pw * Rw, med, low, high))


def runs(e, pf, y, sd, bounds):
    from dgp_amd import calibrate
    P, D = pf.N * pf.sample_size, bounds.shape[0]
    smc = lambda: pf.calibrate_smc(y, sd, bounds, n_particles=R2, seed=3)
    res = smc()
    x0 = np.random.default_rng(3).uniform(bounds[:, 0], bounds[:, 1], (P, R2, D))
    rounds = res.evaluations                                     # (MALA's INIT round stands for SMC's evaluation of the prior particles)
    mala = lambda: pf.calibrate(y, sd, bounds, x0=x0, seed=3, warmup=rounds // 2, n_samples=rounds - rounds // 2)
    ref = mala()
    say('calibrate_smc: %d paths x %d particles, %d stages, %d + 1 walk evaluations; statuses %s; betas of draw 0 %s; acceptance per '
        'stage (median over the draws) %s; steps %.3g .. %.3g; draw_ess %.1f of %d'
        % (P, R2, res.n_stages, res.evaluations, {int(k): int(c) for k, c in zip(*np.unique(res.status, return_counts=True))},
           np.round(res.betas[0], 4), np.round(np.median(res.accept_rate, 0), 2), res.step.min(), res.step.max(), res.draw_ess, P))
    say('log evidence: %.3f .. %.3f (median %.3f), log_norm %.3f' % (res.log_evidence.min(), res.log_evidence.max(),
                                                                     np.median(res.log_evidence), res.log_norm))
    say('pooled mean: smc equal weights %s, evidence weights %s; mala (%d rounds, %d chains per path from uniform starts) %s'
        % (np.round(res.summary()['mean'], 3), np.round(res.summary(weights='evidence')['mean'], 3), ref.rounds, R2,
           np.round(ref.summary()['mean'], 3)))
    ms = np.zeros((3, 2))
    for rnd in range(3):
        for a, (name, f) in enumerate((('calibrate_smc', smc), ('calibrate mala', mala))):
            _, ms[rnd, a] = timed(f)
            say('round %d: %-15s %10.1f ms' % (rnd + 1, name, ms[rnd, a]))
    med = np.median(ms, 0)
    say('medians: calibrate_smc %.1f ms (%d + 1 evaluations), calibrate mala %.1f ms (%d evaluations); per evaluation %.2f and %.2f ms; '
        'smc / mala = %.3f' % (med[0], res.evaluations, med[1], ref.evaluations, med[0] / (res.evaluations + 1), med[1] / ref.evaluations,
                               med[0] / (res.evaluations + 1) * ref.evaluations / med[1]))
    streams = calibrate.SmcStreams(3, P, R2, D)
    _, t_rng = timed(lambda: [streams.prior_uniforms()] + [streams.stage(5) for _ in range(res.n_stages)])
    say('the random numbers of the smc run, drawn on the host: %.1f ms, %.1f %% of it' % (t_rng, 100.0 * t_rng / med[0]))


def main():
    import bench
    from dgp_amd import emulator, optimize
    n, d, N, J, F, NC = 2000, 5, 10, 10, 2048, 2048
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    pf = emu.sample_functions(sample_size=J, n_features=F)
    bounds = np.stack((X.min(0), X.max(0)), 1)
    fc = pf(optimize.candidates(bounds[:, 0], bounds[:, 1], NC, 3))[0]
    y, sd = float(pf(bounds.mean(1)[None])[0].mean()), 0.1 * float(np.median(fc.max(0) - fc.min(0)))
    say('n = %d, d = %d, %d paths, F = %d, box = the range of X, y = %.4g, obs_sd = %.4g' % (n, d, N * J, F, y, sd))
    kernels(e, pf, bounds)
    runs(e, pf, y, sd, bounds)
    say('the same with a sharp observation, obs_sd / 20:')
    runs(e, pf, y, sd / 20.0, bounds)
    say('not measured: hardware counters, other D, P or ess_frac, n_moves other than 4, a prior')


if __name__ == '__main__':
    main()
