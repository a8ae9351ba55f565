#!/usr/bin/env python3
"""Timings of the predictive-mixture kernels (csrc/mixture.hip) against the numpy / scipy formulas on the host, and of
interval() against Monte Carlo quantiles of predict(method='sampling') -- the figures of DESIGN I.15 and
profiles/mixture_bench.txt.

    python tools/gpu_mixture_bench.py [--count 100000] [--threads 16] [--rounds 3] [--no-model]

Device times are between device events around the call's launches (inputs resident, outputs left on the device), host times
are wall clock of the formulas on the same arrays with the rows split over `--threads` threads; the arms alternate, `--rounds`
rounds after one warm-up round, and every round's figure is printed (the summary line takes the median)."""
import argparse
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def host_cdf(mu, var, y):
    from scipy.special import ndtr
    return ndtr((y[None] - mu[:, :, None]) / np.sqrt(var)[:, :, None]).mean(0)


def host_quantile(mu, var, p, iters=60):
    """Vectorised bisection from the components' own p-quantiles, `iters` halvings."""
    from scipy.special import ndtr, ndtri
    sd = np.sqrt(var)
    out = np.empty((mu.shape[1], len(p)))
    for t, pp in enumerate(p):
        ends = mu + ndtri(pp) * sd
        lo, hi = ends.min(0), ends.max(0)
        for _ in range(iters):
            mid = 0.5 * (lo + hi)
            up = ndtr((mid[None] - mu) / sd).mean(0) >= pp
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        out[:, t] = hi
    return out


def host_crps(mu, var, y):
    from scipy.special import erf

    def A(m, v):
        sd = np.sqrt(v)
        return 2 * sd * np.exp(-0.5 * (m / sd) ** 2) / np.sqrt(2 * np.pi) + m * erf(m / (sd * np.sqrt(2)))
    S = mu.shape[0]
    first = A(y[None] - mu, var).sum(0) / S
    second = (2 * np.sqrt(var / np.pi)).sum(0)
    for s in range(S):
        if s + 1 < S:
            second += 2 * A(mu[s][None] - mu[s + 1:], var[s][None] + var[s + 1:]).sum(0)
    return first - second / (2 * S * S)


def threaded(pool, threads, fn, mu, var, *rest):
    """fn on `threads` blocks of the entries (numpy's ufuncs release the interpreter lock)."""
    cuts = np.linspace(0, mu.shape[1], threads + 1).astype(int)
    parts = list(pool.map(lambda i: fn(mu[:, cuts[i]:cuts[i + 1]], var[:, cuts[i]:cuts[i + 1]],
                                       *[r[cuts[i]:cuts[i + 1]] if getattr(r, 'ndim', 0) and len(r) == mu.shape[1] else r for r in rest]),
                          range(threads)))
    return np.concatenate(parts)


def device_ms(eng, call, reps):
    a, b = eng.event(), eng.event()
    eng.record(a)
    for _ in range(reps):
        call()
    eng.record(b)
    eng.sync()
    return eng.elapsed_ms(a, b) / reps


def kernels(args):
    from dgp_amd.ops import Engine
    eng = Engine(0)
    pool = ThreadPoolExecutor(args.threads)
    rng = np.random.default_rng(0)
    p = np.array([0.025, 0.975])
    for S in (10, 50):
        mu = 3.0 * rng.normal(size=(S, args.count))
        var = np.exp(rng.normal(size=(S, args.count)))
        y5 = mu[0][:, None] + rng.normal(size=(args.count, 5))
        y1 = np.ascontiguousarray(y5[:, 0])
        mud, vard, y5d, y1d = (eng.tensor(a) for a in (mu, var, y5, y1))
        lds = ('lds', 'global') if S <= 160 else ('global',)
        arms = [('cdf T=5', 'device', lambda: eng.mixture_eval('cdf', mud, vard, y5d), 20)]
        arms += [('quantile T=2', 'device ' + w, (lambda w=w: eng.mixture_quantile(mud, vard, p, path=w)), 5) for w in lds]
        arms += [('crps', 'device ' + w, (lambda w=w: eng.mixture_crps(mud, vard, y1d, path=w)), 5) for w in lds]
        hosts = [('cdf T=5', lambda: threaded(pool, args.threads, host_cdf, mu, var, y5)),
                 ('quantile T=2', lambda: threaded(pool, args.threads, host_quantile, mu, var, p)),
                 ('crps', lambda: threaded(pool, args.threads, host_crps, mu, var, y1))]
        res = {}
        for rnd in range(args.rounds + 1):
            for what, arm, call, reps in arms:
                ms = device_ms(eng, call, reps)
                if rnd:
                    res.setdefault((what, arm), []).append(ms)
            for what, call in hosts:
                t0 = time.perf_counter()
                call()
                if rnd:
                    res.setdefault((what, 'host x%d threads' % args.threads), []).append(1e3 * (time.perf_counter() - t0))
        # the device and the host formulas compute the same thing
        dq = eng.mixture_quantile(mud, vard, p)[0].cpu().numpy()
        hq = threaded(pool, args.threads, host_quantile, mu, var, p)
        dc = eng.mixture_crps(mud, vard, y1d).cpu().numpy()
        hc = threaded(pool, args.threads, host_crps, mu, var, y1)
        df = eng.mixture_eval('cdf', mud, vard, y5d).cpu().numpy()
        hf = threaded(pool, args.threads, host_cdf, mu, var, y5)
        print('S=%d count=%d: max |device - host|: cdf %.2e  quantile %.2e  crps %.2e' %
              (S, args.count, np.abs(df - hf).max(), np.abs(dq - hq).max(), np.abs(dc - hc).max()))
        for (what, arm), ms in res.items():
            print('S=%-3d %-13s %-22s median %10.3f ms   rounds %s' % (S, what, arm, np.median(ms), ' '.join('%.3f' % m for m in ms)))
        for what in ('cdf T=5', 'quantile T=2', 'crps'):
            host = np.median(res[(what, 'host x%d threads' % args.threads)])
            best = min(np.median(v) for (w, a), v in res.items() if w == what and a.startswith('device'))
            print('S=%-3d %-13s host / device = %.1f' % (S, what, host / best))
        sys.stdout.flush()


def model(args):
    """interval(0.95) against np.quantile of predict(method='sampling', sample_size=50) on the benchmark's model."""
    import bench
    from dgp_amd import emulator
    m, X, Y = bench.build_model(2000, 5, 1, 0)
    m.train(N=10, ess_burn=10, disable=True)
    emu = emulator(m.estimate(burnin=0), N=10, seed=7, device=0)
    xt = np.random.default_rng(5).uniform(size=(8192, 5))
    emu.predict(xt[:32])
    exact = None
    for rnd in range(args.rounds + 1):
        t0 = time.perf_counter()
        lo, hi = emu.predict_dist(xt).interval(0.95)
        t1 = time.perf_counter()
        draws = emu.predict(xt, method='sampling', sample_size=50)[0]     # (M, N * 50)
        mc = np.quantile(draws, [0.025, 0.975], axis=1)
        t2 = time.perf_counter()
        t3 = time.perf_counter()
        emu.predict(xt)
        t4 = time.perf_counter()
        exact = (lo[:, 0], hi[:, 0])
        if rnd:
            sd = np.sqrt(emu.predict(xt)[1][:, 0])
            err = np.concatenate((mc[0] - exact[0], mc[1] - exact[1])) / np.concatenate((sd, sd))
            print('model n=2000 M=8192 N=10: predict_dist + interval %.1f ms | sampling(50) + np.quantile %.1f ms | predict alone %.1f ms | '
                  'Monte Carlo error of the interval ends, in predictive sd: rms %.3f  max %.3f' %
                  (1e3 * (t1 - t0), 1e3 * (t2 - t1), 1e3 * (t4 - t3), np.sqrt((err ** 2).mean()), np.abs(err).max()))
    sys.stdout.flush()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--count', type=int, default=100000)
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--no-model', action='store_true')
    args = ap.parse_args()
    kernels(args)
    if not args.no_model:
        model(args)
