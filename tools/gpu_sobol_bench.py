"""Sobol' indices of function-valued draws at the bench's model shape (profiles/sobol_bench.txt; DESIGN I.16): n = 2000, d = 5
Matern nodes -> one Matern node with `connect`, briefly trained; emulator(N=10); sample_size = 10 (100 paths), F = 2048;
n_base = 8192, so 7 x 8192 = 57 344 design rows.
  (a) paths.sobol(A, B): the sums taken on the device, the last layer never copied to the host;
  (b) what a user does without it: paths(vstack([A, B, AB_1 .. AB_5])) and the estimators in numpy on the (57 344, 100) array.
Arms alternate; three rounds after a warm-up of each; medians.  Then the share of (a) spent in dgpamd_sobol_tiles and
dgpamd_sobol_add, by device events around every call of one more run of (a).
Usage: python tools/gpu_sobol_bench.py [file that also receives the lines]"""
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


def host_estimator(pf, A, B):
    """(first, total) (Dx, P) the way a user writes it: one evaluation of the stacked design, numpy sums."""
    n, D = A.shape
    rows = [A, B]
    for i in range(D):
        AB = A.copy()
        AB[:, i] = B[:, i]
        rows.append(AB)
    f = pf(np.vstack(rows))[0].reshape(D + 2, n, -1)          # (2 + D, n_base, P)
    g = f - f[0, 0]
    V = ((g[0]**2).sum(0) + (g[1]**2).sum(0)) / (2 * n) - ((g[0].sum(0) + g[1].sum(0)) / (2 * n))**2
    first = np.stack([(g[1] * (g[2 + i] - g[0])).sum(0) / n / V for i in range(D)])
    total = np.stack([((g[0] - g[2 + i])**2).sum(0) / (2 * n) / V for i in range(D)])
    return first, total


def main():
    import bench
    from dgp_amd import emulator
    from dgp_amd.sensitivity import saltelli_design
    n, d, N, J, F, n_base = 2000, 5, 10, 10, 2048, 8192
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    pf = emu.sample_functions(sample_size=J, n_features=F)
    A, B = saltelli_design(np.stack((X.min(0), X.max(0)), 1), n_base, seed=3)
    legs = [('(a) paths.sobol(A, B)', lambda: pf.sobol(A, B)), ('(b) paths(vstack) + numpy estimator', lambda: host_estimator(pf, A, B))]
    res, (first, total) = legs[0][1](), legs[1][1]()            # warm both
    say('n = %d, d = %d, %d paths, F = %d, n_base = %d (%d design rows)' % (n, d, N * J, F, n_base, (d + 2) * n_base))
    say('largest |(a) - (b)|: first %.3g, total %.3g (the host sums round in numpy\'s own order)'
        % (np.abs(res.first[0] - first).max(), np.abs(res.total[0] - total).max()))
    say('draw-averaged first-order indices %s, total %s' % (np.round(res.first[0].mean(-1), 4), np.round(res.total[0].mean(-1), 4)))
    ms = np.zeros((3, 2))
    for rnd in range(3):
        for a, (name, f) in enumerate(legs):
            _, ms[rnd, a] = timed(f)
            say('round %d: %-38s %9.1f ms' % (rnd + 1, name, ms[rnd, a]))
    med = np.median(ms, 0)
    say('medians: (a) %.1f ms, (b) %.1f ms, (a) / (b) = %.3f' % (med[0], med[1], med[0] / med[1]))
    # the two new kernels inside (a): device events around every call
    spans = []

    def wrapped(f):
        def g(*args):
            ev0, ev1 = e.event(), e.event()
            e.record(ev0)
            out = f(*args)
            e.record(ev1)
            spans.append((f.__name__, ev0, ev1))
            return out
        return g
    e.sobol_tiles, e.sobol_add = wrapped(e.sobol_tiles), wrapped(e.sobol_add)
    _, whole = timed(legs[0][1])
    del e.sobol_tiles, e.sobol_add
    by = {}
    for name, ev0, ev1 in spans:
        by[name] = by.get(name, 0.0) + e.elapsed_ms(ev0, ev1)
    say('(a) with events: %.1f ms; %d calls: sobol_tiles (its output buffer\'s allocation included) %.3f ms, sobol_add %.3f ms: '
        '%.2f %% of (a)' % (whole, len(spans), by['sobol_tiles'], by['sobol_add'], 100.0 * sum(by.values()) / whole))


if __name__ == '__main__':
    main()
