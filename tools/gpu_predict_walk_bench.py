"""The host glue around the predictive-moment kernels, timed (profiles/predict_walk_bench.txt): a host clock around calls that end in a
synchronise, one warm-up call each, `--repeats` timed calls per row, one line of milliseconds per row.  Public API only, so the same
file times any checkout; two checkouts are compared by running it on them alternately (--summarise reads the runs' outputs).
Rows:
  predict        emulator.predict at the bench model's shape: n = 2000, 5 + 1 Matern-2.5 nodes, 16 384 points, N = 10
  loo            the same emulator's loo(X)
  vecchia        a Vecchia emulator's predict, n = 20 000, d = 8, M = 100 000, m = 50, N = 2
  vecchia_full   the same with full_layer=True
  lgp            lgp.predict of two GP emulators feeding a DGP emulator whose output node's connect hits both feeding outputs and an
                 external input, n = 1000, M = 4096, N = 2
usage: gpu_predict_walk_bench.py [--repeats R] [row ...]   |   gpu_predict_walk_bench.py --summarise PARENT.txt CHILD.txt"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(f, repeats):
    import torch
    f()
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def dense_rows(repeats, rows):
    from bench import build_model
    from dgp_amd import emulator
    model, X, _ = build_model(2000, 5, 100, 0)
    model.train(N=2, ess_burn=10, disable=True)
    emu = emulator(model.estimate(burnin=0), N=10, seed=7)
    xt = np.random.default_rng(5).uniform(size=(16384, 5))
    if 'predict' in rows:
        yield 'predict', timed(lambda: emu.predict(xt), repeats)
    if 'loo' in rows:
        yield 'loo', timed(lambda: emu.loo(X), repeats)


def vecchia_rows(repeats, rows):
    from dgp_amd import dgp, emulator
    rng = np.random.default_rng(7)
    n, d = 20000, 8
    X = rng.uniform(size=(n, d))
    f = np.sin(3 * X[:, 0]) * np.cos(2 * X[:, 1]) + X[:, 2] ** 2 + 0.3 * X[:, 3:].sum(1)
    np.random.seed(1)
    model = dgp(X, ((f - f.mean()) / f.std())[:, None], vecchia=True, m=25, seed=1)
    model.train(N=1, ess_burn=10, disable=True)
    emu = emulator(model.estimate(burnin=0), N=2, seed=3)
    xt = rng.uniform(size=(100000, d))
    if 'vecchia' in rows:
        yield 'vecchia', timed(lambda: emu.predict(xt, m=50), repeats)
    if 'vecchia_full' in rows:
        yield 'vecchia_full', timed(lambda: emu.predict(xt, m=50, full_layer=True), repeats)


def lgp_rows(repeats, rows):
    from dgp_amd import dgp, gp, kernel, combine
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(7)
    np.random.seed(0)
    n = 1000
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-4, **kw)
    xa, xb = rng.uniform(size=(n, 1)), rng.uniform(size=(n, 1))
    gA, gB = gp(xa, np.sin(4 * xa), K()), gp(xb, xb ** 2 - 0.5, K())
    W = np.concatenate((rng.uniform(-1, 1, size=(n, 2)), rng.uniform(size=(n, 1))), 1)   # (two feeding outputs, one external column)
    Y = np.sin(3 * W[:, :1]) * W[:, 1:2] + W[:, 2:] ** 2 + 0.02 * rng.normal(size=(n, 1))
    layers = combine([K(input_dim=np.array([0, 1]), connect=np.array([2])) for _ in range(2)], [K(scale_est=True, connect=np.arange(3))])
    model = dgp(W, Y, layers, seed=4)
    model.train(N=2, ess_burn=3, disable=True)
    sysm = lgp([[container(gA.export(), local_input_idx=np.array([0])), container(gB.export(), local_input_idx=np.array([1]))],
                [container(model.estimate(), local_input_idx=np.array([0, 1]))]], N=2)
    x = [rng.uniform(size=(4096, 2)), [rng.uniform(size=(4096, 1))]]
    yield 'lgp', timed(lambda: sysm.predict(x), repeats)


GROUPS = ((('predict', 'loo'), dense_rows), (('vecchia', 'vecchia_full'), vecchia_rows), (('lgp',), lgp_rows))


def summarise(parent, child):
    """Per row: both medians, the parent's spread (max - min of its repeats) and whether the child's median lies within the parent's
    median plus that spread."""
    def read(path):
        rows = {}
        for line in open(path):
            p = line.split()
            if len(p) > 2 and p[0] == 'row':
                rows.setdefault(p[1], []).extend(float(v) for v in p[2:])
        return rows
    P, C = read(parent), read(child)
    print('%-13s %8s %12s %12s %11s  %s' % ('row', 'repeats', 'parent ms', 'child ms', 'spread ms', 'child <= parent + spread'))
    for row in P:
        spread = max(P[row]) - min(P[row])
        mp, mc = np.median(P[row]), np.median(C[row])
        print('%-13s %8d %12.2f %12.2f %11.2f  %s' % (row, len(P[row]), mp, mc, spread, 'yes' if mc <= mp + spread else 'NO'))


if __name__ == '__main__':
    args = sys.argv[1:]
    if args[:1] == ['--summarise']:
        summarise(*args[1:3])
        sys.exit(0)
    repeats = int(args[args.index('--repeats') + 1]) if '--repeats' in args else 5
    rows = [a for a in args if not a.startswith('--') and not a.isdigit()] or [r for g, _ in GROUPS for r in g]
    for names, fn in GROUPS:
        if set(names) & set(rows):
            for row, ms in fn(repeats, rows):
                print('row %s %s' % (row, ' '.join('%.3f' % v for v in ms)), flush=True)
