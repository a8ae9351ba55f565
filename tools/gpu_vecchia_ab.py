"""Two builds of the C library on the Vecchia kernels at the shapes users run, alternating in fresh processes on one machine
(the build is chosen with DGPAMD_LIB, so it is fixed per process): per build and shape the median over the repeats and the
run-to-run spread (max - min), and whether the second build's median lies within the first's median plus the first's spread.
Shapes: the row kernels at n = 50 000, d = 8, m = 25 (registers) and m = 40 (LDS); vecchia_gp and vecchia_linkgp of both kinds at
100 000 points, D = 8, pm = 50 (registers) and pm = 60 (LDS); vpaths_rows at M = 100 000, m = 50, D = 5 against n = 2000 with ten
right-hand sides; nn_ordered at n = 3000, 8000 (the two selection kernels) and 50 000 (d = 8, m = 25).  Device-event times.
With --bench the shapes are replaced by bench.py's headline (`value`, SI it/s: higher is better).  Needs an MI355X.
usage: gpu_vecchia_ab.py [--bench] PARENT.so CHILD.so [repeats]"""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ('sexp', 'matern2.5')


def worker():
    sys.path.insert(0, ROOT)
    from dgp_amd.ops import default_engine
    e = default_engine(0)
    rng = np.random.default_rng(7)
    out = {}
    ev0, ev1 = e.event(), e.event()

    def timed(name, fn, reps):
        fn()
        e.record(ev0)
        for _ in range(reps):
            fn()
        e.record(ev1)
        out[name] = e.elapsed_ms(ev0, ev1) / reps

    # ---- rows
    n, d, B = 50000, 8, 4
    X = rng.uniform(size=(n, d))
    y = np.sin(3 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.normal(size=n)
    length = np.array([0.8])
    dX, dy, ones = e.tensor(X), e.tensor(y), e.tensor(np.ones(n))
    XB = dX.unsqueeze(0).repeat(B, 1, 1).contiguous()
    for nn in (3000, 8000, 50000):
        xs = e.tensor(X[:nn] / length)
        timed('nn_ordered n=%d' % nn, lambda: e.nn_ordered(xs, 25), 5)
    for m, reps in ((25, 20), (40, 5)):
        NN = e.nn_ordered(e.tensor(X / length), m)
        for kind in KINDS:
            tag = 'rows m=%d %s ' % (m, kind)
            timed(tag + 'llik', lambda: e.vecchia_llik(kind, dX, dy, NN, length, 1e-4, ones), reps)
            timed(tag + 'llik x%d' % B, lambda: e.vecchia_llik_batch(kind, XB, dy, NN, length, 1e-4, ones), reps)
            timed(tag + 'nllik', lambda: e.vecchia_nllik(kind, dX, dy, NN, length, 1e-4, ones, True), reps)
            timed(tag + 'lmatrix', lambda: e.vecchia_lmatrix(kind, dX, NN, length, 1e-4), reps)
    # ---- predictors
    M, D = 100000, 8
    x = rng.uniform(size=(M, D))
    dx, dv = e.tensor(x), e.tensor(rng.uniform(0.0, 0.02, size=(M, D)))
    ln = np.full(D, 0.8)
    for pm, reps in ((50, 5), (60, 3)):
        NN = e.nn_query(e.tensor(x / ln), e.tensor(X / ln), pm)
        for kind in KINDS:
            timed('vecchia_gp pm=%d %s' % (pm, kind), lambda: e.vecchia_gp(kind, dx, dX, NN, dy, 1.2, ln, 1e-4, ones), reps)
            timed('vecchia_linkgp pm=%d %s' % (pm, kind),
                  lambda: e.vecchia_linkgp(kind, dx, dv, None, dX, None, NN, dy, 1.2, ln, 1e-4, ones), reps)
    # ---- sample-path rows
    n2, D2, m2 = 2000, 5, 50
    q, x2 = e.tensor(rng.uniform(size=(1, M, D2)) / 0.5), e.tensor(rng.uniform(size=(1, n2, D2)) / 0.5)
    y2 = e.tensor(rng.normal(size=(1, 10, n2)))
    NN2 = e.vpaths_nn(q, x2, m2)
    for kind in KINDS:
        timed('vpaths_rows m=%d %s' % (m2, kind), lambda: e.vpaths_rows(kind, q, x2, NN2, y2, 1.2, 1e-4), 5)
    e.sync()
    print('AB ' + json.dumps(out), flush=True)


def run_once(lib, bench):
    env = dict(os.environ, DGPAMD_LIB=os.path.abspath(lib))
    cmd = ([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '150', '--warmup', '3', '--no-cpu-baseline']
           if bench else [sys.executable, os.path.abspath(__file__), '--worker'])
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, text=True, timeout=600)
    if r.returncode != 0:
        sys.exit('the run with %s ended with status %d: nothing more is started' % (lib, r.returncode))
    if bench:
        return {'bench.py value (SI it/s)': json.loads(r.stdout.strip().splitlines()[-1])['value']}
    return json.loads(next(l for l in r.stdout.splitlines() if l.startswith('AB '))[3:])


def main(argv):
    bench = '--bench' in argv
    argv = [a for a in argv if a != '--bench']
    libs, repeats = argv[:2], int(argv[2]) if len(argv) > 2 else 5
    runs = [[], []]
    for _ in range(repeats):
        for which in (0, 1):
            runs[which].append(run_once(libs[which], bench))
    print('# parent: %s\n# child:  %s\n# %d alternating repeats each; median and spread (max - min) over them; %s'
          % (libs[0], libs[1], repeats, 'SI it/s, higher is better' if bench else 'ms, lower is better'))
    print('%-36s %10s %10s %10s %10s  %s' % ('shape', 'parent', 'spread', 'child', 'spread', 'child within parent median +- spread'))
    ok = True
    for key in runs[0][0]:
        a, b = (np.array([r[key] for r in runs[w]]) for w in (0, 1))
        ma, mb, sa, sb = np.median(a), np.median(b), a.max() - a.min(), b.max() - b.min()
        good = mb >= ma - sa if bench else mb <= ma + sa
        ok = ok and good
        print('%-36s %10.4g %10.3g %10.4g %10.3g  %s' % (key, ma, sa, mb, sb, 'yes' if good else 'NO'))
    return 0 if ok else 1


if __name__ == '__main__':
    if '--worker' in sys.argv:
        worker()
    else:
        sys.exit(main(sys.argv[1:]))
