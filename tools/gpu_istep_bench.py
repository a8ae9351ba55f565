"""Host-clock time of imp.sample(burnin=10) on a three-layer dense model (n = 2000, d = 5; two nodes in the second hidden layer): the
I-step's device queue over several hidden layers, which bench.py's two-layer model does not run.  One warm-up call per process
(plans, workspaces, code loading), then `--repeats` timed calls; each call ends in the detach's synchronise.  Prints one line per
repeat ("row istep_deep MS") and a JSON line with their mean.  Needs an MI355X.
usage: gpu_istep_bench.py [--repeats R] [--n N] [--d D] [--burnin B]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--n', type=int, default=2000)
    ap.add_argument('--d', type=int, default=5)
    ap.add_argument('--burnin', type=int, default=10)
    a = ap.parse_args()
    from dgp_amd import dgp, kernel, combine
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(a.n, a.d))
    Y = np.sin(3 * X[:, :1]) + X[:, 1:2] ** 2 + 0.05 * rng.normal(size=(a.n, 1))
    K = lambda length, **kw: kernel(length=np.array([length]), name='matern2.5', **kw)
    layers = combine([K(1.0) for _ in range(a.d)], [K(1.2, connect=np.arange(a.d)) for _ in range(2)],
                     [K(0.8, scale_est=True, connect=np.arange(a.d))])
    model = dgp(X, (Y - Y.mean()) / Y.std(), layers, seed=3)
    imp = model.imp
    imp.sample(burnin=a.burnin)
    q0, ms = imp.queued_calls, []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        imp.sample(burnin=a.burnin)
        ms.append(1e3 * (time.perf_counter() - t0))
        print('row istep_deep %.3f' % ms[-1], flush=True)
    assert imp.queued_calls - q0 == a.repeats, 'the calls did not run through the device queue'
    print(json.dumps(dict(row='istep_deep', n=a.n, d=a.d, burnin=a.burnin, repeats=a.repeats, mean_ms=float(np.mean(ms)),
                          min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), stats=imp.stats)))


if __name__ == '__main__':
    main()
