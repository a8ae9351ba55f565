"""Joint sample paths of a linked system (lgp.sample_paths), recorded in profiles/lgp_paths_bench.txt.

(1) GP -> DGP -> GP chain with an external input into the DGP, n = 1000 training points per emulator, M = 1000 test points,
    N = 10 systems, sample_size = 10: wall time of the first call (statistics built on the way) and of warm calls, and the
    time spent in Engine.joint_cov / potrf / mvn_paths (each call synchronised: the sum of the three against the wall time
    says how much of the call is host glue).
(2) Cross-check: a one-container system holding the bench-shaped DGP (tools/gpu_sample_paths_bench.py: n = 2000, 5 Matern
    nodes -> one node with connect) against emulator.sample_paths at the same N, sample_size and M."""
import collections
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(label, f, reps=3):
    import torch
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        print('%-72s %8.1f ms' % ('%s: %s' % (label, 'first call' if r == 0 else 'warm call'), 1e3 * (time.perf_counter() - t0)))
    return out


def split(e, f):
    """Per Engine method, the synchronised time spent in it during f()."""
    import torch
    spent = collections.defaultdict(float)
    calls = collections.Counter()
    orig = {}
    for name in ('joint_cov', 'potrf', 'mvn_paths'):
        orig[name] = getattr(e, name)

        def wrap(*a, _name=name, **kw):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = orig[_name](*a, **kw)
            torch.cuda.synchronize()
            spent[_name] += time.perf_counter() - t0
            calls[_name] += 1
            return r
        setattr(e, name, wrap)
    try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        wall = time.perf_counter() - t0
    finally:
        for name in orig:
            delattr(e, name)
    for name in orig:
        print('  %-10s %3d calls %8.1f ms' % (name, calls[name], 1e3 * spent[name]))
    print('  %-10s           %8.1f ms (wall, synchronised calls)' % ('total', 1e3 * wall))


def main():
    import bench
    from dgp_amd import dgp, emulator, gp, kernel, combine
    from dgp_amd.linkgp import container, lgp
    n, M, N, J = 1000, 1000, 10, 10
    rng = np.random.default_rng(0)
    X1 = rng.uniform(size=(n, 2))
    g1 = gp(X1, np.sin(4 * X1[:, :1]) + X1[:, 1:] ** 2, kernel(length=np.array([0.5]), name='matern2.5', nugget=1e-6))
    W2 = np.concatenate((rng.uniform(-1, 2, size=(n, 1)), rng.uniform(size=(n, 1))), 1)
    Y2 = np.sin(3 * W2[:, :1]) * np.cos(2 * W2[:, 1:])
    # the DGP: column 0 of its input from the first GP, column 1 external (x[1][0])
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', **kw)
    m2 = dgp(W2, Y2, combine([K(input_dim=np.array([0]), connect=np.array([1])) for _ in range(2)],
                             [K(scale_est=True, connect=np.array([1]))]), seed=1)
    m2.train(N=3, ess_burn=3, disable=True)
    X3 = rng.uniform(-1, 1, size=(n, 1))
    g3 = gp(X3, np.tanh(2 * X3), kernel(length=np.array([0.7]), name='sexp', nugget=1e-6))
    np.random.seed(0)
    sysm = lgp([[container(g1.export(), local_input_idx=np.array([0, 1]))],
                [container(m2.estimate(), local_input_idx=np.array([0]))],
                [container(g3.export(), local_input_idx=np.array([0]))]], N=N)
    x = [rng.uniform(size=(M, 2)), [rng.uniform(size=(M, 1))], [None]]
    e = g1.kernel.engine
    out = timed('GP -> DGP -> GP, n = %d, M = %d, N = %d, sample_size = %d' % (n, M, N, J),
                lambda: sysm.sample_paths(x, sample_size=J))
    assert out[0].shape == (1, M, N * J) and np.all(np.isfinite(out[0]))
    split(e, lambda: sysm.sample_paths(x, sample_size=J))

    model, Xb, _ = bench.build_model(2000, 5, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    est = model.estimate()
    emu = emulator(est, N=N, seed=1)
    xb = np.random.default_rng(5).uniform(size=(M, 5))
    timed('emulator.sample_paths, bench DGP (n = 2000), M = %d, N = %d, sample_size = %d' % (M, N, J),
          lambda: emu.sample_paths(xb, sample_size=J))
    np.random.seed(1)
    one = lgp([[container(est, local_input_idx=np.arange(5))]], N=N)
    timed('lgp.sample_paths, one container of the same DGP', lambda: one.sample_paths(xb, sample_size=J))
    split(emu.engine, lambda: one.sample_paths(xb, sample_size=J))


if __name__ == '__main__':
    main()
