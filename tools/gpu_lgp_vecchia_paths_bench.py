"""Vecchia joint sample paths of a linked system (lgp.sample_paths_vecchia), recorded in profiles/lgp_vecchia_paths_bench.txt.
All legs in one process; every figure the median of REPS warm calls with their min-max spread (one unrecorded call first).

(1) The GP -> DGP -> GP chain of tools/gpu_lgp_paths_bench.py (n = 1000 per emulator, N = 10 systems, sample_size = 10, an
    external input into the DGP), m = 50, at M = 1000 and M = 8192: lgp.sample_paths next to lgp.sample_paths_vecchia.
(2) A one-container system of the bench-shaped DGP (n = 2000, 5 Matern nodes -> one node with connect) next to
    emulator.sample_paths_vecchia on the same model, M, m and path count, their calls alternating: the two make the same
    device calls; the host work in which they differ (generator of the normals, comparison of the systems' nodes) is timed.
(3) The chain with every emulator in Vecchia mode at M = 100 000 (the dense method stops at 8192 rows).
--big: leg 3 only, three calls in all (for a rocprofv3 --kernel-trace --stats run of its own)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPS = 5


def timed(label, f, reps=REPS, warm=1):
    import torch
    for _ in range(warm):
        out = f()
    ms = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        ms.append(1e3 * (time.perf_counter() - t0))
    print('%-84s median %9.1f ms  (min %9.1f, max %9.1f, %d calls)' % (label, np.median(ms), min(ms), max(ms), reps), flush=True)
    return out, ms


def alternating(*legs, reps=2 * REPS - 1):
    """The legs' calls in turn (a, b, a, b, ...), so that a drift of the shared host falls on all of them alike."""
    import torch
    outs, ms = [f() for _, f in legs], [[] for _ in legs]
    for _ in range(reps):
        for i, (_, f) in enumerate(legs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            outs[i] = f()
            torch.cuda.synchronize()
            ms[i].append(1e3 * (time.perf_counter() - t0))
    for (label, _), t in zip(legs, ms):
        print('%-84s median %9.1f ms  (min %9.1f, max %9.1f, %d calls)' % (label, np.median(t), min(t), max(t), reps), flush=True)
    return outs, ms


def chain(n, N):
    from dgp_amd import dgp, gp, kernel, combine
    from dgp_amd.linkgp import container, lgp
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
    return lgp([[container(g1.export(), local_input_idx=np.array([0, 1]))],
                [container(m2.estimate(), local_input_idx=np.array([0]))],
                [container(g3.export(), local_input_idx=np.array([0]))]], N=N)


def main():
    import bench
    from dgp_amd import emulator
    from dgp_amd.linkgp import container, lgp
    big_only = '--big' in sys.argv
    n, N, J, m = 1000, 10, 10, 50
    sysm = chain(n, N)
    rng = np.random.default_rng(3)
    if not big_only:
        for M in (1000, 8192):
            x = [rng.uniform(size=(M, 2)), [rng.uniform(size=(M, 1))], [None]]
            tag = 'GP -> DGP -> GP, n = %d, M = %d, %d paths' % (n, M, N * J)
            for name, f in (('lgp.sample_paths', lambda: sysm.sample_paths(x, sample_size=J)),
                            ('lgp.sample_paths_vecchia (m = %d)' % m, lambda: sysm.sample_paths_vecchia(x, sample_size=J, m=m))):
                out, _ = timed('%s: %s' % (tag, name), f)
                assert out[0].shape == (1, M, N * J) and np.all(np.isfinite(out[0]))
        sysm.set_vecchia(False)   # (drops the dense statistics of the chain)

        model, _, _ = bench.build_model(2000, 5, 0, 0)
        model.train(N=5, ess_burn=5, disable=True)
        est = model.estimate()
        emu = emulator(est, N=N, seed=1)
        np.random.seed(1)
        one = lgp([[container(est, local_input_idx=np.arange(5))]], N=N)
        for M in (1000, 8192):
            xb = np.random.default_rng(5).uniform(size=(M, 5))
            tag = 'bench DGP (n = 2000), M = %d, %d paths, m = %d' % (M, N * J, m)
            (oe, ol), (te, tl) = alternating(
                ('%s: emulator.sample_paths_vecchia' % tag, lambda: emu.sample_paths_vecchia(xb, sample_size=J, m=m)),
                ('%s: lgp.sample_paths_vecchia, one container' % tag, lambda: one.sample_paths_vecchia(xb, sample_size=J, m=m)))
            assert oe[0].shape == (M, N * J) and np.all(np.isfinite(oe[0]))
            assert ol[0].shape == (1, M, N * J) and np.all(np.isfinite(ol[0]))
            print('  system - emulator: medians %+.1f ms, minima %+.1f ms; spread of the emulator\'s own calls: %.1f ms'
                  % (np.median(tl) - np.median(te), min(tl) - min(te), max(te) - min(te)), flush=True)
            # the host work in which the two differ: the normals' generator, and the system's comparison of its nodes
            pos = [[s_[0][0].structure[il][j] for s_ in one.all_layer_set] for il, lay in enumerate(est) for j in range(len(lay))]
            host = {}
            for name, f in (('numpy global generator', lambda: [np.random.standard_normal((N, J, M)) for _ in pos]),
                            ('emulator generator', lambda: [emu._sample_rng.standard_normal((N, J, M)) for _ in pos]),
                            ('lgp._node_classes', lambda: [lgp._node_classes(nodes) for nodes in pos])):
                ts = []
                for _ in range(REPS):
                    t0 = time.perf_counter()
                    f()
                    ts.append(1e3 * (time.perf_counter() - t0))
                host[name] = np.median(ts)
            print('  host, per call: the %d blocks of normals %.1f ms by numpy\'s global generator, %.1f ms by the emulator\'s; '
                  'lgp._node_classes over the %d node positions %.1f ms'
                  % (len(pos), host['numpy global generator'], host['emulator generator'], len(pos), host['lgp._node_classes']),
                  flush=True)
        del emu, one

    sysm.set_vecchia(True)
    M = 100000
    x = [rng.uniform(size=(M, 2)), [rng.uniform(size=(M, 1))], [None]]
    out, _ = timed('GP -> DGP -> GP, every emulator in Vecchia mode, n = %d, M = %d, %d paths: lgp.sample_paths_vecchia (m = %d)'
                   % (n, M, N * J, m), lambda: sysm.sample_paths_vecchia(x, sample_size=J, m=m), reps=2 if big_only else REPS)
    assert out[0].shape == (1, M, N * J) and np.all(np.isfinite(out[0]))


if __name__ == '__main__':
    main()
