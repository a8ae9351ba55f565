"""Vecchia joint sample paths at the bench's model shape (profiles/vecchia_paths_bench.txt): n = 2000, d = 5 Matern nodes -> one
Matern node with `connect`, briefly trained; emulator(N=10); sample_size = 10 (100 paths), m = 50.
  1. warm sample_paths against warm sample_paths_vecchia at M = 1000 and M = 8192 (dense emulator);
  2. after to_vecchia(): sample_paths_vecchia at M = 100 000 (dense cannot: MAX_POINTS = 8192), and the number of
     substitution levels of the first-layer node;
  3. dgpamd_vpaths_rows of that node (M = 100 000, one set of rows) by device events, priced in executed f64 operations
     against the 78.6 TF/s peak, beside vecchia_gp at the same points and m (the prediction kernel it is modelled on).
--big: leg 2 only (for a rocprofv3 --kernel-trace --stats run of its own)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 78.6e12


def executed_flops_rows(b, D):
    """f64 operations the register-resident rows kernel executes for one row whose set has b members, all 64 lanes counted
    (an fma is 2): b + 1 columns of the block (per column and dimension a difference and a Matern factor, 6; the exponential
    and the product, 30), the LDL^T elimination (pivot j updates the columns past j in groups of eight, about b - j of them)
    and the back substitution."""
    cols = (b + 1) * (6 * D + 30)
    elim = sum(2 * (b - j + 1) for j in range(b))
    back = 2 * b + 2 * b
    return 64 * (cols + elim + back)


def timed(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def main():
    import torch
    import bench
    from dgp_amd import emulator, vpaths
    big_only = '--big' in sys.argv
    n, d, N, J, m = 2000, 5, 10, 10, 50
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    rng = np.random.default_rng(5)
    if not big_only:
        for M in (1000, 8192):
            x = rng.uniform(size=(M, d))
            for name, f in (('sample_paths', lambda: emu.sample_paths(x, sample_size=J)),
                            ('sample_paths_vecchia', lambda: emu.sample_paths_vecchia(x, sample_size=J, m=m))):
                f()
                out, ms = timed(f)
                assert out[0].shape == (M, N * J) and np.all(np.isfinite(out[0]))
                print('%-21s (dense emulator, M = %6d, %d paths, m = %d): warm %9.1f ms' % (name, M, N * J, m, ms))
    emu.to_vecchia()
    M = 100000
    x = rng.uniform(size=(M, d))
    for label in ('first call', 'second call'):
        out, ms = timed(lambda: emu.sample_paths_vecchia(x, sample_size=J, m=m))
        assert out[0].shape == (M, N * J) and np.all(np.isfinite(out[0]))
        print('sample_paths_vecchia (Vecchia emulator, M = %d, %d paths, m = %d): %-11s %9.1f ms' % (M, N * J, m, label, ms))
    if big_only:
        return
    # the first-layer node's rows and schedule, as vpaths.Vecchia.draw_shared builds them
    nd = emu.all_layer[0][0]
    order = np.random.default_rng(7).permutation(M)
    ordt = torch.as_tensor(order, device=e.device)
    xin = e.tensor(x[:, nd.input_dim])
    q = vpaths._scaled(xin[ordt], nd.length)[None]
    xs = vpaths._scaled(e.tensor(nd._X()), nd.length)[None]
    NN = e.vpaths_nn(q, xs, m)
    y = e.tensor(np.stack([emu.latents[s][0][:, 0] for s in range(N)]))[None].contiguous()
    Lr, NNl, t, sd, info = e.vpaths_rows(nd.name, q, xs, NN, y, nd.scale[0], nd.nugget[0])
    sched = e.vecchia_levels(NNl)
    print('first-layer node: %d substitution levels for M = %d rows (m = %d)' % (int(sched[4 * M + 2].item()), M, m))
    D = xs.shape[2]
    reps = 5
    ev0, ev1 = e.event(), e.event()
    e.record(ev0)
    for _ in range(reps):
        e.vpaths_rows(nd.name, q, xs, NN, y, nd.scale[0], nd.nugget[0])
    e.record(ev1)
    ms = e.elapsed_ms(ev0, ev1) / reps
    b = (NN[0] >= 0).sum(1).cpu().numpy()
    fx = float(sum(executed_flops_rows(int(bv), D) * int(c) for bv, c in zip(*np.unique(b, return_counts=True))))
    print('dgpamd_vpaths_rows, M = %d rows, m = %d, D = %d, %d right-hand sides: %.2f ms; executed %.3f TF -> %.2f TF/s = '
          '%.3f of the f64 peak' % (M, m, D, N, ms, fx / 1e12, fx / ms / 1e9, fx / ms / 1e9 / (PEAK / 1e12)))
    w = e.tensor(nd._X())
    NNp = e.nn_query(e.tensor(x[:, nd.input_dim] / nd.length), e.tensor(nd._X() / nd.length), m)
    args = (nd.name, xin, w, NNp, e.tensor(emu.latents[0][0][:, 0]), nd.scale[0], nd.length, nd.nugget[0],
            e.tensor(np.ones(n)))
    e.vecchia_gp(*args)
    e.record(ev0)
    for _ in range(reps):
        e.vecchia_gp(*args)
    e.record(ev1)
    print('vecchia_gp (prediction), same %d points, pm = %d: %.2f ms' % (M, m, e.elapsed_ms(ev0, ev1) / reps))
    e.record(ev0)
    for _ in range(reps):
        e.vpaths_nn(q, xs, m)
    e.record(ev1)
    print('dgpamd_vpaths_nn, one query set of M = %d rows against n = %d: %.2f ms' % (M, n, e.elapsed_ms(ev0, ev1) / reps))


if __name__ == '__main__':
    main()
