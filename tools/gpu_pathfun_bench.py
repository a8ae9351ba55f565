"""Function-valued posterior draws at the bench's model shape (profiles/pathfun_bench.txt; DESIGN I.12): n = 2000, d = 5
Matern nodes -> one Matern node with `connect`, briefly trained; emulator(N=10); sample_size = 10 (100 paths).
  1. per n_features F in (2048, 8192): the time to create the paths (sample_functions), then the time to evaluate them at
     M = 1000 and M = 8192 rows, alternating with warm sample_paths and sample_paths_vecchia (m = 50) on the same emulator
     and rows; at M = 100 000 alternating with sample_paths_vecchia alone (the dense draw stops at 8192 rows);
  2. dgpamd_pathfun_eval alone by device events at M = 100 000, F = 2048: a first-layer node (shared rows, the MFMA kernel)
     and the output node (per-path rows, the lane kernel), priced in executed f64 operations against the 78.6 TF/s peak.
--big: only the M = 100 000 evaluation at F = 2048 and leg 2 (for a rocprofv3 --kernel-trace --stats run of its own, and
for comparing builds of the library through DGPAMD_LIB).
--grad: the input gradients alone (profiles/pathgrad_bench.txt; DESIGN I.13), F = 2048: at M = 1000, 8192 and 100 000 three
alternating rounds of paths(x), paths.value_and_grad(x) and the forward-difference alternative (paths at x and at x + h e_d,
d + 1 = 6 calls); then dgpamd_pathfun_grad against dgpamd_pathfun_eval by device events at M = 100 000 on a first-layer node
(shared rows) and the output node (per-path rows).
--vecchia: the draws by local conditioning (profiles/vpathfun_bench.txt; DESIGN I.14), F = 2048, m = 50: (a) the bench model in
Vecchia mode -- creating sample_functions_vecchia's paths, then at M = 1000, 8192 and 100 000 three alternating rounds of their
paths(x), sample_paths_vecchia on the same rows, and paths(x) of sample_functions made before the emulator left dense mode;
(b) a gp of configs[4]'s shape (n = 50 000, d = 8, Vecchia mode), 100 paths at M = 100 000; (c) dgpamd_vpathfun_update alone by
device events, shared rows, 100 paths at those rows, against 100 calls of dgpamd_vecchia_gp on the same conditioning sets.
--gradmom: the gradient second moments (profiles/gradmom_bench.txt; DESIGN I.18), F = 2048: at M = 8192 and 100 000 three
alternating rounds of paths.active_subspace(x), of paths.grad(x) followed by the host contraction, and of
paths.value_and_grad(x); then dgpamd_gradmom_tiles alone by device events at Dx = 5 and a synthetic Dx = 64."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 78.6e12
WIDTHS = (2, 4, 6, 8, 10, 16, 32, 64)   # the input widths pathfun.hip compiles (D is padded to the next)
COS_FLOPS = 33    # cos_reduced: 14 fused multiply-adds and 5 additions / multiplications
EXP_FLOPS = 32    # exp_negated: 15 fused multiply-adds and 2 additions / multiplications


def entry_flops(kind, D):
    """f64 operations (an fma is 2) of one generated entry: (feature, correlation)."""
    DT = next(w for w in WIDTHS if w >= D)
    feat = 2 * DT + COS_FLOPS
    corr = (3 * DT + EXP_FLOPS) if kind == 'sexp' else (7 * DT + EXP_FLOPS + 2)
    return feat, corr


def executed_flops(kind, n, M, D, F, P, shared):
    """What dgpamd_pathfun_eval executes, idle lanes and padding counted.  Lane kernel: 256 rows per workgroup, features and
    training rows in tiles of 64, one multiply-add per entry on top.  MFMA kernel: 64 rows per workgroup, tiles of 32, every
    entry generated once per block of 128 paths; the products on v_mfma_f64_16x16x4 over 64 or 128 path columns."""
    up = lambda v, q: -(-v // q) * q
    feat, corr = entry_flops(kind, D)
    if not shared:
        return P * up(M, 256) * (up(F, 64) * (feat + 2) + up(n, 64) * (corr + 2))
    blocks, last = -(-P // 128), (64 if 0 < P % 128 <= 64 else 128)
    gen = blocks * up(M, 64) * (up(F, 32) * feat + up(n, 32) * corr)
    mfma = up(M, 64) * (up(F, 32) + up(n, 32)) * 2 * (128 * (blocks - 1) + last)
    return gen + mfma


def timed(f):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = f()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def grad_arm(emu, e, xs, N, J, n, rng):
    P, F, d = N * J, 2048, 5
    pf = emu.sample_functions(sample_size=J, n_features=F)
    for M in (1000, 8192, 100000):
        x = xs[M]
        steps = [x] + [x + 1e-6 * np.eye(d)[k] for k in range(d)]
        legs = [('paths(x)', lambda: pf(x)),
                ('paths.value_and_grad(x)', lambda: pf.value_and_grad(x)),
                ('%d x paths(x) (forward differences)' % (d + 1), lambda: [pf(xx) for xx in steps])]
        out, (val, g) = legs[0][1](), legs[1][1]()   # warm every shape
        legs[2][1]()
        assert g[0].shape == (M, d, P) and np.all(np.isfinite(g[0])) and np.array_equal(out[0], val[0])
        ms = np.zeros((3, 3))
        for rnd in range(3):   # alternating: each round times every arm once
            for a, (name, f) in enumerate(legs):
                _, ms[rnd, a] = timed(f)
                print('M = %6d, %d paths, round %d: %-36s %10.1f ms' % (M, P, rnd + 1, name, ms[rnd, a]))
        best = ms.min(0)
        print('M = %6d: value_and_grad / paths = %.2f, value_and_grad / %d x paths = %.3f (fastest round of each)'
              % (M, best[1] / best[0], d + 1, best[1] / best[2]))
    M = 100000
    xd = e.tensor(xs[M])
    for (l, k), shared in (((0, 0), True), ((1, 0), False)):
        nf = pf.nodes[l, k]
        D = nf.Omega.shape[1]
        xin = xd[:, :D].contiguous() if shared else e.tensor(rng.normal(size=(P, M, D)))
        times = []
        for f in (lambda: nf(e, xin), lambda: nf.value_and_grad(e, xin)):
            f()
            reps = 3
            ev0, ev1 = e.event(), e.event()
            e.record(ev0)
            for _ in range(reps):
                f()
            e.record(ev1)
            times.append(e.elapsed_ms(ev0, ev1) / reps)
        print('%s rows, %s, %d paths, n = %d, F = %d, M = %d, D = %d: dgpamd_pathfun_eval %.2f ms, dgpamd_pathfun_grad %.2f ms '
              '(%.2f x, against %d evaluations for forward differences)'
              % ('shared' if shared else 'per-path', nf.hyper[0], P, n, F, M, D, times[0], times[1], times[1] / times[0], D + 1))


def device_ms(e, f, reps=3):
    f()
    ev0, ev1 = e.event(), e.event()
    e.record(ev0)
    for _ in range(reps):
        f()
    e.record(ev1)
    return e.elapsed_ms(ev0, ev1) / reps


HBM = 6.3e12     # bytes / s a streaming kernel reaches on the MI355X (8.0e12 on paper)


def gradmom_arm(emu, e, xs, N, J, rng):
    """--gradmom (profiles/gradmom_bench.txt; DESIGN I.18), F = 2048: at M = 8192 and 100 000 three alternating rounds of
    paths.active_subspace(x), of the route without it -- paths.grad(x), then the contraction on the host -- and of
    paths.value_and_grad(x) alone; then dgpamd_gradmom_tiles alone by device events, the output preallocated, at the model's
    Dx = 5 and at a synthetic Dx = 64 (100 paths, one output), against the time to read J once at the streaming HBM rate."""
    from dgp_amd import _lib
    P, F, d = N * J, 2048, 5
    pf = emu.sample_functions(sample_size=J, n_features=F)

    def host_route(x):
        g = pf.grad(x)[0]                                       # (M, Dx, P) on the host
        return np.einsum('mdp,mep->pde', g, g) / len(x)
    for M in (8192, 100000):
        x = xs[M]
        legs = [('paths.active_subspace(x)', lambda: pf.active_subspace(x)),
                ('paths.grad(x) + host einsum', lambda: host_route(x)),
                ('paths.value_and_grad(x)', lambda: pf.value_and_grad(x))]
        res, C = legs[0][1](), legs[1][1]()   # warm every shape
        legs[2][1]()
        assert res.C.shape == (1, P, d, d) and np.abs(res.C[0] - C).max() <= 1e-9 * np.abs(C).max()
        ms = np.zeros((3, 3))
        for rnd in range(3):   # alternating: each round times every arm once
            for a, (name, f) in enumerate(legs):
                _, ms[rnd, a] = timed(f)
                print('M = %6d, %d paths, round %d: %-30s %10.1f ms' % (M, P, rnd + 1, name, ms[rnd, a]))
        best = ms.min(0)
        print('M = %6d: (grad + host einsum) / active_subspace = %.2f, active_subspace / value_and_grad = %.3f (fastest round of each)'
              % (M, best[1] / best[0], best[0] / best[2]))
    for M, Dx in ((8192, 5), (100000, 5), (8192, 64)):
        f, Jd, shift = e.tensor(rng.normal(size=(P, M, 1))), e.tensor(rng.normal(size=(P, M, 1, Dx))), e.zeros(P, 1)
        part = e.gradmom_tiles(f, Jd, shift)
        ptr = [t.data_ptr() for t in (f, Jd, shift, part)]
        ms = device_ms(e, lambda: e._chk(_lib.lib.dgpamd_gradmom_tiles(e.h, P, M, 1, Dx, *ptr)), reps=50)
        read, wrote = 8.0 * Jd.numel(), 8.0 * part.numel()
        print('dgpamd_gradmom_tiles, %d paths, M = %d, K = 1, Dx = %d: %.1f us; J is %.1f MB, read once at %.1f TB/s in %.1f us '
              '-> %.2f of the kernel time (partial sums written: %.1f MB; read + written %.2f TB/s)'
              % (P, M, Dx, 1e3 * ms, read / 1e6, HBM / 1e12, 1e6 * read / HBM, 1e3 * read / HBM / ms, wrote / 1e6,
                 (read + wrote) / ms / 1e9))


def vecchia_arm(emu, xs, N, J, m, rng):
    from dgp_amd import gp, kernel
    P, F = N * J, 2048
    dense = emu.sample_functions(sample_size=J, n_features=F)   # (made while the emulator is dense: it keeps its own copies)
    emu.to_vecchia()
    for label in ('first', 'second'):
        pv, ms = timed(lambda: emu.sample_functions_vecchia(sample_size=J, n_features=F, m=m))
        print('(a) sample_functions_vecchia(sample_size=%d, n_features=%d, m=%d): creating %d paths, %-6s call %9.1f ms'
              % (J, F, m, P, label, ms))
    for M in (1000, 8192, 100000):
        x = xs[M]
        legs = [('sample_functions_vecchia: paths(x)', lambda: pv(x)),
                ('sample_paths_vecchia', lambda: emu.sample_paths_vecchia(x, sample_size=J, m=m)),
                ('sample_functions (dense): paths(x)', lambda: dense(x))]
        for name, f in legs:   # warm every shape
            out = f()
            assert out[0].shape == (M, P) and np.all(np.isfinite(out[0]))
        for rnd in range(3):   # alternating: each round times every method once
            for name, f in legs:
                _, ms = timed(f)
                print('(a) M = %6d, %d paths, round %d: %-36s %10.1f ms' % (M, P, rnd + 1, name, ms))
    n4, d4, M, P = 50000, 8, 100000, 100
    X4 = rng.uniform(size=(n4, d4))
    Y4 = (np.sin(X4.sum(1)) + 0.05 * rng.normal(size=n4))[:, None]
    model = gp(X4, Y4, kernel(length=np.full(d4, 0.5), name='matern2.5', scale=1.0, nugget=1e-4), vecchia=True, m=m)
    paths, ms = timed(lambda: model.sample_functions_vecchia(sample_size=P, n_features=F, m=m))
    print('(b) gp n = %d, d = %d: sample_functions_vecchia(sample_size=%d, n_features=%d, m=%d) %9.1f ms' % (n4, d4, P, F, m, ms))
    x4 = rng.uniform(size=(M, d4))
    for label in ('first', 'second', 'third'):
        out, ms = timed(lambda: paths(x4))
        assert out.shape == (M, P) and np.all(np.isfinite(out))
        print('(b) paths(x), M = %d, %d paths: %-6s call %9.1f ms' % (M, P, label, ms))
    k = model.kernel
    e, nf = k.engine, paths.node
    t = e.tensor
    xs4, xd, Wd = t(x4 / k.length), t(x4), t(k._X())
    NN = e.nn_query(xs4, nf.Ws, m)
    prior, y, ones = e.zeros(M, P), t(Y4[:, 0]), t(np.ones(n4))
    one = device_ms(e, lambda: e.vpathfun_update(k.name, xs4, nf.Ws, NN, nf.r, prior, k.scale[0], k.nugget[0], (0.0, 1e-10, 1e-8)))
    many = device_ms(e, lambda: [e.vecchia_gp(k.name, xd, Wd, NN, y, k.scale[0], k.length, k.nugget[0], ones) for _ in range(P)])
    print('(c) shared rows, %s, M = %d, pm = %d, D = %d, %d paths: dgpamd_vpathfun_update %.2f ms; %d calls of dgpamd_vecchia_gp %.2f ms '
          '(%.2f ms each): one launch / %d calls = %.3f' % (k.name, M, m, d4, P, one, P, many, many / P, P, one / many))
    assert one < many, 'the one launch must be faster than the calls it replaces'


def main():
    import bench
    from dgp_amd import emulator
    big_only = '--big' in sys.argv
    n, d, N, J, m = 2000, 5, 10, 10, 50
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    rng = np.random.default_rng(5)
    xs = {M: rng.uniform(size=(M, d)) for M in (1000, 8192, 100000)}
    emu.sample_paths(xs[1000], sample_size=J)   # (the lazily built statistics are shared by every method below)
    if '--grad' in sys.argv:
        return grad_arm(emu, e, xs, N, J, n, rng)
    if '--vecchia' in sys.argv:
        return vecchia_arm(emu, xs, N, J, m, rng)
    if '--gradmom' in sys.argv:
        return gradmom_arm(emu, e, xs, N, J, rng)
    pfs = {}
    for F in ((2048,) if big_only else (2048, 8192)):
        for label in ('first', 'second'):
            pfs[F], ms = timed(lambda: emu.sample_functions(sample_size=J, n_features=F))
            print('sample_functions(sample_size=%d, n_features=%d): creating %d paths, %-6s call %9.1f ms' % (J, F, N * J, label, ms))
    if big_only:
        for label in ('first call', 'second call'):
            out, ms = timed(lambda: pfs[2048](xs[100000]))
            print('paths(x), F = 2048, M = 100000: %-11s %9.1f ms' % (label, ms))
    for M in (() if big_only else (1000, 8192, 100000)):
        x = xs[M]
        legs = [('paths(x), F = %d' % F, (lambda F=F: pfs[F](x))) for F in (2048, 8192)]
        if M <= 8192:
            legs.append(('sample_paths', lambda: emu.sample_paths(x, sample_size=J)))
        legs.append(('sample_paths_vecchia, m = %d' % m, lambda: emu.sample_paths_vecchia(x, sample_size=J, m=m)))
        for name, f in legs:   # warm every shape
            out = f()
            assert out[0].shape == (M, N * J) and np.all(np.isfinite(out[0]))
        for rnd in range(2 if M == 100000 else 3):   # alternating: each round times every method once
            for name, f in legs:
                _, ms = timed(f)
                print('M = %6d, %d paths, round %d: %-28s %10.1f ms' % (M, N * J, rnd + 1, name, ms))
    # the evaluation kernels alone
    M, F = 100000, 2048
    pf, xd = pfs[F], e.tensor(xs[100000])
    for (l, k), shared in (((0, 0), True), ((1, 0), False)):
        nf = pf.nodes[l, k]
        D = nf.Omega.shape[1]
        xin = xd[:, :D].contiguous() if shared else e.tensor(rng.normal(size=(N * J, M, D)))
        nf(e, xin)
        reps = 3
        ev0, ev1 = e.event(), e.event()
        e.record(ev0)
        for _ in range(reps):
            nf(e, xin)
        e.record(ev1)
        ms = e.elapsed_ms(ev0, ev1) / reps
        fx = executed_flops(nf.hyper[0], n, M, D, F, N * J, shared)
        fa = N * J * M * (n + F) * D
        print('dgpamd_pathfun_eval, %s rows, %s, %d paths, n = %d, F = %d, M = %d, D = %d: %.2f ms; executed %.3f TF -> %.2f TF/s '
              '= %.3f of the f64 peak (work count (n + F) M D per path: %.3f T)'
              % ('shared' if shared else 'per-path', nf.hyper[0], N * J, n, F, M, D, ms, fx / 1e12, fx / ms / 1e9,
                 fx / ms / 1e9 / (PEAK / 1e12), fa / 1e12))


if __name__ == '__main__':
    main()
