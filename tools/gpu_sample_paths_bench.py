"""Joint sample paths at the bench's model shape (profiles/sample_paths_bench_size.txt): n = 2000, d = 5 Matern nodes -> one
Matern node with `connect`, briefly trained; emulator(N=10); sample_paths(x, sample_size=10) at M = 1000 test points.
Prints the wall time of the call (first: with the lazily built statistics; then warm) and the dgpamd_joint_cov rate of
one output-layer call (10 paths of one imputation) in executed flops against the 78.6 TF/s f64-MFMA peak."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 78.6e12


def executed_flops(n, M, r, batch):
    """MFMA flops dgpamd_joint_cov issues: trmm_kernel over the lower 64-tiles of L^-1 times all Mc columns, then
    joint_syrk_kernel's lower tiles of V^T V and the mean tiles, each over every 64-block of n."""
    nb = -(-n // 64)
    Mp, Mc = -(-M // 64) * 64, -(-M // 64) * 64 + (-(-r // 64) * 64 if r else 0)
    nbm, nbr = Mp // 64, (Mc - Mp) // 64
    trmm = nb * (nb + 1) // 2 * (Mc // 64) * 2 * 64 ** 3
    syrk = (nbm * (nbm + 1) // 2 + nbm * nbr) * nb * 2 * 64 ** 3
    return batch * (trmm + syrk)


def main():
    import torch
    import bench
    from dgp_amd import emulator
    n, d, M, N, J = 2000, 5, 1000, 10, 10
    model, X, _ = bench.build_model(n, d, 0, 0)
    model.train(N=5, ess_burn=5, disable=True)
    emu = emulator(model.estimate(), N=N, seed=1)
    e = emu.engine
    x = np.random.default_rng(5).uniform(size=(M, d))
    for label in ('first call (statistics built on the way)', 'warm call', 'warm call'):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = emu.sample_paths(x, sample_size=J)
        torch.cuda.synchronize()
        print('sample_paths(M=%d, N=%d, sample_size=%d): %-42s %8.1f ms' % (M, N, J, label, 1e3 * (time.perf_counter() - t0)))
    assert out[0].shape == (M, N * J) and np.all(np.isfinite(out[0]))
    # one output-layer call alone: the 10 paths of imputation 0
    nd = emu.all_layer[1][0]
    st = emu._joint_stats(1, 0)['per'][0]
    xs = torch.cat((e.tensor(np.random.default_rng(6).normal(size=(J, M, d))), e.tensor(x)[None].expand(J, M, d)), 2).contiguous()
    y = st['y'].reshape(1, -1)
    A = e.empty(J, e.padded_dim(M), e.padded_dim(M))
    args = (nd.name, xs, st['W'], st['Linv'], y, nd.length, nd.scale[0], nd.nugget[0])
    e.joint_cov(*args, A=A)
    ev0, ev1 = e.event(), e.event()
    reps = 5
    e.record(ev0)
    for _ in range(reps):
        e.joint_cov(*args, A=A)
    e.record(ev1)
    ms = e.elapsed_ms(ev0, ev1) / reps
    fx = executed_flops(n, M, 1, J)
    fa = J * (n * n * M + n * M * M)
    print('dgpamd_joint_cov, %d paths, n = %d, M = %d, D = %d: %.2f ms; executed %.3f TF -> %.1f TF/s = %.3f of the f64-MFMA peak '
          '(algorithmic n^2 M + n M^2 per path: %.3f TF -> %.1f TF/s)'
          % (J, n, M, 2 * d, ms, fx / 1e12, fx / ms / 1e9, fx / ms / 1e9 / (PEAK / 1e12), fa / 1e12, fa / ms / 1e9))
    _, info = e.potrf(M, A, batch=J)
    t0 = e.event()
    e.record(t0)
    for _ in range(reps):
        e.joint_cov(*args, A=A)
        e.potrf(M, A, batch=J)
    e.record(ev1)
    print('joint_cov + potrf of the 10 matrices (M = %d): %.2f ms per call' % (M, e.elapsed_ms(t0, ev1) / reps))


if __name__ == '__main__':
    main()
