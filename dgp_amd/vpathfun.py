"""Function-valued posterior draws by local conditioning (emulator.sample_functions_vecchia, gp.sample_functions_vecchia;
DESIGN I.14).

pathfun.py's draw  f(x) = sqrt(scale) (phi(x)^T theta + c(x, W) R^-1 r),  r = y / sqrt(scale) - Phi(W) theta - sqrt(nugget omega) * eps,
needs the n x n factor of R.  A Vecchia model predicts by conditioning each row on its m nearest training rows (gp_vecch), and
Matheron's rule goes through that predictor unchanged:
    f(x) = sqrt(scale) (phi(x)^T theta + b(x)^T r[N(x)]),   b(x) = A_N^-1 c(W_N, x),
N(x) the m nearest training rows of x in coordinates divided by the lengths, A_N their correlation block with diagonal
1 + nugget omega_j.  The mean over (theta, eps) is gp_vecch's mean for every F; the variance tends to gp_vecch's (less the
nugget term noise=True adds back).  Creation is O(n F) per path and keeps nothing n x n; a row costs O(m^3 + m D) whatever n
is.  The draw is a deterministic function of x, piecewise smooth: it jumps where N(x) changes, by about the Vecchia error,
so it has no gradient (grad / value_and_grad raise).

VecchiaNodePaths has NodePaths' interface and is built from the same draws (pathfun.draw_node) on the training side
vpaths.Vecchia takes, train = (W, omega); pathfun.PathFunctions and pathfun.GpPaths evaluate it as they evaluate NodePaths.
"""
import warnings

import numpy as np
import torch

from .paths import JITTERS
from .vpaths import _scaled

LADDER = (0.0,) + tuple(JITTERS)   # added to a conditioning block's diagonal, tried in order row by row (unit scale)


SCAN_BELOW = 20000   # training rows below which the one-wave scan finds a row's neighbours faster than dgpamd_nn_query


def neighbours(e, q, ws, m):
    """N(x) of the scaled rows q (R, D) among the scaled training rows ws (n, D): (R, min(m, n)) int64, nearest first, in
    exact (distance, index) order whichever kernel finds them.  dgpamd_nn_query streams large training sets (13.7 ms for
    100 000 rows against n = 50 000, where the scan takes 62.7), but below n = 20 000 it selects with one workgroup per row,
    1.7 us a row at n = 2000, D = 10; there dgpamd_vpaths_nn with one test row per path -- its candidates are then the n
    training rows alone -- scans them with one wave per row in 27 ns (DESIGN I.14).  With m >= n every row takes all n
    rows in index order: not kernel._pred_nn's cyclic list, which would tie a row's order of summation to its position in
    the call."""
    n = ws.shape[0]
    if m >= n:
        return torch.arange(n, device=q.device).expand(q.shape[0], n).contiguous()
    if n < SCAN_BELOW and m <= 256:
        return e.vpaths_nn(q[:, None, :], ws[None], m).reshape(q.shape[0], m)
    return e.nn_query(q, ws, m)


def residuals(e, hyper, W, Omega, b, theta, y, eps, omega):
    """r (P, n) = y / sqrt(scale) - Phi(W) theta - sqrt(nugget omega) * eps: what pathfun.weights solves against, here used as
    it is.  Phi(W) theta is dgpamd_pathfun_eval with n = 0 at x = W."""
    kind, length, scale, nugget = hyper
    r = y / np.sqrt(scale) - e.pathfun_eval(kind, W, None, Omega, b, theta, None, length, 1.0)
    r -= eps * (np.sqrt(nugget) if omega is None else torch.sqrt(nugget * omega))
    return r.contiguous()


class VecchiaNodePaths:
    """P locally conditioned function-valued draws of one GP node, with pathfun.NodePaths' interface.  hyper =
    paths.hyper(node); Omega (F, D), b (F,), theta (P, F) the prior draw; Ws the training inputs divided by the lengths,
    (n, D) for every path or (G, n, D) with group (host ints (P,), sorted) picking each path's; omega (n,) or None; r the
    residuals, neighbour-major (n, P) with one training set and (P, n) with groups; m the conditioning-set size.  All its own
    copies, nothing n x n.  where(p) names path p's node in an error.  Every evaluation leaves its device status words in
    `pending`; status() reads them (one transfer) and empties the list."""

    def __init__(self, hyper, Omega, b, theta, Ws, omega, r, m, group=None, where=lambda p: 'the node'):
        kind, length, scale, nugget = hyper
        self.hyper = (kind, np.array(length, dtype=np.float64), float(scale), float(nugget))
        self.Omega, self.b, self.theta, self.Ws, self.omega, self.r, self.m = Omega, b, theta, Ws, omega, r, int(m)
        self.group = None if group is None else np.asarray(group, dtype=np.int32).copy()
        self.where, self.pending = where, []

    @classmethod
    def build_shared(cls, e, hyper, train, Y, draws, rep, m, where='the node'):
        """One training set for every path, train = (W (n, D), omega (n,) or None), rows Y (R, n) of right-hand sides: path q
        of the R * rep is conditioned on row q // rep.  draws = draw_node's, on the device."""
        Om, b, theta, eps = draws
        W, omega = train
        r = residuals(e, hyper, W, Om, b, theta, Y.repeat_interleave(rep, 0), eps, omega)
        return cls(hyper, Om, b, theta, _scaled(W, hyper[1]), None if omega is None else omega.clone(), r.T.contiguous(), m,
                   where=lambda p: where)

    @classmethod
    def build_per_group(cls, e, hyper, train, y, draws, group, m, where):
        """Every group its own training set: train[g] = (W, omega), y[g] (n,) (lists, or paths.PerGroup; omega is the first
        group's: a node holds one set of replicate weights); group host ints (P,), the paths of group 0, then those of
        group 1, ...; where(p) names path p."""
        Om, b, theta, eps = draws
        ends = np.searchsorted(group, np.arange(group[-1] + 2))
        Ws, rs, omega = [], [], train[int(group[0])][1]
        for g in range(len(ends) - 1):
            W, mine = train[g][0], slice(ends[g], ends[g + 1])
            Ws.append(_scaled(W, hyper[1]))
            rs.append(residuals(e, hyper, W, Om, b, theta[mine], y[g], eps[mine], omega))
        return cls(hyper, Om, b, theta, torch.stack(Ws), None if omega is None else omega.clone(), torch.cat(rs), m, group, where)

    def _update(self, e, xs, Ws, r, prior, out, first):
        """One dgpamd_vpathfun_update call on scaled rows xs ((M, D) shared, (J, M, D) per path) against the scaled training
        set Ws; `first` is the index of its first path."""
        kind, _, scale, nugget = self.hyper
        NN = neighbours(e, xs.reshape(-1, xs.shape[-1]), Ws, self.m)
        out, info = e.vpathfun_update(kind, xs, Ws, NN, r, prior, scale, nugget, LADDER, self.omega, out=out)
        self.pending.append((info, first, 0 if xs.dim() == 2 else xs.shape[1]))
        return out

    def __call__(self, e, x):
        """The paths at x: (M, D) shared by every path, or (P, M, D).  Returns (P, M) (shared x: a view of the kernel's (M, P))."""
        kind, length, _, _ = self.hyper
        prior = e.pathfun_eval(kind, x, None, self.Omega, self.b, self.theta, None, length, 1.0)
        xs = _scaled(x, length)
        if x.dim() == 2:
            assert self.group is None, 'rows shared by every path need one training set'
            return self._update(e, xs, self.Ws, self.r, prior.T.contiguous(), None, 0).T
        out = e.empty(*prior.shape)
        if self.group is None:   # (one training set, every path its own rows)
            return self._update(e, xs, self.Ws, self.r.T.contiguous(), prior, out, 0)
        ends = np.searchsorted(self.group, np.arange(self.group[-1] + 2))
        for g in range(len(ends) - 1):   # the rows of one group's paths in one launch
            mine = slice(ends[g], ends[g + 1])
            self._update(e, xs[mine], self.Ws[g], self.r[mine], prior[mine], out[mine], int(ends[g]))
        return out

    def value_and_grad(self, e, x):
        raise NotImplementedError('sample_functions_vecchia: a draw made by local conditioning is only piecewise differentiable '
                                  '(it jumps where a row\'s nearest training rows change), so grad and value_and_grad are not '
                                  'offered; sample_functions gives differentiable draws of a dense model')

    def noise_sd(self):
        return np.sqrt(self.hyper[2] * self.hyper[3])

    def status(self, e):
        """(rows that needed a jitter rung, the name of the first path with a block that failed the whole ladder or None) over
        the evaluations since the last call."""
        if not self.pending:
            return 0, None
        info = e.fetch(torch.stack([p[0] for p in self.pending])).reshape(-1, 2)
        pending, self.pending = self.pending, []
        failed = None
        for (_, first, M), (_, bad) in zip(pending, info):
            if bad > 0 and failed is None:
                failed = self.where(first + (int(bad) - 1) // M if M else first)
        return int(info[:, 0].sum()), failed


def check_status(e, nodes):
    """After an evaluation call: numpy.linalg.LinAlgError if a conditioning block failed the whole jitter ladder, one
    RuntimeWarning if some rows needed a rung of it."""
    rungs = 0
    for nf in nodes:
        n, failed = nf.status(e)
        rungs += n
        if failed is not None:
            raise np.linalg.LinAlgError('sample_functions_vecchia: a conditioning block of %s is not positive definite, even with '
                                        '%g added to its diagonal' % (failed, LADDER[-1] * nf.hyper[2]))
    if rungs:
        warnings.warn('dgp_amd: sample_functions_vecchia: %d conditioning block(s) did not factor and were rebuilt with up to %g '
                      'times the scale added to their diagonal' % (rungs, LADDER[-1]), RuntimeWarning)


def emulator_nodes(emu, sample_size, n_features, m):
    """The (layer, node) -> VecchiaNodePaths mapping of an emulator, on the training side sample_paths_vecchia hands its
    drawer: the node's inputs with global columns, the imputation's latents below layer 1."""
    from . import pathfun, paths
    e, S, J = emu.engine, emu.N, int(sample_size)

    def node(l, k, nd, draw):
        omega = None if nd.rep is None else e.tensor(nd.W_diag)
        if l == 0:
            W = e.tensor(nd._X())
            return VecchiaNodePaths.build_shared(e, paths.hyper(nd), (W, omega), e.tensor(np.stack([emu._ys(s, l, k) for s in range(S)])),
                                                 draw(W.shape[1]), J, m, 'layer 1, node %d (shared by every imputation)' % (k + 1))
        train = paths.PerGroup(lambda s: (e.tensor(emu._train_in(s, l, nd, True)), omega))
        return VecchiaNodePaths.build_per_group(e, paths.hyper(nd), train, paths.PerGroup(lambda s: e.tensor(emu._ys(s, l, k))),
                                                draw(emu._train_in(0, l, nd, True).shape[1]), np.repeat(np.arange(S), J), m,
                                                lambda p: 'layer %d, node %d, imputation %d' % (l + 1, k + 1, p // J + 1))
    return pathfun.build_nodes(emu, J, n_features, node)
