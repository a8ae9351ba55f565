"""Vecchia joint sample paths of GP nodes (emulator.sample_paths_vecchia, gp.sample_paths_vecchia; DESIGN I.11).

The M test rows are taken in one order pi.  Position i is drawn from its Gaussian conditional given c(i), the min(m, n + i)
nearest of the n training rows and the path's test rows drawn before it (coordinates [inputs | global inputs] / length):
    v_i = sum_train b_ij y_j + sum_test b_ij v_j + sqrt(d_i) z_i,   b_i = A^-1 a,   d_i = scale (1 + nugget - a^T b_i),
A the correlation block over c(i) (diagonal 1 + nugget * omega_j on training members, 1 + nugget on test members) and
a = k(c(i), u_i).  With m >= n + M - 1 this is the dense joint of paths.py exactly.  dgpamd_vpaths_nn finds the sets,
dgpamd_vpaths_rows turns each into one row of a sparse unit-lower system and dgpamd_vecchia_spsolve_levels solves it:
linear in M, no cap on M.  Nothing is kept across calls.  Vecchia is the drawer, with the interface of paths.Dense
(train = (W, omega): training inputs with global columns, and the nugget's replicate weights or None).
"""
import warnings

import numpy as np
import torch

from .paths import JITTERS, check_2d


def check_m(m):
    if int(m) < 1:
        raise ValueError('sample_paths_vecchia: the conditioning-set size m must be at least 1 (got %r)' % (m,))


def check_args(x, m):
    """sample_paths' refusal of a non-2-D x, and m >= 1 (before anything touches the device)."""
    check_2d(x)
    check_m(m)


def _scaled(t, length):
    """t / length over the last axis (the coordinates of kernel._pred_nn)."""
    return (t / torch.as_tensor(np.asarray(length, dtype=np.float64), device=t.device)).contiguous()


def _chunk(e, M, m, D, nrhs):
    """Paths per call: neighbour and row arrays (~16 (m + 1) bytes per row and path), the scaled inputs, right-hand sides
    and level schedule of a chunk within half of the free device memory."""
    per = M * (8 * m + 16 * (m + 1) + 8 * (D + 2 * nrhs + 4) + 16)
    free = torch.cuda.mem_get_info(e.device)[0]
    return int(max(1, free // 2 // per))


def _rows(e, kind, q, xs, NN, y, scale, nugget, omega, group, where_of):
    """dgpamd_vpaths_rows under paths._factor's policy: a block that does not factor is rebuilt with scale * JITTERS added to
    its diagonal, one warning each; one that still does not raises numpy.linalg.LinAlgError naming where_of(path)."""
    M = q.shape[1]
    out = e.vpaths_rows(kind, q, xs, NN, y, scale, nugget, omega, group)
    bad = int(e.fetch(out[4])[0])
    for jit in JITTERS:
        if bad == 0:
            return out
        warnings.warn('dgp_amd: sample_paths_vecchia: a conditioning block of %s did not factor; retried with %g added to '
                      'its diagonal' % (where_of((bad - 1) // M), jit * scale), RuntimeWarning)
        out = e.vpaths_rows(kind, q, xs, NN, y, scale, nugget, omega, group, jitter=jit)
        bad = int(e.fetch(out[4])[0])
    if bad == 0:
        return out
    raise np.linalg.LinAlgError('sample_paths_vecchia: a conditioning block of %s is not positive definite, even with %g '
                                'added to its diagonal' % (where_of((bad - 1) // M), JITTERS[-1] * scale))


def _solve(e, Lrows, NNl, rhs):
    """x = the level-scheduled substitution of the rows (nmat, M, m+1) for rhs (nmat, nrhs, M)."""
    sched = e.vecchia_levels(NNl)
    return e.vecchia_spsolve_levels(Lrows, NNl, np.ones(Lrows.shape[0]), rhs, sched)


class Vecchia:
    """The drawer of one sample_paths_vecchia call: conditioning sets of size m, the rows of x drawn in the order `order`
    (M host ints), the same for every node and path."""

    def __init__(self, m, order):
        self.m, self.order = int(m), np.asarray(order)

    def draw_shared(self, e, hyper, x, train, Y, Z, rep, where='the node'):
        """One node whose paths all see the test inputs x (M, D) (a first-layer node, a gp): one neighbour search and one
        set of rows for every path.  train (W (n, D), omega (n) or None), Y (r, n) right-hand sides -- path q uses row
        q // rep --, Z (P, M) device normals indexed by x's rows; where names the node in an error.  Returns (P, M), rows
        in x's order."""
        (kind, length, scale, nugget), (W, omega) = hyper, train
        M, n = x.shape[0], W.shape[0]
        mm = min(self.m, n + M - 1)
        ordt = torch.as_tensor(self.order, device=x.device)
        q, xs = _scaled(x[ordt], length)[None], _scaled(W, length)[None]
        NN = e.vpaths_nn(q, xs, mm)
        Lrows, NNl, t, sd, _ = _rows(e, kind, q, xs, NN, Y.reshape(1, -1, n).contiguous(), scale, nugget, omega, None,
                                     lambda p: where)
        src = torch.arange(Z.shape[0], device=x.device) // rep
        rhs = Z[:, ordt] + (t[0] / sd)[src]
        v = _solve(e, Lrows, NNl, rhs[None].contiguous())[0]
        out = torch.empty_like(v)
        out[:, ordt] = v
        return out

    def draw_per_path(self, e, hyper, xs, train, y, Z, group=None, where=lambda p: 'path %d' % (p + 1)):
        """One node, every path its own test inputs xs (P, M, D) (a deeper node): per chunk of paths one neighbour search
        and one set of rows per path, the paths as the matrices of one substitution.  group None: train (W (n, D), omega)
        and y (n) serve every path; else host ints (P,) and train, y indexable by group (read chunk by chunk, only for the
        chunk's groups; omega is the first group's: one call holds one set of replicate weights).  Z (P, M) device normals
        indexed by x's rows; where(p) names path p in an error.  Returns (P, M), rows in x's order."""
        kind, length, scale, nugget = hyper
        P, M, D = xs.shape
        if group is None:
            train, y, group = [train], [y], np.zeros(P, np.int64)
        group = np.asarray(group)
        W0, omega = train[int(group[0])]
        n = W0.shape[0]
        mm = min(self.m, n + M - 1)
        ordt = torch.as_tensor(self.order, device=xs.device)
        out = e.empty(P, M)
        step = _chunk(e, M, mm, D, 1)
        for p0 in range(0, P, step):
            p1 = min(P, p0 + step)
            gs = np.unique(group[p0:p1])
            local = torch.as_tensor(np.searchsorted(gs, group[p0:p1]).astype(np.int32), device=xs.device)
            xg = torch.stack([_scaled(train[int(g)][0], length) for g in gs])
            yg = torch.stack([y[int(g)].reshape(-1) for g in gs]).reshape(len(gs), 1, n).contiguous()
            q = _scaled(xs[p0:p1][:, ordt], length)
            NN = e.vpaths_nn(q, xg, mm, local)
            Lrows, NNl, t, sd, _ = _rows(e, kind, q, xg, NN, yg, scale, nugget, omega, local,
                                         lambda p, p0=p0: where(p0 + p))
            rhs = Z[p0:p1][:, ordt] + t[:, 0] / sd
            out[p0:p1, ordt] = _solve(e, Lrows, NNl, rhs[:, None].contiguous())[:, 0]
        return out
