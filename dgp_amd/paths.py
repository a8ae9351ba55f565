"""Joint posterior sample paths of GP nodes (emulator.sample_paths, gp.sample_paths).

A node with training inputs W (global columns appended), outputs y and R = L L^T has at test inputs X* the joint posterior
    mu = K(X*,W) R^-1 y = V^T w,   Sigma = scale (K(X*,X*) + nugget I - V^T V),   V = L^-1 K(W,X*),  w = L^-1 y.
The statistics are L^-1 (what dgpamd_potri leaves in the factored buffer); dgpamd_joint_cov forms V, Sigma and mu,
dgpamd_potrf factors Sigma and dgpamd_mvn_paths draws mu + chol(Sigma) e.  Dense nodes only: Vecchia nodes, and more
than MAX_POINTS rows, are drawn by the sparse algorithm of vpaths.py (sample_paths_vecchia).

Dense here and vpaths.Vecchia are the two drawers of one interface, so that a walk (pathwalk.walk, lgp._paths_node) holds
"the drawer" without knowing which:
    draw_shared(e, hyper, x, train, Y, Z, rep, where)         one set of test inputs for every path
    draw_per_path(e, hyper, xs, train, y, Z, group, where)    every path its own test inputs
hyper = hyper(node); train is what the drawer needs of a training set -- (W, Linv) here, (W, omega) there; the normals Z
and the result are (P, M), one row per path, in both.
"""
import warnings

import numpy as np
import torch

from .ops import raise_not_pd

MAX_POINTS = 8192   # test points per call (Sigma is M x M on the device)
JITTERS = (1e-10, 1e-8)   # multiples of scale added to Sigma's diagonal when it does not factor


def hyper(nd):
    """What a drawer needs of a GP node (or a gp model's kernel) beside its training set."""
    return nd.name, nd.length, nd.scale[0], nd.nugget[0]


class PerGroup:
    """g -> build(g): a group's training set or outputs, made when draw_per_path's chunk asks for it (and dropped with the
    chunk unless the builder keeps it)."""

    def __init__(self, build):
        self.build = build

    def __getitem__(self, g):
        return self.build(int(g))


def check_2d(x):
    if x.ndim != 2:
        raise Exception('The testing input has to be a numpy 2d-array')


def check_points(x):
    check_2d(x)
    if len(x) > MAX_POINTS:
        raise ValueError('sample_paths draws at most %d test points jointly (got %d): split x' % (MAX_POINTS, len(x)))


def factor_inverse(e, kind, Xl, Xg, W, length, nugget, where):
    """L^-1 of R = K(W, W) + nugget diag(W_diag) as a padded (Np x Np) device buffer (lower tiles valid).  Raises
    numpy.linalg.LinAlgError naming `where` when R is not positive definite (predict falls back to pinvh there; a joint
    Gaussian draw has no sound equivalent)."""
    n = Xl.shape[0]
    Np = e.padded_dim(n)
    A = e.empty(Np, Np)
    e.kmatrix(kind, Xl, None, Xg, length, nugget, W=W, out=A, full=False)
    work = e.potrf_workspace(n, 1)
    _, info = e.potrf(n, A, work=work)
    bad = int(e.fetch(info)[0])
    if bad < 0:
        raise_not_pd(bad)
    if bad > 0:
        raise np.linalg.LinAlgError('sample_paths: the training correlation matrix of %s is not positive definite (leading '
                                    'minor %d); predict() uses its pseudo-inverse there, a joint draw cannot' % (where, bad))
    e.potri(n, A, e.workspace(('pathsAinv', n), Np * Np * 8).view(torch.float64)[:Np * Np].view(Np, Np), 0, work)
    return A


def inverse_with_rhs(e, kind, Xl, Xg, W, length, nugget, Y, key):
    """(R^-1, R^-1 Y) of R = K(W, W) + nugget diag(W_diag) for prediction: R^-1 a padded (Np x Np) device buffer, valid
    [:n, :n]; Y (r, n) right-hand sides that ride along the one factorisation, R^-1 Y (r, n).  When R is not numerically
    positive definite the pseudo-inverse takes over, as in the reference (kernel_class.py:749-751).  key names the cached
    workspace that holds the factor."""
    n, r = Xl.shape[0], Y.shape[0]
    Np = e.padded_dim(n)
    A = e.workspace((key, n), Np * Np * 8)
    Ainv = e.empty(Np, Np)
    e.kmatrix(kind, Xl, None, Xg, length, nugget, W=W, out=A, full=False, Y=Y)
    work = e.potrf_workspace(n, 1)
    _, info = e.potrf(n, A, work=work)
    e.potri(n, A, Ainv, r, work)
    if int(info.cpu().numpy()[0]):
        K = e.kmatrix(kind, Xl, None, Xg, length, nugget, W=W, full=True)
        Ainv.zero_()
        Ainv[:n, :n] = e.pinvh(K)
        return Ainv, (Y @ Ainv[:n, :n]).contiguous()
    return Ainv, (-Ainv[n:n + r, :n]).contiguous()


def _chunk(e, n, M, r, c):
    """Items per dgpamd_joint_cov / dgpamd_potrf call: <= 64 and within half of the free device memory."""
    Mp = e.padded_dim(M)
    npad, Mc = -(-n // 64) * 64, -(-M // 64) * 64 + (-(-r // 64) * 64 if r else 0)
    per = 8 * (Mp * Mp + 2 * npad * Mc + M * (r + c) * 2) + e.potrf_workspace(M, 1).numel()
    free = torch.cuda.mem_get_info(e.device)[0]
    return int(max(1, min(64, free // 2 // per)))


def _factor(e, M, A, scale, build):
    """dgpamd_potrf on the joint_cov buffers A (batch, Mp, Mp).  A lost hand-off (info < 0) switches the engine to the
    per-block-step factorisation and rebuilds the buffers once, as dgp.train does; a buffer that does not factor
    (info > 0) is rebuilt alone and retried with scale * JITTERS added to its diagonal, one warning each."""
    B = A.shape[0]
    _, info = e.potrf(M, A, batch=B)
    info = e.fetch(info).astype(np.int64)
    if (info < 0).any():
        warnings.warn('dgp_amd: sample_paths: the one-launch factorisation lost a hand-off; this engine now factors with one '
                      'launch per block step (set_potrf_mode(0))', RuntimeWarning)
        e.sync()
        e.set_potrf_mode(0)
        build(None, A)
        _, info = e.potrf(M, A, batch=B)
        info = e.fetch(info).astype(np.int64)
        if (info < 0).any():
            raise_not_pd(int(info[info < 0][0]))
    for b in np.nonzero(info > 0)[0]:
        ok = False
        for jit in JITTERS:
            warnings.warn('dgp_amd: sample_paths: a joint covariance did not factor; retried with %g added to its diagonal'
                          % (jit * scale), RuntimeWarning)
            Ab = A[b:b + 1]
            build(int(b), Ab)
            Ab[0].diagonal()[:M] += jit * scale
            _, i1 = e.potrf(M, Ab, batch=1)
            i1 = int(e.fetch(i1)[0])
            if i1 < 0:
                raise_not_pd(i1)
            if i1 == 0:
                ok = True
                break
        if not ok:
            raise np.linalg.LinAlgError('sample_paths: a joint posterior covariance is not positive definite, even with %g '
                                        'added to its diagonal' % (JITTERS[-1] * scale))


def _stack(ts):
    """The groups' tensors stacked, or the one tensor they all are (shared by every group: joint_cov's group stride 0)."""
    return ts[0] if all(t is ts[0] for t in ts) else torch.stack(ts)


class Dense:
    """The dense drawer: train = (W, Linv), the training inputs with global columns and factor_inverse's L^-1.  `where` is
    not used: what can fail here by a node's own doing already failed, by name, in factor_inverse."""

    def draw_shared(self, e, hyper, x, train, Y, Z, rep, where=None):
        """One node, one set of test inputs x (M, D) shared by every path, rows Y (r, n) of right-hand sides: Sigma is
        factored once; path q is mean column q // rep + chol(Sigma) Z[q].  Z: (P, M) device normals.  Returns (P, M) (a
        view of the device call's (M, P): the one place that transposes)."""
        (kind, length, scale, nugget), (W, Linv) = hyper, train
        M = x.shape[0]

        def build(_, A):
            e.joint_cov(kind, x, W, Linv, Y, length, scale, nugget, A=A)

        A = e.empty(1, e.padded_dim(M), e.padded_dim(M))
        _, mean = e.joint_cov(kind, x, W, Linv, Y, length, scale, nugget, A=A)
        _factor(e, M, A, scale, build)
        return e.mvn_paths(A, mean, Z.T[None].contiguous(), rep=rep)[0].T

    def draw_per_path(self, e, hyper, xs, train, y, Z, group=None, where=None):
        """One node, every path its own test inputs xs (P, M, D) and normals Z (P, M): Sigma is formed and factored per
        path, one joint_cov -> potrf -> mvn_paths chain per chunk of paths.  group None: one group, train (W (n, D),
        Linv (ld, ld)), y (n,).  Else host ints (P,) picking each path's group, and train, y are indexable by group: read
        chunk by chunk, only for the groups of the chunk (a tensor that several groups hold is passed once).  Returns
        (P, M)."""
        kind, length, scale, nugget = hyper
        P, M, _ = xs.shape
        if group is None:
            train, y, group = [train], [y], np.zeros(P, np.int64)
        group = np.asarray(group)
        W0, L0 = train[int(group[0])]
        n, ld = W0.shape[0], L0.shape[-1]
        out = e.empty(P, M)
        step = _chunk(e, n, M, 1, 1)
        gcap = max(1, torch.cuda.mem_get_info(e.device)[0] // 4 // (ld * ld * 8))   # groups' L^-1 stacked in one chunk
        p0 = 0
        while p0 < P:
            p1, seen = min(P, p0 + step), set()
            for i in range(p0, p1):
                seen.add(int(group[i]))
                if len(seen) > gcap:
                    p1 = i
                    break
            gs = np.unique(group[p0:p1])
            local = np.searchsorted(gs, group[p0:p1])
            sets = [train[int(g)] for g in gs]
            Wc, Lc, Yc = _stack([t[0] for t in sets]), _stack([t[1] for t in sets]), _stack([y[int(g)] for g in gs])
            Yc = Yc.reshape(1, n) if Yc.dim() == 1 else Yc.reshape(len(gs), 1, n)
            xc = xs[p0:p1].contiguous()

            def build(b, A, xc=xc, Wc=Wc, Lc=Lc, Yc=Yc, local=local):
                xb, gb = (xc, local) if b is None else (xc[b:b + 1].contiguous(), local[b:b + 1])
                e.joint_cov(kind, xb, Wc, Lc, Yc, length, scale, nugget, group=gb, A=A)

            A = e.empty(p1 - p0, e.padded_dim(M), e.padded_dim(M))
            _, mean = e.joint_cov(kind, xc, Wc, Lc, Yc, length, scale, nugget, group=local, A=A)
            _factor(e, M, A, scale, build)
            out[p0:p1] = e.mvn_paths(A, mean, Z[p0:p1].reshape(p1 - p0, M, 1).contiguous())[:, :, 0]
            p0 = p1
        return out
