"""The outputs of every Vecchia entry point of the C library on seeded inputs, into one .npz: two builds that are meant to compute
the same bits (a refactoring of the kernels against its parent) run this once each on the same machine -- the build is chosen with
DGPAMD_LIB -- and tools/gpu_vecchia_compare.py compares every array.  Each entry point runs under DGPAMD_VECCHIA_LDS = 0 and 1; the
neighbour searches also with DGPAMD_NN_STORE_ONCE unset, 1 and 2 (a context keeps the switches it was created under: one engine each).
Entry points: nn_ordered, nn_query (also nx = 3000 and 6000: the two selection kernels), vecchia_llik, llik_batch, nllik, lmatrix,
het_rows, vecchia_gp, vecchia_linkgp (both kinds, Dz = 0 and Dz > 0), vpaths_nn, vpaths_rows.  Shapes: n of a few hundred, m in
{3, 12, 25, 30, 40} (the sample-path rows also 51 and 80), pm in {10, 50, 60}, D in {1, 8, 20}.  Needs an MI355X.
usage: gpu_vecchia_dump.py OUT.npz"""
import contextlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = {}
KINDS = ('sexp', 'matern2.5')


def put(name, *tensors):
    for i, t in enumerate(tensors):
        OUT['%s.%d' % (name, i)] = t.detach().cpu().numpy()


@contextlib.contextmanager
def engine_under(**switches):
    """A fresh Engine created with DGPAMD_<name> = value in the environment (None: unset), closed afterwards."""
    from dgp_amd.ops import Engine
    before = {k: os.environ.pop('DGPAMD_' + k, None) for k in switches}
    try:
        os.environ.update({'DGPAMD_' + k: str(v) for k, v in switches.items() if v is not None})
        e = Engine(0)
    finally:
        for k, v in before.items():
            os.environ.pop('DGPAMD_' + k, None)
            if v is not None:
                os.environ['DGPAMD_' + k] = v
    try:
        yield e
        e.sync()
    finally:
        e.close()


def searches(e, tag):
    rng = np.random.default_rng(1)
    for n, D, m in ((301, 1, 3), (301, 8, 25), (301, 20, 40), (3000, 8, 25), (6000, 8, 30), (6000, 20, 12)):
        X = rng.uniform(size=(n, D))
        X[7] = X[3]   # a tie
        Q = rng.uniform(size=(257, D))
        put('%s.nn_ordered.n%d.D%d.m%d' % (tag, n, D, m), e.nn_ordered(e.tensor(X), m))
        put('%s.nn_query.n%d.D%d.m%d' % (tag, n, D, m), e.nn_query(e.tensor(Q), e.tensor(X), m))


def het_rows(e, kind, X, impNN, length, scale, gamma, y):
    import torch
    from dgp_amd import ops
    n, D = X.shape
    mp1 = impNN.shape[1]
    length = ops._f64(length)
    Lrows, t = e.empty(n, mp1), e.empty(n)
    NNl, info = e.empty(n, mp1, dtype=torch.int64), e.empty(1, dtype=torch.int32)
    e._chk(e._enter() or ops.lib.dgpamd_vecchia_het_rows(e.h, ops.KIND[kind], n, D, mp1 - 1, ops._dp(X), ops._dp(impNN), ops._hp(length),
                                                         len(length), float(scale), ops._dp(gamma), ops._dp(y), ops._dp(Lrows),
                                                         ops._dp(NNl), ops._dp(t), ops._dp(info)))
    return Lrows, NNl, t, info


def rows(e, tag):
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(2)
    n = 301
    for D in (1, 8, 20):
        X = rng.uniform(size=(n, D))
        y = np.sin(3 * X[:, 0]) + 0.1 * rng.normal(size=n)
        w, gamma = rng.uniform(0.5, 2.0, size=n), rng.uniform(0.01, 0.3, size=n)
        XB = np.stack([X, X + 0.01 * rng.normal(size=X.shape), rng.uniform(size=X.shape)])
        for ard in (False, True) if D > 1 else (False,):
            ln = rng.uniform(0.4, 1.2, size=D) if ard else np.array([0.7])
            dX, dy, dw = e.tensor(X), e.tensor(y), e.tensor(w)
            for m in (3, 12, 25, 30, 40):
                NN = e.nn_ordered(e.tensor(X / ln), m)
                impNN = e.tensor(O.imp_nn_array(X / ln, m), dtype=NN.dtype)
                for kind in KINDS:
                    name = '%s.%s.D%d.%s.m%d' % (tag, kind, D, 'ard' if ard else 'iso', m)
                    put(name + '.llik', e.vecchia_llik(kind, dX, dy, NN, ln, 1e-3, dw))
                    put(name + '.llik_batch', e.vecchia_llik_batch(kind, e.tensor(XB), dy, NN, ln, 1e-3, dw))
                    for nugget_est in (False, True):
                        put('%s.nllik%d' % (name, nugget_est), e.vecchia_nllik(kind, dX, dy, NN, ln, 1e-3, dw, nugget_est)[0])
                    put(name + '.lmatrix', e.vecchia_lmatrix(kind, dX, NN, ln, 1e-3))
                    put(name + '.het_rows', *het_rows(e, kind, dX, impNN, ln, 1.3, e.tensor(gamma), dy))


def predictors(e, tag):
    rng = np.random.default_rng(3)
    n, M = 301, 203
    for pm in (10, 50, 60):
        for D in (1, 8, 20):
            W, x = rng.uniform(size=(n, D)), rng.uniform(size=(M, D))
            y, w = rng.normal(size=n), rng.uniform(0.5, 2.0, size=n)
            ln = rng.uniform(0.4, 1.2, size=D)
            NN = e.nn_query(e.tensor(x / ln), e.tensor(W / ln), pm)
            NN[5, pm - 3:] = -1   # a short set
            for kind in KINDS:
                put('%s.%s.vecchia_gp.pm%d.D%d' % (tag, kind, pm, D),
                    *e.vecchia_gp(kind, e.tensor(x), e.tensor(W), NN, e.tensor(y), 1.4, ln, 1e-3, e.tensor(w)))
        for Dw, Dz in ((1, 0), (8, 0), (3, 2), (8, 8), (20, 0), (12, 8)):
            w1, mu, v = rng.uniform(size=(n, Dw)), rng.uniform(size=(M, Dw)), rng.uniform(0.0, 0.05, size=(M, Dw))
            v[:, 0] = 0.0 if Dw > 1 else v[:, 0]   # a deterministic input
            wg, z = (rng.uniform(size=(n, Dz)), rng.uniform(size=(M, Dz))) if Dz else (None, None)
            y, w = rng.normal(size=n), rng.uniform(0.5, 2.0, size=n)
            ln = rng.uniform(0.4, 1.2, size=Dw + Dz)
            allw, allq = (w1, mu) if not Dz else (np.hstack((w1, wg)), np.hstack((mu, z)))
            NN = e.nn_query(e.tensor(allq / ln), e.tensor(allw / ln), pm)
            NN[5, pm - 3:] = -1
            T = lambda a: None if a is None else e.tensor(a)   # noqa: E731
            for kind in KINDS:
                put('%s.%s.vecchia_linkgp.pm%d.Dw%d.Dz%d' % (tag, kind, pm, Dw, Dz),
                    *e.vecchia_linkgp(kind, T(mu), T(v), T(z), T(w1), T(wg), NN, T(y), 1.4, ln, 1e-3, T(w)))


def paths(e, tag):
    import torch
    rng = np.random.default_rng(4)
    n, M, P = 45, 70, 3
    group = torch.as_tensor(np.array([1, 0, 1], np.int32), device=e.device)
    for m in (3, 12, 25, 30, 40, 51, 80):
        for D in (1, 8, 20):
            X, Q = rng.uniform(size=(2, n, D)) * 2, rng.uniform(size=(P, M, D)) * 2
            Y = rng.normal(size=(2, 3, n))
            omega = rng.choice([1.0, 0.5, 1 / 3], size=n)
            NN = e.vpaths_nn(e.tensor(Q), e.tensor(X), m, group)
            put('%s.vpaths_nn.m%d.D%d' % (tag, m, D), NN)
            for kind in KINDS:
                for om in (None, omega):
                    put('%s.%s.vpaths_rows.m%d.D%d.omega%d' % (tag, kind, m, D, om is not None),
                        *e.vpaths_rows(kind, e.tensor(Q), e.tensor(X), NN, e.tensor(Y), 1.7, 3e-3, None if om is None else e.tensor(om),
                                       group))


if __name__ == '__main__':
    for lds in (0, 1):
        with engine_under(VECCHIA_LDS=lds, NN_STORE_ONCE=None) as e:
            tag = 'lds%d' % lds
            rows(e, tag)
            predictors(e, tag)
            paths(e, tag)
        for once in (None, 1, 2):
            with engine_under(VECCHIA_LDS=lds, NN_STORE_ONCE=once) as e:
                searches(e, 'lds%d.once%s' % (lds, once))
    np.savez(sys.argv[1], **OUT)
    print('%d arrays -> %s (library: %s)' % (len(OUT), sys.argv[1], os.environ.get('DGPAMD_LIB', 'the tree\'s own')))
