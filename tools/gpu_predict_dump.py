"""Everything the predictive-moment side computes on fixed seeds, into one .npz: two checkouts that are meant to compute the same (a
host-side refactoring against its parent) run this once each on the same machine and tools/gpu_predict_compare.py compares every
array.  Public API only.  A call that raises is recorded as its exception's text: both checkouts must refuse alike.
Emulators (N imputations, M = 37 test rows): a 'two-connect' SExp (n = 60); b three Matern-2.5 layers with per-dimension
lengthscales (n = 130: linkgp_cells groups the training points); c Hetero top with replicates; d Categorical top; e one GP layer under
a Poisson node.  Per emulator predict (plain, full_layer, aggregation=False, sampling), loo (also with replicate rows), metric ALM /
MICE / VIGF, nllik; after to_vecchia() the same with m = 7 and m >= n, and for a and b under DGPAMD_NN_SHARE=0.  gp models dense and
Vecchia, with and without replicates: predict, loo, metric.  lgp systems: f one DGP emulator; g GP -> GP; h two GPs feeding a DGP
emulator whose output node's connect hits both feeding outputs and an external input; i the same with that emulator in Vecchia
mode; g10 the recorded GP -> DGP -> GP chains.  Needs an MI355X.
usage: gpu_predict_dump.py OUT.npz [case ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from test_gpu_pathfun import _gp, _model   # noqa: E402

OUT = {}
M = 37


def put(name, value):
    """An array, or a (nested) list of arrays: one entry per array, the list indices in its name."""
    if isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            put('%s.%d' % (name, i), v)
    else:
        OUT[name] = np.asarray(value)


def call(name, fn):
    np.random.seed(3)   # (likelihood nodes and gp / lgp sampling draw from numpy's global generator)
    try:
        put(name, fn())
    except Exception as exc:   # noqa: BLE001
        put(name, '%s: %s' % (type(exc).__name__, exc))


def emulator_model(which):
    """(X as given to dgp, trained model, imputations)."""
    from dgp_amd import dgp, kernel, combine, Hetero, Poisson
    if which == 'a':
        return _model('two-connect', kind='sexp') + (2,)
    if which == 'd':
        return _model('categorical') + (2,)
    rng = np.random.default_rng(6)
    if which == 'b':
        K = lambda **kw: kernel(length=np.array([0.8, 1.3]), name='matern2.5', nugget=1e-4, **kw)
        X = rng.uniform(size=(130, 2))
        Y = np.sin(5 * X[:, :1]) + X[:, 1:] ** 2 + 0.02 * rng.normal(size=(130, 1))
        layers, N = combine([K(), K()], [K(), K()], [K(scale_est=True)]), 3
    elif which == 'c':
        x = np.sort(rng.uniform(size=45))
        x = np.concatenate((x, x[:20]))
        X = x[:, None]
        Y = (np.sin(6 * x) + (0.05 + 0.5 * x ** 2) * rng.normal(size=len(x)))[:, None]
        layers, N = combine([kernel(length=np.array([0.5]), name='sexp', scale_est=True),
                             kernel(length=np.array([0.5]), name='sexp', scale_est=True)], [Hetero()]), 2
    else:
        X = rng.uniform(size=(40, 2))
        Y = rng.poisson(np.exp(1 + np.sin(4 * X[:, [0]]))).astype(float)
        layers, N = combine([kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-4, scale_est=True)], [Poisson()]), 2
    model = dgp(X, Y, layers, seed=4)
    model.train(N=3, ess_burn=3, disable=True)
    return X, model, N


def emulator_calls(tag, emu, model, X, x, y, **m):
    """m: {} for a dense emulator, m=... for a Vecchia one."""
    call(tag + '.predict', lambda: emu.predict(x, **m))
    call(tag + '.predict_full', lambda: emu.predict(x, full_layer=True, **m))
    call(tag + '.predict_per_imputation', lambda: emu.predict(x, aggregation=False, **m))
    call(tag + '.predict_sampling', lambda: emu.predict(x, method='sampling', sample_size=3, full_layer=True, **m))
    Xu = np.unique(X, axis=0) if model.indices is not None else X
    for name, Xl in (('loo', Xu), ('loo_replicates', np.concatenate((Xu, Xu[:5])) if model.indices is not None else None)):
        if Xl is not None:
            call('%s.%s' % (tag, name), lambda: emu.loo(Xl, **m))
            call('%s.%s_sampling' % (tag, name), lambda: emu.loo(Xl, method='sampling', sample_size=3, **m))
    for method in ('ALM', 'MICE', 'VIGF'):
        call('%s.metric_%s' % (tag, method), lambda: emu.metric(x, method=method, obj=model, score_only=True, **m))
    call(tag + '.nllik', lambda: emu.nllik(x, y, **m))


def emulator_case(which):
    from dgp_amd import emulator
    X, model, N = emulator_model(which)
    emu = emulator(model.estimate(), N=N, seed=5)
    put(which + '.N', N)
    top = emu.all_layer[-1][0]
    put(which + '.likelihood', any(nd.type == 'likelihood' for nd in emu.all_layer[-1]))
    put(which + '.categorical', getattr(top, 'name', None) == 'Categorical')
    if getattr(top, 'name', None) == 'Categorical':
        put(which + '.categorical_link', '%s:%s' % (top.num_classes, top.link))
        put(which + '.categorical_input_dim', np.asarray(top.input_dim))
    rng = np.random.default_rng(8)
    x = rng.uniform(size=(M, X.shape[1]))
    y = rng.poisson(2.0, size=(M, 1)).astype(float) if which == 'e' else rng.normal(size=(M, 1))
    emulator_calls(which + '.dense', emu, model, X, x, y)
    emu.to_vecchia()
    for m in (7, 200):
        emulator_calls('%s.vecchia_m%d' % (which, m), emu, model, X, x, y, m=m)
    if which in 'ab':
        os.environ['DGPAMD_NN_SHARE'] = '0'
        try:
            emulator_calls(which + '.vecchia_m7_noshare', emu, model, X, x, y, m=7)
        finally:
            del os.environ['DGPAMD_NN_SHARE']


def gp_case(case):
    kind = case.split('-')[0]
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    connect = None
    if 'replicates' in case:
        X, connect = np.concatenate((X, X[:15])), np.array([2])
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    g = _gp(kind, X, Y, connect=connect)
    x = rng.uniform(size=(M, 3))
    for tag, m in (('dense', {}), ('vecchia_m7', dict(m=7)), ('vecchia_m200', dict(m=200))):
        if tag == 'vecchia_m7':
            np.random.seed(2)
            g.to_vecchia()
        tag = '%s.%s' % (case, tag)
        call(tag + '.predict', lambda: g.predict(x, **m))
        call(tag + '.predict_sampling', lambda: g.predict(x, method='sampling', sample_size=3, **m))
        call(tag + '.loo', lambda: g.loo(**m))
        for method in ('ALM', 'MICE', 'VIGF'):
            call('%s.metric_%s' % (tag, method), lambda: g.metric(x, method=method, score_only=True, **m))


def dgp_container(structure, idx):
    """container(structure, idx) with a seeded imputer (the constructor's draws from fresh entropy), built as the tests' _chain does."""
    from dgp_amd.imputation import imputer, DrawStream
    from dgp_amd.linkgp import container
    c = container.__new__(container)
    c.type, c.structure, c.vecch, c.local_input_idx = 'dgp', structure, False, idx
    c.imp = imputer(structure, True, draws=DrawStream(9))
    c.imp.sample(burnin=50)
    return c


def lgp_system(which):
    """(system, x as lgp.predict takes it)."""
    from dgp_amd import dgp, kernel, combine
    from dgp_amd.linkgp import container, lgp
    rng = np.random.default_rng(7)
    np.random.seed(0)
    if which == 'f':
        X, model = _model('two-connect')
        return lgp([[dgp_container(model.estimate(), np.array([0, 1]))]], N=2), rng.uniform(size=(M, 2))
    if which == 'g':
        X1 = rng.uniform(size=(40, 2))
        g1 = _gp('matern2.5', X1, np.sin(4 * X1[:, :1]) + X1[:, 1:] ** 2)
        W2 = rng.uniform(-1.5, 2.0, size=(40, 1))
        g2 = _gp('sexp', W2, np.cos(2 * W2))
        return lgp([[container(g1.export(), local_input_idx=np.array([0, 1]))],
                    [container(g2.export(), local_input_idx=np.array([0]))]]), rng.uniform(size=(M, 2))
    xa, xb = rng.uniform(size=(40, 1)), rng.uniform(size=(40, 1))
    gA, gB = _gp('sexp', xa, np.sin(4 * xa)), _gp('matern2.5', xb, xb ** 2 - 0.5)
    W = np.concatenate((rng.uniform(-1, 1, size=(45, 2)), rng.uniform(size=(45, 1))), 1)   # (two feeding outputs, one external column)
    Y = np.sin(3 * W[:, :1]) * W[:, 1:2] + W[:, 2:] ** 2 + 0.02 * rng.normal(size=(45, 1))
    K = lambda **kw: kernel(length=np.array([1.0]), name='matern2.5', nugget=1e-4, **kw)
    layers = combine([K(input_dim=np.array([0, 1]), connect=np.array([2])) for _ in range(2)], [K(scale_est=True, connect=np.arange(3))])
    model = dgp(W, Y, layers, seed=4)
    model.train(N=3, ess_burn=3, disable=True)
    sysm = lgp([[container(gA.export(), local_input_idx=np.array([0])), container(gB.export(), local_input_idx=np.array([1]))],
                [dgp_container(model.estimate(), np.array([0, 1]))]], N=2)
    if which == 'i':
        sysm.set_vecchia([[False, False], [True]])
    return sysm, [rng.uniform(size=(M, 2)), [rng.uniform(size=(M, 1))]]


def g10_chain(tag):
    from test_gpu_lgp_paths import _chain
    from dgp_amd.ops import default_engine

    def golden(name):
        with np.load(os.path.join(ROOT, 'tests', 'golden', name + '.npz'), allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    return _chain(default_engine(), golden, tag)


def lgp_case(which):
    sysm, x = g10_chain(which[4:]) if which.startswith('g10_') else lgp_system(which)
    m = dict(m=7) if which == 'i' else {}
    call(which + '.predict', lambda: sysm.predict(x, **m))
    call(which + '.predict_full', lambda: sysm.predict(x, full_layer=True, **m))
    call(which + '.predict_sampling', lambda: sysm.predict(x, method='sampling', sample_size=3, **m))


CASES = dict([(c, lambda c=c: emulator_case(c)) for c in 'abcde']
             + [(c, lambda c=c: gp_case(c)) for c in ('matern2.5-replicates-connect', 'sexp-plain')]
             + [(c, lambda c=c: lgp_case(c)) for c in ('f', 'g', 'h', 'i', 'g10_sexp', 'g10_matern')])

if __name__ == '__main__':
    for name in sys.argv[2:] or CASES:
        CASES[name]()
    np.savez(sys.argv[1], **OUT)
    raised = sorted(k for k, v in OUT.items() if v.dtype.kind == 'U')
    print('%d arrays -> %s; %d calls raised: %s' % (len(OUT), sys.argv[1], len(raised), ', '.join(raised)))
