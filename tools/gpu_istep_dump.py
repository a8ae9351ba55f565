"""What the I-step leaves on fixed seeds, into one .npz: two checkouts that are meant to run the same chain (a host-side refactoring
against its parent) run this once each on the same machine; `--compare` holds every array of the two dumps to numpy.array_equal.
Per case two imp.sample(burnin=4) calls, then every hidden layer's latents, the imputer's stats, the next three uniforms and
queued_calls.  Cases, each with first batch 12 and 2 (later batches min(4, batch)): the dense two-layer model with one and three
output nodes (n = 300, d = 3; with batch 2 also under DGPAMD_ESS_RESUME=0), a Vecchia node upstairs, Vecchia in both layers, three
layers dense and Vecchia (n = 260), a Poisson top (n = 180).  Needs an MI355X.
usage: gpu_istep_dump.py OUT.npz        gpu_istep_dump.py --compare PARENT.npz CHILD.npz"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def model_of(shape):
    from dgp_amd import dgp, kernel, combine, Poisson
    K = lambda length, name='matern2.5', **kw: kernel(length=np.array([length]), name=name, **kw)
    np.random.seed(7)   # (Vecchia orderings and likelihood warm starts draw from numpy's global generator)
    if shape.startswith('dense'):
        nout, n, d = int(shape[5:]), 300, 3
        X = np.random.default_rng(5).uniform(size=(n, d))
        Y = np.stack([np.sin(3 * X[:, 0] + k) + X[:, 1] ** 2 * (k + 1) for k in range(nout)], 1)
        layers = combine([K(1.0) for _ in range(d)],
                         [K(0.8, 'sexp' if k % 2 else 'matern2.5', scale_est=True, connect=np.arange(d)) for k in range(nout)])
        return dgp(X, (Y - Y.mean(0)) / Y.std(0), layers, seed=3)
    if shape == 'poisson':
        n, d = 180, 2
        rng = np.random.default_rng(23)
        X = rng.uniform(size=(n, d))
        Y = rng.poisson(np.exp(1.2 + np.sin(4 * X[:, 0]) + X[:, 1])).astype(float)[:, None]
        return dgp(X, Y, combine([K(1.0) for _ in range(d)], [K(0.9, scale_est=True, connect=np.arange(d))], [Poisson()]), seed=3)
    n, d = 260, 3
    X = np.random.default_rng(11).uniform(size=(n, d))
    Y = np.sin(3 * X[:, :1]) + X[:, 1:2] ** 2
    ls = [[K(1.0) for _ in range(d)]]
    if shape.startswith('three'):
        ls.append([K(1.2, 'sexp' if k else 'matern2.5', connect=np.arange(d)) for k in range(2)])
    ls.append([K(0.8, scale_est=True, connect=np.arange(d))])
    model = dgp(X, (Y - Y.mean(0)) / Y.std(0), combine(*ls), seed=3, vecchia=shape in ('vecchia_all', 'three_layers_vecchia'), m=12)
    if shape == 'vecchia_top':   # dense hidden layer, Vecchia node upstairs
        top = model.all_layer[-1][0]
        top.vecch, top.m = True, 12
        model.imp.update_ord_nn()
    return model


def dump(out):
    res = {}
    shapes = ['dense1', 'dense3', 'vecchia_top', 'vecchia_all', 'three_layers', 'three_layers_vecchia', 'poisson']
    cases = [(s, b, None) for s in shapes for b in (12, 2)] + [('dense1', 2, '0'), ('dense3', 2, '0')]
    for shape, batch, resume in cases:
        os.environ.pop('DGPAMD_ESS_RESUME', None)
        if resume is not None:
            os.environ['DGPAMD_ESS_RESUME'] = resume
        imp = model_of(shape).imp
        imp.batch, imp.batch_next, imp._batch_default = batch, min(4, batch), False
        for _ in range(2):
            imp.sample(burnin=4)
        tag = '%s.b%d%s' % (shape, batch, '' if resume is None else '.resume' + resume)
        for l, layer in enumerate(imp.all_layer[:-1]):
            res['%s.latents%d' % (tag, l)] = np.stack([nd.output[:, 0] for nd in layer], 1)
        res[tag + '.stats'] = np.array([imp.stats[k] for k in ('proposals', 'updates', 'batches')])
        res[tag + '.uniforms'] = np.array(imp.draws.uniform_peek(3))
        res[tag + '.queued_calls'] = np.array(imp.queued_calls)
        print('%-32s stats %s queued_calls %d' % (tag, res[tag + '.stats'].tolist(), imp.queued_calls), flush=True)
    np.savez(out, **res)
    print('%d arrays -> %s' % (len(res), out))


def compare(parent, child):
    P, C = np.load(parent), np.load(child)
    bad = sorted(set(P.files) ^ set(C.files))
    print('%-44s %-14s %s' % ('array', 'shape', 'numpy.array_equal'))
    for key in sorted(set(P.files) & set(C.files)):
        same = P[key].shape == C[key].shape and P[key].dtype == C[key].dtype and np.array_equal(P[key], C[key])
        print('%-44s %-14s %s' % (key, P[key].shape, 'yes' if same else 'NO'))
        if not same:
            bad.append(key)
    print('%d arrays compared, %d differ or are missing on one side%s' % (len(P.files), len(bad), ': ' + ', '.join(bad) if bad else ''))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(compare(*sys.argv[2:4]) if sys.argv[1] == '--compare' else dump(sys.argv[1]))
