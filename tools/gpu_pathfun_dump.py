"""Everything sample_functions computes on fixed seeds, into one .npz: two checkouts that are meant to compute the same (a host-side
refactoring against its parent) run this once each on the same machine and every array is compared with numpy.array_equal.
Cases: the 'two-connect', 'three' and 'hetero' emulators and both gp models of tests/test_gpu_pathfun.py.  Per case: paths(x) with and
without full_layer, value_and_grad(x, full_layer=True) where the draws are differentiable, paths(x, noise=True), every node's Omega, b,
theta, v, and the generator's next draw after creation.  The likelihood node of 'hetero' samples from numpy's global generator, seeded
before every call.  Needs an MI355X.
usage: gpu_pathfun_dump.py OUT.npz"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]
from test_gpu_pathfun import _gp, _model   # noqa: E402

OUT = {}


def put(name, value):
    """An array, or a (nested) list of arrays: one entry per array, the list indices in its name."""
    if isinstance(value, (list, tuple)):
        for i, v in enumerate(value):
            put('%s.%d' % (name, i), v)
    else:
        OUT[name] = np.asarray(value)


def put_node(name, nf):
    for attr in ('Omega', 'b', 'theta', 'v', 'W'):
        put('%s.%s' % (name, attr), getattr(nf, attr).cpu().numpy())


def emulator_case(which):
    from dgp_amd import emulator
    X, model = _model(which)
    emu = emulator(model.estimate(), N=2, seed=5)
    x = np.random.default_rng(8).uniform(size=(40, X.shape[1]))
    pf = emu.sample_functions(sample_size=3, n_features=200)
    put(which + '.next_draw', copy.deepcopy(emu._sample_rng).standard_normal(8))
    for (l, k), nf in pf.nodes.items():
        put_node('%s.node%d_%d' % (which, l, k), nf)
    np.random.seed(3)
    put(which + '.paths', pf(x))
    np.random.seed(3)
    put(which + '.paths_full', pf(x, full_layer=True))
    if all(nd.type == 'gp' for layer in pf.layers for nd in layer):
        put(which + '.value_and_grad', pf.value_and_grad(x, full_layer=True))
    np.random.seed(3)
    put(which + '.paths_noise', pf(x, full_layer=True, noise=True))


def gp_case(case):
    kind = case.split('-')[0]
    rng = np.random.default_rng(11)
    X = rng.uniform(size=(60, 3))
    connect = None
    if 'replicates' in case:
        X, connect = np.concatenate((X, X[:15])), np.array([2])
    Y = (np.sin(3 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.normal(size=len(X)))[:, None]
    m = _gp(kind, X, Y, connect=connect)
    np.random.seed(21)
    paths = m.sample_functions(sample_size=3, n_features=200)
    put(case + '.next_draw', np.random.standard_normal(8))
    put_node(case + '.node', paths.node)
    x = rng.uniform(size=(35, 5))   # columns 3 and 4 are not read by the model
    put(case + '.paths', paths(x))
    put(case + '.value_and_grad', paths.value_and_grad(x))
    np.random.seed(5)
    put(case + '.paths_noise', paths(x, noise=True))


if __name__ == '__main__':
    for which in ('two-connect', 'three', 'hetero'):
        emulator_case(which)
    for case in ('matern2.5-replicates-connect', 'sexp-plain'):
        gp_case(case)
    np.savez(sys.argv[1], **OUT)
    print('%d arrays -> %s' % (len(OUT), sys.argv[1]))
