"""The reference-signature operator API (dgp_amd.functions, dgp_amd.vecchia) called exactly as a
dgpsi caller would -- positional arguments, numpy in / numpy out -- with the RAW arguments the golden fixtures recorded
from the reference (g7: functions.gp / link_gp, g4: fmvn, g8: every vecchia.* function).  Needs an MI355X: -m gpu.
Tolerances as in test_gpu_ops.py (the same kernels run underneath); index arrays bit-exact."""
import numpy as np
import pytest

from conftest import case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module', autouse=True)
def _device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')


def matern_link_reference(fn, *args):
    """What a golden file records for a Matern-2.5 linked prediction is the reference's float64 expression of the factors, which is
    off by more than these tolerances where the recorded inputs reach v/l^2 >~ 0.3 (tests/linkfun_ref.py).  The library follows the
    integral, so the expected values are the oracle's `fn` on the same recorded arguments with its three factors on the integral
    (linkfun_ref.oracle_on_the_integral); test_oracle_golden.py pins the unpatched oracle to the recorded values."""
    import linkfun_ref
    from oracle import dgp_oracle as O
    with linkfun_ref.oracle_on_the_integral(O):
        return getattr(O, fn)(*args)


def close(a, b, rtol=1e-10, atol=1e-13):
    np.testing.assert_allclose(np.asarray(a, float), np.asarray(b, float), rtol=rtol, atol=atol)


def test_functions_gp_and_link_gp_with_the_fixtures_raw_arguments(golden):
    from dgp_amd import functions as F
    g = golden('g7_predict')
    for c in range(int(g['n_cases'])):
        d = case(g, 'c%d_' % c)
        name, nl, X = str(d['name']), int(d['n_local']), d['X']
        w1, gw1 = X[:, :nl], (X[:, nl:] if 'z' in d else None)
        z = d['z'] if 'z' in d else None
        # functions.py:380 -- scale / nugget arrive as 1-element arrays (kernel_class.py:622)
        m, v = F.gp(d['x'], z, w1, gw1, d['Rinv'], d['Rinv_y'], d['scale'], d['length'], d['nugget'], name)
        assert m.shape == v.shape == (len(d['x']),)
        close(m, d['gp_m'], rtol=1e-9, atol=1e-11)
        close(v, d['gp_v'], rtol=1e-7, atol=1e-9)
        # functions.py:397 -- scale / nugget as scalars (kernel_class.py:667); R2sexp / Psexp are not needed
        lm, lv = F.link_gp(d['lm_in'], d['lv_in'], z, w1, gw1, d['Rinv'], d['Rinv_y'], None, None, d['scale'][0], d['length'],
                           d['nugget'][0], name)
        ref_m, ref_v = d['link_m'], d['link_v']
        if name == 'matern2.5':
            ref_m, ref_v = matern_link_reference('link_gp_predict', d['lm_in'], d['lv_in'], z, w1, gw1, d['Rinv'], d['Rinv_y'], d['scale'],
                                                 d['length'], d['nugget'], name)
        close(lm, ref_m, rtol=1e-8, atol=1e-10)
        close(lv, ref_v, rtol=1e-6, atol=1e-8)


def test_functions_fmvn_and_update_f(golden):
    from dgp_amd import functions as F
    g = golden('g4_fmvn')
    cov = g['cov']
    # the reference draws its normals inside fmvn (numba's generator); here they come from numpy's global one -- reproduce
    # the draw, then the fixture's own (cov, z) -> sample pins the arithmetic
    st = np.random.get_state()
    np.random.seed(123)
    zz = np.random.randn(len(cov))
    np.random.seed(123)
    out = F.fmvn(cov)
    np.random.set_state(st)
    Lc = np.linalg.cholesky(cov)
    close(out, Lc @ zz, rtol=1e-9, atol=1e-11)
    close(Lc @ g['z'], g['sample'], rtol=1e-9, atol=1e-11)
    with pytest.raises(np.linalg.LinAlgError):
        F.fmvn(np.array([[1.0, 2.0], [2.0, 1.0]]))
    close(F.update_f(g['f'], g['nu'], float(g['theta'])), g['fp'], rtol=1e-14, atol=1e-15)


def test_vecchia_functions_with_the_fixtures_raw_arguments(golden):
    from dgp_amd import vecchia as V
    g = golden('g8_vecchia')
    NN = V.nn(g['nn_x'], int(g['nn_m']))
    assert NN.dtype == np.int64
    np.testing.assert_array_equal(NN, g['NNarray'])
    np.testing.assert_array_equal(V.get_pred_nn(g['pq'], g['nn_x'], 12), g['pred_nn'])
    for c in range(int(g['n_cases'])):
        d = case(g, 'v%d_' % c)
        name = str(d['name'])
        X, y, NNa = d['X'], d['y'], d['NN']
        n = len(X)
        sc, ng, ln = float(d['scale']), float(d['nugget']), d['length']
        nugget_est, scale_est = bool(d['flags'][0]), bool(d['flags'][1])
        ones = np.ones(n)
        np.testing.assert_array_equal(V.nn(X / ln, 6), NNa)
        close(V.vecchia_llik(X, y, NNa, sc, ln, ng, ones, name), d['llik'], rtol=1e-9)
        nll, grad, s2 = V.vecchia_nllik(X, y, NNa, sc, ln, ng, ones, name, scale_est, nugget_est, n, -1.0)
        close(nll, d['nll'], rtol=1e-9)
        close(grad, d['grad'], rtol=1e-7, atol=1e-8)
        close(s2, d['scale_out'], rtol=1e-9)
        Lm = V.L_matrix(X, NNa, ln, ng, name)
        close(Lm, d['Lmat'], rtol=1e-8, atol=1e-8 * np.abs(d['Lmat']).max())
        close(V.forward_solve_sp(d['Lmat'] / np.sqrt(sc), NNa, d['b']), d['spsolve'], rtol=1e-9, atol=1e-11)   # (as fmvn_sp calls it, vecchia.py:138-139)
        gm, gv = V.gp_vecch(d['xq'], X, d['pNN'], y, sc, ln, ng, ones, name)
        close(gm, d['gpv_m'], rtol=1e-8, atol=1e-10)
        close(gv, d['gpv_v'], rtol=1e-7, atol=1e-10)
        lm, lv = V.link_gp_vecch(d['lm_in'], d['lv_in'], d['lz_in'], X[:, :2], X[:, 2:], d['pNN'], y, sc, ln, ng, ones, name)
        ref_m, ref_v = d['lgv_m'], d['lgv_v']
        if name == 'matern2.5':
            ref_m, ref_v = matern_link_reference('link_gp_vecch', d['lm_in'], d['lv_in'], d['lz_in'], X[:, :2], X[:, 2:], d['pNN'], y, sc, ln, ng,
                                                 ones, name)
        close(lm, ref_m, rtol=1e-7, atol=1e-9)
        close(lv, ref_v, rtol=1e-6, atol=1e-8)
