"""The Matern-2.5 linked-GP factors of csrc/linkfun.hpp against the exact values of the integrals they stand for.

matern_I_dim, matern_Jd, matern_Jd0 and the separable matern_role_S / matern_role_T pair are evaluated on the device through
dgpamd_debug_linkfn (the functions themselves, one lane per case) on the ~4000 cases of tests/golden/linkfun_exact.npz: v/l^2 from
1e-12 to 1600, equal points, points 1e-7 lengthscales apart, points on and either side of m, v == 0, v = 1e-300, points 1e5
lengthscales away.  The fixture carries mpmath's values rounded to double (tests/linkfun_ref.py; tests/test_linkfun_host.py checks
them against the defining integral without a GPU), so nothing here needs mpmath.  The bound per case is max(32 E_b, 64 2^-53)
relative, E_b the error of the float64 numpy restatement of the same algorithm in the case's v/l^2 bucket (measured by the host test,
capped there, carried by the fixture): the factor 32 is test_gpu_hetero_posterior.py's allowance for fma contraction and the
device's exp / erfc / erfcx.  Then the kernels end to end -- linkgp_predict in both forms and with drop=, vecchia_linkgp under
both VECCHIA_LDS settings -- against I and J assembled from exact per-dimension factors in numpy.longdouble
(tests/golden/linkfun_e2e.npz).  Every test prints its worst ratio to the bound before it asserts.  Needs an MI355X: -m gpu."""
import ctypes as C

import numpy as np
import pytest

import linkfun_ref as R

gpu = pytest.mark.gpu
LD = np.longdouble
EPS = 2.0 ** -53


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


@pytest.fixture(scope='module')
def fx():
    z = R.load()
    for a in z.values():
        a.setflags(write=False)
    return z


def probe(eng, fn, args):
    return eng.debug_linkfn(fn, eng.tensor(np.ascontiguousarray(args))).cpu().numpy()


def case_bound(fx):
    """(E of each case's bucket, the relative bound max(32 E, 64 2^-53))."""
    E = fx['E_b'][R.bucket_of(fx['ratio'])]
    return E, np.maximum(32.0 * E, 64.0 * EPS)


@gpu
@pytest.mark.parametrize('fn', R.FNS)
def test_factor_against_the_exact_integral(eng, fx, fn):
    """Every case: finite, in [0, 1 + 32 E_b], and within max(32 E_b, 64 2^-53) relative of the exact value (exact values below
    1e-280 -- the far points -- are held to |got| <= 1e-279)."""
    args, exact = fx['args'], fx[R.exact_key(fn)]
    got = probe(eng, fn, args)
    E, bound = case_bound(fx)
    rel = R.relative_error(got, exact)
    b = R.bucket_of(fx['ratio'])
    for k in range(len(R.BUCKET_EDGES)):
        i = np.where(b == k)[0]
        w = i[np.argmax(rel[i] / bound[i])]
        print('%-6s v/l^2 <= %-6g worst error / bound = %.3g  (error %.2e, bound %.2e, args %s)' %
              (fn, R.BUCKET_EDGES[k], rel[w] / bound[w], rel[w], bound[w], args[w]))
    assert np.all(np.isfinite(got))
    assert np.all(got >= 0.0) and np.all(got <= 1.0 + 32.0 * E)
    bad = np.where(~(rel <= bound))[0]
    assert len(bad) == 0, (len(bad), args[bad[:5]], got[bad[:5]], exact[bad[:5]])


@gpu
def test_deterministic_input_is_the_product_of_point_correlations(eng, fx):
    """v == 0: every function returns matern_point(m - X1) matern_point(m - X2) (I: one factor).  The reference is the same
    float64 expression, operation for operation -- none of its operations can contract into an fma -- so the device differs
    by its exp alone: 1 ulp per factor against numpy's 1, the product's rounding: 4 ulp.  (Against the exact value the
    argument of exp, up to 134 here, costs 134 ulp by its own rounding.)"""
    args = fx['args'][fx['args'][:, 3] == 0.0]
    assert len(args) >= 30
    X1, X2, m, v, l = args.T

    def point(d):
        a = np.abs(d)
        return (1.0 + R.SQ5 * a / l + 5.0 * d * d / (3.0 * l * l)) * np.exp(-R.SQ5 * a / l)
    k1, k2 = point(m - X1), point(m - X2)
    for fn, ref in (('i', k1), ('jd', k1 * k2), ('jsep', k1 * k2), ('jd0', k1 * k1), ('jsep0', k1 * k1)):
        got = probe(eng, fn, args)
        ulp = np.abs(got - ref) / np.spacing(ref)
        print('%-6s v == 0: %.2f ulp' % (fn, ulp.max()))
        assert np.all(ulp <= 4.0), (fn, ulp.max())


@gpu
def test_direct_factor_is_symmetric_bit_for_bit(eng, fx):
    args = fx['args']
    swapped = args[:, [1, 0, 2, 3, 4]]
    assert np.array_equal(probe(eng, 'jd', args), probe(eng, 'jd', swapped))
    assert np.array_equal(probe(eng, 'jsep', args), probe(eng, 'jsep', swapped))


@gpu
def test_device_erfcx(eng, fx):
    """exp(t^2) erfc(t) as the device evaluates it, t >= 0 up to 1e300.  Every tail of linkfun.hpp is proportional to it, so
    its relative error goes into the factors one to one; of the 64 2^-53 the factor tests allow where the algorithm itself
    is exact, 16 2^-53 (8 ulp) are its share."""
    t, exact = fx['erfcx_t'], fx['erfcx_exact']
    a = np.zeros((len(t), 5))
    a[:, 0] = t
    got = probe(eng, 'erfcx', a)
    rel = np.abs(got - exact) / exact
    w = np.argmax(rel)
    print('erfcx: worst %.2f x 2^-53 at t = %r' % (rel[w] / EPS, t[w]))
    assert np.all(np.isfinite(got)) and np.all(rel <= 16 * EPS)


@gpu
def test_bad_arguments(eng):
    """dgpamd_debug_linkfn: an unknown fn, count <= 0 or a null pointer is DGPAMD_BAD_ARG (2), as dgpamd_debug_mathfn has it."""
    from dgp_amd._lib import lib
    a, o = eng.tensor(np.ones((4, 5))), eng.empty(4)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.dgpamd_debug_linkfn(eng.h, 0, 4, p(a), p(o)) == 0
    for fn, count, pa, po in ((-1, 4, p(a), p(o)), (len(eng.LINKFN), 4, p(a), p(o)), (0, 0, p(a), p(o)), (0, -3, p(a), p(o)),
                              (0, 4, None, p(o)), (0, 4, p(a), None)):
        assert lib.dgpamd_debug_linkfn(eng.h, fn, count, pa, po) == 2, (fn, count)


# ------------------------------------------------------------------------------------------------ the kernels end to end
@pytest.fixture(scope='module')
def e2e():
    z = R.load_e2e()
    z.update(R.e2e_inputs())
    for a in z.values():
        a.setflags(write=False)
    return z


def point_E(fx, e2e, Dw):
    """E of a test point: the largest E_b among its dimensions."""
    return fx['E_b'][R.bucket_of(e2e['ratio'][:, :Dw])].max(axis=1)


def check_moments(what, got_m, got_v, e2e, key, E):
    """mean within max(32 E, 1e-12) sum |I_i ry_i|, variance within the same factor times the sum of the absolute terms of
    its expression; the reference is longdouble on exact factors."""
    f = np.maximum(32.0 * E, 1e-12)
    rm, rv = R.join(e2e[key + '_mean_hi'], e2e[key + '_mean_lo']), R.join(e2e[key + '_var_hi'], e2e[key + '_var_lo'])
    em = (np.abs(got_m.astype(LD) - rm) / (f * e2e[key + '_mabs'])).astype(float)
    ev = (np.abs(got_v.astype(LD) - rv) / (f * e2e[key + '_vabs'])).astype(float)
    print('%-28s mean: worst error / bound = %.3g (test point %d)   variance: %.3g (test point %d)' %
          (what, em.max(), em.argmax(), ev.max(), ev.argmax()))
    assert np.all(np.isfinite(got_m)) and np.all(np.isfinite(got_v))
    assert np.all(em <= 1.0), (what, 'mean', em.argmax(), em.max())
    assert np.all(ev <= 1.0), (what, 'variance', ev.argmax(), ev.max())


def dense_args(eng, e2e, Dw, Dz):
    key = 'w%dz%d_' % (Dw, Dz)
    W = e2e['W']
    t = eng.tensor
    return (t(e2e['m'][:, :Dw]), t(e2e['v'][:, :Dw]), t(e2e['z'][:, :Dz]) if Dz else None, t(W[:, :Dw]), t(W[:, 3:3 + Dz]) if Dz else None,
            np.concatenate((R.E2E_LENGTH[:Dw], R.E2E_LENGTH[3:3 + Dz])), t(e2e[key + 'Rinv']), R.E2E_N, t(e2e[key + 'ry']),
            R.E2E_SCALE, R.E2E_NUGGET)


@gpu
@pytest.mark.parametrize('Dw,Dz', R.E2E_CONFIGS)
def test_linkgp_predict_against_exact_factors(eng, fx, e2e, Dw, Dz):
    """dgpamd_linkgp_predict, direct and separable form: n = 70 (two 64-blocks: diagonal and off-diagonal tiles), M = 40 test
    points whose dimensions mix v/l^2 = 1e-8 .. 100."""
    args = dense_args(eng, e2e, Dw, Dz)
    E = point_E(fx, e2e, Dw)
    try:
        for direct in (True, False):
            eng.set_linkgp_direct(direct)
            m, v = eng.linkgp_predict('matern2.5', *args)
            check_moments('predict %s Dw=%d Dz=%d' % ('direct' if direct else 'separable', Dw, Dz), m.cpu().numpy(), v.cpu().numpy(), e2e,
                          'w%dz%d_dense' % (Dw, Dz), E)
    finally:
        eng.set_linkgp_direct(False)


@gpu
@pytest.mark.parametrize('Dw,Dz', R.E2E_CONFIGS)
def test_linkgp_predict_with_drop_against_exact_factors(eng, fx, e2e, Dw, Dz):
    """dgpamd_linkgp_loo (linkgp_predict with drop=): every test point leaves one training point out -- the first, the last, the
    one it sits on, others by index.  The reference downdates the same float64 (Rinv, Rinv y) in longdouble."""
    import torch
    m, v = eng.linkgp_predict('matern2.5', *dense_args(eng, e2e, Dw, Dz), drop=eng.tensor(R.e2e_drop(), dtype=torch.int32))
    check_moments('predict drop= Dw=%d Dz=%d' % (Dw, Dz), m.cpu().numpy(), v.cpu().numpy(), e2e, 'w%dz%d_drop' % (Dw, Dz), point_E(fx, e2e, Dw))


@gpu
@pytest.mark.parametrize('lds', ['0', '1'])
@pytest.mark.parametrize('Dw,Dz', R.E2E_CONFIGS)
def test_vecchia_linkgp_against_exact_factors(eng, fx, e2e, Dw, Dz, lds):
    """dgpamd_vecchia_linkgp, register and LDS kernels, conditioning on all 70 points (the dense answer) and on the 20 nearest."""
    import torch
    from test_gpu_ops import engine_under
    E = point_E(fx, e2e, Dw)
    W = e2e['W']
    length = np.concatenate((R.E2E_LENGTH[:Dw], R.E2E_LENGTH[3:3 + Dz]))
    with engine_under(VECCHIA_LDS=lds) as e:
        t = e.tensor
        for name, pm in (('vn', R.E2E_N), ('v20', R.E2E_PM)):
            NN = R.e2e_neighbours(e2e, Dw, Dz, pm)
            m, v = e.vecchia_linkgp('matern2.5', t(e2e['m'][:, :Dw]), t(e2e['v'][:, :Dw]), t(e2e['z'][:, :Dz]) if Dz else None,
                                    t(W[:, :Dw]), t(W[:, 3:3 + Dz]) if Dz else None, t(NN, dtype=torch.int64), t(e2e['y']),
                                    R.E2E_SCALE, length, R.E2E_NUGGET, t(np.ones(R.E2E_N)))
            check_moments('vecchia LDS=%s pm=%d Dw=%d Dz=%d' % (lds, pm, Dw, Dz), m.cpu().numpy(), v.cpu().numpy(), e2e,
                          'w%dz%d_%s' % (Dw, Dz, name), E)


@gpu
def test_single_entries_read_out_of_the_kernels(eng, fx, e2e):
    """Dw = 1: a one-hot ry = e_i makes mean = I_i, and ry = 0, nugget = -1, scale = 1, Rinv = -(e_i e_j^T + e_j e_i^T)/2 makes
    var = |J_ij|.  20 pairs (diagonal ones, pairs within and across the two 64-tiles) read single entries out of
    dgpamd_linkgp_predict: the direct form's equal the probe's matern_I_dim / matern_Jd / matern_Jd0 bit for bit, and both
    forms' lie within the factor bound of the exact values."""
    n, M = R.E2E_N, R.E2E_M
    W, m, v = e2e['W'][:, :1], e2e['m'][:, :1], e2e['v'][:, :1]
    E = point_E(fx, e2e, 1)
    bound = np.maximum(32.0 * E, 64.0 * EPS)
    t = eng.tensor
    try:
        for p, (i, j) in enumerate(R.E2E_PAIRS):
            pa = np.stack((np.full(M, W[i, 0]), np.full(M, W[j, 0]), m[:, 0], v[:, 0], np.full(M, R.E2E_LENGTH[0])), axis=1)
            ry = np.zeros(n)
            ry[i] = 1.0
            Rinv = np.zeros((n, n))
            Rinv[i, j] -= 0.5
            Rinv[j, i] -= 0.5
            for direct in (True, False):
                eng.set_linkgp_direct(direct)
                mean, _ = eng.linkgp_predict('matern2.5', t(m), t(v), None, t(W), None, R.E2E_LENGTH[:1], t(np.zeros((n, n))), n, t(ry), 1.0, -1.0)
                _, var = eng.linkgp_predict('matern2.5', t(m), t(v), None, t(W), None, R.E2E_LENGTH[:1], t(Rinv), n, t(np.zeros(n)), 1.0, -1.0)
                mean, var = mean.cpu().numpy(), var.cpu().numpy()
                assert np.array_equal(mean, probe(eng, 'i', pa)), (i, j, direct)
                if direct:   # (the separable kernel sums a pair's 15 products in its own order: held to the exact value alone)
                    assert np.array_equal(var, probe(eng, 'jd0' if i == j else 'jd', pa)), (i, j)
                assert np.all(np.abs(mean - e2e['pair_I'][:, p]) <= bound * e2e['pair_I'][:, p]), (i, j, direct)
                assert np.all(np.abs(var - e2e['pair_J'][:, p]) <= bound * e2e['pair_J'][:, p]), (i, j, direct)
    finally:
        eng.set_linkgp_direct(False)
