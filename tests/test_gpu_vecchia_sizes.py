"""The Vecchia row kernels at every compiled block size, and the Vecchia prediction kernels at their dispatch limits, against
the numpy oracle (oracle/dgp_oracle.py).  Needs an MI355X: -m gpu.

A. vecchia_llik / vecchia_llik_batch / vecchia_nllik / vecchia_lmatrix.  Conditioning sets of m <= 30 points take the
   register-resident kernel of csrc/vecchia_row4.hpp, compiled at the block sizes BS in {4, 8, 12, 16, 20, 24, 26, 28, 31}:
   launch_vrow4 sends nb = m + 1 to the next compiled size and the kernel pads the set IN FRONT with BS - nb identity rows.
   The sweep over m = 0..34 sends
       BS =  4: m = 0..3      BS =  8: m = 4..7      BS = 12: m = 8..11
       BS = 16: m = 12..15    BS = 20: m = 16..19    BS = 24: m = 20..23
       BS = 26: m = 24, 25    BS = 28: m = 26, 27    BS = 31: m = 28, 29, 30
   (the last m of each group is the exact fit, the first the largest padding; m = 15 -> 16 crosses to a lane's second block
   row and its second neighbour load), m = 31..34 and 62..66, 69 to the LDS kernel of csrc/vecchia_rows.hip (its loops
   stride by 64 lanes: a 65-row block at m = 63 / 64), and m <= 30 a second time to the LDS kernel (DGPAMD_VECCHIA_LDS=1).
   Both engines run under DGPAMD_POISON_LDS=1: no unwritten LDS may reach a result.
B. vecchia_gp (register kernel to VG_BC = 51 neighbours and D <= 16) and vecchia_linkgp (to VL_BC = 50, Dw, Dz <= 8) on
   either side of each limit, every test point against the oracle.

The reference is trusted because the problems are well conditioned: every conditioning block is a principal submatrix of
the problem's full correlation matrix (nugget included), whose condition number the tests compute on the host and hold
below 1e6 -- the float64 oracle's own error is then about cond x 2e-16 <= 2e-10, inside every tolerance used here.  (With
the nugget 1e-3 and weights >= 0.5 the smallest eigenvalue is at least 5e-4 and the largest at most the number of
points, 237 at the most: the bound holds for any lengthscale.)"""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NUGGET, COND_MAX = 1e-3, 1e6
SCALE = 4.0   # of the order of quad / n in the row problems: the two terms of (logdet + quad / scale) / 2 do not cancel
ROW_SIZES = list(range(35)) + [62, 63, 64, 65, 66, 69]
ROW_REG_MAX_M = 30                      # nb = m + 1 <= VR_MAXB = 31
GP_REG = dict(pm=51, D=16)              # VG_BC, and the widest instance of the register kernel
LINK_REG = dict(pm=50, Dw=8, Dz=8)      # VL_BC


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


@pytest.fixture(scope='module')
def engines(eng):
    """'default': the dispatch as shipped (register kernels up to their limits, LDS kernels beyond); 'lds': the LDS kernels at
    every size.  Every CU's LDS is filled with NaNs before each Vecchia launch of either."""
    from test_gpu_ops import engine_under
    with contextlib.ExitStack() as stack:
        yield {'default': stack.enter_context(engine_under(POISON_LDS=1, VECCHIA_LDS=0)),
               'lds': stack.enter_context(engine_under(POISON_LDS=1, VECCHIA_LDS=1))}


def npy(t):
    return t.detach().cpu().numpy()


class Worst:
    """The largest error seen per comparison, as a fraction of its tolerance (printed at the end of a test: pytest -s)"""

    def __init__(self):
        self.seen = {}

    def check(self, what, where, got, ref, rtol, atol=0.0):
        got, ref = np.asarray(got, float), np.asarray(ref, float)
        assert got.shape == ref.shape, (what, where, got.shape, ref.shape)
        tol = atol + rtol * np.abs(ref)
        err = np.abs(got - ref)
        with np.errstate(divide='ignore', invalid='ignore'):
            frac = np.where(err == 0.0, 0.0, err / tol)
        worst = float(np.max(frac)) if frac.size else 0.0
        if not worst <= 1.0:   # (a NaN fails)
            bad = np.argwhere(~(frac <= 1.0))[0]
            raise AssertionError('%s at %s: first entry %s (row %d) is %r, the oracle has %r; error %.3g of the tolerance %.3g + %.3g |ref|'
                                 % (what, where, tuple(bad), bad[0] if len(bad) else 0, got[tuple(bad)], ref[tuple(bad)], worst, atol, rtol))
        if worst >= self.seen.get(what, (-1.0, ''))[0]:
            self.seen[what] = (worst, where)

    def report(self, title):
        print('\n%s: largest error / tolerance' % title)
        for what, (w, where) in sorted(self.seen.items()):
            print('  %-34s %.3g  (%s)' % (what, w, where))


def assert_conditioned(X, length, name, weights):
    """cond of the full correlation matrix of the points X with 1 + nugget x weights on the diagonal, and with the sparse
    factor's 1 + nugget: it bounds the condition number of every conditioning block (a principal submatrix of it)"""
    from oracle import dgp_oracle as O
    for w in (weights, np.ones(len(X))):
        c = np.linalg.cond(O.k_matrix(X, length, NUGGET, name, w))
        assert c < COND_MAX, (name, X.shape, c)


# ------------------------------------------------------------------ A. the row kernels
def rows_problem(seed, n, D, ard, name, length=None):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, D))
    y = np.sin(3 * X[:, 0]) + X[:, -1] ** 2 + 0.1 * rng.normal(size=n)
    if length is None:
        length = np.array([0.6, 0.7, 0.85][:D]) if ard else np.array([0.7])
    w = rng.uniform(0.5, 2.0, size=n)
    XB = np.stack([X, X + 0.01 * rng.normal(size=X.shape), rng.uniform(size=X.shape)])   # X, X perturbed, unrelated inputs
    for Xj in XB:
        assert_conditioned(Xj, length, name, w)
    return dict(X=X, y=y, length=np.asarray(length, float), w=w, XB=XB, n=n, name=name)


def rows_reference(p, NN):
    """Everything the four entries return, from the oracle as it is:
    quad = n x scale_out of vecchia_nllik(scale_est=True); logdet = -2 vecchia_llik(scale=inf) (the quadratic term divided
    away exactly); the two are tied back to vecchia_nllik(scale_est=False) = (logdet + quad / scale) / 2 at 1e-12.  For the
    other members of the batch quad = -2 vecchia_llik(scale=1) - logdet, a difference that may cost one digit at the most."""
    from oracle import dgp_oracle as O
    X, y, ln, w, n, name = p['X'], p['y'], p['length'], p['w'], p['n'], p['name']
    r = {}
    r['nllA'], r['gA'], s2 = O.vecchia_nllik(X, y, NN, 1.0, ln, NUGGET, w, name, True, False, n, 0.0)    # nugget_est False
    r['nllB'], r['gB'], _ = O.vecchia_nllik(X, y, NN, SCALE, ln, NUGGET, w, name, False, True, n, 0.0)   # nugget_est True
    r['s2'] = s2
    parts = []
    for j, Xj in enumerate(p['XB']):
        logdet = -2.0 * O.vecchia_llik(Xj, y, NN, np.inf, ln, NUGGET, w, name)
        quad = s2 * n if j == 0 else -2.0 * O.vecchia_llik(Xj, y, NN, 1.0, ln, NUGGET, w, name) - logdet
        assert abs(logdet) + quad <= 10 * quad
        parts.append((quad, logdet))
    r['parts'] = np.array(parts)
    quad, logdet = r['parts'][0]
    np.testing.assert_allclose(0.5 * (logdet + quad / SCALE), r['nllB'], rtol=1e-12)
    # the two values are sums of terms of either sign: they may lose one digit to cancellation at the most, so that their
    # relative tolerance measures the kernels (whose parts are held to the same tolerance one by one) and not the subtraction
    assert abs(logdet) + quad / SCALE <= 10 * abs(2 * r['nllB']) and abs(logdet) + n * abs(np.log(s2)) <= 10 * abs(2 * r['nllA'])
    r['L'] = O.L_matrix(X, NN, ln, NUGGET, name)
    return r


def check_rows(worst, e, where, p, NN, r):
    """One engine's four row entries on problem p with the neighbour array NN, against rows_reference's r.  Tolerances:
    sums 1e-9 (test_vecchia_kernels_golden); gradients 1e-7 + 1e-8 max|g| (test_vecchia_llik_nllik_at_64_inputs); sparse-factor
    rows 1e-8 + 1e-8 max|L|; batch member 0 against the single call 1e-14 (+ 1e-13: test_vecchia_row_kernels_register_and_lds_versions_agree)."""
    import torch
    name, n, ln = p['name'], p['n'], p['length']
    dy, dw, dNN = e.tensor(p['y']), e.tensor(p['w']), e.tensor(NN, dtype=torch.int64)
    dXB = e.tensor(p['XB'])
    dX = dXB[0]
    single = npy(e.vecchia_llik(name, dX, dy, dNN, ln, NUGGET, dw))
    worst.check('llik quad', where, single[0], r['parts'][0, 0], 1e-9)
    worst.check('llik logdet', where, single[1], r['parts'][0, 1], 1e-9)
    batch = npy(e.vecchia_llik_batch(name, dXB, dy, dNN, ln, NUGGET, dw))
    assert batch.shape == (3, 2)
    for j in range(3):
        worst.check('llik_batch quad', where + ', member %d' % j, batch[j, 0], r['parts'][j, 0], 1e-9)
        worst.check('llik_batch logdet', where + ', member %d' % j, batch[j, 1], r['parts'][j, 1], 1e-9)
    worst.check('llik_batch member 0 = single', where, batch[0], single, 1e-14, 1e-13)
    for nugget_est in (False, True):
        o, P = e.vecchia_nllik(name, dX, dy, dNN, ln, NUGGET, dw, nugget_est)
        o = npy(o)
        quad, logdet, dquad, dlogdet = o[0], o[1], o[2:2 + P], o[2 + P:]
        tag = 'nllik(nugget_est=%s) ' % nugget_est
        if nugget_est:      # fixed scale
            nll, g, nll_ref, g_ref = 0.5 * (logdet + quad / SCALE), 0.5 * (dlogdet - dquad / SCALE), r['nllB'], r['gB']
        else:               # estimated scale, as test_vecchia_kernels_golden forms it
            s2 = quad / n
            worst.check(tag + 'scale', where, s2, r['s2'], 1e-9)
            nll, g, nll_ref, g_ref = 0.5 * (logdet + n * np.log(s2)), 0.5 * (dlogdet - dquad / s2), r['nllA'], r['gA']
        worst.check(tag + 'quad', where, quad, r['parts'][0, 0], 1e-9)
        worst.check(tag + 'logdet', where, logdet, r['parts'][0, 1], 1e-9)
        worst.check(tag + 'value', where, nll, nll_ref, 1e-9)
        worst.check(tag + 'gradient', where, g, g_ref, 1e-7, 1e-8 * np.abs(g_ref).max())
    L = npy(e.vecchia_lmatrix(name, dX, dNN, ln, NUGGET))
    worst.check('lmatrix', where, L, r['L'], 1e-8, 1e-8 * np.abs(r['L']).max())


def row_engines(engines, m):
    """(label, engine): the default dispatch, and below the hand-over the LDS kernel as well"""
    out = [('register kernel' if m <= ROW_REG_MAX_M else 'LDS kernel (default dispatch)', engines['default'])]
    if m <= ROW_REG_MAX_M:
        out.append(('LDS kernel (DGPAMD_VECCHIA_LDS=1)', engines['lds']))
    return out


@pytest.mark.parametrize('ard', [False, True], ids=['one_lengthscale', 'lengthscale_per_dimension'])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_row_kernels_at_every_conditioning_set_size(engines, name, ard):
    """n = 70 (the last row block of the four-rows-per-wave kernel is half dead), D = 3, nugget weights in [0.5, 2], neighbour
    arrays from O.nn_ordered; m = 0..34, 62..66 and n - 1 = 69; see the module docstring for what each m runs."""
    from oracle import dgp_oracle as O
    p = rows_problem(70 + ard, 70, 3, ard, name)
    worst = Worst()
    for m in ROW_SIZES:
        NN = O.nn_ordered(p['X'] / p['length'], m)
        assert NN.shape == (70, m + 1)
        r = rows_reference(p, NN)
        for label, e in row_engines(engines, m):
            check_rows(worst, e, 'm = %d, %s, %s' % (m, name, label), p, NN, r)
    worst.report('rows n = 70 %s ard = %s' % (name, ard))


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_row_kernels_with_fewer_points_than_the_conditioning_set(engines, eng, name):
    """n = 5 asked for m = 30 and m = 40.  The search clamps m to n - 1: O.nn_ordered and Engine.nn_ordered both return a
    (5, 5) array, which the row entries take as m = 4 (BS = 8, two row blocks, rows 0..3 ragged).  The C ABI also accepts the
    array at the width asked for, (5, m + 1) with -1 beyond the valid entries: then EVERY row is ragged, m = 30 runs the
    register kernel at BS = 31 with 26 to 30 identity rows in front and m = 40 the LDS kernel; the oracle skips the -1 entries
    and returns an (5, m + 1) sparse factor with zeros behind the valid entries."""
    import torch
    from oracle import dgp_oracle as O
    p = rows_problem(5, 5, 3, True, name)
    worst = Worst()
    for m in (30, 40):
        NN = O.nn_ordered(p['X'] / p['length'], m)
        assert NN.shape == (5, 5)
        dNN = eng.nn_ordered(eng.tensor(p['X'] / p['length']), m)
        assert dNN.shape == (5, 5) and dNN.dtype == torch.int64
        np.testing.assert_array_equal(npy(dNN), NN)
        wide = np.full((5, m + 1), -1, dtype=np.int64)
        wide[:, :5] = NN
        for arr, shape in ((NN, 'clamped (5, 5)'), (wide, 'padded (5, %d)' % (m + 1))):
            r = rows_reference(p, arr)
            assert r['L'].shape == arr.shape
            for label, e in row_engines(engines, arr.shape[1] - 1):
                check_rows(worst, e, 'n = 5, m = %d %s, %s, %s' % (m, shape, name, label), p, arr, r)
    worst.report('rows n = 5 %s' % name)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_row_kernels_across_the_input_widths_of_the_padded_rows(engines, name):
    """D in {1, 7, 8, 9, 16, 17}: the register kernel keeps the scaled inputs in LDS rows padded with zeros to a multiple of
    eight columns (VR4_DP) and reads them in chunks of eight; m = 25 (BS = 26, the default) and m = 40 (LDS kernel); one
    lengthscale per dimension, of order sqrt(D) as in test_gpu_wide_inputs.vecchia_problem."""
    from oracle import dgp_oracle as O
    worst = Worst()
    for D in (1, 7, 8, 9, 16, 17):
        length = np.random.default_rng(100 + D).uniform(0.5, 1.0, size=D) * np.sqrt(D)
        p = rows_problem(200 + D, 70, D, True, name, length=length)
        for m in (25, 40):
            NN = O.nn_ordered(p['X'] / p['length'], m)
            r = rows_reference(p, NN)
            for label, e in row_engines(engines, m):
                check_rows(worst, e, 'D = %d, m = %d, %s, %s' % (D, m, name, label), p, NN, r)
    worst.report('rows D sweep %s' % name)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_row_kernels_with_a_single_point(engines, name):
    """n = 1: one row, an empty conditioning set (m = 0, a (1, 1) neighbour array), three of the wave's four row slots dead"""
    from oracle import dgp_oracle as O
    worst = Worst()
    for ard in (False, True):
        p = rows_problem(300 + ard, 1, 3, ard, name)
        NN = O.nn_ordered(p['X'] / p['length'], 0)
        assert NN.shape == (1, 1) and NN[0, 0] == 0
        r = rows_reference(p, NN)
        for label, e in row_engines(engines, 0):
            check_rows(worst, e, 'n = 1, %s, ard = %s, %s' % (name, ard, label), p, NN, r)
    worst.report('rows n = 1 %s' % name)


# ------------------------------------------------------------------ B. the prediction kernels
N_TRAIN, M_TEST = 200, 37   # 37 test points: off the four-per-workgroup grid of the register kernels


def pred_lengths(rng, lo, hi, D):
    return rng.uniform(lo, hi, size=D) * max(1.0, np.sqrt(D / 3.0))   # (of order sqrt(D): the blocks stay far from the identity)


def gp_problem(name, D, seed):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N_TRAIN, D))
    y = np.sin(X.sum(1)) + 0.1 * rng.normal(size=N_TRAIN)
    x = rng.uniform(size=(M_TEST, D))
    length = pred_lengths(rng, 0.5, 1.5, D)
    w = rng.uniform(0.5, 2.0, size=N_TRAIN)
    assert_conditioned(np.vstack((X, x)), length, name, np.concatenate((w, np.ones(M_TEST))))   # (the blocks hold the test point)
    return dict(X=X, y=y, x=x, length=length, w=w)


def check_gp(worst, engines, name, p, D, pm):
    """Tolerances of test_vecchia_kernels_golden: mean 1e-8 + 1e-10, variance 1e-7 + 1e-10"""
    import torch
    from oracle import dgp_oracle as O
    NN = O.pred_nn(p['x'] / p['length'], p['X'] / p['length'], pm)
    assert NN.shape == (M_TEST, pm)
    mr, vr = O.gp_vecch(p['x'], p['X'], NN, p['y'], SCALE, p['length'], NUGGET, p['w'], name)
    reg = pm <= GP_REG['pm'] and D <= GP_REG['D']
    for label, e in [('register kernel' if reg else 'LDS kernel (default dispatch)', engines['default'])] + \
                    ([('LDS kernel (DGPAMD_VECCHIA_LDS=1)', engines['lds'])] if reg else []):
        m_, v_ = e.vecchia_gp(name, e.tensor(p['x']), e.tensor(p['X']), e.tensor(NN, dtype=torch.int64), e.tensor(p['y']), SCALE,
                              p['length'], NUGGET, e.tensor(p['w']))
        where = 'D = %d, pm = %d, %s, %s' % (D, pm, name, label)
        worst.check('vecchia_gp mean', where, npy(m_), mr, 1e-8, 1e-10)
        worst.check('vecchia_gp variance', where, npy(v_), vr, 1e-7, 1e-10)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_vecchia_gp_around_the_register_kernels_limits(engines, name):
    """vecchia_gp against O.gp_vecch at all 37 test points: 1..3 neighbours, 49..53 (the register kernel ends at 51), 63..65
    (the LDS kernel's loops stride by 64 lanes; the block has pm + 2 rows) at D = 3; 40 neighbours at D = 15, 16, 17 (the
    register kernel ends at 16)."""
    worst = Worst()
    p = gp_problem(name, 3, 400)
    for pm in (1, 2, 3, 49, 50, 51, 52, 53, 63, 64, 65):
        check_gp(worst, engines, name, p, 3, pm)
    for D in (15, 16, 17):
        check_gp(worst, engines, name, gp_problem(name, D, 400 + D), D, 40)
    worst.report('vecchia_gp %s' % name)


def link_problem(name, Dw, Dz, seed):
    rng = np.random.default_rng(seed)
    W = rng.uniform(size=(N_TRAIN, Dw))
    Wg = rng.uniform(size=(N_TRAIN, Dz)) if Dz else None
    y = np.sin(W.sum(1)) + 0.1 * rng.normal(size=N_TRAIN)
    mm = rng.uniform(-0.2, 1.2, size=(M_TEST, Dw))
    vv = 10.0 ** rng.uniform(-5, -1, size=(M_TEST, Dw))
    vv[0] = 0.0                                           # one test point without input variance
    z = rng.uniform(size=(M_TEST, Dz)) if Dz else None
    length = pred_lengths(rng, 0.8, 2.0, Dw + Dz)
    w = rng.uniform(0.5, 2.0, size=N_TRAIN)
    Xall = W if not Dz else np.concatenate((W, Wg), 1)
    xq = mm if not Dz else np.concatenate((mm, z), 1)
    assert_conditioned(Xall, length, name, w)
    return dict(W=W, Wg=Wg, y=y, mm=mm, vv=vv, z=z, length=length, w=w, Xall=Xall, xq=xq)


def check_linkgp(worst, engines, name, p, Dw, Dz, pm):
    """Tolerances of test_vecchia_kernels_golden: mean 1e-7 + 1e-9, variance 1e-6 + 1e-8.  The reference is the oracle as it
    is, for the Matern kind too: its float64 expression of the Matern linked factors is only good to these tolerances while
    v / l^2 stays below 0.3 (tests/linkfun_ref.py), and the input variances (<= 0.1) and lengthscales (>= 0.8) here keep it
    below 0.16 -- asserted.  (On these problems the oracle with its factors on the integral, test_gpu_ops.integral_oracle,
    differs from it by 3e-5 of the mean's tolerance and 1.2e-2 of the variance's at the most; it takes three times as long.)"""
    import torch
    from oracle import dgp_oracle as O
    assert np.max(p['vv'] / p['length'][:Dw] ** 2) < 0.3
    NN = O.pred_nn(p['xq'] / p['length'], p['Xall'] / p['length'], pm)
    assert NN.shape == (M_TEST, pm)
    mr, vr = O.link_gp_vecch(p['mm'], p['vv'], p['z'], p['W'], p['Wg'], NN, p['y'], SCALE, p['length'], NUGGET, p['w'], name)
    reg = pm <= LINK_REG['pm'] and Dw <= LINK_REG['Dw'] and Dz <= LINK_REG['Dz']
    for label, e in [('register kernel' if reg else 'LDS kernel (default dispatch)', engines['default'])] + \
                    ([('LDS kernel (DGPAMD_VECCHIA_LDS=1)', engines['lds'])] if reg else []):
        t = e.tensor
        m_, v_ = e.vecchia_linkgp(name, t(p['mm']), t(p['vv']), t(p['z']) if Dz else None, t(p['W']), t(p['Wg']) if Dz else None,
                                  t(NN, dtype=torch.int64), t(p['y']), SCALE, p['length'], NUGGET, t(p['w']))
        where = '(Dw, Dz) = (%d, %d), pm = %d, %s, %s' % (Dw, Dz, pm, name, label)
        worst.check('vecchia_linkgp mean', where, npy(m_), mr, 1e-7, 1e-9)
        worst.check('vecchia_linkgp variance', where, npy(v_), vr, 1e-6, 1e-8)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_vecchia_linkgp_around_the_register_kernels_neighbour_limit(engines, name):
    """vecchia_linkgp against O.link_gp_vecch at all 37 test points (input variances 1e-5..1e-1, test point 0 at zero
    variance): 1, 2 and 48..52 neighbours at (Dw, Dz) = (3, 2); the register kernels end at 50."""
    worst = Worst()
    p = link_problem(name, 3, 2, 500)
    for pm in (1, 2, 48, 49, 50, 51, 52):
        check_linkgp(worst, engines, name, p, 3, 2, pm)
    worst.report('vecchia_linkgp neighbours %s' % name)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_vecchia_linkgp_around_the_register_kernels_width_limits(engines, name):
    """The same with 40 neighbours at (Dw, Dz) = (8, 0), (9, 0), (8, 8), (8, 9), (9, 8): the register kernels end at 8 local
    and 8 global columns."""
    worst = Worst()
    for Dw, Dz in ((8, 0), (9, 0), (8, 8), (8, 9), (9, 8)):
        check_linkgp(worst, engines, name, link_problem(name, Dw, Dz, 500 + 10 * Dw + Dz), Dw, Dz, 40)
    worst.report('vecchia_linkgp widths %s' % name)
