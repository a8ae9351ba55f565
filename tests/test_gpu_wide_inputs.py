"""Every width-dependent kernel at widths up to DGPAMD_MAXD = 64 input columns, against the oracle or an extended-precision
restatement of it.  Needs an MI355X: -m gpu.

Each launcher sizes its dynamic LDS from the node's width.  The widths swept here are where those sizes cross the 64 KB a
launch gets without opting in and the 160 KB of a CU (dgp_amd/csrc/common.hpp, set_lds):
  gradient reductions      (2 D 64 + 8 P + 256) doubles: past 64 KB from D = 59 (P = D + 1) or 62 (P = 1)
  direct J kernel          Matern past 64 KB from Dw = 21, SExp from Dw = 43
  SExp J, first form       past 160 KB from Dw = 49 (Dz = 0) or 40 (Dz = 24): the direct kernel takes over
  Matern leave-one-out     past 160 KB at Dw = 63 and 64 with 32 test points per workgroup: 16 are taken there
  gp cross correlation     exactly 64 KB at D = 64
K is kept well conditioned (nugget >= 1e-2, lengthscales of order sqrt(D)) wherever a factorisation is compared, so that
the tolerances measure the kernels, not cond(K)."""
import numpy as np
import pytest

from far_ref import far_inputs

pytestmark = pytest.mark.gpu

SQ5 = np.sqrt(np.longdouble(5))


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def close(a, b, rtol, atol):
    np.testing.assert_allclose(np.asarray(a, float), np.asarray(b, float), rtol=rtol, atol=atol)


def split_cols(D):
    """(local, global) column counts of a D-wide node, in the proportion of the K-assembly test's 40 + 24"""
    Dg = D * 24 // 64
    return D - Dg, Dg


def corr_terms(X, length, name):
    """K (n, n) and the per-dimension derivative coefficients C (D, n, n), dK/dlog l_d = C_d K, in np.longdouble
    (the oracle's k_matrix_fod, kernel_class.py:304-359, restated in extended precision)."""
    Xl = np.asarray(X, np.longdouble) / np.asarray(length, np.longdouble)
    n, D = Xl.shape
    C = np.empty((D, n, n), np.longdouble)
    s = np.zeros((n, n), np.longdouble)
    pr = np.ones((n, n), np.longdouble)
    for d in range(D):
        r = np.abs(Xl[:, d][:, None] - Xl[:, d][None, :])
        if name == 'sexp':
            C[d] = 2 * r * r
            s += r * r
        else:
            e1, e2 = 1 + SQ5 * r, np.longdouble(5) / 3 * r * r
            C[d] = e2 * e1 / (e1 + e2)
            pr *= e1 + e2
            s += r
    K = np.exp(-s) if name == 'sexp' else pr * np.exp(-SQ5 * s)
    return K, C


def test_restatement_is_the_oracle():
    """corr_terms against O.k_matrix_fod at 1e-14: both are the same closed forms, one in extended precision (the
    double result rounds each of its few dozen operations once, and the entries are O(1))."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(1)
    X = rng.uniform(size=(65, 64))
    X[1] = X[0]
    length = rng.uniform(2.0, 6.0, size=64)
    for name in ('sexp', 'matern2.5'):
        K, C = corr_terms(X, length, name)
        Kr, fod = O.k_matrix_fod(X, length, 0.0, name, False)
        off = ~np.eye(65, dtype=bool)
        close(np.asarray(K, float)[off], Kr[off], rtol=0, atol=1e-14)
        close(np.asarray(C * K, float), fod, rtol=0, atol=1e-14)
        K1, C1 = corr_terms(X, length[:1], name)
        _, fod1 = O.k_matrix_fod(X, length[:1], 0.0, name, False)
        close(np.asarray(C1.sum(0) * K1, float), fod1[0], rtol=0, atol=1e-13)


# ------------------------------------------------------------------ A. dgpamd_grad_reduce on its own
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 150])
@pytest.mark.parametrize('D', [1, 16, 44, 58, 59, 61, 62, 64])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_grad_reduce_vs_extended_precision(eng, name, D, n):
    """dgpamd_grad_reduce with K^-1 given: the padded buffer as dgpamd_potrf_inv leaves it (K^-1 in the tiles, -alpha in
    row n, train.hip grad_reduce_body), so the reduction is checked without any conditioning error of a factorisation.
    Gathered, non-contiguous local columns plus global ones; duplicate rows (r = 0 in the derivative coefficient); nlen 1
    and D; nugget_est on and off; replicate weights W or none.
    Reference: the traces sum_ij Kinv_ij dK_ij and quadratic forms alpha' dK alpha in np.longdouble from the same K^-1.
    Tolerance: 1e-12 * sum_ij |term| per parameter.  The kernel's terms carry a few ulp each (table exponential, scaled
    inputs, the coefficient's reciprocal) and the reduction tree adds O(log n) roundings, so 1e-12 of the absolute sum is
    about 1e3 x the expected error and does not depend on cond(K); dropping a dimension, a tile or the ragged edge moves a
    sum by O(1 / D) of it."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(1000 * D + n)
    Dl, Dg = split_cols(D)
    ldloc = Dl + 7
    Xloc = rng.uniform(size=(n, ldloc))
    G = rng.uniform(size=(n, Dg))
    if n >= 2:
        Xloc[1], G[1] = Xloc[0], G[0]
    if n >= 63:
        Xloc[n - 1], G[n - 1] = Xloc[n // 2], G[n // 2]
    colmap = rng.permutation(ldloc)[:Dl]
    X = np.concatenate((Xloc[:, colmap], G), 1)
    y = rng.normal(size=n)
    Wrep = 1.0 / rng.integers(1, 4, size=n)
    Np = eng.padded_dim(n)
    dXl, dG = eng.tensor(Xloc), (eng.tensor(G) if Dg else None)
    dW = eng.tensor(Wrep)
    for length in (rng.uniform(0.4, 0.8, size=D) * np.sqrt(D), np.array([0.6 * np.sqrt(D)])):
        nugget = 0.05
        Kd = O.k_matrix(X, length, nugget, name)
        K, C = corr_terms(X, length, name)
        if len(length) == 1:
            C = C.sum(0, keepdims=True)
        for nugget_est, W in ((False, None), (False, Wrep), (True, None), (True, Wrep)):
            Kw = Kd.copy()
            if W is not None:
                Kw[np.arange(n), np.arange(n)] = 1.0 + nugget * W
            Kinv = np.linalg.inv(Kw)
            Kinv = 0.5 * (Kinv + Kinv.T)
            alpha = Kinv @ y
            buf = np.zeros((Np, Np))
            buf[:n, :n] = Kinv
            buf[n, :n] = -alpha
            out, P = eng.grad_reduce(name, dXl, colmap, dG, length, nugget, nugget_est, eng.tensor(buf),
                                     W=dW if W is not None else None)
            out = npy(out)
            KiL, aL = Kinv.astype(np.longdouble), alpha.astype(np.longdouble)
            off = ~np.eye(n, dtype=bool)
            T = [(KiL * C[p] * K)[off] for p in range(len(C))]
            Q = [(np.outer(aL, aL) * C[p] * K)[off] for p in range(len(C))]
            if nugget_est:
                w = np.ones(n) if W is None else W
                T.append(nugget * w * np.diag(KiL))
                Q.append(nugget * w * aL * aL)
            assert P == len(T)
            for p in range(P):
                for got, terms, what in ((out[p], T[p], 'trace'), (out[P + p], Q[p], 'quad')):
                    ref, mag = terms.sum(), np.abs(terms).sum()
                    assert abs(np.longdouble(got) - ref) <= 1e-12 * mag, (what, p, got, float(ref), float(mag), len(length), nugget_est, W is not None)


@pytest.mark.parametrize('s', [1.0, 1e4])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_grad_reduce_beyond_the_exponent_range(eng, name, s):
    """The same reduction where every off-diagonal correlation underflows: inputs i s (1, 1) for row i against a lengthscale of
    1e-5 (squared-exponential exponents 2e10 i^2 and beyond 2^63, Matern ones sqrt5 2e5 i and sqrt5 2e9 i: far beyond 2^31 ln 2 =
    1.4886e9, where the table exponential's integer part leaves the bits its exponent is cut from), n = 65, shared and per-column
    lengthscales.  K^-1 is GIVEN as a dense symmetric matrix and alpha as a dense vector, so that every entry of dK carries
    weight.  In extended precision every lengthscale term is exactly 0: the sums may be 1e-300 here at the most; the nugget's
    sums keep the sibling's 1e-12 of their absolute sum."""
    rng = np.random.default_rng(65)
    n, nugget = 65, 1e-6
    X = far_inputs(n, s)
    Kinv = rng.normal(size=(n, n))
    Kinv = 0.5 * (Kinv + Kinv.T)
    alpha = rng.normal(size=n)
    Np = eng.padded_dim(n)
    buf = np.zeros((Np, Np))
    buf[:n, :n] = Kinv
    buf[n, :n] = -alpha
    KiL, aL = Kinv.astype(np.longdouble), alpha.astype(np.longdouble)
    off = ~np.eye(n, dtype=bool)
    for length in (np.array([1e-5, 1e-5]), np.array([1e-5])):
        K, C = corr_terms(X, length, name)
        if len(length) == 1:
            C = C.sum(0, keepdims=True)
        out, P = eng.grad_reduce(name, eng.tensor(X), None, None, length, nugget, True, eng.tensor(buf))
        out = npy(out)
        assert P == len(C) + 1
        for p in range(len(C)):
            assert not (KiL * C[p] * K)[off].any() and not (np.outer(aL, aL) * C[p] * K)[off].any()
            assert abs(out[p]) <= 1e-300 and abs(out[P + p]) <= 1e-300, (p, out[p], out[P + p], len(length))
        for got, terms in ((out[P - 1], nugget * np.diag(KiL)), (out[2 * P - 1], nugget * aL * aL)):
            assert abs(np.longdouble(got) - terms.sum()) <= 1e-12 * np.abs(terms).sum(), (got, float(terms.sum()), len(length))


# ------------------------------------------------------------------ B. dgpamd_llik_batch against the oracle
N_B = 130
WIDTHS = [64, 1, 33, 7]


@pytest.fixture(scope='module')
def llik_nodes():
    """64 nodes (DGPAMD_MAXB) of n = 130 rows: widths cycling 64, 1, 33, 7, both kinds, nlen 1 and D, nugget_est, some with
    replicate weights; each with its oracle ingredients (O.k_matrix_fod, np.linalg.inv) and the absolute term sums."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(77)
    n = N_B
    nodes = []
    for b in range(64):
        D = WIDTHS[b % 4]
        Dl, Dg = split_cols(D)
        Xl, G = rng.uniform(size=(n, Dl)), rng.uniform(size=(n, Dg))
        name = ('sexp', 'matern2.5')[(b // 4) % 2]
        nlen = D if (b // 8) % 2 == 0 else 1
        length = rng.uniform(0.4, 0.8, size=nlen) * np.sqrt(D)
        nugget = float(rng.uniform(0.05, 0.1))   # (with W >= 1/2: the smallest eigenvalue >= 0.025, cond(K) <= 130.1 / 0.025)
        nugget_est = b % 3 != 0
        W = 1.0 / rng.integers(1, 3, size=n) if b % 5 == 1 else None
        y = rng.normal(size=n)
        X = np.concatenate((Xl, G), 1)
        K, fod = O.k_matrix_fod(X, length, nugget, name, nugget_est, W)
        assert np.linalg.cond(K) <= 1e4
        Kinv = np.linalg.inv(K)
        a = Kinv @ y
        ref = dict(logdet=np.linalg.slogdet(K)[1], quad=y @ a,
                   tr=np.array([np.sum(Kinv * f) for f in fod]), trmag=np.array([np.sum(np.abs(Kinv * f)) for f in fod]),
                   qq=np.array([a @ f @ a for f in fod]), qqmag=np.array([np.abs(a) @ np.abs(f) @ np.abs(a) for f in fod]))
        nodes.append(dict(name=name, Xl=Xl, G=G, length=length, nugget=nugget, nugget_est=nugget_est, W=W, y=y, ref=ref))
    return nodes


@pytest.mark.parametrize('mode', [1, 0])
@pytest.mark.parametrize('B', [1, 2, 3, 4, 5, 64])
def test_llik_batch_wide_vs_oracle(eng, llik_nodes, B, mode):
    """dgpamd_llik_batch (Engine.llik_plan) with nodes of widths 1..64 in one batch: the gradient kernel's LDS is sized from
    the batch's Dmax / Pmax.  B <= 3 passes the arguments by value (grad_reduce_multi_val_kernel), B = 4, 5, 64 copies them
    to the device (grad_reduce_multi_kernel).  Potrf mode 1 reads alpha from column n of L^-T, mode 0 from row n of the inverse.
    Reference: the oracle's K and dK (O.k_matrix_fod), inverted in double; cond(K) <= 1e4 is asserted.
    Tolerance: logdet and y'K^-1y 1e-10 relative (the factorisation's error is ~cond x eps = 2e-12); traces and quadratic
    forms 1e-9 of their absolute term sums (the inverse's entries carry the same cond x eps relative error)."""
    nodes = llik_nodes[:B]
    specs = [dict(kind=c['name'], Xloc=eng.tensor(c['Xl']), Xglob=eng.tensor(c['G']) if c['G'].shape[1] else None,
                  nlen=len(c['length']), nugget_est=c['nugget_est'], W=None if c['W'] is None else eng.tensor(c['W']),
                  y=eng.tensor(c['y'])) for c in nodes]
    eng.set_potrf_mode(mode)
    try:
        plan = eng.llik_plan(N_B, specs)
        for b, c in enumerate(nodes):
            plan.set(b, c['length'], c['nugget'])
        out = plan.run(list(range(B)))
    finally:
        eng.set_potrf_mode(1)
    for b, c in enumerate(nodes):
        r, h = c['ref'], out[b]
        P = len(r['tr'])
        assert len(h) == 3 + 2 * P and h[-1] == 0, (b, h[-1])
        assert abs(h[0] - r['logdet']) <= 1e-10 * max(1.0, abs(r['logdet'])), (b, h[0], r['logdet'])
        assert abs(h[1] - r['quad']) <= 1e-10 * abs(r['quad']), (b, h[1], r['quad'])
        assert np.all(np.abs(h[2:2 + P] - r['tr']) <= 1e-9 * r['trmag']), (b, h[2:2 + P] - r['tr'], r['trmag'])
        assert np.all(np.abs(h[2 + P:2 + 2 * P] - r['qq']) <= 1e-9 * r['qqmag']), (b, h[2 + P:2 + 2 * P] - r['qq'], r['qqmag'])


# ------------------------------------------------------------------ C. prediction at wide inputs
N_C, M_C = 130, 34   # three 64-row tiles with a ragged edge; one 32-point workgroup of the J kernels and a remainder


def pred_problem(name, Dw, Dz, seed):
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(seed)
    D = Dw + Dz
    X = rng.uniform(size=(N_C, D))
    y = rng.normal(size=N_C)
    length = rng.uniform(0.5, 1.0, size=D) * np.sqrt(D)
    nug = 1e-2
    st = O.compute_stats(X, y, length, nug, name, Dw)
    assert np.linalg.cond(st['Rinv']) <= 1e4
    mm = rng.uniform(-0.2, 1.2, size=(M_C, Dw))
    vv = 10.0 ** rng.uniform(-5, -1, size=(M_C, Dw))
    vv[0] = 0.0
    vv[1, Dw - 1] = 0.0
    vv[M_C - 1, :Dw // 2] = 0.0
    z = rng.uniform(size=(M_C, Dz)) if Dz else None
    return dict(X=X, y=y, length=length, nug=nug, st=st, mm=mm, vv=vv, z=z, Dw=Dw, Dz=Dz, rng=rng)


def linkgp(eng, name, p, drop=None):
    import torch
    Dw, Dz, X = p['Dw'], p['Dz'], p['X']
    m, v = eng.linkgp_predict(name, eng.tensor(p['mm']), eng.tensor(p['vv']), eng.tensor(p['z']) if Dz else None,
                              eng.tensor(X[:, :Dw]), eng.tensor(X[:, Dw:]) if Dz else None, p['length'],
                              eng.tensor(p['st']['Rinv']), N_C, eng.tensor(p['st']['Rinv_y']), 1.3, p['nug'],
                              drop=None if drop is None else eng.tensor(drop, dtype=torch.int32))
    return npy(m), npy(v)


@pytest.mark.parametrize('D', [16, 17, 63, 64])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_gp_predict_wide_vs_oracle(eng, name, D):
    """dgpamd_gp_predict (cross_corr_kernel stages 2 D 64 doubles: 64 KB at D = 64) against O.gp_predict.
    Tolerance as test_gpu_ops' gp tests: mean 1e-9, variance 1e-7 relative (a difference of O(scale) terms, cond(R) <= 1e4)."""
    from oracle import dgp_oracle as O
    p = pred_problem(name, D, 0, 300 + D)
    x = p['rng'].uniform(size=(M_C, D))
    mr, vr = O.gp_predict(x, p['X'], p['st']['Rinv'], p['st']['Rinv_y'], 1.4, p['length'], p['nug'], name)
    m, v = eng.gp_predict(name, eng.tensor(x), eng.tensor(p['X']), p['length'], eng.tensor(p['st']['Rinv']), N_C,
                          eng.tensor(p['st']['Rinv_y']), 1.4, p['nug'])
    close(npy(m), mr, rtol=1e-9, atol=1e-11)
    close(npy(v), vr, rtol=1e-7, atol=1e-9)


@pytest.mark.parametrize('Dw,Dz', [(14, 0), (15, 0), (31, 0), (48, 0), (49, 0), (64, 0), (40, 24)])
def test_sexp_linkgp_wide_vs_oracle(eng, Dw, Dz):
    """SExp link_gp, default forms: the second form to Dw = 14, the first (MFMA) form from 15 while it fits in a CU's LDS
    (to 48 at Dz = 0), the direct kernel beyond (49 and 64 at Dz = 0; 40 + 24).  Zero input variances included.
    Reference O.link_gp_predict; tolerance as test_gpu_ops' link_gp tests: mean 1e-8, variance 1e-6 relative."""
    from oracle import dgp_oracle as O
    p = pred_problem('sexp', Dw, Dz, 400 + Dw + Dz)
    X = p['X']
    mr, vr = O.link_gp_predict(p['mm'], p['vv'], p['z'], X[:, :Dw], X[:, Dw:] if Dz else None, p['st']['Rinv'],
                               p['st']['Rinv_y'], 1.3, p['length'], p['nug'], 'sexp', gemm_form=True)
    m, v = linkgp(eng, 'sexp', p)
    close(m, mr, rtol=1e-8, atol=1e-10)
    close(v, vr, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('Dw,Dz', [(64, 0), (40, 24)])
def test_matern_linkgp_separable_wide_vs_oracle(eng, Dw, Dz):
    """Matern link_gp in its default separable form (records + linkgp_Jsep_kernel) at 64 columns.
    Reference O.link_gp_predict; tolerance mean 1e-8, variance 1e-6 relative (test_gpu_ops' link_gp tolerances)."""
    from oracle import dgp_oracle as O
    p = pred_problem('matern2.5', Dw, Dz, 500 + Dw + Dz)
    X = p['X']
    mr, vr = O.link_gp_predict(p['mm'], p['vv'], p['z'], X[:, :Dw], X[:, Dw:] if Dz else None, p['st']['Rinv'],
                               p['st']['Rinv_y'], 1.3, p['length'], p['nug'], 'matern2.5')
    m, v = linkgp(eng, 'matern2.5', p)
    close(m, mr, rtol=1e-8, atol=1e-10)
    close(v, vr, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('Dw', [21, 43, 64])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_linkgp_direct_wide_vs_oracle(eng, name, Dw):
    """linkgp_J_kernel<K, false> (set_linkgp_direct(True)): past 64 KB of LDS from Dw = 21 (Matern) and 43 (SExp).
    Reference O.link_gp_predict; tolerance mean 1e-8, variance 1e-6 relative (test_gpu_ops' link_gp tolerances)."""
    from oracle import dgp_oracle as O
    p = pred_problem(name, Dw, 0, 600 + Dw)
    mr, vr = O.link_gp_predict(p['mm'], p['vv'], None, p['X'], None, p['st']['Rinv'], p['st']['Rinv_y'], 1.3, p['length'],
                               p['nug'], name, gemm_form=True)
    eng.set_linkgp_direct(True)
    try:
        m, v = linkgp(eng, name, p)
    finally:
        eng.set_linkgp_direct(False)
    close(m, mr, rtol=1e-8, atol=1e-10)
    close(v, vr, rtol=1e-6, atol=1e-8)


@pytest.mark.parametrize('Dw', [62, 63, 64])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_linkgp_loo_wide_vs_oracle_refit(eng, name, Dw):
    """dgpamd_linkgp_loo: test point t conditioned on all training points but drop[t].  The Matern form needs exactly
    160 KB at Dw = 62 and would need more at 63 and 64 with 32 test points per workgroup: 16 are taken there.
    Reference: O.link_gp_predict with the statistics refitted on the n - 1 remaining points; tolerance mean 1e-8,
    variance 1e-6 relative as test_gpu_ops' leave-one-out test."""
    from oracle import dgp_oracle as O
    p = pred_problem(name, Dw, 0, 700 + Dw)
    X, y = p['X'], p['y']
    drop = p['rng'].integers(0, N_C, size=M_C).astype(np.int32)
    drop[0], drop[1] = 0, N_C - 1
    m, v = linkgp(eng, name, p, drop=drop)
    for t in range(M_C):
        keep = np.delete(np.arange(N_C), drop[t])
        s2 = O.compute_stats(X[keep], y[keep], p['length'], p['nug'], name, Dw)
        mr, vr = O.link_gp_predict(p['mm'][t:t + 1], p['vv'][t:t + 1], None, X[keep], None, s2['Rinv'], s2['Rinv_y'], 1.3,
                                   p['length'], p['nug'], name, gemm_form=True)
        close(m[t], mr[0], rtol=1e-8, atol=1e-10)
        close(v[t], vr[0], rtol=1e-6, atol=1e-9)


# ------------------------------------------------------------------ D. Vecchia at 64 inputs
def vecchia_problem(seed, D=64, n=130):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, D))
    y = rng.normal(size=n)
    length = rng.uniform(0.5, 1.0, size=D) * np.sqrt(D)
    return rng, X, y, length


@pytest.mark.parametrize('m', [20, 90])
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_vecchia_llik_nllik_at_64_inputs(eng, name, m):
    """vecchia_llik / vecchia_nllik at D = 64: m = 20 runs the register row kernel, m = 90 the LDS row kernel at 114 KiB.
    Reference O.vecchia_llik / O.vecchia_nllik (nn_ordered neighbours, oracle's own); tolerance as test_gpu_ops' Vecchia
    golden test: value 1e-9, gradient 1e-7 relative (per-row Cholesky of size m + 1, nugget 1e-2)."""
    import torch
    from oracle import dgp_oracle as O
    rng, X, y, length = vecchia_problem(800 + m)
    n, nug, sc = len(X), 1e-2, 1.2
    NN = O.nn_ordered(X / length, m)
    nd = rng.uniform(0.5, 1.0, size=n)
    dX, dy, dNN, dnd = eng.tensor(X), eng.tensor(y), eng.tensor(NN, dtype=torch.int64), eng.tensor(nd)
    out = npy(eng.vecchia_llik(name, dX, dy, dNN, length, nug, dnd))
    close(-0.5 * (out[1] + out[0] / sc), O.vecchia_llik(X, y, NN, sc, length, nug, nd, name), rtol=1e-9, atol=0)
    o, P = eng.vecchia_nllik(name, dX, dy, dNN, length, nug, dnd, True)
    o = npy(o)
    nll, g, _ = O.vecchia_nllik(X, y, NN, sc, length, nug, nd, name, False, True, n, 0.0)
    close(0.5 * (o[1] + o[0] / sc), nll, rtol=1e-9, atol=0)
    close(0.5 * (o[2 + P:] - o[2:2 + P] / sc), g, rtol=1e-7, atol=1e-8 * np.abs(g).max())


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_vecchia_gp_linkgp_at_64_inputs(eng, name):
    """vecchia_gp (D = 64, 100 neighbours: 133 KiB of LDS) and vecchia_linkgp (Dw + Dz = 40 + 24, 60 neighbours: 90 KiB
    SExp, 103 KiB Matern) against O.gp_vecch / O.link_gp_vecch.  Tolerances as test_gpu_ops' Vecchia golden test: gp mean
    1e-8, variance 1e-7; link_gp mean 1e-7, variance 1e-6 relative."""
    import torch
    from oracle import dgp_oracle as O
    rng, X, y, length = vecchia_problem(900)
    n, nug, sc, M = len(X), 1e-2, 1.2, 37
    nd = rng.uniform(0.5, 1.0, size=n)
    x = rng.uniform(size=(M, 64))
    pNN = O.pred_nn(x / length, X / length, 100)
    gm, gv = eng.vecchia_gp(name, eng.tensor(x), eng.tensor(X), eng.tensor(pNN, dtype=torch.int64), eng.tensor(y), sc, length,
                            nug, eng.tensor(nd))
    mr, vr = O.gp_vecch(x, X, pNN, y, sc, length, nug, nd, name)
    close(npy(gm), mr, rtol=1e-8, atol=1e-10)
    close(npy(gv), vr, rtol=1e-7, atol=1e-10)
    Dw, Dz = 40, 24
    mm = rng.uniform(size=(M, Dw))
    vv = 10.0 ** rng.uniform(-5, -1, size=(M, Dw))
    vv[0] = 0.0
    z = rng.uniform(size=(M, Dz))
    lNN = O.pred_nn(np.concatenate((mm, z), 1) / length, X / length, 60)
    lm, lv = eng.vecchia_linkgp(name, eng.tensor(mm), eng.tensor(vv), eng.tensor(z), eng.tensor(X[:, :Dw]), eng.tensor(X[:, Dw:]),
                                eng.tensor(lNN, dtype=torch.int64), eng.tensor(y), sc, length, nug, eng.tensor(nd))
    mr, vr = O.link_gp_vecch(mm, vv, z, X[:, :Dw], X[:, Dw:], lNN, y, sc, length, nug, nd, name)
    close(npy(lm), mr, rtol=1e-7, atol=1e-9)
    close(npy(lv), vr, rtol=1e-6, atol=1e-8)


def test_vecchia_refuses_what_does_not_fit_in_lds(eng):
    """At D = 64 a conditioning set past a CU's 160 KB of LDS (rows m = 120: 180 KiB; vecchia_gp 130 neighbours: 203 KiB;
    vecchia_linkgp 100 neighbours: 235 KiB) is refused with DGPAMD_BAD_ARG before anything is launched, and the engine
    still works afterwards."""
    import torch
    from dgp_amd.ops import DgpAmdError
    from oracle import dgp_oracle as O
    rng, X, y, length = vecchia_problem(901, n=140)
    n = len(X)
    dX, dy, ones = eng.tensor(X), eng.tensor(y), eng.tensor(np.ones(n))
    NN = eng.tensor(O.nn_ordered(X / length, 120), dtype=torch.int64)
    for call in (lambda: eng.vecchia_llik('sexp', dX, dy, NN, length, 1e-2, ones),
                 lambda: eng.vecchia_nllik('matern2.5', dX, dy, NN, length, 1e-2, ones, True),
                 lambda: eng.vecchia_gp('sexp', dX[:5], dX, eng.tensor(O.pred_nn(X[:5], X, 130), dtype=torch.int64), dy, 1.0,
                                        length, 1e-2, ones),
                 lambda: eng.vecchia_linkgp('matern2.5', dX[:5, :40], eng.tensor(np.full((5, 40), 1e-2)), dX[:5, 40:], dX[:, :40],
                                            dX[:, 40:], eng.tensor(O.pred_nn(X[:5], X, 100), dtype=torch.int64), dy, 1.0,
                                            length, 1e-2, ones)):
        with pytest.raises(DgpAmdError, match='rc=2'):
            call()
    out = npy(eng.vecchia_llik('sexp', dX, dy, eng.tensor(O.nn_ordered(X / length, 10), dtype=torch.int64), length, 1e-2, ones))
    assert np.all(np.isfinite(out))


# ------------------------------------------------------------------ E. one model-level check
@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
def test_kernel_llik_with_40_local_and_24_global_inputs(eng, name):
    """dgp_amd.kernel_class.kernel with 40 local input columns and 24 global ones (connect), nugget_est: kernel.llik runs
    the Python staging, K assembly, the factorisation and dgpamd_grad_reduce at full width.  Reference O.nll_grad;
    tolerance nll 1e-10, gradient 1e-9 relative to its largest entry, at cond(K) <= 1e4 as in the batch test."""
    from dgp_amd.kernel_class import kernel
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(64)
    n, Dl, Dg = 150, 40, 24
    k = kernel(length=rng.uniform(0.4, 0.8, size=Dl + Dg) * 8.0, scale=1.1, nugget=0.03, name=name, nugget_est=True,
               connect=np.arange(Dg), engine=eng)
    k.input = rng.uniform(size=(n, Dl))
    k.global_input = rng.uniform(size=(n, Dg))
    k.output = rng.normal(size=(n, 1))
    x = k.log_t()
    assert np.linalg.cond(O.k_matrix(k._X(), k.length, k.nugget[0], name)) <= 1e4
    rnll, rg, _ = O.nll_grad(x, k._X(), k.output, name, k.scale, k.nugget[0], True, False, 'ga', k.prior_coef)
    nll, g = k.llik(x)
    assert abs(float(np.ravel(nll)[0]) - rnll) <= 1e-10 * abs(rnll), (nll, rnll)
    close(g, rg, rtol=0, atol=1e-9 * np.abs(rg).max())
