"""Reference for linked-GP predictions under shifted inputs.

A linked-GP prediction depends on the training inputs W and the test means m only through W - m and W_i - W_j (and on the
global inputs through Wg - z), so adding one constant per column to W and m (and to Wg and z) leaves it unchanged.  The
problems generated here make that shift EXACT in float64: every coordinate lies on a dyadic grid (W0, Wg0, z0 multiples of
2^-10, m0 of 2^-12) and every offset is a power of two up to 2^20, so that (W0 + off) - off == W0 bit for bit and every
difference a kernel may form is the offset-0 difference, bit for bit.  The exact prediction is therefore computed ONCE, at
offset 0, in np.longdouble, and holds for every shift.

What lives here:
* problem() / shifted(): the generator and the shifts (with the exactness assertions).
* exact_sexp(): mean_t, var_t = |sum_ij C_ij J_ij(t) - mean_t^2 + scale (1 + nugget)| of the SExp linked GP from a = W0 - m0
  as in oracle.IJ, in long double, with C = ry ry^T - scale Rinv from the float64 (Rinv, Rinv y) the device is given, and the
  sensitivity sums  A_t = sum_ij |C_ij| J_ij (1 + E_ij)  and  B_t = sum_i |ry_i| I_i (1 + e_i)  (E_ij, e_i: the exponents
  of J_ij and I_i) the bounds are made of.  drop=: the leave-one-out variant, its weights the long-double downdate of the
  same float64 arrays (what csrc/linkgp_direct.hip states); loo_refit() is the refit on the other n - 1 points.
* exact_sexp_vecchia(): the same prediction conditioned on each test point's own neighbours, K inverted in long double.
* exact_gp() / gp_bounds(): the plain GP prediction at deterministic inputs (v = 0) with its sums and its own counts, for
  Engine.gp_predict.
* restated_var(): float64 restatements of the PAIR EXPONENT alone -- 'expanded' (row term + column term + dot product from
  the raw coordinates: the SExp first and second forms before they were centred), 'direct' ((w_i - 2m) + w_j, then squared:
  linkgp_J_kernel) and 'centred' (expanded after subtracting W[0] from W and m) -- everything else in long double.  They
  exist to show that the bound below discriminates: the host test holds 'direct' and 'centred' to it and requires
  'expanded' to break it from offset 2^6 on.
* var_bound() / mean_bound(): the bounds, their constants c_a, c_s, c_m counted below.  Nothing about the shift enters them.

The constants are counts of roundings (units of eps = 2^-53) along the path of ONE pair, read from csrc/linkgp_sexp.hip,
linkgp.hpp, linkgp_direct.hip and linkgp.hip.  Roundings of different dimensions act on their own terms and do not add up
in a relative count; what grows with the width is the depth of an accumulation and the prefactor's product.
  c_a, relative to 1 + E_ij:
    a term of the pair exponent    the coefficient c1 = 1 / (8 v + 2 l^2) (4: 8v, l l, +, 1/), the centred w' = w - c and
                                   m' = m - c and w' - 2 m' (3), c1 w' (1), the product with w_j' (its own rounding 1, the
                                   fma 1); a row term c1 w' w' has the three of w' twice: the longest path               12
    their accumulation             base_ij, Dw products, rr_i and ss_j in one MFMA chain (Dz global terms in rr, ss)      Dw + Dz + 2
    the exponential                common.hpp: 3.5e-16 for the table form = 3.2 eps                                     4
    the weight C_ij                wt (ry_i ry_j - scale Rinv_ij): 4; leave-one-out three more products and two more
                                   differences                                                                          10
    the sums                       fma into a lane's 16 pairs (16), 6 wave steps, 4 waves (2), <= 6 tiles and the 64-lane
                                   finalize (6), the final multiply-adds (4)                                            34
    the prefactor                  1 / sqrt(prod_k (1 + 4 v_k / l_k^2)): 4 per dimension, sqrt, 1/, the product          4 Dw + 3
    c_a = 5 Dw + Dz + 65   (70 at Dw = 1, 82 at (3, 2), 135 and 140 at 14 and 15)
  c_s, on mean^2 + scale (1 + nugget): mu mu, the difference, scale (1 + nugget) (2), the sum, and the margin of a power
    of two: c_s = 8.
  c_m, relative to 1 + e_i: a term a^2 / (2 v + l^2) (subtraction, square, 3 for the denominator, the division: 6), their
    accumulation (Dw + Dz), exp (2), the weight (leave-one-out: 3), the sums (n / 256 -> 1, 6 wave steps, 3: 10), the
    prefactor (4 Dw + 3):  c_m = 5 Dw + Dz + 24.
These are counts, not worst-case bounds: a centred term of the expanded forms can exceed the exponent it belongs to by the
ratio (|w_i'| + |w_j'| + 2 |m'|)^2 / (w_i' + w_j' - 2 m')^2, which is of order one on average over the generator's box
(coordinates within one or two lengthscales of the centre) and not bounded pair by pair.  The restatements show the
room: the difference-first orders sit below 3e-3 of the bound, the expanded order at 1.8 to 40 times the bound at offset
2^6, 4e2 to 5e3 times at 2^10 and 4e8 to 5e9 times at 2^20 (test_linkshift_host.py asserts both sides)."""
import os

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -53
C_S = 8.0

M_TEST = 34
NUGGET = 1e-2
SCALE = 1.3
SHAPES = [(1, 0), (3, 2), (14, 0), (15, 0)]             # (Dw, Dz)
SIZES = [65, 130]
OFFSETS = [0.0, 2.0 ** 6, 2.0 ** 10, 2.0 ** 14, 2.0 ** 20, -2.0 ** 10]
_COLUMN = [2.0 ** 10, -2.0 ** 6, 2.0 ** 14, 0.0, -2.0 ** 20, 2.0 ** 6, 2.0 ** 20]


def shifts(D):
    """name -> the (D,) offsets of one shift: the common ones and one per-column vector."""
    out = {'%+g' % o if o else '0': np.full(D, o) for o in OFFSETS}
    out['columns'] = np.array([_COLUMN[k % len(_COLUMN)] for k in range(D)])
    return out


def shift_size(off):
    """The largest offset of a shift (what the host test's `from 2^6 on` reads)."""
    return float(np.max(np.abs(off))) if len(off) else 0.0


def problem(name, n, Dw, Dz, seed):
    """One linked-GP problem on the dyadic grids, with its float64 training statistics (oracle.compute_stats at W0)."""
    from oracle import dgp_oracle as O
    rng = np.random.default_rng(seed)
    D = Dw + Dz
    W0 = rng.integers(0, 1024, size=(n, Dw)) / 1024.0
    Wg0 = rng.integers(0, 1024, size=(n, Dz)) / 1024.0
    m0 = rng.integers(-819, 4916, size=(M_TEST, Dw)) / 4096.0            # multiples of 2^-12 in [-0.2, 1.2]
    z0 = rng.integers(0, 1024, size=(M_TEST, Dz)) / 1024.0
    v = 10.0 ** rng.uniform(-5, -1, size=(M_TEST, Dw))
    v[0] = 0.0
    v[1, Dw - 1] = 0.0
    v[M_TEST - 1, :Dw // 2] = 0.0
    y = rng.normal(size=n)
    length = rng.uniform(0.5, 1.0, size=D) * np.sqrt(D) / 2         # (0.5 / 0.75 / 1 at three columns; cond(R) <= 1e4 asserted)
    X0 = np.concatenate((W0, Wg0), 1)
    st = O.compute_stats(X0, y, length, NUGGET, name, Dw)
    assert np.linalg.cond(st['Rinv']) <= 1e4
    return dict(name=name, n=n, Dw=Dw, Dz=Dz, W0=W0, Wg0=Wg0, m0=m0, z0=z0, v=v, y=y, length=length, Rinv=st['Rinv'],
                ry=st['Rinv_y'], scale=SCALE, nugget=NUGGET)


def shifted(p, off):
    """(W, m, Wg, z) of problem p with off[k] added to column k of W and m (k < Dw) and of Wg and z (k >= Dw); asserts that
    the shift is exact: taking it away again gives the grid values back, so every difference is the offset-0 one."""
    Dw = p['Dw']
    ow, og = np.asarray(off[:Dw], float), np.asarray(off[Dw:], float)
    W, m, Wg, z = p['W0'] + ow, p['m0'] + ow, p['Wg0'] + og, p['z0'] + og
    assert np.array_equal(W - ow, p['W0']) and np.array_equal(m - ow, p['m0'])
    assert np.array_equal(Wg - og, p['Wg0']) and np.array_equal(z - og, p['z0'])
    assert np.array_equal(W[:, None, :] - m[None, :, :], p['W0'][:, None, :] - p['m0'][None, :, :])
    assert np.array_equal(W[:, None, :] - W[None, :, :], p['W0'][:, None, :] - p['W0'][None, :, :])
    return W, m, Wg, z


# ------------------------------------------------------------------------------------------------ exact values
def _global_terms(Wg, z_t, lg):
    d = (np.asarray(Wg, LD) - np.asarray(z_t, LD)) / np.asarray(lg, LD)
    return np.sum(d * d, axis=1)


def sexp_factors(W, Wg, m_t, v_t, z_t, length):
    """(I (n,), e (n,), J (n, n), E (n, n)) of one test point in long double: I = I1 exp(-e), J = J1 exp(-E) with
    e_i = sum_k a_ik^2 / (2 v_k + l_k^2) + g_i,  E_ij = sum_k (a_ik + a_jk)^2 / (8 v_k + 2 l_k^2) + (a_ik - a_jk)^2 / (2 l_k^2)
    + g_i + g_j,  a = W - m,  g_i = sum_g ((Wg_ig - z_g) / l_g)^2  (oracle.IJ and cross_corr, restated)."""
    W = np.asarray(W, LD)
    n, Dw = W.shape
    l, v = np.asarray(length, LD), np.asarray(v_t, LD)
    a = W - np.asarray(m_t, LD)
    g = _global_terms(Wg, z_t, l[Dw:]) if Wg is not None and np.shape(Wg)[1] else np.zeros(n, LD)
    e = np.sum(a * a / (2 * v + l[:Dw] ** 2), axis=1) + g
    E = g[:, None] + g[None, :]
    for k in range(Dw):
        s, d = a[:, k][:, None] + a[:, k][None, :], a[:, k][:, None] - a[:, k][None, :]
        E = E + s * s / (8 * v[k] + 2 * l[k] ** 2) + d * d / (2 * l[k] ** 2)
    I1 = 1 / np.sqrt(np.prod(1 + 2 * v / l[:Dw] ** 2))
    J1 = 1 / np.sqrt(np.prod(1 + 4 * v / l[:Dw] ** 2))
    return I1 * np.exp(-e), e, J1 * np.exp(-E), E


def downdate(Rinv, ry, d):
    """(R_-d)^-1 embedded (zero row / column d) and (R_-d)^-1 y from the given Rinv, Rinv y, in long double."""
    R, r = np.asarray(Rinv, LD), np.asarray(ry, LD)
    u = R[:, d].copy()
    Rk = R - np.outer(u, u) / u[d]
    rk = r - u * (r[d] / u[d])
    Rk[d, :], Rk[:, d], rk[d] = 0, 0, 0
    return Rk, rk


def moments(I, e, J, E, Rinv, ry, scale, nugget):
    """(mean, var, A, B) of one test point from its factors and (long double) statistics."""
    Rinv, ry = np.asarray(Rinv, LD), np.asarray(ry, LD)
    C = np.outer(ry, ry) - LD(scale) * Rinv
    mean = np.dot(I, ry)
    var = np.abs(np.sum(C * J) - mean * mean + LD(scale) * (1 + LD(nugget)))
    return mean, var, np.sum(np.abs(C) * J * (1 + E)), np.sum(np.abs(ry) * I * (1 + e))


def exact_sexp(p, drop=None):
    """dict(mean, var, A, B), each (M,) long double, of the SExp problem p at offset 0."""
    out = []
    for t in range(M_TEST):
        I, e, J, E = sexp_factors(p['W0'], p['Wg0'], p['m0'][t], p['v'][t], p['z0'][t], p['length'])
        Rinv, ry = (p['Rinv'], p['ry']) if drop is None else downdate(p['Rinv'], p['ry'], int(drop[t]))
        out.append(moments(I, e, J, E, Rinv, ry, p['scale'], p['nugget']))
    a = np.array(out, dtype=LD)
    return dict(mean=a[:, 0], var=a[:, 1], A=a[:, 2], B=a[:, 3])


def ld_sexp_corr(X, length, nugget):
    Xl = np.asarray(X, LD) / np.asarray(length, LD)
    d = Xl[:, None, :] - Xl[None, :, :]
    K = np.exp(-np.sum(d * d, axis=2))
    K[np.arange(len(K)), np.arange(len(K))] = 1 + LD(nugget)
    return K


def loo_refit(p, drop, tests):
    """(mean, var) of the test points `tests`, each conditioned on the n - 1 training points other than drop[t], the
    statistics refitted on them in long double (linkfun_ref's Cholesky inverse)."""
    from linkfun_ref import _ld_inverse
    X0 = np.concatenate((p['W0'], p['Wg0']), 1)
    out = []
    for t in tests:
        keep = np.delete(np.arange(p['n']), int(drop[t]))
        Ri = _ld_inverse(ld_sexp_corr(X0[keep], p['length'], p['nugget']))
        I, e, J, E = sexp_factors(p['W0'][keep], p['Wg0'][keep], p['m0'][t], p['v'][t], p['z0'][t], p['length'])
        out.append(moments(I, e, J, E, Ri, Ri @ np.asarray(p['y'], LD)[keep], p['scale'], p['nugget'])[:2])
    a = np.array(out, dtype=LD)
    return a[:, 0], a[:, 1]


def exact_sexp_vecchia(p, NN):
    """(mean, var), each (M,) long double, of Engine.vecchia_linkgp with unit nugget weights: test point t conditioned on
    the training points NN[t], their correlation matrix built and inverted in long double from W0, Wg0 and y."""
    from linkfun_ref import _ld_inverse
    X0, y = np.concatenate((p['W0'], p['Wg0']), 1), np.asarray(p['y'], LD)
    out, inverse = [], {}
    for t in range(M_TEST):
        idx = NN[t]
        key = tuple(sorted(idx))
        if key not in inverse:                 # (pm = n: every test point has the same set, rotated)
            o = np.array(key)
            inverse[key] = (o, _ld_inverse(ld_sexp_corr(X0[o], p['length'], p['nugget'])))
        o, Ki = inverse[key]
        I, e, J, E = sexp_factors(p['W0'][o], p['Wg0'][o], p['m0'][t], p['v'][t], p['z0'][t], p['length'])
        out.append(moments(I, e, J, E, Ki, Ki @ y[o], p['scale'], p['nugget'])[:2])
    a = np.array(out, dtype=LD)
    return a[:, 0], a[:, 1]


def gp_c_a(p):
    """gp_predict's count (csrc/gp_predict.hip), relative to 1 + e_i + e_j: each correlation r = exp(-e) has the staged
    coordinate (2), the difference, the square and its accumulation (D), exp (2): D + 5, twice; the product with Rinv_ij (2);
    the MFMA's chain over the training points (n), the four rows of a lane, two shuffles, four waves, <= 3 row blocks (11),
    scale and the final difference (3)."""
    return 2.0 * (p['Dw'] + p['Dz'] + 5) + 2 + p['n'] + 11 + 3


def gp_c_m(p):
    """... of the mean: one correlation (D + 5), the product, a quarter of the training points in one chain, two sums."""
    return p['Dw'] + p['Dz'] + 5 + 1 + p['n'] / 4.0 + 2


def gp_bounds(ex, p):
    """(mean bound, variance bound) of gp_predict: the variance |scale (1 + nugget - q)| has no mean^2 term."""
    return EPS * gp_c_m(p) * ex['B'], EPS * (gp_c_a(p) * ex['A'] + C_S * LD(p['scale']) * (1 + LD(p['nugget'])))


def exact_gp(p):
    """Engine.gp_predict at the deterministic inputs x = [m0 | z0]: mean = r . ry, var = |scale (1 + nugget - r^T Rinv r)|,
    r_i = exp(-e_i); A = scale sum_ij |Rinv_ij| r_i r_j (1 + e_i + e_j), B = sum_i |ry_i| r_i (1 + e_i)."""
    Rinv, ry = np.asarray(p['Rinv'], LD), np.asarray(p['ry'], LD)
    out = []
    for t in range(M_TEST):
        r, e, _, _ = sexp_factors(p['W0'], p['Wg0'], p['m0'][t], np.zeros(p['Dw']), p['z0'][t], p['length'])
        q = np.outer(r, r)
        out.append((np.dot(r, ry), np.abs(LD(p['scale']) * (1 + LD(p['nugget']) - np.sum(Rinv * q))),
                    LD(p['scale']) * np.sum(np.abs(Rinv) * q * (1 + e[:, None] + e[None, :])), np.sum(np.abs(ry) * r * (1 + e))))
    a = np.array(out, dtype=LD)
    return dict(mean=a[:, 0], var=a[:, 1], A=a[:, 2], B=a[:, 3])


# ------------------------------------------------------------------------------------------------ the bounds
def c_a(p):
    return 5.0 * p['Dw'] + p['Dz'] + 65.0


def c_m(p):
    return 5.0 * p['Dw'] + p['Dz'] + 24.0


def var_bound(ex, p):
    return EPS * (c_a(p) * ex['A'] + C_S * (ex['mean'] ** 2 + LD(p['scale']) * (1 + LD(p['nugget']))))


def mean_bound(ex, p):
    return EPS * c_m(p) * ex['B']


def worst_ratio(got, exact, bound):
    """max_t |got - exact| / bound, as a float."""
    return float(np.max(np.abs(np.asarray(got, LD) - exact) / bound))


# ------------------------------------------------------------------------------------------------ float64 restatements of the pair exponent
def restated_exponent(order, W, Wg, m_t, v_t, z_t, length):
    """E (n, n) in float64 in the order of one device form (no fused multiply-adds: they change last bits, not the order)."""
    W, m_t = np.asarray(W, float), np.asarray(m_t, float)
    n, Dw = W.shape
    l = np.asarray(length, float)
    if order == 'centred':
        m_t, W = m_t - W[0], W - W[0]
    c1 = 1.0 / (8.0 * np.asarray(v_t, float) + 2.0 * l[:Dw] * l[:Dw])
    base = np.zeros((n, n))
    for k in range(Dw):
        d = W[:, k][:, None] - W[:, k][None, :]
        base = base + (d * d) * (1.0 / (2.0 * l[k] * l[k]))
    g = np.zeros(n)
    for q in range(np.shape(Wg)[1] if Wg is not None else 0):
        dg = (np.asarray(Wg, float)[:, q] - z_t[q]) * (1.0 / l[Dw + q])
        g = g + dg * dg
    wi = W - 2.0 * m_t                                     # (w_i - 2 m: every form begins with it)
    if order == 'direct':
        e = base + g[:, None] + g[None, :]
        for k in range(Dw):
            s = wi[:, k][:, None] + W[:, k][None, :]
            e = e + (s * s) * c1[k]
        return e
    rr, ss, dot = np.zeros(n), np.zeros(n), base.copy()
    for k in range(Dw):
        cw = c1[k] * wi[:, k]
        rr = rr + cw * wi[:, k]
        ss = ss + (c1[k] * W[:, k]) * W[:, k]
        dot = dot + (2.0 * cw)[:, None] * W[:, k][None, :]    # (the MFMA accumulates on top of base_ij)
    return dot + (rr + g)[:, None] + (ss + g)[None, :]


def restated_var(order, p, W, Wg, m, z, mean_exact):
    """var (M,) with the pair exponent from restated_exponent and everything else in long double."""
    Rinv, ry = np.asarray(p['Rinv'], LD), np.asarray(p['ry'], LD)
    C = np.outer(ry, ry) - LD(p['scale']) * Rinv
    l, out = np.asarray(p['length'], LD), []
    for t in range(M_TEST):
        E = restated_exponent(order, W, Wg, m[t], p['v'][t], z[t], p['length'])
        J1 = 1 / np.sqrt(np.prod(1 + 4 * np.asarray(p['v'][t], LD) / l[:p['Dw']] ** 2))
        out.append(np.abs(np.sum(C * (J1 * np.exp(-np.asarray(E, LD)))) - mean_exact[t] ** 2 + LD(p['scale']) * (1 + LD(p['nugget']))))
    return np.array(out, dtype=LD)


# ------------------------------------------------------------------------------------------------ Matern: exact values, recorded
# The exact Matern factors are linkfun_ref's integrals (mpmath, 120 digits): 34 Dw n (n + 1) / 2 of them per shape, minutes on
# eight cores at the small shapes below and hours at Dw = 14, 15.  `python tests/linkshift_ref.py` (the repository root and tests/ on PYTHONPATH) evaluates them once and
# records the predictions in tests/golden/linkshift_matern.npz together with the float64 statistics they were made with
# (the device is then handed exactly those).
MATERN_EXACT_CASES = [(65, 1, 0), (65, 3, 2), (130, 1, 0), (130, 3, 2)]
FIXTURE_MATERN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'linkshift_matern.npz')


def loo_drop(n):
    """The training point each test point leaves out: 0, 63, 64 and n - 1 first (the tiles' edges), then by index."""
    drop = (11 * np.arange(M_TEST) + 5) % n
    drop[:4] = [0, 63, 64, n - 1]
    return drop.astype(np.int32)


def seed_of(n, Dw, Dz):
    return 1000 * n + 10 * Dw + Dz


def matern_exact(p, processes=8):
    """(dense, loo): dict(mean, var, A, B) each, long double, of the Matern problem p at offset 0 from the exact integrals;
    A_t = sum_ij |C_ij| J_ij, B_t = sum_i |ry_i| I_i (a Matern factor has no exponent to weigh)."""
    import multiprocessing
    from linkfun_ref import _e2e_dim_job, _ld_corr
    n, Dw, Dz = p['n'], p['Dw'], p['Dz']
    jobs = [(t, k, p['W0'][:, k], p['m0'][t, k], p['v'][t, k], p['length'][k]) for t in range(M_TEST) for k in range(Dw)]
    I, J = np.ones((M_TEST, n), LD), np.ones((M_TEST, n, n), LD)
    with multiprocessing.Pool(processes) as pool:
        for t, k, Iv, Jv in pool.imap_unordered(_e2e_dim_job, jobs):
            I[t] *= Iv
            J[t] *= Jv
    drop, zero, zero2 = loo_drop(n), np.zeros(n, LD), np.zeros((n, n), LD)
    dense, loo = [], []
    for t in range(M_TEST):
        if Dz:
            Iz = _ld_corr(p['Wg0'], p['z0'][t:t + 1], p['length'][Dw:])[:, 0]
            I[t] *= Iz
            J[t] *= np.outer(Iz, Iz)
        dense.append(moments(I[t], zero, J[t], zero2, p['Rinv'], p['ry'], p['scale'], p['nugget']))
        Rk, rk = downdate(p['Rinv'], p['ry'], int(drop[t]))
        loo.append(moments(I[t], zero, J[t], zero2, Rk, rk, p['scale'], p['nugget']))
    pack = lambda rows: dict(zip(('mean', 'var', 'A', 'B'), np.array(rows, dtype=LD).T))
    return pack(dense), pack(loo)


def write_fixture_matern():
    from linkfun_ref import _split
    out = {}
    for (n, Dw, Dz) in MATERN_EXACT_CASES:
        p = problem('matern2.5', n, Dw, Dz, seed_of(n, Dw, Dz))
        key = 'n%dw%dz%d_' % (n, Dw, Dz)
        out[key + 'Rinv'], out[key + 'ry'] = p['Rinv'], p['ry']
        for name, ex in zip(('dense', 'loo'), matern_exact(p)):
            for what in ('mean', 'var'):
                out[key + name + '_' + what + '_hi'], out[key + name + '_' + what + '_lo'] = _split(ex[what])
            out[key + name + '_A'], out[key + name + '_B'] = ex['A'].astype(np.float64), ex['B'].astype(np.float64)
        print(key, 'done', flush=True)
    np.savez_compressed(FIXTURE_MATERN, **out)
    print('%s (%d bytes)' % (FIXTURE_MATERN, os.path.getsize(FIXTURE_MATERN)))


def matern_problem(n, Dw, Dz):
    """The Matern problem of one shape; at the recorded shapes with the recorded statistics, and (dense, loo) exact values."""
    from linkfun_ref import join
    p = problem('matern2.5', n, Dw, Dz, seed_of(n, Dw, Dz))
    if (n, Dw, Dz) not in MATERN_EXACT_CASES:
        return p, None, None
    key = 'n%dw%dz%d_' % (n, Dw, Dz)
    with np.load(FIXTURE_MATERN) as z:
        # (the same generator and LAPACK give the same statistics to rounding; the recorded ones are what the exact values hold for)
        assert np.allclose(z[key + 'Rinv'], p['Rinv'], rtol=0, atol=1e-9 * np.abs(p['Rinv']).max())
        p['Rinv'], p['ry'] = z[key + 'Rinv'], z[key + 'ry']
        ex = [dict(mean=join(z[key + nm + '_mean_hi'], z[key + nm + '_mean_lo']), var=join(z[key + nm + '_var_hi'], z[key + nm + '_var_lo']),
                   A=z[key + nm + '_A'].astype(LD), B=z[key + nm + '_B'].astype(LD)) for nm in ('dense', 'loo')]
    return p, ex[0], ex[1]


def matern_rho(p):
    """(M,) the relative error a Matern I or J of test point t may carry: per local dimension 32 E_b of its v / l^2 bucket --
    what tests/test_gpu_linkfn.py allows each device factor against the exact integrals (E_b: linkfun_ref's measured error
    of the fixed algorithm, recorded in tests/golden/linkfun_exact.npz) -- and 8 eps for a dimension with v = 0 and for each
    global dimension of either point (the point correlation: a difference, a division, a polynomial, an exponential)."""
    import linkfun_ref
    E_b = linkfun_ref.load()['E_b']
    l2 = np.asarray(p['length'], float)[:p['Dw']] ** 2
    ratio = p['v'] / l2
    per = np.where(p['v'] == 0.0, 8 * EPS, 32.0 * E_b[np.minimum(linkfun_ref.bucket_of(ratio), len(E_b) - 1)])
    return np.asarray(per.sum(axis=1) + 16 * EPS * p['Dz'], LD)


def matern_bounds(ex, p):
    """(mean bound, variance bound): every J_ij and I_i within rho_t (matern_rho), then as for SExp without the exponent and
    the prefactor -- the weight (10), the sums (34), the product over the dimensions (Dw + Dz) on A_t; c_s on the rest; the
    mean's own error reaches the variance through mean^2 -- and for the mean the weight (3), the sums (10), the product."""
    rho = matern_rho(p)
    bm = (rho + EPS * (p['Dw'] + p['Dz'] + 13)) * ex['B']
    bv = (rho + EPS * (p['Dw'] + p['Dz'] + 44)) * ex['A'] + 2 * np.abs(ex['mean']) * bm + EPS * C_S * (ex['mean'] ** 2 + LD(p['scale']) * (1 + LD(p['nugget'])))
    return bm, bv


if __name__ == '__main__':
    write_fixture_matern()
