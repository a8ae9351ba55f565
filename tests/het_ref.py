"""Extended-precision reference of the exact conditional-posterior draw of a Hetero likelihood's mean latent, dense and Vecchia
(likelihood_class.py:134-243, vecchia.py:426-446,599-610), with the inputs, the error measures and the acceptance rules that
tests/test_het_ref_host.py (no GPU) and tests/test_gpu_hetero_posterior.py (MI355X) share.

Everything numerical is plain numpy in numpy.longdouble (x87 extended, eps = 2^-63): the kernels, a Cholesky written column by
column, the substitutions.  The package under test is never imported here; the input builders ask the float64 oracle for the
neighbour arrays only (index arrays, exact).

Acceptance rule of the rows, the draws and the dense draws (`accept`): E_ref is the error of the float64 oracle against this
file in the same norm, computed by the caller; the device must stay within max(MARGIN * E_ref, FLOOR).  The device runs the same
algorithm in the same precision as numpy, in another summation order and with reciprocals in place of divisions, hence the
margin; the rigorous forward bound b (3 b + 17) 2^-53 kappa_2 is 1e2 .. 1e5 times wider than what either achieves and is kept
as an outer assertion only (`rigorous_rows_bound`)."""
import functools

import numpy as np

LD = np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps <= 2.0 ** -63)
U = 2.0 ** -53
MARGIN = 32.0
FLOOR = 64 * U
SQ5 = np.sqrt(LD(5))
JITTER = LD(10) ** -10   # (the float64 code adds the double nearest to 1e-10: 3e-27 away, far below anything compared here)
SCALE = 1.3
KAPPA_MAX = 1e6


def corr(Xa, Xb, length, name):
    """Correlation of every row of Xa with every row of Xb; leading axes broadcast: (..., a, D), (..., b, D) -> (..., a, b)."""
    ell = np.asarray(length, LD)
    A = np.asarray(Xa, LD) / ell
    B = np.asarray(Xb, LD) / ell
    r = np.abs(A[..., :, None, :] - B[..., None, :, :])
    if name == 'sexp':
        return np.exp(-(r * r).sum(-1))
    if name == 'matern2.5':
        return (1 + SQ5 * r + LD(5) / 3 * r * r).prod(-1) * np.exp(-SQ5 * r.sum(-1))
    raise ValueError(name)


def chol(A):
    """Lower Cholesky factor of the (stack of) symmetric matrices A (..., b, b), column by column (left-looking)."""
    A = np.asarray(A, LD)
    b = A.shape[-1]
    L = np.zeros_like(A)
    for j in range(b):
        v = A[..., j:, j] - (L[..., j:, :j] * L[..., j:j + 1, :j]).sum(-1)
        if not np.all(v[..., 0] > 0):
            raise np.linalg.LinAlgError('pivot %d is not positive' % j)
        d = np.sqrt(v[..., 0])
        L[..., j:, j] = v / d[..., None]
    return L


def solve_lower(L, x):
    """L^-1 x, forward substitution; L (b, b), x (b,)."""
    x = np.array(x, LD)
    for i in range(len(x)):
        x[i] = (x[i] - (L[i, :i] * x[:i]).sum()) / L[i, i]
    return x


def solve_upper_T(L, x):
    """L^-T x, back substitution; L (..., b, b), x (..., b)."""
    x = np.array(x, LD)
    b = x.shape[-1]
    for c in range(b - 1, -1, -1):
        x[..., c] = (x[..., c] - (L[..., c + 1:, c] * x[..., c + 1:]).sum(-1)) / L[..., c, c]
    return x


class Rows:
    """What `rows` returns.  idx (n, b): the block order, impNN[i][::-1] (own observation, own latent last); lat (n, b): entry is
    a latent; u (n, b) longdouble: L_i^-T e_last; Lrows (n, b) longdouble, NNl (n, b) int64, t (n,) longdouble: the layout of
    dgpamd_vecchia_het_rows; cond (n,): 2-norm condition number of every block (float64 numpy)."""


def block_matrices(X_ord, idx, scale, length, name, gamma):
    """The blocks scale corr + diag(gamma on observation entries + 1e-10), (n, b, b) longdouble."""
    n = X_ord.shape[0]
    lat = idx >= n
    P = np.asarray(X_ord, LD)[np.where(lat, idx - n, idx)]
    A = LD(scale) * corr(P, P, length, name)
    b = idx.shape[1]
    d = LD(scale) + np.where(lat, LD(0), np.asarray(gamma, LD)[np.where(lat, 0, idx)]) + JITTER
    A[:, np.arange(b), np.arange(b)] = d
    return A


def assemble(idx, u, n, y=None, lat=None):
    """(Lrows, NNl, t) of dgpamd_vecchia_het_rows from the block order idx and the block vectors u: row i = [u of the own latent,
    u of the latent neighbours in block order, 0 ..], NNl[i] = [i, their ordered indices, 0 ..], t_i = sum over the
    observation entries of u y.  lat: the latent / observation flags where they are not to be idx >= n (the host test's
    deliberately wrong rows)."""
    b = idx.shape[1]
    if lat is None:
        lat = idx >= n
    Lrows = np.zeros((n, b), u.dtype)
    NNl = np.zeros((n, b), np.int64)
    Lrows[:, 0] = u[:, -1]
    NNl[:, 0] = np.arange(n)
    for i in range(n):
        sel = np.nonzero(lat[i, :-1])[0]
        Lrows[i, 1:1 + len(sel)] = u[i, sel]
        NNl[i, 1:1 + len(sel)] = idx[i, sel] % n
    t = None
    if y is not None:
        t = (np.where(lat, 0, u) * np.asarray(y, u.dtype)[idx % n]).sum(1)
    return Lrows, NNl, t


def rows(X_ord, impNN, scale, length, name, gamma, y=None):
    """The sparse factor's rows for ordered inputs X_ord (n, D), conditioning sets impNN (n, m + 1) in the stacked vector
    [observations 0..n-1 ; latents n..2n-1] (kernel.ord_nn(pointer=True): no padding), gamma (n,) per ordered site."""
    X_ord = np.asarray(X_ord, float)
    impNN = np.asarray(impNN, np.int64)
    n = X_ord.shape[0]
    assert impNN.shape[0] == n and np.all(impNN >= 0) and np.all(impNN < 2 * n)
    R = Rows()
    R.n = n
    R.idx = impNN[:, ::-1].copy()
    R.lat = R.idx >= n
    A = block_matrices(X_ord, R.idx, scale, length, name, gamma)
    R.cond = np.linalg.cond(np.asarray(A, float))
    L = chol(A)
    e = np.zeros(R.idx.shape, LD)
    e[:, -1] = 1
    R.u = solve_upper_T(L, e)
    R.Lrows, R.NNl, R.t = assemble(R.idx, R.u, n, y)
    return R


def sparse_forward(Lrows, NNl, b):
    """x with sum_j Lrows[i, j] x[NNl[i, j]] = b_i (slot 0 is the diagonal), rows in order, in longdouble."""
    Lrows = np.asarray(Lrows, LD)
    b = np.asarray(b, LD)
    n = len(b)
    x = np.zeros(n, LD)
    for i in range(n):
        x[i] = (b[i] - (Lrows[i, 1:] * x[NNl[i, 1:]]).sum()) / Lrows[i, 0]
    return x


def draw_vecchia(X_ord, impNN, scale, length, name, gamma, y, z, R=None):
    """f = U_l^-T (z - U_ol^T y) in ordered coordinates (Hetero.post_het_vecch)."""
    if R is None or R.t is None:
        R = rows(X_ord, impNN, scale, length, name, gamma, y)
    return sparse_forward(R.Lrows, R.NNl, np.asarray(z, LD) - R.t)


def site_terms(gamma, y, mask=None, n_sites=None):
    """(gamma_eff, y_eff) per site (Hetero.posterior_terms): with replicates (observation i at site mask[i]) the
    precision-weighted 1 / (M' Gamma^-1 M) and its product with M' Gamma^-1 y."""
    gamma, y = np.asarray(gamma, LD), np.asarray(y, LD).reshape(-1)
    if mask is None:
        return gamma, y
    Gi = 1 / gamma
    s0, s1 = np.zeros(n_sites, LD), np.zeros(n_sites, LD)
    np.add.at(s0, mask, Gi)
    np.add.at(s1, mask, Gi * y)
    return 1 / s0, s1 / s0


def draw_dense(K, scale, gamma_eff, y_eff, sd):
    """Hetero.post_het1 with v = scale K: f = v (v + diag Gamma)^-1 (y - u - w) + u, u = chol(v) sd[:, 0],
    w = sqrt(Gamma) sd[:, 1]."""
    v = LD(scale) * np.asarray(K, LD)
    g, y, sd = np.asarray(gamma_eff, LD), np.asarray(y_eff, LD).reshape(-1), np.asarray(sd, LD)
    n = len(y)
    u = chol(v) @ sd[:, 0]
    w = np.sqrt(g) * sd[:, 1]
    vG = v.copy()
    vG[np.arange(n), np.arange(n)] += g
    C = chol(vG)
    return v @ solve_upper_T(C, solve_lower(C, y - u - w)) + u


def sparse_residual(Lrows, NNl, x, b):
    """(|L x - b|, |L| |x|) componentwise for the sparse lower-triangular rows, in longdouble."""
    prod = np.asarray(Lrows, LD) * np.asarray(x, LD)[NNl]
    return np.abs(prod.sum(1) - np.asarray(b, LD)), np.abs(prod).sum(1)


def dot_terms(A, x):
    """(sum_j a_ij x_j, sum_j |a_ij x_j|) in longdouble for the rows of A."""
    prod = np.asarray(A, LD) * np.asarray(x, LD)
    return prod.sum(-1), np.abs(prod).sum(-1)


# ------------------------------------------------------------------ error measures and acceptance
def rows_error(Lrows, t, R, y):
    """(largest relative 2-norm error of a row of Lrows, largest error of t_i relative to |u_obs|_2 |y_obs|_2 of its block)."""
    d = np.asarray(Lrows, LD) - R.Lrows
    eL = np.sqrt((d * d).sum(1)) / np.sqrt((R.Lrows * R.Lrows).sum(1))
    uo = np.where(R.lat, 0, R.u)
    yo = np.where(R.lat, 0, np.asarray(y, LD)[np.where(R.lat, 0, R.idx)])
    et = np.abs(np.asarray(t, LD) - R.t) / (np.sqrt((uo * uo).sum(1)) * np.sqrt((yo * yo).sum(1)))
    return float(eL.max()), float(et.max())


def draw_error(f, f_ref):
    """max |f - f_ref| / max |f_ref|"""
    f_ref = np.asarray(f_ref, LD)
    return float(np.abs(np.asarray(f, LD).reshape(-1) - f_ref).max() / np.abs(f_ref).max())


def tolerance(e_ref, margin=MARGIN):
    return max(margin * e_ref, FLOOR)


def accept(err, e_ref, margin=MARGIN):
    return bool(np.isfinite(err)) and err <= tolerance(e_ref, margin)


def rigorous_rows_bound(R):
    """b (3 b + 17) 2^-53 kappa_2, the forward bound of a block's Cholesky and back substitution, largest over the rows."""
    b = R.idx.shape[1]
    return float(b * (3 * b + 17) * U * R.cond.max())


def rows_accepted(Lrows, NNl, t, R, y, e_ref, margin=MARGIN):
    """The check the GPU test applies to dgpamd_vecchia_het_rows: NNl exact (padding included), Lrows and t within
    the tolerance of their oracle errors e_ref = (eL, et), and within the rigorous bound.  Returns (ok, eL, et)."""
    if not np.array_equal(np.asarray(NNl), R.NNl):
        return False, np.inf, np.inf
    eL, et = rows_error(Lrows, t, R, y)
    outer = rigorous_rows_bound(R)
    ok = accept(eL, e_ref[0], margin) and accept(et, e_ref[1], margin) and eL <= outer and et <= outer
    return ok, eL, et


# ------------------------------------------------------------------ inputs
VECCHIA_CASES = [(65, 1, 3), (130, 2, 1), (130, 2, 2), (20, 2, 50), (257, 12, 7), (200, 8, 31), (400, 3, 25), (140, 2, 64),
                 (140, 2, 100), (1100, 3, 25)]
ARD_CASES = [(257, 12, 7), (400, 3, 25), (140, 2, 64)]
DENSE_N = [1, 2, 63, 64, 65, 128, 130, 200]
NAMES = ['sexp', 'matern2.5']


def points(rng, n, D):
    """Uniform in [0, 1]^D; in one dimension a jittered grid in random order (random points collide: kappa_2 of a block reached 2e8)."""
    if D == 1:
        return ((rng.permutation(n) + 0.5 + rng.uniform(-0.25, 0.25, size=n)) / n)[:, None]
    return rng.uniform(size=(n, D))


class Case:
    pass


@functools.lru_cache(maxsize=None)
def vecchia_case(n, D, m, name):
    """Fixed inputs of one Vecchia case: ordered points X, lengthscales (n^(-1/D) per dimension, times 3 from D = 6; +-30 % per
    dimension in ARD_CASES), gamma = exp(N(-1, 0.7^2)), observations y, normals z, and the conditioning sets of the oracle."""
    from oracle import dgp_oracle as O
    c = Case()
    rng = np.random.default_rng(7000 + 131 * n + 17 * D + m + (0 if name == 'sexp' else 1000000))
    c.n, c.D, c.m, c.name, c.scale = n, D, m, name, SCALE
    c.X = points(rng, n, D)
    c.length = np.full(D, float(n) ** (-1.0 / D) * (3.0 if D >= 6 else 1.0))
    if (n, D, m) in ARD_CASES:
        c.length = c.length * rng.uniform(0.7, 1.3, size=D)
    c.gamma = np.exp(rng.normal(-1.0, 0.7, size=n))
    c.y = np.sin(4 * c.X[:, 0]) + np.sqrt(c.gamma) * rng.normal(size=n)
    c.z = rng.normal(size=n)
    c.impNN = O.imp_nn_array(c.X / c.length, m)
    for a in (c.X, c.length, c.gamma, c.y, c.z, c.impNN):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def vecchia_reference(n, D, m, name):
    """(case, longdouble rows, longdouble draw, oracle rows error (eL, et), oracle draw error) -- computed once per process."""
    from oracle import dgp_oracle as O
    c = vecchia_case(n, D, m, name)
    R = rows(c.X, c.impNN, c.scale, c.length, name, c.gamma, c.y)
    f = draw_vecchia(c.X, c.impNN, c.scale, c.length, name, c.gamma, c.y, c.z, R=R)
    g2 = np.concatenate((c.gamma, c.gamma))
    Uo = O.U_matrix_rows(c.X, c.impNN, c.scale, c.length, name, g2)
    Lo, NNo, to = assemble(R.idx, Uo, n, c.y)
    assert np.array_equal(NNo, R.NNl)
    e_rows = rows_error(Lo, to, R, c.y)
    e_draw = draw_error(O.post_het_vecch(c.X, c.impNN, c.scale, c.length, name, g2, c.y, c.z), f)
    return c, R, f, e_rows, e_draw


@functools.lru_cache(maxsize=None)
def dense_case(n, name):
    """Fixed inputs of one dense case: D = 2, length 1.5 n^(-1/2), nugget 1e-4; K itself comes from the caller (the oracle on the
    host, the device's own kernel-matrix assembly in the GPU test)."""
    c = Case()
    rng = np.random.default_rng(9000 + 7 * n + (0 if name == 'sexp' else 1000000))
    c.n, c.name, c.scale, c.nugget = n, name, SCALE, 1e-4
    c.X = rng.uniform(size=(n, 2))
    c.length = np.array([1.5 * float(n) ** -0.5])
    c.gamma = np.exp(rng.normal(-1.0, 0.7, size=n))
    c.y = np.sin(4 * c.X[:, 0]) + np.sqrt(c.gamma) * rng.normal(size=n)
    c.sd = rng.normal(size=(n, 2))
    # replicates: 1-3 observations per site
    c.mask = np.repeat(np.arange(n), rng.integers(1, 4, size=n))
    c.gamma_obs = np.exp(rng.normal(-1.0, 0.7, size=len(c.mask)))
    c.y_obs = np.sin(4 * c.X[c.mask, 0]) + np.sqrt(c.gamma_obs) * rng.normal(size=len(c.mask))
    for a in (c.X, c.length, c.gamma, c.y, c.sd, c.mask, c.gamma_obs, c.y_obs):
        a.setflags(write=False)
    return c


def dense_reference(c, K, rep=False):
    """(longdouble draw, oracle error) of dense case c with the float64 kernel matrix K."""
    from oracle import dgp_oracle as O
    K = np.asarray(K, float)
    if rep:
        g, y = site_terms(c.gamma_obs, c.y_obs, c.mask, c.n)
        fo = O.post_het2(c.scale * K, c.gamma_obs, c.mask, c.y_obs, c.sd)
    else:
        g, y = c.gamma, c.y
        fo = O.post_het1(c.scale * K, c.gamma, c.y, c.sd)
    f = draw_dense(K, c.scale, g, y, c.sd)
    return f, draw_error(fo, f)
