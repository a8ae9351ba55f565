"""Numpy restatement of function-valued posterior draws by local conditioning (DESIGN I.14), for
tests/test_vpathfun_host.py, tests/test_gpu_vpathfun.py and tests/test_gpu_vpathfun_model.py.

    r_p    = y / sqrt(s) - Phi(W) theta_p - sqrt(eta omega) * eps_p
    f_p(x) = sqrt(s) (phi(x)^T theta_p + b(x)^T r_p[N(x)]),   b(x) = A_N^-1 a
N(x) the m nearest training rows of x in coordinates divided by the lengths (nearest first, ties to the smaller index; all n in
index order when m >= n), A_N their correlation block with diagonal 1 + jitter + eta omega_j, a = c(W_N, x).  Written from the
two formulas: its correlation is its own (test_vpathfun_host.py holds it to the oracle's), the prior part and r are
tests/pathfun_ref.py's.
"""
import numpy as np

import pathfun_ref as R

SQ5 = np.sqrt(5.0)
LADDER = (0.0, 1e-10, 1e-8)


def corr(d, kind):
    """Correlation of points whose SCALED coordinates differ by d (..., D)."""
    if kind == 'sexp':
        return np.exp(-(d * d).sum(-1))
    a = np.abs(d)
    return (1.0 + SQ5 * a + (5.0 / 3.0) * a * a).prod(-1) * np.exp(-SQ5 * a.sum(-1))


def neighbours(xs, Ws, m, pad=None):
    """N(x) of scaled rows xs (R, D) among scaled training rows Ws (n, D): (R, pad or min(m, n)) int64, -1 padded."""
    n = len(Ws)
    if m >= n:
        NN = np.tile(np.arange(n, dtype=np.int64), (len(xs), 1))
    else:
        d = ((xs[:, None, :] - Ws[None, :, :]) ** 2).sum(-1)
        NN = np.argsort(d, axis=1, kind='stable')[:, :m].astype(np.int64)
    if pad is not None and pad > NN.shape[1]:
        NN = np.concatenate((NN, np.full((len(xs), pad - NN.shape[1]), -1, np.int64)), 1)
    return NN


def blocks(xs, Ws, NN, kind, nugget, omega=None, jitter=0.0):
    """(A (R, pm, pm), a (R, pm)): padded members are unit rows of A and zeros of a, so that b is zero there."""
    valid = NN >= 0
    idx = np.where(valid, NN, 0)
    Z = Ws[idx]
    A = corr(Z[:, :, None, :] - Z[:, None, :, :], kind) * (valid[:, :, None] & valid[:, None, :])
    om = np.ones(len(Ws)) if omega is None else omega
    k = np.arange(NN.shape[1])
    A[:, k, k] = np.where(valid, 1.0 + jitter + nugget * om[idx], 1.0)
    return A, corr(Z - xs[:, None, :], kind) * valid


def coefficients(xs, Ws, NN, kind, nugget, omega=None, jitter=0.0, chunk=256):
    """b (R, pm), float64 numpy solves."""
    out = np.empty(NN.shape)
    for i in range(0, len(xs), chunk):
        A, a = blocks(xs[i:i + chunk], Ws, NN[i:i + chunk], kind, nugget, omega, jitter)
        out[i:i + chunk] = np.linalg.solve(A, a[..., None])[..., 0]
    return out


def coefficients_longdouble(xs, Ws, NN, kind, nugget, omega=None, jitter=0.0):
    """b (R, pm) from a Cholesky solve in numpy.longdouble of the same float64 blocks."""
    out = np.empty(NN.shape, np.longdouble)
    for i in range(len(xs)):
        A, a = blocks(xs[i:i + 1], Ws, NN[i:i + 1], kind, nugget, omega, jitter)
        A, v = A[0].astype(np.longdouble), a[0].astype(np.longdouble)
        k = len(v)
        for j in range(k):
            A[j, j] = np.sqrt(A[j, j])
            A[j + 1:, j] /= A[j, j]
            A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
        for j in range(k):
            v[j] = (v[j] - A[j, :j] @ v[:j]) / A[j, j]
        for j in range(k - 1, -1, -1):
            v[j] = (v[j] - A[j + 1:, j] @ v[j + 1:]) / A[j, j]
        out[i] = v
    return out


def update(B, NN, r):
    """(sum_j b_j r[N_j], sum_j |b_j r_j|), each (P, R), for b (R, pm) and r (P, n)."""
    idx = np.where(NN >= 0, NN, 0)
    t = B[None] * r[:, idx]   # (P, R, pm)
    return t.sum(-1), np.abs(t).sum(-1)


def evaluate(x, W, Omega, b, theta, r, kind, length, scale, nugget, m, omega=None):
    """f (P, M) at x (M, D) shared by every path: r (P, n) = pathfun_ref.bracket's."""
    xs, Ws = x / length, W / length
    NN = neighbours(xs, Ws, m)
    B = coefficients(xs, Ws, NN, kind, nugget, omega)
    return np.sqrt(scale) * (theta @ R.phi(x, Omega, b).T + update(B, NN, r)[0])


def evaluate_per_path(x, W, Omega, b, theta, r, kind, length, scale, nugget, m, omega=None):
    """f (P, M) at x (P, M, D), every path its own rows, one training set W."""
    out = np.empty(x.shape[:2])
    for p in range(len(x)):
        out[p] = evaluate(x[p], W, Omega, b, theta[p:p + 1], r[p:p + 1], kind, length, scale, nugget, m, omega)[0]
    return out


def variance(x, W, Omega, b, kind, length, scale, nugget, m, omega=None):
    """(variance of f(x) over (theta, eps) given the features (M,), the limit s (1 - a^T A_N^-1 a) (M,), |b|_1 (M,))."""
    xs, Ws = x / length, W / length
    NN = neighbours(xs, Ws, m)
    A, a = blocks(xs, Ws, NN, kind, nugget, omega)
    B = np.linalg.solve(A, a[..., None])[..., 0]
    om = np.ones(len(W)) if omega is None else omega
    Px, PW = R.phi(x, Omega, b), R.phi(W, Omega, b)
    var = np.empty(len(x))
    for i in range(len(x)):
        g = Px[i] - B[i] @ PW[NN[i]]   # [1, -b] Phi
        var[i] = scale * (g @ g + nugget * (B[i] ** 2 * om[NN[i]]).sum())
    return var, scale * (1.0 - (a * B).sum(1)), np.abs(B).sum(1)
