"""Numpy restatement of function-valued posterior draws (DESIGN I.12), for tests/test_pathfun_host.py and
tests/test_gpu_pathfun.py.  Correlations are the oracle's (cross_corr, corr_matrix).

    phi(x) = sqrt(2/F) cos(Omega x + b)
    v_p    = R^-1 (y / sqrt(s) - Phi(W) theta_p - sqrt(eta omega) * eps_p),   R = c(W, W) + eta diag(omega)
    f_p(x) = sqrt(s) (phi(x)^T theta_p + c(x, W) v_p)
"""
import numpy as np

from oracle import dgp_oracle as O

EPS = np.finfo(float).eps


def phi(x, Omega, b):
    """(M, F)."""
    return np.sqrt(2.0 / len(b)) * np.cos(x @ Omega.T + b)


def train_corr(W, kind, length, nugget, omega=None):
    n = len(W)
    R = O.corr_matrix(W, length, kind)
    R[np.arange(n), np.arange(n)] = 1.0 + nugget * (1.0 if omega is None else omega)
    return R


def bracket(W, y, Omega, b, theta, eps, scale, nugget, omega=None):
    """r (P, n): what R^-1 is applied to.  y (n,) or (P, n); theta (P, F); eps (P, n)."""
    om = np.ones(len(W)) if omega is None else omega
    return y / np.sqrt(scale) - theta @ phi(W, Omega, b).T - np.sqrt(nugget * om) * eps


def weights(W, y, Omega, b, theta, eps, kind, length, scale, nugget, omega=None):
    """v (P, n)."""
    R = train_corr(W, kind, length, nugget, omega)
    return np.linalg.solve(R, bracket(W, y, Omega, b, theta, eps, scale, nugget, omega).T).T


def evaluate(x, W, Omega, b, theta, v, kind, length, scale):
    """f (P, M) at x (M, D); W None or v None: the prior part alone."""
    f = theta @ phi(x, Omega, b).T
    if W is not None and v is not None and len(W):
        f = f + v @ O.cross_corr(W, x, length, kind)
    return np.sqrt(scale) * f


def tolerance(x, W, Omega, b, theta, v, kind, length, scale, const=8.0):
    """The forward-error bound of evaluate per (path, row), (P, M):
        const eps sqrt(s) [ sqrt(2/F) sum_f |theta_f| (D |Omega_f . x + b_f| + 4) + (D + 4) sum_i |v_i| c(x, W_i) ]:
    the argument of a cosine is a sum of D + 1 terms whose rounding, relative to the argument, passes through |sin| <= 1
    into the cosine, plus the cosine's, the coefficient's and the sum's own roundings (4); a correlation is a product
    of D factors, the exponential and the sum (D + 4)."""
    D, F = x.shape[1], len(b)
    t = np.sqrt(2.0 / F) * np.abs(theta) @ (D * np.abs(x @ Omega.T + b) + 4.0).T
    if W is not None and v is not None and len(W):
        t = t + (D + 4.0) * np.abs(v) @ O.cross_corr(W, x, length, kind)
    return const * EPS * np.sqrt(scale) * t


def moments(x, W, y, Omega, b, kind, length, scale, nugget, omega=None):
    """(mean (M,), covariance (M, M), B (M, n)) of f(x) over (theta, eps) given the features:
    mean = sqrt(s) B y / sqrt(s) = B y with B = c(x, W) R^-1; covariance = s (A A^T + eta B diag(omega) B^T),
    A = Phi(x) - B Phi(W)."""
    om = np.ones(len(W)) if omega is None else omega
    R = train_corr(W, kind, length, nugget, omega)
    B = np.linalg.solve(R, O.cross_corr(W, x, length, kind)).T
    A = phi(x, Omega, b) - B @ phi(W, Omega, b)
    return B @ y, scale * (A @ A.T + nugget * (B * om) @ B.T), B


def exact_cov(x, W, kind, length, scale, nugget, omega=None):
    """s (K** - K*^T R^-1 K*) (no nugget on the test diagonal)."""
    R = train_corr(W, kind, length, nugget, omega)
    Ks = O.cross_corr(W, x, length, kind)
    return scale * (O.cross_corr(x, x, length, kind) - Ks.T @ np.linalg.solve(R, Ks))


SEED_DIST = 4   # the global-generator seed of the distributional check: the restatement alone passes it (test_pathfun_host.py)


def dist_case():
    """The gp model and rows of the distributional check: (X (50, 2), Y (50, 1), x (20, 2), kind, lengths, scale, nugget,
    F, P)."""
    rng = np.random.default_rng(1)
    n, M = 50, 20
    X = rng.uniform(size=(n, 2))
    Y = (np.sin(4 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.normal(size=n))[:, None]
    x = rng.uniform(size=(M, 2))
    return X, Y, x, 'matern2.5', np.full(2, 0.7), 1.9, 1e-2, 4096, 4000


def dist_z(draws, mean, Sigma, C):
    """The two statistics of the distributional check for draws (M, P): max |sample mean - mean| / sqrt(Sigma_ii / P) (<= 5)
    and max |sample covariance - C| / sqrt((C_ii C_jj + C_ij^2) / P) (<= 6)."""
    P = draws.shape[1]
    zm = np.abs(draws.mean(1) - mean) / np.sqrt(np.diag(Sigma) / P)
    zc = np.abs(np.cov(draws) - C) / np.sqrt((np.outer(np.diag(C), np.diag(C)) + C ** 2) / P)
    return zm.max(), zc.max()
