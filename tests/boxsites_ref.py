"""Field calibration (dgp_amd/fieldcal.py, csrc/boxsites.hip, DESIGN I.24) restated in numpy, written from the text of
include/dgp_amd.h and of the data model: whiten (the host factorisation, by another route than fieldcal's: the explicit inverse
of numpy's Cholesky factor), fold (dgpamd_boxsites_fold's sums in the kernel's order and with its skip rule, so that the device's
outputs can be compared with array_equal), and the field log posterior by np.linalg.solve on the covariance itself, which
knows nothing of either and checks both."""
import numpy as np

F = np.float64


def covariances(T, K, obs_sd, obs_cov):
    """Sigma (K, T, T) = obs_cov_k + diag(obs_sd_tk^2)."""
    sd = np.broadcast_to(np.asarray(obs_sd, dtype=F), (T, K))
    cov = np.zeros((K, T, T)) if obs_cov is None else np.broadcast_to(np.asarray(obs_cov, dtype=F), (K, T, T))
    return np.array([cov[k] + np.diag(sd[:, k] ** 2) for k in range(K)])


def whiten(y, obs_sd, obs_cov):
    """(W (K, T, T), ybar (T K,), w (T K,), log_norm) of y (T, K), NaN unobserved: W_k the inverse of the Cholesky factor of
    Sigma_k over output k's observed sites, zero in the rows and columns of the others; ybar[t K + k] = (W_k y_k)_t,
    w[t K + k] = 1 where observed; log_norm = -sum_k (T_k / 2 log 2 pi + sum log diag L_k)."""
    y = np.asarray(y, dtype=F)
    T, K = y.shape
    Sigma, seen = covariances(T, K, obs_sd, obs_cov), ~np.isnan(y)
    W, ybar, log_norm = np.zeros((K, T, T)), np.zeros((T, K)), 0.0
    for k in range(K):
        at = np.nonzero(seen[:, k])[0]
        if len(at) == 0:
            continue
        L = np.linalg.cholesky(Sigma[k][np.ix_(at, at)])
        W[k][np.ix_(at, at)] = np.tril(np.linalg.inv(L))
        ybar[at, k] = W[k][np.ix_(at, at)] @ y[at, k]
        log_norm -= 0.5 * len(at) * np.log(2.0 * np.pi) + np.log(np.diag(L)).sum()
    return W, ybar.reshape(-1), seen.astype(F).reshape(-1), float(log_norm)


def fold(f, J, W, cols):
    """(ft (Q, T K), Jt (Q, T K, Dt)): ft[q, t K + k] = sum_{s <= t} W[k, t, s] f[q, s, k] and Jt[q, t K + k, d] = the same sum
    over J[q, s, k, cols[d]], each from 0.0 in the order of s, every product rounded before it is added, a term whose W is
    exactly 0 skipped.  f (Q, T, K), J (Q, T, K, Dx) or None (Jt None).  The loop runs over s; all rows t >= s take their
    term of that s at once, which is the kernel's order for every one of them."""
    f, W = np.asarray(f, dtype=F), np.asarray(W, dtype=F)
    Q, T, K = f.shape
    ft = np.zeros((Q, T, K))
    Jc = None if J is None else np.ascontiguousarray(np.asarray(J, dtype=F)[..., list(cols)])
    Jt = None if J is None else np.zeros(Jc.shape)
    with np.errstate(invalid='ignore'):
        for s in range(T):
            w = W[:, s:, s].T                                 # (T - s, K): W[k, t, s] of the rows t >= s
            on = w != 0.0
            np.add(ft[:, s:], w[None] * f[:, s, None, :], out=ft[:, s:], where=on[None])
            if J is not None:
                np.add(Jt[:, s:], w[None, :, :, None] * Jc[:, s, None], out=Jt[:, s:], where=on[None, :, :, None])
    return ft.reshape(Q, T * K), None if J is None else Jt.reshape(Q, T * K, -1)


def fold_scalar(f, J, W, cols):
    """fold, one scalar operation at a time: the text of the header as loops.  For small shapes."""
    Q, T, K = f.shape
    ft, Jt = np.zeros((Q, T, K)), np.zeros((Q, T, K, len(cols)))
    for q in range(Q):
        for t in range(T):
            for k in range(K):
                acc, accJ = F(0.0), [F(0.0)] * len(cols)
                for s in range(t + 1):
                    if W[k, t, s] != 0.0:
                        acc = acc + F(W[k, t, s]) * F(f[q, s, k])
                        accJ = [a + F(W[k, t, s]) * F(J[q, s, k, c]) for a, c in zip(accJ, cols)]
                ft[q, t, k], Jt[q, t, k] = acc, accJ
    return ft.reshape(Q, T * K), Jt.reshape(Q, T * K, len(cols))


def quadratic_form(r, Sigma):
    """sum_k r_k^T Sigma_k^-1 r_k over the observed (non-NaN) entries of r (T, K), by np.linalg.solve."""
    total = 0.0
    for k in range(r.shape[1]):
        at = np.nonzero(~np.isnan(r[:, k]))[0]
        if len(at):
            total += r[at, k] @ np.linalg.solve(Sigma[k][np.ix_(at, at)], r[at, k])
    return total


def field_logp(y, f, obs_sd, obs_cov, theta=None, pv=None, pm=None):
    """The field log posterior up to its constant, -1/2 sum_k r_k^T Sigma_k^-1 r_k - 1/2 sum_d pv_d (theta_d - pm_d)^2 with
    r = y - f over the observed entries of y (T, K); f (..., T, K) -> (...)."""
    y, f = np.asarray(y, dtype=F), np.asarray(f, dtype=F)
    Sigma = covariances(*y.shape, obs_sd, obs_cov)
    out = np.empty(f.shape[:-2])
    for idx in np.ndindex(*out.shape):
        out[idx] = -0.5 * quadratic_form(y - f[idx], Sigma)
    if pv is not None:
        on = np.asarray(pv) > 0.0
        out = out - 0.5 * np.sum(np.asarray(pv)[on] * (np.asarray(theta)[..., on] - np.asarray(pm)[on]) ** 2, -1)
    return out


def line_case():
    """The one-parameter case of the issue: K = 1, f(c, theta) = theta c at c = linspace(0.2, 1, 5),
    Sigma = 0.05^2 I + 0.1^2 exp(-(c - c')^2 / (2 0.3^2)); cond(Sigma) = 12.5.  Returns (c, obs_sd, obs_cov, Sigma)."""
    c = np.linspace(0.2, 1.0, 5)
    cov = 0.1 ** 2 * np.exp(-(c[:, None] - c[None]) ** 2 / (2.0 * 0.3 ** 2))
    return c, 0.05, cov, cov + 0.05 ** 2 * np.eye(5)
