"""Calibration against field data (DESIGN I.24): T measurements at known control settings, shared calibration parameters,
errors correlated across the sites,
    y_t = f(c_t, theta) + delta(c_t) + eps_t,   t = 1 .. T
(Kennedy and O'Hagan 2001; Higdon et al. 2004; Bayarri et al. 2007), delta's covariance across the sites given as obs_cov.

The chains and the SMC of calibrate.py take a problem through two closures and a pseudo-observation (w, ybar) over K
independent outputs.  This module turns "T sites x K outputs with a T x T error covariance per output" into that form:
whiten() factors Sigma_k = obs_cov_k + diag(obs_sd_tk^2) = L_k L_k^T once, on the host, and with W_k = L_k^-1
    -1/2 sum_k r_k^T Sigma_k^-1 r_k = -1/2 sum_j w_j (ybar_j - ft_j)^2,   ft = W f,  ybar = W y,  j = t K + k,
over K' = T K pseudo-outputs; every round the walk runs at the chains' T rows each and dgpamd_boxsites_fold applies W to its
values and to the calibration columns of its Jacobian, on the device, in the layouts the step kernels read."""
import numpy as np
import scipy.linalg
import torch

from . import pathfun

MAX_SITES = 256
MAX_ROWS = None      # per-path rows of one walk call: None -- what pathfun._rows_per_call allows; an int forces smaller blocks of chains


class FieldProblem:
    """What calibrate() and calibrate_smc() take in place of observation(y, obs_sd, K): K = T K pseudo-outputs, Dx = Dtheta
    calibration columns, the pseudo-observation (ybar, w), log_norm, the closures values(xd (M, Dtheta)) -> (P, M, K) and
    value_and_jac(xt (P, R, Dtheta)) -> ((P, R, K), (P, R, K, Dtheta)) over whitened values, and width, the doubles per row and
    path of values.  columns: the calibration columns of the walk's input; controls (T, Dc)."""

    def __init__(self, K, Dx, ybar, w, log_norm, values, value_and_jac, width, columns, controls):
        self.K, self.Dx, self.ybar, self.w, self.log_norm = K, Dx, ybar, w, log_norm
        self.values, self.value_and_jac, self.width, self.columns, self.controls = values, value_and_jac, width, columns, controls


def whiten(y, obs_sd, obs_cov, K):
    """(W (K, T, T), ybar (T K,), w (T K,), log_norm) of y (T, K), NaN an unobserved entry, under errors of covariance
    Sigma_k = obs_cov_k + diag(obs_sd_tk^2) across the sites of output k, the outputs independent.  obs_sd: a positive scalar,
    (K,) or (T, K); obs_cov: None, (T, T) or (K, T, T), symmetric.  Sigma_k is restricted to the observed sites of output k and
    factored, L_k L_k^T; W_k is L_k^-1 embedded in (T, T), lower triangular, the rows and columns of unobserved sites exactly
    zero; ybar[t K + k] = (W_k y_k)_t with y 0 where it was not observed, w[t K + k] = 1 where (t, k) was observed, else 0;
    log_norm = -sum_k (T_k / 2 log 2 pi + sum log diag L_k).  With obs_cov None, W_k is the diagonal 1 / obs_sd."""
    y = np.asarray(y, dtype=np.float64)
    if y.ndim == 1 and K == 1:
        y = y[:, None]
    if y.ndim != 2 or y.shape[0] < 1 or y.shape[1] != K:
        raise ValueError('calibrate: with controls y must be (T, K), one row per site, with K = %d outputs' % K)
    T = y.shape[0]
    if np.any(np.isinf(y)):
        raise ValueError('calibrate: y must be finite (NaN marks an unobserved entry)')
    seen = ~np.isnan(y)
    if not seen.any():
        raise ValueError('calibrate: y has no finite entry')
    sd = np.asarray(obs_sd, dtype=np.float64)
    if sd.shape not in ((), (K,), (T, K)) or not np.all(np.isfinite(sd)) or not np.all(sd > 0.0):
        raise ValueError('calibrate: obs_sd must be a positive number, (K,) = (%d,) or (T, K) = (%d, %d) positive numbers' % (K, T, K))
    sd = np.broadcast_to(sd, (T, K))
    if obs_cov is not None:
        cov = np.asarray(obs_cov, dtype=np.float64)
        if cov.shape not in ((T, T), (K, T, T)) or not np.all(np.isfinite(cov)):
            raise ValueError('calibrate: obs_cov must be (T, T) = (%d, %d) or (K, T, T) finite numbers' % (T, T))
        cov = np.broadcast_to(cov, (K, T, T))
        if np.any(np.abs(cov - cov.transpose(0, 2, 1)) > 1e-12 * np.abs(cov).max()):
            raise ValueError('calibrate: obs_cov must be symmetric')
    W, ybar, log_norm = np.zeros((K, T, T)), np.zeros((T, K)), 0.0
    for k in range(K):
        at = np.nonzero(seen[:, k])[0]
        if len(at) == 0:
            continue
        if obs_cov is None:
            Wk, logdet = np.diag(1.0 / sd[at, k]), np.sum(np.log(sd[at, k]))
        else:
            S = 0.5 * (cov[k][np.ix_(at, at)] + cov[k][np.ix_(at, at)].T) + np.diag(sd[at, k] * sd[at, k])
            try:
                L = np.linalg.cholesky(S)
            except np.linalg.LinAlgError:
                raise ValueError('calibrate: obs_cov + diag(obs_sd^2) of output %d is not positive definite' % k) from None
            Wk = np.tril(scipy.linalg.solve_triangular(L, np.eye(len(at)), lower=True))
            logdet = np.sum(np.log(np.diag(L)))
        W[k][np.ix_(at, at)] = Wk
        ybar[at, k] = Wk @ y[at, k]
        log_norm -= 0.5 * len(at) * np.log(2.0 * np.pi) + logdet
    return W, ybar.reshape(-1), seen.astype(np.float64).reshape(-1), float(log_norm)


def check_controls(controls, control_columns, bounds, what):
    """(controls (T, Dc), control columns (Dc,), calibration columns (Dtheta,), Dx = Dtheta + Dc) after the refusals."""
    c = np.asarray(controls, dtype=np.float64)
    if c.ndim != 2 or not 1 <= c.shape[0] <= MAX_SITES or c.shape[1] < 1 or not np.all(np.isfinite(c)):
        raise ValueError('%s: controls must be (T, Dc) finite numbers, 1 <= T <= %d sites and Dc >= 1' % (what, MAX_SITES))
    if control_columns is None:
        raise ValueError('%s: controls need control_columns, their columns of the input' % what)
    cc = np.asarray(control_columns)
    if cc.ndim != 1 or cc.shape[0] != c.shape[1] or not np.issubdtype(cc.dtype, np.integer) or len(set(cc.tolist())) != len(cc):
        raise ValueError('%s: control_columns must be Dc = %d distinct ints' % (what, c.shape[1]))
    b = np.asarray(bounds, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != 2 or not 1 <= b.shape[0] <= 64:
        raise ValueError('%s: with controls bounds must be (Dtheta, 2), one [low, high] per calibration column, 1 <= Dtheta <= 64' % what)
    Dx = b.shape[0] + len(cc)
    if cc.min() < 0 or cc.max() >= Dx:
        raise ValueError('%s: control_columns must lie in 0 .. Dtheta + Dc - 1 = %d' % (what, Dx - 1))
    theta = np.setdiff1d(np.arange(Dx), cc)
    return c, cc.astype(np.int64), theta, Dx


def prepare(lane_problem, what, y, obs_sd, bounds, controls, control_columns, obs_cov):
    """What PathFunctions.calibrate, GpPaths.calibrate and their _smc siblings pass on: (lane_problem's tuple, FieldProblem
    or None).  lane_problem(bounds, what) is the container's _lane_problem.  Without controls: the tuple for `bounds` and
    None, today's path."""
    if controls is None:
        if obs_cov is not None or control_columns is not None:
            raise ValueError('%s: obs_cov and control_columns need controls' % what)
        return lane_problem(bounds, what), None
    c, cc, theta, Dx = check_controls(controls, control_columns, bounds, what)
    lane = lane_problem(np.zeros((Dx, 2)), what)          # (its check: Dtheta + Dc covers every column the model reads)
    e, P, K, _, values, value_and_jac, width = lane
    W, ybar, w, log_norm = whiten(y, obs_sd, obs_cov, K)
    T = len(c)
    if W.shape[1] != T:
        raise ValueError('%s: y has %d rows, controls %d sites' % (what, W.shape[1], T))
    return lane, FieldProblem(T * K, len(theta), ybar, w, log_norm,
                              *site_closures(e, P, K, Dx, values, value_and_jac, width, W, c, cc, theta), width * T, theta, c)


def site_closures(e, P, K, Dx, values, value_and_jac, width, W, controls, control_columns, theta_columns):
    """(values, value_and_jac) of a FieldProblem from the walk's own.  A chain's theta becomes T rows of the walk, the controls in
    their columns; the walk's (.., T, K) values and (.., T, K, Dx) Jacobian go through Engine.boxsites_fold.  The rows live in
    one (Q, T, Dx) tensor per shape of the trial points: the controls are written once, every round copies the theta columns in."""
    T, Dt = len(controls), len(theta_columns)
    plan = e.boxsites_plan(W, theta_columns)
    cd, ccd, thd = e.tensor(controls), torch.as_tensor(control_columns, device=e.device), torch.as_tensor(theta_columns, device=e.device)
    keep = {}

    def rows(key, n):
        """The (n, T, Dx) rows of shape `key` and its fold outputs, made at first use."""
        if key not in keep:
            X = e.zeros(n, T, Dx)
            X[:, :, ccd] = cd
            keep[key] = X, (e.empty(n, T * K), e.empty(n, T * K, Dt))
        return keep[key]

    def shared(xd):
        # M shared theta rows -> M T shared rows of the walk -> the fold with Q = P M (the values alone)
        M = xd.shape[0]
        X = e.zeros(M, T, Dx)
        X[:, :, ccd] = cd
        X[:, :, thd] = xd[:, None, :]
        f = values(X.view(M * T, Dx)).contiguous()
        return e.boxsites_fold(f.view(P * M, T, K), None, plan)[0].view(P, M, T * K)

    def per_path(xt):
        R = xt.shape[1]
        Q = P * R
        X, out = rows(('lane', R), Q)
        X[:, :, thd] = xt.reshape(Q, 1, Dt)
        X4 = X.view(P, R, T, Dx)
        # the walk with its Jacobian holds about this many doubles per row and path
        step = pathfun._rows_per_call(e, P, width + (3 * K + 4) * Dx) if MAX_ROWS is None else int(MAX_ROWS)
        step = max(1, step // T)                          # chains of a draw per walk call
        if step >= R:
            f, J = value_and_jac(X.view(P, R * T, Dx))
            f, J = f.contiguous(), J.contiguous()
        else:                                             # contiguous blocks of chains; a row's values do not depend on its block
            f, J = e.empty(P, R, T, K), e.empty(P, R, T, K, Dx)
            for r0 in range(0, R, step):
                r1 = min(R, r0 + step)
                fb, Jb = value_and_jac(X4[:, r0:r1].reshape(P, (r1 - r0) * T, Dx))
                f[:, r0:r1] = fb.reshape(P, r1 - r0, T, K)
                J[:, r0:r1] = Jb.reshape(P, r1 - r0, T, K, Dx)
        ft, Jt = e.boxsites_fold(f.view(Q, T, K), J.view(Q, T, K, Dx), plan, out=out)
        return ft.view(P, R, T * K), Jt.view(P, R, T * K, Dt)
    return shared, per_path
