"""Numpy restatement of the input gradients of function-valued posterior draws (DESIGN I.13), for
tests/test_pathgrad_host.py and tests/test_gpu_pathgrad.py.  Correlations are the oracle's (cross_corr), as in pathfun_ref.

    f_p(x)       = sqrt(s) (  sqrt(2/F) sum_f theta_pf cos(Omega_f . x + b_f)          + sum_i v_pi c(x, W_i) )
    df_p / dx_d  = sqrt(s) ( -sqrt(2/F) sum_f theta_pf Omega_fd sin(Omega_f . x + b_f) + sum_i v_pi c(x, W_i) q_d(x, W_i) )
    sexp:       q_d = -2 t_d / g_d,                                                        t_d = (x_d - W_id) / g_d
    matern2.5:  q_d = -(5/3) t_d (1 + sqrt5 r_d) / (1 + sqrt5 r_d + (5/3) r_d^2) / g_d,    r_d = |t_d|
"""
import numpy as np

from oracle import dgp_oracle as O

EPS = np.finfo(float).eps
SQRT5 = np.sqrt(5.0)


def lengths_of(length, D):
    g = np.asarray(length, dtype=np.float64).reshape(-1)
    return np.full(D, g[0]) if g.size == 1 else g.reshape(D)


def q(x, W, kind, length):
    """q_d(x_m, W_i) = d log c(x_m, W_i) / d x_md, (n, M, D)."""
    g = lengths_of(length, x.shape[1])
    t = (x[None, :, :] - W[:, None, :]) / g
    if kind == 'sexp':
        return -2.0 * t / g
    if kind != 'matern2.5':
        raise ValueError(kind)
    r = np.abs(t)
    return -(5.0 / 3.0) * t * (1.0 + SQRT5 * r) / (1.0 + SQRT5 * r + (5.0 / 3.0) * r * r) / g


def grad(x, W, Omega, b, theta, v, kind, length, scale):
    """df_p / dx_d at the rows of x (M, D): (P, M, D); W None or v None: the prior part alone."""
    F = len(b)
    out = -np.sqrt(2.0 / F) * np.einsum('pf,mf,fd->pmd', theta, np.sin(x @ Omega.T + b), Omega)
    if W is not None and v is not None and len(W):
        out = out + np.einsum('pi,im,imd->pmd', v, O.cross_corr(W, x, length, kind), q(x, W, kind, length))
    return np.sqrt(scale) * out


def tolerance(x, W, Omega, b, theta, v, kind, length, scale, const=8.0):
    """The forward-error bound of grad per (path, row, column), (P, M, D):
        const eps sqrt(s) [ sqrt(2/F) sum_f |theta_f| |Omega_fd| (D |Omega_f . x + b_f| + 4)
                            + sum_i |v_i| c(x, W_i) ((D + 6) |q_d| + 2 kappa_d (|x_d| + |W_id|) / g_d) ],
    kappa_d = 2 / g_d (sexp), (5/3) / g_d (matern2.5).  The sine takes the rounding of its argument as the cosine does
    (pathfun_ref.tolerance) and is multiplied by Omega_fd; a term of the second sum is the correlation (D + 4) times q_d (2
    more), and q_d moves by at most kappa_d per unit of t_d, whose own error is the rounding of x_d / g_d and W_id / g_d
    before their difference: absolute, not relative to t_d (it is what is left where x sits on a training row)."""
    D, F = x.shape[1], len(b)
    g = lengths_of(length, D)
    t = np.sqrt(2.0 / F) * np.einsum('pf,mf,fd->pmd', np.abs(theta), D * np.abs(x @ Omega.T + b) + 4.0, np.abs(Omega))
    if W is not None and v is not None and len(W):
        kappa = (2.0 if kind == 'sexp' else 5.0 / 3.0) / g
        per = (D + 6.0) * np.abs(q(x, W, kind, length)) + 2.0 * kappa * (np.abs(x)[None, :, :] + np.abs(W)[:, None, :]) / g
        t = t + np.einsum('pi,im,imd->pmd', np.abs(v), O.cross_corr(W, x, length, kind), per)
    return const * EPS * np.sqrt(scale) * t


def scatter(g, columns, Dx):
    """(..., D) -> (..., Dx): column i of g added into column columns[i]."""
    out = np.zeros(g.shape[:-1] + (Dx,))
    for i, c in enumerate(columns):
        out[..., int(c)] += g[..., i]
    return out


def chain(g, below, input_dim, connect, Dx):
    """The Jacobian (P, M, Dx) of a deeper node with respect to the emulator's input: g (P, M, D_node) its own gradient, the
    first len(input_dim) columns fed by the nodes input_dim of the layer below, whose Jacobians are below (P, M, K, Dx), the
    rest by the columns `connect` of the input."""
    kd = len(input_dim)
    J = np.einsum('pmk,pmkx->pmx', g[..., :kd], below[:, :, list(input_dim), :])
    return J if connect is None else J + scatter(g[..., kd:], connect, Dx)


def central(f, x, h=1e-6):
    """Central differences of f: (M, Dx) -> (P, M) at step h, (P, M, Dx)."""
    cols = []
    for d in range(x.shape[1]):
        e = np.zeros(x.shape[1])
        e[d] = h
        cols.append((f(x + e) - f(x - e)) / (2.0 * h))
    return np.stack(cols, 2)
