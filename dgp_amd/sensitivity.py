"""Variance-based sensitivity analysis of an emulated function: Sobol' indices of function-valued posterior draws (Le Gratiet,
Cannamela and Iooss 2014; DESIGN I.16).

Every draw of emulator.sample_functions / gp.sample_functions is a deterministic function of x, so the pick-freeze estimators
apply to it as they would to the simulator: with A, B two independent base samples of n_base rows and AB_i = A with column i
taken from B,
    V       = (sum f_A^2 + sum f_B^2) / 2 n_base - ((sum f_A + sum f_B) / 2 n_base)^2
    first_i = (1 / n_base)   sum f_B (f_AB_i - f_A) / V        (Saltelli et al. 2010)
    total_i = (1 / 2 n_base) sum (f_A - f_AB_i)^2 / V          (Jansen 1999)
per draw.  The spread of an index over the draws is its posterior uncertainty; its spread over base samples (another seed of
saltelli_design) the Monte-Carlo error.  The sums are taken on the device by dgpamd_sobol_tiles / dgpamd_sobol_add from the
values as the layer walk leaves them -- only f_A, f_B and one f_AB_i of a block of rows exist at a time, and none of them
visits the host -- on g = f - shift, shift = f_A at the first row of the design (the estimators do not depend on it), in an
order fixed by the rows alone: 64-row tiles, a fixed tree inside a tile, the tiles one after the other.  The blocks of rows
that the free device memory dictates start at multiples of 64, so the sums do not depend on them by a bit.

Derivative-based analysis of the same draws (Constantine, Dow and Wang 2014; Sobol' and Kucherenko 2009; DESIGN I.18): with
X a uniform sample of the box (uniform_design),
    C = (1 / n_rows) sum_rows grad f grad f^T
is each draw's estimate of E_x[grad f grad f^T].  The eigenvectors of S C S, S = diag((b - a) / 2) (the box mapped to
[-1, 1]^Dx), span the active subspace; the diagonal nu_i of C is the derivative-based global sensitivity measure, and
total_i <= nu_i (b_i - a_i)^2 / (pi^2 V) bounds the total Sobol' index from one gradient pass.  gradient_moments takes the
sums on the device (dgpamd_gradmom_tiles / dgpamd_sobol_add) from the values and the Jacobian as the layer walk leaves them,
in the same 64-row tiles and tile order; only the final sums visit the host.
"""
import warnings

import numpy as np

from . import pathfun, paths

TILE = 64   # rows of a tile of dgpamd_sobol_tiles: blocks of rows start at its multiples


def saltelli_design(bounds, n_base, seed=None, qmc=False):
    """(A, B), each (n_base, D): two independent samples, uniform on the box bounds (D, 2) = [[low, high], ...].
    qmc False: np.random.default_rng(seed).uniform(size=(n_base, 2 D)), columns 0 .. D - 1 for A and D .. 2 D - 1 for B.
    qmc True: the first n_base points of scipy's scrambled Sobol' sequence in 2 D dimensions (random_base2), split the same
    way; n_base must be a power of two."""
    bounds = np.asarray(bounds, dtype=np.float64)
    if bounds.ndim != 2 or bounds.shape[1] != 2 or bounds.shape[0] < 1:
        raise ValueError('saltelli_design: bounds must be (D, 2), one [low, high] per input')
    if not np.all(np.isfinite(bounds)) or np.any(bounds[:, 1] < bounds[:, 0]):
        raise ValueError('saltelli_design: every bound must be finite with low <= high')
    n_base, D = int(n_base), bounds.shape[0]
    if n_base < 1:
        raise ValueError('saltelli_design: n_base must be at least 1')
    if qmc:
        if n_base & (n_base - 1):
            raise ValueError('saltelli_design: qmc=True needs n_base a power of two (the Sobol\' sequence is balanced there), got %d' % n_base)
        from scipy.stats import qmc as _qmc
        u = _qmc.Sobol(d=2 * D, scramble=True, seed=seed).random_base2(n_base.bit_length() - 1)
    else:
        u = np.random.default_rng(seed).uniform(size=(n_base, 2 * D))
    low, width = bounds[:, 0], bounds[:, 1] - bounds[:, 0]
    return low + width * u[:, :D], low + width * u[:, D:]


def indices_from_sums(base, pair, n_base):
    """(first, total, V) from the pick-freeze sums.  base (..., 4): sum g_A, sum g_B, sum g_A^2, sum g_B^2; pair (D, ..., 2):
    sum g_B (g_AB - g_A), sum (g_A - g_AB)^2.  first and total (D, ...), V (...).  V == 0 (a constant draw) gives NaN
    indices; nothing is clipped: an estimate below 0 or above 1 shows the Monte-Carlo error it carries."""
    B = n_base
    s1, s2, q1, q2 = (base[..., c] for c in range(4))
    U, T = pair[..., 0], pair[..., 1]
    V = (q1 + q2) / (2 * B) - ((s1 + s2) / (2 * B))**2
    Vd = np.where(V == 0.0, np.nan, V)
    first = (U / B) / Vd
    total = (T / (2 * B)) / Vd
    return first, total, V


def check_design(A, B):
    """What sobol(A, B) asks of its base samples."""
    paths.check_2d(A)
    paths.check_2d(B)
    if A.shape != B.shape:
        raise ValueError('sobol: A and B must have one shape (n_base, Dx), got %s and %s' % (A.shape, B.shape))
    if len(A) < 2:
        raise ValueError('sobol: n_base must be at least 2')


def pick_freeze(e, evaluate, A, B, P, width):
    """The pick-freeze sums of P paths over the design (A, B), host arrays (n_base, Dx): evaluate(xd) -> (P, M, K)
    contiguous device tensor, the paths at the rows of the device tensor xd (M, Dx), the same bits at the same rows in every
    call.  Blocks of rows of pathfun._row_blocks (`width` doubles per row and path) that start at multiples of 64.  Returns
    host arrays {'base': (P, K, 4), 'pair': (Dx, P, K, 2), 'shift': (P, K)}."""
    Dx = A.shape[1]
    shift = base = pair = None
    for _, ab in pathfun._row_blocks(e, np.concatenate((A, B), 1), P, width, multiple=TILE):
        Ad, Bd = e.tensor(ab[:, :Dx]), e.tensor(ab[:, Dx:])
        fA = evaluate(Ad)
        if shift is None:
            K = fA.shape[2]
            shift, base, pair = fA[:, 0, :].clone(), e.zeros(P, K, 4), e.zeros(Dx, P, K, 2)
        fB = evaluate(Bd)
        e.sobol_add(e.sobol_tiles(fA, fB, None, shift), base)
        for i in range(Dx):
            ABd = Ad.clone()
            ABd[:, i] = Bd[:, i]
            e.sobol_add(e.sobol_tiles(fA, fB, evaluate(ABd), shift), pair[i])
    return {'base': base.cpu().numpy(), 'pair': pair.cpu().numpy(), 'shift': shift.cpu().numpy()}


class SobolResult:
    """Sobol' indices of every posterior draw.  first, total: (K, Dx, P) -- output, input column of the design, draw; P =
    N * sample_size, column s * sample_size + j path j of imputation s, as in sample_functions' container.  variance, mean:
    (K, P), each draw's variance and mean over the design (the 2 n_base rows of A and B).  sums: the raw device sums, host
    arrays 'base' (P, K, 4), 'pair' (Dx, P, K, 2), 'shift' (P, K) (indices_from_sums' arguments).  n_base.  For a gp model
    the K axis is dropped: (Dx, sample_size) and (sample_size,)."""

    def __init__(self, sums, n_base, squeeze=False):
        self.sums, self.n_base = sums, int(n_base)
        first, total, V = indices_from_sums(sums['base'], sums['pair'], self.n_base)
        mean = sums['shift'] + (sums['base'][..., 0] + sums['base'][..., 1]) / (2 * self.n_base)
        self.first, self.total = first.transpose(2, 0, 1), total.transpose(2, 0, 1)
        self.variance, self.mean = V.T, mean.T
        if squeeze:
            self.first, self.total, self.variance, self.mean = self.first[0], self.total[0], self.variance[0], self.mean[0]

    def summary(self, level=0.95):
        """{'first': {'mean', 'lower', 'upper'}, 'total': {...}}: per output and input ((K, Dx); (Dx,) for a gp model) the
        mean over the draws and the equal-tailed interval of probability `level` (nanmean, nanquantile: a draw with zero
        variance has no indices)."""
        if not 0.0 < level < 1.0:
            raise ValueError('summary: level must lie in (0, 1)')
        tail = 0.5 * (1.0 - level)
        out = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)   # (every draw NaN: NaN, without numpy's warning)
            for name in ('first', 'total'):
                a = getattr(self, name)
                out[name] = {'mean': np.nanmean(a, -1), 'lower': np.nanquantile(a, tail, axis=-1),
                             'upper': np.nanquantile(a, 1.0 - tail, axis=-1)}
        return out


# ---------------------------------------------------------------- active subspaces and DGSM (DESIGN I.18)
MAX_WIDTH = 64   # columns of the Jacobian that dgpamd_gradmom_tiles takes


def _check_bounds(bounds, what):
    """bounds as a float64 (D, 2) array of finite [low, high] rows, low <= high."""
    bounds = np.asarray(bounds, dtype=np.float64)
    if bounds.ndim != 2 or bounds.shape[1] != 2 or bounds.shape[0] < 1:
        raise ValueError('%s: bounds must be (D, 2), one [low, high] per input' % what)
    if not np.all(np.isfinite(bounds)) or np.any(bounds[:, 1] < bounds[:, 0]):
        raise ValueError('%s: every bound must be finite with low <= high' % what)
    return bounds


def uniform_design(bounds, n_rows, seed=None, qmc=False):
    """X (n_rows, D): a sample uniform on the box bounds (D, 2) = [[low, high], ...].
    qmc False: np.random.default_rng(seed).uniform(size=(n_rows, D)).  qmc True: the first n_rows points of scipy's scrambled
    Sobol' sequence in D dimensions (random_base2); n_rows must be a power of two."""
    bounds = _check_bounds(bounds, 'uniform_design')
    n_rows, D = int(n_rows), bounds.shape[0]
    if n_rows < 1:
        raise ValueError('uniform_design: n_rows must be at least 1')
    if qmc:
        if n_rows & (n_rows - 1):
            raise ValueError('uniform_design: qmc=True needs n_rows a power of two (the Sobol\' sequence is balanced there), got %d' % n_rows)
        from scipy.stats import qmc as _qmc
        u = _qmc.Sobol(d=D, scramble=True, seed=seed).random_base2(n_rows.bit_length() - 1)
    else:
        u = np.random.default_rng(seed).uniform(size=(n_rows, D))
    return bounds[:, 0] + (bounds[:, 1] - bounds[:, 0]) * u


def n_sums(Dx):
    """NC, the sums dgpamd_gradmom_tiles keeps per path and output: sum g, sum g^2, Dx sums of J_d, the packed upper triangle."""
    return 2 + Dx + Dx * (Dx + 1) // 2


def check_rows(X, bounds=None):
    """What active_subspace(X, bounds) asks of its design; returns bounds as a (Dx, 2) array, or None."""
    paths.check_2d(X)
    if len(X) < 2:
        raise ValueError('active_subspace: X must have at least 2 rows')
    if not 1 <= X.shape[1] <= MAX_WIDTH:
        raise ValueError('active_subspace: X must have 1 to %d columns, got %d' % (MAX_WIDTH, X.shape[1]))
    if bounds is None:
        return None
    bounds = _check_bounds(bounds, 'active_subspace')
    if bounds.shape[0] != X.shape[1]:
        raise ValueError('active_subspace: bounds has %d rows, X %d columns' % (bounds.shape[0], X.shape[1]))
    return bounds


def gradient_moments(e, value_and_jac, X, P, width):
    """The sums behind C of P paths over the rows of X, a host array (n_rows, Dx): value_and_jac(xd) -> ((P, M, K),
    (P, M, K, Dx)) device tensors, the paths and their Jacobian at the rows of the device tensor xd (M, Dx), the same bits
    at the same rows in every call.  Blocks of rows of pathfun._row_blocks (`width` doubles per row and path: the caller
    counts the Jacobians and NC / 64 per output for the partial sums) that start at multiples of 64.  shift = the values at the first row.
    Returns host arrays {'sums': (P, K, NC), 'shift': (P, K)}, sums[..., :] = sum g, sum g^2, sum J_d, sum J_d J_e (d <= e)."""
    shift = sums = None
    for _, xb in pathfun._row_blocks(e, X, P, width, multiple=TILE):
        f, J = value_and_jac(e.tensor(xb))
        if shift is None:
            shift, sums = f[:, 0, :].clone(), e.zeros(P, f.shape[2], n_sums(X.shape[1]))
        e.sobol_add(e.gradmom_tiles(f, J, shift), sums)
    return {'sums': sums.cpu().numpy(), 'shift': shift.cpu().numpy()}


def _orient(V):
    """Eigenvectors (..., Dx, k), one per column, each with its largest-magnitude component (the first of equals) positive."""
    top = np.take_along_axis(V, np.argmax(np.abs(V), -2)[..., None, :], -2)
    return V * np.where(top < 0.0, -1.0, 1.0)


def _eigh_desc(A):
    """np.linalg.eigh of the symmetric matrices A (..., Dx, Dx), eigenvalues descending, eigenvectors oriented."""
    lam, V = np.linalg.eigh(A)
    return lam[..., ::-1], _orient(V[..., ::-1])


class ActiveSubspaceResult:
    """The gradient second moment of every posterior draw and what follows from it.  sums: gradient_moments' host arrays
    'sums' (P, K, NC) and 'shift' (P, K); n_rows the rows they were taken over; bounds (Dx, 2) or None.  P = N * sample_size,
    column s * sample_size + j path j of imputation s, as in sample_functions' container.
    C (K, P, Dx, Dx): each draw's (1 / n_rows) sum grad f grad f^T, symmetric, in the units of x.  dgsm (K, Dx, P): its
    diagonal nu_i.  mean_grad (K, Dx, P).  mean, variance (K, P): each draw's over the rows (the variance from the shifted
    sums).  scale (Dx,): (b - a) / 2, ones without bounds.  eigenvalues (K, P, Dx), descending, and eigenvectors
    (K, P, Dx, Dx), [..., :, j] the j-th, largest-magnitude component positive: those of S C S, S = diag(scale).
    total_bound (K, Dx, P): nu_i (b_i - a_i)^2 / (pi^2 V) >= total_i, NaN where V == 0; ValueError without bounds.
    For a gp model (squeeze) the K axis is dropped."""

    def __init__(self, sums, n_rows, bounds=None, squeeze=False):
        self.sums, self.n_rows, self.squeeze = sums, int(n_rows), bool(squeeze)
        S, n = np.asarray(sums['sums'], dtype=np.float64), self.n_rows
        NC = S.shape[-1]
        Dx = int(round((np.sqrt(8.0 * NC - 7.0) - 3.0) / 2.0))
        if S.ndim != 3 or Dx < 1 or n_sums(Dx) != NC:
            raise ValueError('ActiveSubspaceResult: sums must be (P, K, 2 + Dx + Dx (Dx + 1) / 2)')
        self.bounds = None if bounds is None else _check_bounds(bounds, 'ActiveSubspaceResult')
        if self.bounds is not None and self.bounds.shape[0] != Dx:
            raise ValueError('ActiveSubspaceResult: bounds has %d rows, the sums %d columns' % (self.bounds.shape[0], Dx))
        self.scale = np.ones(Dx) if self.bounds is None else 0.5 * (self.bounds[:, 1] - self.bounds[:, 0])
        s1, s2 = S[..., 0] / n, S[..., 1] / n
        mean, V = sums['shift'] + s1, s2 - s1**2
        iu = np.triu_indices(Dx)
        C = np.empty(S.shape[:2] + (Dx, Dx))
        C[..., iu[0], iu[1]] = S[..., 2 + Dx:] / n
        C[..., iu[1], iu[0]] = S[..., 2 + Dx:] / n
        self._K = C.transpose(1, 0, 2, 3)                                    # (K, P, Dx, Dx)
        self._scaled = self._K * self.scale[:, None] * self.scale[None, :]
        self._lam, self._vec = _eigh_desc(self._scaled)
        self._var = V.T
        out = dict(C=self._K, dgsm=np.diagonal(self._K, axis1=-2, axis2=-1).transpose(0, 2, 1),
                   mean_grad=(S[..., 2:2 + Dx] / n).transpose(1, 2, 0), mean=mean.T, variance=self._var,
                   eigenvalues=self._lam, eigenvectors=self._vec)
        for name, a in out.items():
            setattr(self, name, a[0] if squeeze else a)

    def _out(self, a):
        return a[0] if self.squeeze else a

    @property
    def total_bound(self):
        if self.bounds is None:
            raise ValueError('total_bound: the bound needs the box (b_i - a_i); give bounds')
        width2 = (self.bounds[:, 1] - self.bounds[:, 0])**2
        Vd = np.where(self._var == 0.0, np.nan, self._var)
        nu = np.diagonal(self._K, axis1=-2, axis2=-1).transpose(0, 2, 1)
        return self._out(nu * width2[None, :, None] / (np.pi**2 * Vd[:, None, :]))

    def activity_scores(self, k):
        """(K, Dx, P): alpha_i(k) = sum_{j < k} lambda_j w_ij^2 of S C S (Constantine and Diaz 2017); k = Dx gives its diagonal."""
        k = int(k)
        if not 1 <= k <= len(self.scale):
            raise ValueError('activity_scores: k must lie in 1 .. Dx')
        return self._out(np.einsum('kpij,kpj->kip', self._vec[..., :k]**2, self._lam[..., :k]))

    def subspace(self, k, output=0):
        """(W (Dx, k), distance (P,)): the k leading eigenvectors of the mean over the draws of S C S for output `output`,
        and every draw's distance ||W W^T - W_p W_p^T||_2 to that subspace (the sine of the largest principal angle)."""
        k, output = int(k), int(output)
        if not 1 <= k <= len(self.scale):
            raise ValueError('subspace: k must lie in 1 .. Dx')
        if not 0 <= output < self._scaled.shape[0]:
            raise ValueError('subspace: output must lie in 0 .. %d' % (self._scaled.shape[0] - 1))
        W = _eigh_desc(self._scaled[output].mean(0))[1][:, :k]
        Wp = self._vec[output][:, :, :k]
        return W, np.linalg.norm(W @ W.T - Wp @ Wp.transpose(0, 2, 1), 2, axis=(-2, -1))

    def summary(self, level=0.95):
        """{'dgsm': {'mean', 'lower', 'upper'}, 'eigenvalues': {...}, 'total_bound': {...}}: the mean over the draws and the
        equal-tailed interval of probability `level` (nanmean, nanquantile); 'total_bound' only with bounds."""
        if not 0.0 < level < 1.0:
            raise ValueError('summary: level must lie in (0, 1)')
        tail = 0.5 * (1.0 - level)
        out = {}
        with warnings.catch_warnings():
            warnings.simplefilter('ignore', RuntimeWarning)   # (every draw NaN: NaN, without numpy's warning)
            for name in ('dgsm', 'eigenvalues') + (() if self.bounds is None else ('total_bound',)):
                a = getattr(self, name)
                if name == 'eigenvalues':
                    a = np.moveaxis(a, -2, -1)                # (draws last, as the others)
                out[name] = {'mean': np.nanmean(a, -1), 'lower': np.nanquantile(a, tail, axis=-1),
                             'upper': np.nanquantile(a, 1.0 - tail, axis=-1)}
        return out
