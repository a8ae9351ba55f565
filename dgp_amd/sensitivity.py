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
