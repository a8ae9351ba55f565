"""Host reference of the dense factorisation (csrc/chol.hip, csrc/potrf_step.hpp, csrc/potrf_mega.hpp, csrc/diagfac.hpp): backward errors of dgpamd_potrf,
dgpamd_potrf_inv and dgpamd_potri_batched in extended arithmetic, LAPACK's values of the same measures on the same input,
and matrices that fail at a chosen pivot.  numpy / scipy / mpmath only.

Why residuals.  A forward comparison with LAPACK's factor cannot be held tighter than cond(A) u, and the kernel matrices of
the models reach cond 1e9: a factor that lost six digits passes rtol 1e-8.  Residuals do not depend on the conditioning: a
backward-stable Cholesky has ||A - L L^T||_F / ||A||_F of a few u = 2^-53 at every cond(A), and LAPACK, which obeys the same
a-priori bound, is the yardstick: device <= BOUND_FACTOR * max(LAPACK's value on the same input, 1 u)  (bound()).

Measures (all returned in units of u; L = the device's factor, rows and columns < n, w = buffer row n after the
factorisation = L^-1 y, tr / tc = tile row / column of 64):
    eps_L      ||A - L L^T||_F / ||A||_F
    eps_w      ||L w - y||_2 / (||L||_F ||w||_2 + ||y||_2)
    corner     | -A[n,n] - w.w | / (w.w): a-priori at most (n + 2) u, the any-order bound of a length-n dot product of
               non-negative terms (corner_bound(); w.w is taken exactly from the device's own w)
    eps_T      ||L T^T - I||_F and ||T^T L - I||_F, each over ||L||_F ||T||_F, T masked to tr <= tc
    eps_S      ||A S - I||_F / (||A||_F ||S||_F)
    eps_alpha  ||A alpha - y||_2 / (||A||_F ||alpha||_2 + ||y||_2), alpha = -(row n of S)
    eps_logdet |logdet - ref| / (n + |ref|), ref = 2 sum log of the pivots of a Cholesky column loop in numpy.longdouble
               (`well` family only: elsewhere the log-determinant's forward error is cond(A) u and says nothing).  The unit:
               the sum of n logarithms, each good to an ulp of a number of order one, rounded to an ulp of the result.

Extended arithmetic.  numpy.longdouble products (64-bit significands, error n 2^-64 of the product of magnitudes: below u / 64
of every measure for n <= 320, tests/test_chol_ref_host.py) up to n = FULL_MAX = 320; above, double-double (Veltkamp split,
TwoProduct, TwoSum, vectorised over the rows; error n 2^-104) and never the residual matrix R itself: R is applied to V, an
n x 8 matrix of seeded +-1 entries (E ||R V||_F^2 / 8 = ||R||_F^2; the products with +-1 are exact, the sums are not and are
taken in double-double as well), ||R V||_F / sqrt(8) estimates ||R||_F."""
import functools
import hashlib
import math

import numpy as np

U = 2.0**-53
FULL_MAX = 320       # full residual matrices in longdouble up to here, double-double probes above
NPROBE = 8
BOUND_FACTOR = 4.0   # different summation order and blocking than LAPACK's
LD = np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63   # (x87 extended; elsewhere every product is double-double)


# ---------------------------------------------------------------------------------------------------- inputs
def seed_of(n, family):
    return 7000 + 10 * n + ('well', 'matern', 'sexp').index(family)


def _sqdist(X):
    d = X[:, None, :] - X[None, :, :]
    return (d * d).sum(-1)


def family(name, n, seed=None, nugget=None):
    """(K, y) of one matrix family, built on the host in float64 (the device is handed exactly these numbers).
    well: G G^T / (n + 3) + 0.5 I, cond ~ 9; matern: Matern-2.5 of 3 uniform inputs, length 0.8, nugget 1e-8;
    sexp: exp(-d^2 / length^2), length 0.6, nugget 1e-6 (cond 1e8 .. 3e9 at n = 320 .. 511 for the last two)."""
    rng = np.random.default_rng(seed_of(n, name) if seed is None else seed)
    if name == 'well':
        G = rng.normal(size=(n, n + 3))
        K = G @ G.T / (n + 3) + 0.5 * np.eye(n)
    else:
        X = rng.uniform(size=(n, 3))
        d2 = _sqdist(X)
        if name == 'matern':
            r = np.sqrt(5.0 * d2) / 0.8
            K = (1.0 + r + r * r / 3.0) * np.exp(-r) + (1e-8 if nugget is None else nugget) * np.eye(n)
        elif name == 'sexp':
            K = np.exp(-d2 / 0.36) + (1e-6 if nugget is None else nugget) * np.eye(n)
        else:
            raise ValueError(name)
    K = 0.5 * (K + K.T)
    y = rng.normal(size=n)
    return K, y


def buffer(K, y, Np):
    """The augmented buffer the entry points take: M[:n,:n] = K, M[n,:n] = y."""
    n = K.shape[0]
    M = np.zeros((Np, Np))
    M[:n, :n] = K
    M[n, :n] = y
    return M


def failing(K, p, kind):
    """A copy of K whose first leading minor that is not positive is minor p (1-based).
    neg: K[p-1,p-1] = its Schur value K[i,:i] K[:i,:i]^-1 K[:i,i] minus 0.1 (pivot p is -0.1); zero: the identity with 0 at p;
    nan_diag: NaN at (p,p); nan_row: NaN at (p,1), both triangles, p >= 2 (exact elimination first meets a NaN pivot at p)."""
    n = K.shape[0]
    assert 1 <= p <= n
    i = p - 1
    A = K.copy()
    if kind == 'neg':
        s = K[i, :i] @ np.linalg.solve(K[:i, :i], K[:i, i]) if i else 0.0
        A[i, i] = s - 0.1
    elif kind == 'zero':
        A = np.eye(n)
        A[i, i] = 0.0
    elif kind == 'nan_diag':
        A[i, i] = np.nan
    elif kind == 'nan_row':
        assert p >= 2
        A[i, 0] = A[0, i] = np.nan
    else:
        raise ValueError(kind)
    return A


def tiles(n):
    return np.arange(n)[:, None] // 64, np.arange(n)[None, :] // 64


def mask_T(T, n):
    """potrf_inv's T where it is defined: tile row <= tile column."""
    tr, tc = tiles(n)
    return np.where(tr <= tc, T[:n, :n], 0.0)


def complete_S(S, n):
    """Symmetric completion of the tr >= tc tiles of potrf_inv's S."""
    tr, tc = tiles(n)
    return np.where(tr >= tc, S[:n, :n], S[:n, :n].T)


def probes(n):
    return np.random.default_rng(99 + n).integers(0, 2, size=(n, NPROBE)) * 2.0 - 1.0


# ---------------------------------------------------------------------------------------------------- extended arithmetic
_SPLITTER = 134217729.0   # 2^27 + 1


def _split(a):
    c = _SPLITTER * a
    hi = c - (c - a)
    return hi, a - hi


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def dd_matmul(A, Bh, Bl=None):
    """A (float64, m x k) times the double-double matrix Bh + Bl (k x q) -> (hi, lo).  One rank-one step per column of A,
    restricted to the rows between that column's first and last non-zero (triangular factors cost half)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    m, kk = A.shape
    q = Bh.shape[1]
    Ah, Al = _split(A)
    Bhh, Bhl = _split(Bh)
    sh, sl = np.zeros((m, q)), np.zeros((m, q))
    nz = A != 0.0
    first = np.argmax(nz, axis=0)
    last = m - np.argmax(nz[::-1], axis=0)
    some = nz.any(axis=0)
    for k in range(kk):
        if not some[k]:
            continue
        r = slice(first[k], last[k])
        a, ah, al = A[r, k:k + 1], Ah[r, k:k + 1], Al[r, k:k + 1]
        p = a * Bh[k]
        e = ((ah * Bhh[k] - p) + ah * Bhl[k] + al * Bhh[k]) + al * Bhl[k]   # TwoProduct: a * Bh[k] = p + e exactly
        if Bl is not None:
            e += a * Bl[k]
        s, t = _two_sum(sh[r], p)
        t += sl[r] + e
        hi = s + t
        sl[r] = t - (hi - s)
        sh[r] = hi
    return sh, sl


class _LongDouble:
    name = 'longdouble'

    @staticmethod
    def prod(mats):
        X = mats[-1].astype(LD)
        for M in reversed(mats[:-1]):
            X = M.astype(LD) @ X
        return X

    @staticmethod
    def diff(X, Y):
        return X - Y


class _DoubleDouble:
    name = 'double-double'

    @staticmethod
    def prod(mats):
        X = (np.asarray(mats[-1], dtype=np.float64), None)
        for M in reversed(mats[:-1]):
            X = dd_matmul(M, *X)
        return X

    @staticmethod
    def diff(X, Y):
        s, t = _two_sum(X[0], -Y[0])
        if X[1] is not None:
            t = t + X[1]
        if Y[1] is not None:
            t = t - Y[1]
        return s.astype(LD) + t.astype(LD)


class _Mpmath:
    """60 digits: the check of the other two (tests/test_chol_ref_host.py), n <= 40."""
    name = 'mpmath'

    @staticmethod
    def prod(mats):
        import mpmath
        with mpmath.workdps(60):
            X = mpmath.matrix(np.asarray(mats[-1], dtype=np.float64).tolist())
            for M in reversed(mats[:-1]):
                X = mpmath.matrix(np.asarray(M, dtype=np.float64).tolist()) * X
        return X

    @staticmethod
    def diff(X, Y):
        import mpmath
        with mpmath.workdps(60):
            R = X - Y
            return np.array([[LD(float(R[i, j])) for j in range(R.cols)] for i in range(R.rows)], dtype=LD)


LONGDOUBLE, DOUBLEDOUBLE, MPMATH = _LongDouble, _DoubleDouble, _Mpmath


def arith_for(n):
    return LONGDOUBLE if (n <= FULL_MAX and HAVE_LD) else DOUBLEDOUBLE


def fro(x):
    x = np.asarray(x, dtype=LD)
    return float(np.sqrt((x * x).sum()))


def _resid_norm(plus, minus, n, ar=None, probe=None):
    """||prod(plus) - prod(minus)||_F of n-row square products; above FULL_MAX (or with probe=True) the estimate through the
    +-1 probes."""
    ar = arith_for(n) if ar is None else ar
    probe = n > FULL_MAX if probe is None else probe
    if probe:
        V = probes(n)
        return fro(ar.diff(ar.prod(plus + [V]), ar.prod(minus + [V]))) / math.sqrt(NPROBE)
    return fro(ar.diff(ar.prod(plus), ar.prod(minus)))


def exact_dot(a, b):
    """a.b correctly rounded: the exact products (TwoProduct) summed exactly (math.fsum)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ah, al = _split(a)
    bh, bl = _split(b)
    p = a * b
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return math.fsum(np.concatenate((p, e)))


# ---------------------------------------------------------------------------------------------------- measures, in units of u
def eps_L(A, L, ar=None, probe=None):
    n = A.shape[0]
    return _resid_norm([A], [L, np.ascontiguousarray(L.T)], n, ar, probe) / fro(A) / U


def panel_residuals(A, L, ar=None):
    """Per 64-column block k with rows below it: ||P_k L_kk^T - B_k||_F / ||A||_F in units of u, P_k = L[k1:, k0:k1] the
    panel and B_k = A[k1:, k0:k1] - sum_{j<k} P_j-terms what the solve was handed -- by construction the block column of
    L L^T - A below its diagonal block.  A triangular solve leaves u |P_k| |L_kk^T|; multiplying by an explicit inverse W_k of
    L_kk leaves up to kappa_2(L_kk) times that.  Full residual: n <= FULL_MAX."""
    n = A.shape[0]
    ar = arith_for(n) if ar is None else ar
    Rm = ar.diff(ar.prod([L, np.ascontiguousarray(L.T)]), ar.prod([A]))
    return [fro(Rm[k0 + 64:, k0:k0 + 64]) / fro(A) / U for k0 in range(0, n - 64, 64)]


def kappa_diag_blocks(L):
    """max over the 64-blocks k that have rows below them of kappa_2(L_kk) (1 when there is none)."""
    n = L.shape[0]
    return max([float(np.linalg.cond(L[k0:k0 + 64, k0:k0 + 64])) for k0 in range(0, n - 64, 64)] + [1.0])


def bound_eps_L(name, lapack_value, L_lapack):
    """The bound of eps_L.  `well`: bound().  matern, sexp: the panels are solved by multiplying with the explicit inverse W_k of
    the diagonal block's factor, which admits a growth of kappa_2(L_kk) over a triangular solve (accuracy of the
    factorisation): the larger of bound() and BOUND_FACTOR x LAPACK's value x max_k kappa_2(L_kk), kappa_2 from LAPACK's factor."""
    if name == 'well':
        return bound(lapack_value)
    return max(bound(lapack_value), BOUND_FACTOR * lapack_value * kappa_diag_blocks(L_lapack))


def blocked_model(K, explicit_inverse, chunk, nb=64):
    """A right-looking blocked Cholesky in float64 numpy that differs from LAPACK's in two switches, the two ways the device's
    does: the panel is multiplied by the explicit inverse of the diagonal block's factor (or solved against it), and the
    trailing update is rounded into the tile after every `chunk` products (the device: every product; a GEMM that sums a
    64-block from zero first: 64).  The lower factor."""
    from scipy.linalg import solve_triangular
    n = K.shape[0]
    A = np.tril(K).copy()
    for k0 in range(0, n, nb):
        k1 = min(k0 + nb, n)
        D = A[k0:k1, k0:k1]
        Lkk = np.linalg.cholesky(D + np.tril(D, -1).T)
        A[k0:k1, k0:k1] = Lkk
        if k1 == n:
            break
        if explicit_inverse:
            P = A[k1:, k0:k1] @ solve_triangular(Lkk, np.eye(k1 - k0), lower=True).T
        else:
            P = solve_triangular(Lkk, A[k1:, k0:k1].T, lower=True).T
        A[k1:, k0:k1] = P
        for c0 in range(0, k1 - k0, chunk):
            A[k1:, k1:] -= np.tril(P[:, c0:c0 + chunk] @ P[:, c0:c0 + chunk].T)
    return np.tril(A)


def eps_vec(M, x, y, normM, ar=None):
    """||M x - y||_2 / (normM ||x||_2 + ||y||_2): eps_w with (L, w, y, ||L||_F), eps_alpha with (A, alpha, y, ||A||_F)."""
    n = M.shape[0]
    ar = arith_for(n) if ar is None else ar
    r = fro(ar.diff(ar.prod([M, x[:, None]]), ar.prod([y[:, None]])))
    return r / (normM * fro(x) + fro(y)) / U


def eps_w(L, w, y, ar=None):
    return eps_vec(L, w, y, fro(L), ar)


def eps_alpha(A, alpha, y, ar=None):
    return eps_vec(A, alpha, y, fro(A), ar)


def corner(c, w):
    """(| -c - w.w | / w.w in units of u, the a-priori bound in the same units); c = buffer entry [n,n] after the call."""
    ww = exact_dot(w, w)
    return abs(-c - ww) / ww / U, float(len(w) + 2)


def eps_T(L, Tm, ar=None, probe=None):
    """(right, left): ||L T^T - I||_F and ||T^T L - I||_F over ||L||_F ||T||_F; Tm = mask_T(T, n)."""
    n = L.shape[0]
    Tt = np.ascontiguousarray(Tm.T)
    d = fro(L) * fro(Tm) * U
    eye = np.eye(n)
    return (_resid_norm([L, Tt], [eye], n, ar, probe) / d, _resid_norm([Tt, L], [eye], n, ar, probe) / d)


def eps_S(A, S, ar=None, probe=None):
    n = A.shape[0]
    return _resid_norm([A, S], [np.eye(n)], n, ar, probe) / (fro(A) * fro(S)) / U


def logdet_ref(K):
    """2 sum log of the pivots of a Cholesky column loop in numpy.longdouble, as a longdouble."""
    if not HAVE_LD:
        raise RuntimeError('logdet_ref needs a numpy.longdouble with a 64-bit significand')
    n = K.shape[0]
    L = np.zeros((n, n), dtype=LD)
    A = K.astype(LD)
    for j in range(n):
        c = A[j:, j] - L[j:, :j] @ L[j, :j]
        L[j:, j] = c / np.sqrt(c[0])
    return 2 * np.log(np.diagonal(L)).sum()


def eps_logdet(logdet, ref, n):
    return float(abs(LD(logdet) - ref) / (n + abs(ref))) / U


def bound(lapack_value):
    return BOUND_FACTOR * max(lapack_value, 1.0)


# ---------------------------------------------------------------------------------------------------- LAPACK on the same input
@functools.lru_cache(maxsize=None)
def lapack_values(n, name, nugget=None):
    """LAPACK's value of every measure that does not depend on the device's output, on family(name, n): dict with eps_L, eps_w,
    eps_S (dpotri), eps_alpha (cho_solve), eps_logdet and the reference log-determinant (`well` only), and LAPACK's factor."""
    from scipy.linalg import cho_solve, solve_triangular
    from scipy.linalg.lapack import dpotrf, dpotri
    K, y = family(name, n, nugget=nugget)
    c, info = dpotrf(K, lower=1, clean=1)
    assert info == 0, (n, name, info)
    L = np.tril(c)
    w = solve_triangular(L, y, lower=True)
    si, info = dpotri(c, lower=1)
    assert info == 0
    S = np.tril(si) + np.tril(si, -1).T
    alpha = cho_solve((c, True), y)
    out = dict(L=L, eps_L=eps_L(K, L), eps_w=eps_w(L, w, y), eps_S=eps_S(K, S), eps_alpha=eps_alpha(K, alpha, y))
    if name == 'well':
        out['logdet_ref'] = logdet_ref(K)
        out['eps_logdet'] = eps_logdet(2 * np.log(np.diagonal(L)).sum(), out['logdet_ref'], n)
    return out


_trtri_cache = {}


def lapack_eps_T(L):
    """eps_T of dtrtri applied to the device's own L (both invert the same matrix); cached on L's bytes: the two modes'
    factors are equal."""
    from scipy.linalg.lapack import dtrtri
    key = hashlib.sha1(np.ascontiguousarray(L).tobytes()).hexdigest()
    if key not in _trtri_cache:
        inv, info = dtrtri(L, lower=1)
        assert info == 0
        _trtri_cache[key] = eps_T(L, np.ascontiguousarray(np.tril(inv).T))
    return _trtri_cache[key]
