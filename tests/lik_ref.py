"""Exact log-densities of the likelihood nodes (Poisson, NegBin, ZIP, ZINB, Categorical with its four links), the magnitudes their
rounding errors may scale with, and the input grids of tests/test_lik_host.py and tests/test_gpu_lik.py.  No GPU, and no import
of the package: the formulas under test (dgp_amd/likelihood_class.py on the host, lik_point in csrc/train.hip on the device)
must not check themselves.

exact()     the log-density of one observation from its DEFINITION in mpmath at 60 digits; the inputs are the doubles given.
terms()     T: what the rounding error of a stable float64 evaluation is allowed to scale with (written out per kind there).
stable64()  that stable evaluation in numpy / scipy float64 -- used only to measure the constant c below.

The bound.  A value passes when |got - exact| <= c * 2^-53 * T + 2^-1074; the last term is the spacing of the subnormal doubles
(log ncdf(40) = -3.7e-350 is not a double, and 0 is the closest one).  A sum over observations passes when
|got - sum exact_i| <= c * 2^-53 * sum T_i + (ceil(per / 256) + 8 + 32) * 2^-53 * sum |exact_i|, per = ceil(nobs / 32): the
thread-strided pass, the tree of depth 8 and the 32 chunks added in order (lik_partial_kernel / lik_sum_kernel).

c per kind.  C_MEASURED[kind] is the largest |stable64 - exact| / (2^-53 T) over every input of the two test files (grid rows at
which float(exact) is finite), measured on the CPU by tests/test_lik_host.py::test_stable64_within_measured_c, which asserts
that it is not exceeded.  C[kind] = 4 * C_MEASURED[kind] is what the host restatement and the device are held to: the device's
exp / log1p / lgamma / erfc are other routines than numpy's and scipy's, a few ulp apart.

    kind        measured      C
    Poisson       1.88       7.52
    NegBin        3.08      12.32
    ZIP           2.58      10.32
    ZINB          3.27      13.08
    logit         1.42       5.68
    probit        1.69       6.76
    softmax       1.92       7.68
    robustmax     0.90       3.60
"""
import functools
import math

import mpmath as mp
import numpy as np

DPS = 60                        # digits of every mpmath evaluation here (set per call: mpmath's global precision is left alone)
U = 2.0 ** -53
TINY = 2.0 ** -1074
KINDS = ('Poisson', 'NegBin', 'ZIP', 'ZINB', 'logit', 'probit', 'softmax', 'robustmax')
NCOL = {'Poisson': 1, 'NegBin': 2, 'ZIP': 2, 'ZINB': 3, 'logit': 1, 'probit': 1}
C_MEASURED = {'Poisson': 1.88, 'NegBin': 3.08, 'ZIP': 2.58, 'ZINB': 3.27, 'logit': 1.42, 'probit': 1.69, 'softmax': 1.92, 'robustmax': 0.90}
C = {k: 4.0 * v for k, v in C_MEASURED.items()}
EPS = 1e-3                      # robustmax_eps of the tests
PROBIT_SWITCH = -35.0           # where log ncdf goes over to the asymptotic series (lik_log_ndtr, likelihood_class._log_ndtr)
COUNTS = (0.0, 1.0, 2.0, 63.0, 64.0, 65.0, 100.0, 1000.0, 1e6)
WILD = (-40.0, -37.0, -30.0, -20.0, -10.0, 10.0, 20.0, 30.0, 36.0, 37.0, 40.0)


# ------------------------------------------------------------------ exact values
def _m(x):
    return mp.mpf(float(x))


def _log1pexp(x):
    """log(1 + e^x) in mpmath."""
    return mp.log1p(mp.exp(x)) if x < 0 else x + mp.log1p(mp.exp(-x))


def _negbin(y, f1, f2):
    size, a = mp.exp(-f2), f1 + f2
    return mp.loggamma(y + size) - mp.loggamma(size) - mp.loggamma(y + 1) + y * a - (y + size) * _log1pexp(a)


@mp.workdps(DPS)
def exact(kind, y, f, classes=None, eps=None):
    """log p(y | f) as an mpmath number (mp.nan where a latent that is read is NaN; the robustmax rule below).

    Poisson    y f - e^f - loggamma(y + 1)
    NegBin     size = e^-f2, a = f1 + f2: loggamma(y + size) - loggamma(size) - loggamma(y + 1) + y a - (y + size) log(1 + e^a)
    ZIP        log pi = -log(1 + e^-f_pi), log(1 - pi) = -log(1 + e^f_pi), P = Poisson(f_lam): y = 0: log(pi + (1 - pi) e^P),
               y > 0: log(1 - pi) + P
    ZINB       the same with P = NegBin(f1, f2), f_pi the third latent
    logit      y f - log(1 + e^f)
    probit     log ncdf(f) for y = 1, log ncdf(-f) for y = 0
    softmax    f_y - log sum_k e^(f_k)
    robustmax  log(1 - eps) where y is the FIRST arg-max of f, else log(eps / (K - 1)); a NaN counts as the maximum, the
               first NaN wins (numpy.argmax, lik_point)
    """
    f = [float(v) for v in np.atleast_1d(f)]
    y = float(y)
    if kind == 'robustmax':
        best = 0
        for k in range(1, len(f)):
            if f[best] != f[best]:
                break
            if f[k] != f[k] or f[k] > f[best]:
                best = k
        return mp.log1p(-_m(eps)) if best == int(y) else mp.log(_m(eps) / (classes - 1))
    if any(v != v for v in f):
        return mp.nan
    f = [_m(v) for v in f]
    ym = _m(y)
    if kind == 'Poisson':
        return ym * f[0] - mp.exp(f[0]) - mp.loggamma(ym + 1)
    if kind == 'NegBin':
        return _negbin(ym, f[0], f[1])
    if kind in ('ZIP', 'ZINB'):
        p = ym * f[0] - mp.exp(f[0]) - mp.loggamma(ym + 1) if kind == 'ZIP' else _negbin(ym, f[0], f[1])
        fpi = f[-1]
        lpi, l1m = -_log1pexp(-fpi), -_log1pexp(fpi)
        if y != 0:
            return l1m + p
        hi = max(lpi, l1m + p)
        return hi + mp.log(mp.exp(lpi - hi) + mp.exp(l1m + p - hi))
    if kind == 'logit':
        return ym * f[0] - _log1pexp(f[0])
    if kind == 'probit':
        x = f[0] if y == 1 else -f[0]
        return mp.log1p(-mp.erfc(x / mp.sqrt(2)) / 2) if x > 0 else mp.log(mp.erfc(-x / mp.sqrt(2)) / 2)
    if kind == 'softmax':
        top = max(f)
        return f[int(y)] - top - mp.log(mp.fsum(mp.exp(v - top) for v in f))
    raise ValueError(kind)


@mp.workdps(DPS)
def to_float(v):
    """The double nearest to an mpmath number; +-inf beyond the double range, NaN for NaN."""
    if mp.isnan(v):
        return math.nan
    if abs(v) > mp.mpf(2) ** 1024:
        return math.copysign(math.inf, float(mp.sign(v)))
    return float(v)


@mp.workdps(DPS)
def split(v):
    """(hi, lo) doubles with hi + lo = v to 2^-106 |v|: what math.fsum adds up in place of a rounded value."""
    hi = to_float(v)
    return hi, (float(v - mp.mpf(hi)) if math.isfinite(hi) else 0.0)


# ------------------------------------------------------------------ the stable float64 form and its magnitude
def _lae0(x):
    return np.logaddexp(0.0, x)


def lgamma_rise(y, size):
    """log Gamma(y + size) - log Gamma(size) in float64, without the cancellation of the two values:
    whole counts up to 64: sum_{j<y} log(size + j); beyond, size >= 64: the difference of the two Stirling series,
    (size + y - 1/2) log1p(y / size) + y log(size) - y + [1/(12x) - 1/(360x^3) + 1/(1260x^5)] between size and size + y
    (the next term is below 1.2e-16 from x = 64 on); beyond, size < 64: the plain difference, in which nothing cancels that
    lgamma(y + 1) does not cover."""
    from scipy.special import gammaln
    y, size = np.broadcast_arrays(np.asarray(y, dtype=float), np.asarray(size, dtype=float))
    with np.errstate(all='ignore'):
        x2 = size + y
        corr = lambda x: (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0) / (x * x)) / (x * x)) / x
        stirling = (x2 - 0.5) * np.log1p(y / size) - y + y * np.log(size) + (corr(x2) - corr(size))
        out = np.where(size >= 64.0, stirling, gammaln(x2) - gammaln(size))
        small = (y >= 0.0) & (y <= 64.0) & (y == np.floor(y))
        if small.any():
            acc = np.zeros(y.shape)
            for j in range(int(y[small].max())):
                acc = acc + np.where(j < y, np.log(size + j), 0.0)
            out = np.where(small, acc, out)
    return out


def _negbin64(y, f1, f2):
    from scipy.special import gammaln
    size, a = np.exp(-f2), f1 + f2
    return lgamma_rise(y, size) - gammaln(y + 1.0) + y * a - (y + size) * _lae0(a)


def log_ndtr64(x):
    """log ncdf(x): log1p(-erfc(x / sqrt 2) / 2) above 0, log(erfc(-x / sqrt 2) / 2) down to PROBIT_SWITCH, the five-term
    asymptotic series of the Mills ratio below."""
    from scipy.special import erfc
    x = np.asarray(x, dtype=float)
    with np.errstate(all='ignore'):
        r = 1.0 / (x * x)
        ser = 1.0 + r * (-1.0 + r * (3.0 + r * (-15.0 + r * (105.0 + r * (-945.0)))))
        tail = -0.5 * x * x - np.log(-x) - 0.9189385332046727 + np.log(ser)
        mid = np.log(0.5 * erfc(-x * 0.7071067811865476))
        up = np.log1p(-0.5 * erfc(x * 0.7071067811865476))
        return np.where(x > 0.0, up, np.where(x > PROBIT_SWITCH, mid, tail))


def zero_inflated64(f_pi, p):
    """log(pi + (1 - pi) e^p), pi = expit(f_pi), p <= 0 the base count model's log-probability of a zero.  With
    q = (1 - pi)(1 - e^p) the probability of a count above zero: log1p(-q) while q < 1/2 -- there logaddexp(log pi,
    log(1 - pi) + p) is the difference of two numbers that may be far larger than the answer -- and that logaddexp beyond,
    with log pi = -logaddexp(0, -f_pi) and log(1 - pi) = -logaddexp(0, f_pi) (log1p(-expit(f)) loses e^f ulps)."""
    from scipy.special import expit
    q = expit(-f_pi) * -np.expm1(p)
    return np.where(q < 0.5, np.log1p(-q), np.logaddexp(-_lae0(-f_pi), -_lae0(f_pi) + p))


def stable64(kind, y, f, classes=None, eps=None):
    """The stable form in float64.  y: (n,), f: (n, ncol) -> (n,)."""
    from scipy.special import gammaln
    y, f = np.asarray(y, dtype=float), np.asarray(f, dtype=float)
    with np.errstate(all='ignore'):
        if kind == 'Poisson':
            return y * f[:, 0] - np.exp(f[:, 0]) - gammaln(y + 1.0)
        if kind == 'NegBin':
            return _negbin64(y, f[:, 0], f[:, 1])
        if kind in ('ZIP', 'ZINB'):
            p = y * f[:, 0] - np.exp(f[:, 0]) - gammaln(y + 1.0) if kind == 'ZIP' else _negbin64(y, f[:, 0], f[:, 1])
            return np.where(y == 0, zero_inflated64(f[:, -1], p), -_lae0(f[:, -1]) + p)
        if kind == 'logit':
            return y * f[:, 0] - _lae0(f[:, 0])
        if kind == 'probit':
            return y * log_ndtr64(f[:, 0]) + (1.0 - y) * log_ndtr64(-f[:, 0])
        yi = y.astype(int)
        if kind == 'robustmax':
            hit = np.argmax(f, axis=1) == yi
            return np.where(hit, np.log1p(-eps), np.log(eps / (classes - 1)))
        top = np.max(f, axis=1)
        return f[np.arange(len(yi)), yi] - (np.log(np.sum(np.exp(f - top[:, None]), axis=1)) + top)


def _negbin_terms(y, f1, f2):
    from scipy.special import gammaln, expit
    size, a = np.exp(-f2), f1 + f2
    return y * np.abs(f2) + y * np.abs(a) + gammaln(y + 1.0) + (y + size) * _lae0(a) + np.abs(a) * (y + size) * expit(a)


@mp.workdps(DPS)
def terms(kind, y, f, classes=None, eps=None, ex=None):
    """T (n,): the sum of the absolute values of the stable form's terms, plus the first-order effect of rounding each
    intermediate combination of latents (a = f1 + f2 is rounded before (y + size) log(1 + e^a) reads it: |a| (y + size) expit(a)).

    Poisson    |y f| + e^f + lgamma(y + 1)
    NegBin     y |log size| + y |a| + lgamma(y + 1) + (y + size) log1p(e^a) + |a| (y + size) expit(a)      (not |lgamma(size)|)
    ZIP        logaddexp(0, f_pi) + lam + |y f_lam| + lgamma(y + 1)
    ZINB       logaddexp(0, f_pi) + T_NegBin
    logit      |y f| + logaddexp(0, f)
    probit     |log ncdf(x)| + |x| npdf(x) / ncdf(x), x = f or -f  (ex: the exact values, rounded; the second term: x / sqrt 2 is
               rounded before erfc reads it, which in the upper tail, where log ncdf(x) = -ncdf(-x), is x^2 ulps of the answer)
    softmax    |f_y| + |top| + log s,  s = sum_k e^(f_k - top)
    robustmax  |value|                                     (ex)
    """
    from scipy.special import gammaln
    y, f = np.asarray(y, dtype=float), np.asarray(f, dtype=float)
    with np.errstate(all='ignore'):
        if kind == 'Poisson':
            return np.abs(y * f[:, 0]) + np.exp(f[:, 0]) + gammaln(y + 1.0)
        if kind == 'NegBin':
            return _negbin_terms(y, f[:, 0], f[:, 1])
        if kind == 'ZIP':
            return _lae0(f[:, 1]) + np.exp(f[:, 0]) + np.abs(y * f[:, 0]) + gammaln(y + 1.0)
        if kind == 'ZINB':
            return _lae0(f[:, 2]) + _negbin_terms(y, f[:, 0], f[:, 1])
        if kind == 'logit':
            return np.abs(y * f[:, 0]) + _lae0(f[:, 0])
        if kind == 'robustmax':
            return np.abs(np.asarray(ex, dtype=float))
        if kind == 'probit':
            x = [_m(v if yy == 1 else -v) for v, yy in zip(f[:, 0], y)]
            slope = [to_float(abs(v) * mp.npdf(v) / (mp.erfc(-v / mp.sqrt(2)) / 2)) if not mp.isnan(v) else math.nan for v in x]
            return np.abs(np.asarray(ex, dtype=float)) + np.asarray(slope)
        top = np.max(f, axis=1)
        fy = f[np.arange(len(y)), y.astype(int)]
        return np.abs(fy) + np.abs(top) + np.log(np.sum(np.exp(f - top[:, None]), axis=1))


def point_bound(kind, T):
    return C[kind] * U * T + TINY


def sum_bound(kind, nobs, sum_T, sum_abs):
    per = -(-nobs // 32)
    return C[kind] * U * sum_T + (-(-per // 256) + 8 + 32) * U * sum_abs


# ------------------------------------------------------------------ input grids
def _ulps(x):
    return [np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)]


def _latin(ncol):
    """Rows over WILD in which every two columns meet in every pairing: all 121 pairs of the first two, a third column
    WILD[(i + 2 j) mod 11] (a Latin square: it meets each of the other two in every pairing as well)."""
    rows = []
    for i, a in enumerate(WILD):
        for j, b in enumerate(WILD):
            rows.append([a, b, WILD[(i + 2 * j) % 11]][:ncol])
    return rows


@functools.lru_cache(maxsize=None)
def latent_grid(kind):
    """(R, ncol) latent rows of one count / two-class kind, R a multiple of 64 (one call takes 64 candidate blocks):
    the wild values in every pairing the kind has columns for, the switch points with their neighbouring doubles, and ordinary
    values in [-3, 3] filling up."""
    ncol = NCOL[kind]
    rng = np.random.default_rng(sum(map(ord, kind)))
    rows = [[v] for v in WILD] if ncol == 1 else _latin(ncol)
    if kind in ('NegBin', 'ZINB'):   # a = f1 + f2 = 0 (lik_logaddexp's a == b branch) and its neighbours
        for f1 in _ulps(1.25) + _ulps(-2.5):
            rows.append([f1, -np.sign(f1) * abs(round(f1, 2)), 0.3][:ncol])
        rows += [[0.0, 0.0, 0.0][:ncol], [4.5, -37.0, -1.0][:ncol], [4.0, -15.0, 2.0][:ncol]]
    if kind in ('logit', 'Poisson'):
        rows += [[v] for v in _ulps(0.0) + [2.0 ** -52, -2.0 ** -52]]
    if kind == 'probit':
        for s in (-20.0, 0.0, PROBIT_SWITCH, -PROBIT_SWITCH, 20.0):
            rows += [[v] for v in _ulps(s)]
        rows += [[-20.0 - 1e-7], [20.0 + 1e-7], [-25.0], [25.0], [-34.0], [-36.0]]
    if kind in ('ZIP', 'ZINB'):      # (the table of the issue)
        rows += [[1.0, 30.0], [1.0, 36.0], [1.0, 37.0]] if kind == 'ZIP' else [[1.0, -1.0, 30.0], [1.0, -1.0, 37.0]]
    R = -(-len(rows) // 64) * 64
    F = np.concatenate((np.asarray(rows, dtype=float), rng.uniform(-3.0, 3.0, size=(R - len(rows), ncol))))
    return F


def point_ys(kind):
    return COUNTS if kind in ('Poisson', 'NegBin', 'ZIP', 'ZINB') else (0.0, 1.0)


@functools.lru_cache(maxsize=None)
def point_reference(kind, y):
    """(F, ex, lo, T) of one count / two-class kind at observation y: the grid, exact = ex + lo per row (ex the nearest
    double), T per row."""
    F = latent_grid(kind)
    ex, lo = np.array([split(exact(kind, y, row)) for row in F]).T
    return F, ex, lo, terms(kind, np.full(len(F), y), F, ex=ex)


SPREADS = (0.0, 1.0, 700.0, 1500.0)


@functools.lru_cache(maxsize=None)
def class_grid(kind, K):
    """(64, K) latent rows of a K-class softmax / robustmax node."""
    rng = np.random.default_rng(1000 + K + (kind == 'softmax'))
    rows = []
    if kind == 'softmax':   # the top column first, last, in the middle; the rest `spread` below it; around 0 and far from it
        for spread in SPREADS:
            for pos in (0, K - 1, K // 2):
                for base in (0.0, -800.0, 1000.0):
                    r = np.full(K, base) + rng.uniform(-0.5, 0.5, size=K) * (spread > 0)
                    r[pos] = base + spread + (0.5 if spread > 0 else 0.0)
                    rows.append(r)
        rows += [np.full(K, v) for v in (0.0, -40.0, 37.0)]
    else:
        for pos in (0, K - 1, K // 2):
            r = rng.uniform(-3, 3, size=K)
            r[pos] = 5.0
            rows.append(r.copy())                    # a single maximum
            r[(pos + 1) % K] = 5.0
            rows.append(r.copy())                    # tied maxima: the first index wins
            r[:] = 5.0
            rows.append(r.copy())                    # all tied
        rows += [np.full(K, v) for v in (0.0, -40.0)]
        r = rng.uniform(-3, 3, size=K)
        rows.append(np.sort(r))                                          # increasing: the last wins
        rows.append(np.sort(r)[::-1].copy())                             # decreasing: the first wins
        r = np.zeros(K)
        r[K - 1] = np.nextafter(0.0, 1.0)                               # a maximum by one subnormal
        rows.append(r)
    F = np.concatenate((np.asarray(rows), rng.uniform(-3.0, 3.0, size=(64 - len(rows), K))))
    assert F.shape == (64, K)
    return F


def class_ys(K):
    return sorted({0, K - 1, K // 2})


@functools.lru_cache(maxsize=None)
def class_reference(kind, K, y):
    F = class_grid(kind, K)
    ex, lo = np.array([split(exact(kind, y, row, classes=K, eps=EPS)) for row in F]).T
    return F, ex, lo, terms(kind, np.full(64, float(y)), F, classes=K, eps=EPS, ex=ex)


def nan_class_rows(K):
    """Robustmax rows with NaN latents and the class the first-NaN rule elects: (F (4, K), winners)."""
    F = np.tile(np.linspace(-1.0, 1.0, K), (4, 1))
    F[0, K - 1] = np.nan                      # a NaN in the last column, behind the maximum so far
    F[1, 0] = np.nan                          # in the first column
    F[2, K // 2] = F[2, K - 1] = np.nan       # two: the first wins
    F[3, 0] = 9.0
    F[3, K - 1] = np.nan                      # behind a larger value
    return F, [K - 1, 0, K // 2, K - 1]


# Inputs at which the definition is not a finite double: (kind, y, latent row, class of the result)
NONFINITE = [
    ('Poisson', 2.0, [710.0], '-inf'),            # e^710 overflows
    ('Poisson', 2.0, [np.nan], 'nan'),
    ('NegBin', 2.0, [np.nan, 0.5], 'nan'),
    ('NegBin', 100.0, [0.5, np.nan], 'nan'),
    ('ZIP', 0.0, [0.5, np.nan], 'nan'),
    ('ZIP', 3.0, [np.nan, 0.5], 'nan'),
    ('ZIP', 3.0, [710.0, 0.5], '-inf'),
    ('ZINB', 0.0, [0.5, 0.5, np.nan], 'nan'),
    ('ZINB', 70.0, [0.5, np.nan, 0.5], 'nan'),
    ('logit', 1.0, [np.nan], 'nan'),
    ('probit', 1.0, [np.nan], 'nan'),
    ('probit', 0.0, [np.nan], 'nan'),
]


def same_class(v, cls):
    return bool(np.isnan(v)) if cls == 'nan' else bool(v == -np.inf)


# ------------------------------------------------------------------ sum geometry: 300 pairs, tiled
SUM_Y = (0.0, 1.0, 2.0, 3.0, 5.0, 17.0, 63.0, 64.0, 65.0, 100.0)
SUM_NOBS = (1, 2, 31, 32, 33, 255 * 32 + 1, 8192, 8193, 20000)
SUM_N = 300                      # latent rows of a block under a replicate map


@functools.lru_cache(maxsize=None)
def sum_reference(kind):
    """30 latent rows x the 10 counts of SUM_Y: the 300 distinct (y, latent row) pairs every sum test is tiled from.
    Returns (L (30, ncol), hi (10, 30), lo (10, 30), T (10, 30)): exact = hi + lo."""
    ncol = NCOL[kind]
    rng = np.random.default_rng(77 + ncol)
    L = rng.uniform(-3.0, 3.0, size=(30, ncol))
    L[:6] = rng.uniform(-12.0, 6.0, size=(6, ncol))       # some far from ordinary (size up to e^12, rates down to e^-12)
    hi, lo, T = np.empty((10, 30)), np.empty((10, 30)), np.empty((10, 30))
    for v, y in enumerate(SUM_Y):
        for l in range(30):
            hi[v, l], lo[v, l] = split(exact(kind, y, L[l]))
        T[v] = terms(kind, np.full(30, y), L)
    return L, hi, lo, T


def sum_case(kind, nobs, B, mapped=True):
    """Inputs of one summed call and its reference.  Under a replicate map: SUM_N latent rows per block, observation i reads
    row rep[i] = (131 i + 7) mod 300 (a permutation of the rows with repeats from i = 300 on, not monotone).  Without: nobs rows.
    Block b holds row r -> L[(7 r + 11 b + (r // 30) b) mod 30]: different latents per block.  y_i = SUM_Y[(3 i + i // 10) mod 10].
    Returns dict(FP (B, n, ncol), y, rep or None, want (B,), bound (B,))."""
    L, hi, lo, T = sum_reference(kind)
    n = SUM_N if mapped else nobs
    i = np.arange(nobs)
    rep = (131 * i + 7) % n if mapped else None
    yv = (3 * i + i // 10) % 10
    r = np.arange(n)
    want, bound = np.empty(B), np.empty(B)
    FP = np.empty((B, n, L.shape[1]))
    for b in range(B):
        lb = (7 * r + 11 * b + (r // 30) * b) % 30
        FP[b] = L[lb]
        l = lb[rep] if mapped else lb
        want[b] = math.fsum(np.concatenate((hi[yv, l], lo[yv, l])))
        bound[b] = sum_bound(kind, nobs, math.fsum(T[yv, l]), math.fsum(np.abs(hi[yv, l])))
    return dict(FP=FP, y=np.asarray(SUM_Y)[yv], rep=rep, want=want, bound=bound)
