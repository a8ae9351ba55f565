"""Reference for the predictive-mixture kernels (csrc/mixture.hip, DESIGN I.15): the equal-weight mixture of S Gaussians in
mpmath at 50 digits, and the error bounds the device results are held to.

One entry is (mu, var): two sequences of S doubles, taken exactly.  A component with var <= 0 is a point mass at mu.

Bounds.  eps = 2^-53, C = 8 (the project's constant, DESIGN I.12 / I.13), z_s = (y - mu_s) / sigma_s.
  cdf, sf    C eps (1/S) sum_s [tail(z_s) + phi(z_s) (|y| + |mu_s|) / sigma_s]  +  (S - 1) eps (1/S) sum_s tail(z_s)
             -- a relative error on each component's tail, and the rounding of z_s carried through the density; the last term is
             the recursive sum of the S tails itself, (n - 1) eps sum |terms| for n terms in a fixed order (Higham, Accuracy and
             Stability of Numerical Algorithms, eq. 4.4), which C cannot hold for every S: at S = 200 the first two terms alone
             were met to 0.35 on the device, at S <= 7 to 0.21.  A point mass counts with its step, 0 or 1, as its tail: the
             step is exact, the mean of the steps is rounded.  Plus 2^-1022, the absolute floor where a tail leaves the normal
             range of a double.
  logpdf     the same two terms for the density d_s = phi(z_s) / sigma_s, i.e. d_s [1 + |z_s| (|y| + |mu_s|) / sigma_s], divided by
             the mixture density f; two rounding terms of the log-sum-exp form are added, which the two terms do not hold:
             d_s |log(sigma_s sqrt 2)| (the component's log-normaliser, -log(sigma_s sqrt 2), is itself rounded: eps |log| absolute in the
             exponent, so relative in d_s), and 1 + |log f| (the final log of the sum and the additions that assemble the result);
             and (S - 1) eps for the recursive sum of the S exponentials, as for the cdf.
  crps       C eps [(1/S) sum_s B(y - mu_s, var_s) + (1/2S^2) sum_s sum_t B(mu_s - mu_t, var_s + var_t)],
             B(m, v) = |A(m, v)| + |m| |2 Phi(m / sqrt v) - 1|: A's value and the rounding of its argument m (dA/dm = 2 Phi - 1);
             plus the two recursive sums, (n - 1) eps sum |A| with n = S terms in the first and n = S (S + 1) / 2 in the second
             (the device sums the pairs s < t and the diagonal; met to 0.33 at S = 65 without this term, to 0.14 at S <= 7).
  quantile   a backward error: with delta = 4 eps max(|q|, max_s |mu_s|) and B the cdf bound at q,
             F(q - delta) - B <= p <= F(q + delta) + B; where f(q) max_s sigma_s >= 1e-3 also the forward error
             |q - q*| <= delta + B / f(q), checked as F(q - D) <= p <= F(q + D), D = delta + B / f(q) (F is monotone: the
             same statement), and against q* from bisection where a test asks for it.
"""
import math

import mpmath as mp
import numpy as np

mp.mp.dps = 50
EPS = 2.0 ** -53
C = 8.0
TINY = 2.0 ** -1022      # below the normal range a double has no relative precision: the absolute floor of every bound
_SQRT2 = mp.sqrt(2)
_HALF = mp.mpf(1) / 2


def _comps(mu, var):
    return [(mp.mpf(float(m)), mp.mpf(float(v))) for m, v in zip(mu, var)]


def _tail(m, v, y, upper):
    """P(N(m, v) <= y), or > y."""
    if v <= 0:
        below = y >= m
        return mp.mpf(1 if below != upper else 0)
    x = (y - m) / mp.sqrt(2 * v)
    return _HALF * mp.erfc(x if upper else -x)


def cdf(mu, var, y, upper=False):
    y = mp.mpf(float(y))
    c = _comps(mu, var)
    return mp.fsum(_tail(m, v, y, upper) for m, v in c) / len(c)


def sf(mu, var, y):
    return cdf(mu, var, y, upper=True)


def pdf(mu, var, y):
    y = mp.mpf(float(y))
    c = _comps(mu, var)
    return mp.fsum(mp.npdf(y, m, mp.sqrt(v)) for m, v in c if v > 0) / len(c)


def logpdf(mu, var, y):
    f = pdf(mu, var, y)
    return mp.log(f) if f > 0 else mp.mpf('-inf')


def A(m, v):
    """E|N(m, v)| = 2 sqrt(v) phi(m / sqrt v) + m (2 Phi(m / sqrt v) - 1); A(m, 0) = |m|."""
    if v <= 0:
        return abs(m)
    sd = mp.sqrt(v)
    return 2 * sd * mp.npdf(m / sd) + m * mp.erf(m / (sd * _SQRT2))


def _A_and_B(m, v):
    """A(m, v) and B(m, v) = |A| + |m| |2 Phi - 1|, the magnitude its error bound is made of."""
    if v <= 0:
        return abs(m), 2 * abs(m)
    sd = mp.sqrt(v)
    odd = m * mp.erf(m / (sd * _SQRT2))       # (>= 0: erf has the sign of m)
    a = 2 * sd * mp.npdf(m / sd) + odd
    return a, a + odd


def crps_and_bound(mu, var, y, c=C):
    """(CRPS, its error bound), the pair sum over s < t doubled plus the diagonal: S (S + 1) / 2 terms."""
    y = mp.mpf(float(y))
    cs = _comps(mu, var)
    S = len(cs)
    first = [_A_and_B(y - m, v) for m, v in cs]
    diag = [_A_and_B(mp.mpf(0), 2 * v) for m, v in cs]
    off = [_A_and_B(cs[s][0] - cs[t][0], cs[s][1] + cs[t][1]) for s in range(S) for t in range(s + 1, S)]
    value = mp.fsum(a for a, _ in first) / S - (mp.fsum(a for a, _ in diag) + 2 * mp.fsum(a for a, _ in off)) / (2 * S * S)
    bound = mp.fsum(b for _, b in first) / S + (mp.fsum(b for _, b in diag) + 2 * mp.fsum(b for _, b in off)) / (2 * S * S)
    sums = (S - 1) * mp.fsum(a for a, _ in first) / S + \
        (S * (S + 1) // 2 - 1) * (mp.fsum(a for a, _ in diag) + 2 * mp.fsum(a for a, _ in off)) / (2 * S * S)
    return value, float(EPS * (c * bound + sums))


def crps(mu, var, y):
    return crps_and_bound(mu, var, y)[0]


def quantile(mu, var, p, lo=None, hi=None, width=None):
    """inf{q : F(q) >= p} by bisection on the exact cdf, from [lo, hi] (default: the components' own p-quantiles, which
    bracket it) down to `width` (default 1e-30 of the scale)."""
    p = mp.mpf(float(p))
    c = _comps(mu, var)
    if lo is None:
        zp = _SQRT2 * mp.erfinv(2 * p - 1)
        ends = [m + zp * mp.sqrt(max(v, 0)) for m, v in c]
        lo, hi = min(ends), max(ends)
    lo, hi = mp.mpf(lo), mp.mpf(hi)
    F = lambda q: mp.fsum(_tail(m, v, q, False) for m, v in c) / len(c)
    if F(lo) >= p:
        return lo
    if width is None:
        width = mp.mpf(10) ** -30 * max(abs(lo), abs(hi), 1)
    while hi - lo > width:
        mid = (lo + hi) / 2
        if F(mid) >= p:
            hi = mid
        else:
            lo = mid
    return hi


# ------------------------------------------------------------------------------------------------------------------------- bounds
def _phi(z):
    return math.exp(-0.5 * z * z) / math.sqrt(2 * math.pi) if abs(z) < 38.5 else 0.0


def cdf_bound(mu, var, y, upper=False, c=C):
    y = float(y)
    tot = tail = 0.0
    for m, v in zip(mu, var):
        m, v = float(m), float(v)
        if v <= 0:
            tail += 1.0 if (y >= m) != upper else 0.0
            continue
        sd = math.sqrt(v)
        z = (y - m) / sd
        tail += 0.5 * math.erfc(z / math.sqrt(2) if upper else -z / math.sqrt(2))
        tot += _phi(z) * (abs(y) + abs(m)) / sd
    return EPS * ((c + len(mu) - 1) * tail + c * tot) / len(mu) + TINY


def logpdf_bound(mu, var, y, c=C):
    y = float(y)
    tot = 0.0
    for m, v in zip(mu, var):
        m, v = float(m), float(v)
        if v <= 0:
            continue
        sd = math.sqrt(v)
        z = (y - m) / sd
        tot += mp.npdf(z) / sd * (1 + abs(z) * (abs(y) + abs(m)) / sd + abs(math.log(sd * math.sqrt(2))))
    f = pdf(mu, var, y)
    if f == 0:
        return float('inf')
    return float(c * EPS * (tot / len(mu) / f + 1 + abs(mp.log(f))) + (len(mu) - 1) * EPS)


def crps_bound(mu, var, y, c=C):
    return crps_and_bound(mu, var, y, c)[1]


def quantile_delta(mu, q):
    return 4 * EPS * max(abs(float(q)), max(abs(float(m)) for m in mu))


def quantile_check(mu, var, p, q, c=C):
    """The quantile statement for one device result q.  Returns (ok, worst ratio, text): ratio is how far p lies outside
    [F(q - delta), F(q + delta)] in units of the cdf bound B (<= 1 passes), and where the density allows it how far outside
    [F(q - D), F(q + D)], D = delta + B / f(q)."""
    q = float(q)
    qm = mp.mpf(q)
    pm = mp.mpf(float(p))
    delta = mp.mpf(quantile_delta(mu, q))
    Bq = mp.mpf(cdf_bound(mu, var, q, c=c))
    lo, hi = _exact_cdf(mu, var, qm - delta), _exact_cdf(mu, var, qm + delta)
    excess = max(lo - pm, pm - hi, 0)
    ratio = 0.0 if excess <= 0 else float(excess / Bq) if Bq > 0 else float('inf')
    text = 'backward: F(q-d)=%s p=%s F(q+d)=%s B=%s' % (mp.nstr(lo, 20), mp.nstr(pm, 20), mp.nstr(hi, 20), mp.nstr(Bq, 5))
    ok = ratio <= 1.0
    f = _exact_pdf(mu, var, qm)
    smax = math.sqrt(max(max(float(v) for v in var), 0.0))
    if f * smax >= 1e-3:
        D = delta + Bq / f
        lo2, hi2 = _exact_cdf(mu, var, qm - D), _exact_cdf(mu, var, qm + D)
        fwd = lo2 <= pm <= hi2
        text += '; forward: F(q-D)=%s F(q+D)=%s D=%s' % (mp.nstr(lo2, 20), mp.nstr(hi2, 20), mp.nstr(D, 5))
        ok = ok and fwd
    return ok, ratio, text


def _exact_cdf(mu, var, y):
    """cdf at an mpmath argument (cdf() takes doubles)."""
    c = _comps(mu, var)
    return mp.fsum(_tail(m, v, y, False) for m, v in c) / len(c)


def _exact_pdf(mu, var, y):
    c = _comps(mu, var)
    return mp.fsum(mp.npdf(y, m, mp.sqrt(v)) for m, v in c if v > 0) / len(c)


# ------------------------------------------------------------------------------------------------------------ numpy formulas
def np_cdf(mu, var, y):
    """The mixture cdf by scipy on (S, ...) arrays (the model tests' comparison; var > 0)."""
    from scipy.special import ndtr
    return ndtr((y - mu) / np.sqrt(var)).mean(0)


def np_crps(mu, var, y):
    from scipy.special import erf

    def An(m, v):
        sd = np.sqrt(v)
        return 2 * sd * np.exp(-0.5 * (m / sd) ** 2) / np.sqrt(2 * np.pi) + m * erf(m / (sd * np.sqrt(2)))
    S = mu.shape[0]
    first = An(y - mu, var).mean(0)
    second = sum(An(mu[s] - mu[t], var[s] + var[t]) for s in range(S) for t in range(S)) / (2 * S * S)
    return first - second
