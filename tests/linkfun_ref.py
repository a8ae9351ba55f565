"""Reference for the Matern-2.5 linked-GP factors of csrc/linkfun.hpp: I = E[k(x, Z)] and J = E[k(x1, Z) k(x2, Z)], Z ~ N(m, v),
k(d) = (1 + sqrt5 |d|/l + 5 d^2 / (3 l^2)) exp(-sqrt5 |d|/l).

Three things live here.

* exact_I / exact_J (mpmath): the closed form of the integral, region by region (z below both points, between them, above
  both).  In a region the integrand is a quartic in z times exp(alpha z) N(z; m, v) = exp(..) N(z; m + alpha v, v), and the
  truncated moments of a normal follow from the zeroth one by the usual recurrence.  Every tail probability is an erfc of a
  positive argument -- never 1 + erf, which needs ~4.3 v/l^2 decimal digits to hold one -- and DPS digits are carried.
  tests/test_linkfun_host.py checks it against mpmath.quad of the defining integral.

* cases(): the deterministic case set, built by index (no random numbers): for 21 values of v/l^2 (the decades 1e-12 .. 1e3 and
  4, 25, 100, 400, 1600), l in {0.05, 1, 3}, m in {0, 1.5, -40}, 21 pairs of points with (x - m)/l drawn from
  {0, +-1e-8, +-0.01, +-0.5, +-2, +-10, +-60} -- equal points, points 1e-7 lengthscales apart, a point on m -- plus the
  structured edges v == 0, v = 1e-300 and a point 1e5 lengthscales away.  `python -m tests.linkfun_ref` evaluates the exact
  values on it, rounds them to double and writes tests/golden/linkfun_exact.npz (and the second fixture of the end-to-end
  tests, tests/golden/linkfun_e2e.npz), so that the GPU tests need no mpmath.

* fixed_*: a float64 numpy restatement, operation for operation, of the algorithm of csrc/linkfun.hpp (scipy's erfc / erfcx
  for the device's).  Its largest relative error against the exact values per v/l^2 bucket, over every function and case
  with exact >= 1e-280, is E_b; the GPU tests allow the device 32 E_b.  Measured on the full set (stored in the fixture as
  `E_b`; test_linkfun_host.py recomputes them and holds them to the caps of BUCKET_CAPS):

      v/l^2     <= 0.1    <= 4      <= 25     <= 100    <= 400    <= 1600
      I         3.7e-14   2.9e-14   2.7e-14   3.9e-15   1.0e-15   5.6e-16
      Jd        9.8e-14   4.9e-12   3.2e-08   3.2e-07   5.8e-09   6.7e-07
      Jd0       8.1e-14   5.9e-14   4.9e-14   3.8e-15   1.1e-15   9.3e-16
      Jsep      6.8e-14   9.3e-13   1.8e-09   3.1e-08   3.6e-08   1.3e-06
      Jsep0     6.8e-14   8.1e-13   2.1e-09   3.0e-08   2.0e-08   8.0e-07
      E_b       9.8e-14   4.9e-12   3.2e-08   3.2e-07   3.6e-08   1.3e-06     (caps 1e-12 1e-10 1e-7 1e-5 1e-4 1e-2)

  What is left above 1e-13 is the region BETWEEN two points that lie within 1e-7 lengthscales of each other far out in a tail: the
  reference's moment polynomials survive there (in normalised coordinates) and cancel like x^4.  The tails themselves are sums
  of positive terms.
"""
import os

import numpy as np

SQ5 = np.sqrt(5.0)
DPS = 120
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FIXTURE = os.path.join(GOLDEN, 'linkfun_exact.npz')
FIXTURE_E2E = os.path.join(GOLDEN, 'linkfun_e2e.npz')

RATIOS = [10.0 ** e for e in range(-12, 4)] + [4.0, 25.0, 100.0, 400.0, 1600.0]
LENGTHS = [0.05, 1.0, 3.0]
MEANS = [0.0, 1.5, -40.0]
UNITS = [0.0, 1e-8, -1e-8, 0.01, -0.01, 0.5, -0.5, 2.0, -2.0, 10.0, -10.0, 60.0, -60.0]
BUCKET_EDGES = [0.1, 4.0, 25.0, 100.0, 400.0, 1600.0]          # a case's bucket: the first edge with v/l^2 <= edge
BUCKET_CAPS = [1e-12, 1e-10, 1e-7, 1e-5, 1e-4, 1e-2]
TINY = 1e-280                                                   # exact values below it are held to |got| <= 1e-279
FNS = ('i', 'jd', 'jd0', 'jsep', 'jsep0')                       # Engine.LINKFN's factor names, fixture key 'exact_' + ...


# ------------------------------------------------------------------------------------------------ the case set
def cases():
    """(args (N, 5) = X1, X2, m, v, l ; ratio (N,) = the nominal v/l^2 of each case (0 for v == 0))."""
    rows, ratio = [], []
    nu = len(UNITS)
    c = 0
    for R in RATIOS:
        for l in LENGTHS:
            for m in MEANS:
                v = R * l * l
                pairs = [(UNITS[((c + 9 * p) % (nu * nu)) // nu], UNITS[((c + 9 * p) % (nu * nu)) % nu]) for p in range(17)]
                u = UNITS[c % nu]
                pairs += [(u, u), (u, u + 1e-7), (u - 1e-7, u), (0.0, UNITS[(c // nu) % nu])]
                for (u1, u2) in pairs:
                    rows.append((m + u1 * l, m + u2 * l, m, v, l))
                    ratio.append(R)
                c += 1
    for l in LENGTHS:
        for m in MEANS:
            for (u1, u2) in ((0.0, 0.0), (0.5, -2.0), (-10.0, -10.0), (2.0, 60.0)):
                rows.append((m + u1 * l, m + u2 * l, m, 0.0, l))            # the matern_point branch
                ratio.append(0.0)
                rows.append((m + u1 * l, m + u2 * l, m, 1e-300, l))
                ratio.append(1e-300 / (l * l))
            for R in (1e-8, 1.0, 100.0):
                for (u1, u2) in ((1e5, 1e5), (-1e5, 0.5), (1e5, -1e5), (2.0, 1e5)):
                    rows.append((m + u1 * l, m + u2 * l, m, R * l * l, l))    # exact value 0 or denormal
                    ratio.append(R)
    return np.array(rows, dtype=np.float64), np.array(ratio, dtype=np.float64)


def bucket_of(ratio):
    return np.searchsorted(np.array(BUCKET_EDGES), np.asarray(ratio), side='left')


# ------------------------------------------------------------------------------------------------ exact values (mpmath)
def _mp():
    import mpmath
    return mpmath


def _polymul(p, q):
    mp = _mp()
    r = [mp.mpf(0)] * (len(p) + len(q) - 1)
    for i, a in enumerate(p):
        for j, b in enumerate(q):
            r[i + j] += a * b
    return r


def _truncated_moments(lo, hi, mu, w, nmax):
    """int_lo^hi z^n N(z; mu, w) dz, n = 0 .. nmax (lo / hi may be None for -inf / +inf); every tail through erfc of an argument >= 0."""
    mp = _mp()
    s2 = mp.sqrt(2 * w)
    phi = lambda z: mp.exp(-(z - mu) ** 2 / (2 * w)) / mp.sqrt(2 * mp.pi * w)
    if lo is None and hi is None:
        m0 = mp.mpf(1)
    elif lo is None:
        t = (hi - mu) / s2
        m0 = mp.erfc(-t) / 2 if t <= 0 else 1 - mp.erfc(t) / 2
    elif hi is None:
        t = (lo - mu) / s2
        m0 = mp.erfc(t) / 2 if t >= 0 else 1 - mp.erfc(-t) / 2
    else:
        ta, tb = (lo - mu) / s2, (hi - mu) / s2
        if ta >= 0:
            m0 = (mp.erfc(ta) - mp.erfc(tb)) / 2
        elif tb <= 0:
            m0 = (mp.erfc(-tb) - mp.erfc(-ta)) / 2
        else:
            m0 = 1 - (mp.erfc(-ta) + mp.erfc(tb)) / 2
    edge = lambda n: (0 if hi is None else hi ** n * phi(hi)) - (0 if lo is None else lo ** n * phi(lo))
    M = [m0, mu * m0 - w * edge(0)]
    for n in range(1, nmax):
        M.append(mu * M[n] + n * w * M[n - 1] - w * edge(n))
    return M[:nmax + 1]


def _expect(points, w):
    """E[prod_i k(p_i - Z)], Z ~ N(0, w), unit lengthscale; points: one or two mpf."""
    mp = _mp()
    s5 = mp.sqrt(5)
    pts = sorted(points)
    bounds = [None] + pts + [None]
    total = mp.mpf(0)
    for r in range(len(pts) + 1):
        lo, hi = bounds[r], bounds[r + 1]
        if lo is not None and hi is not None and lo == hi:
            continue
        poly, alpha, beta = [mp.mpf(1)], mp.mpf(0), mp.mpf(0)
        for i, p in enumerate(pts):
            s = -1 if i < r else 1                        # |p - z| = s (p - z): the points below this region have z > p
            # 1 + sqrt5 s (p - z) + 5/3 (p - z)^2 in powers of z
            poly = _polymul(poly, [1 + s5 * s * p + mp.mpf(5) / 3 * p * p, -s5 * s - mp.mpf(10) / 3 * p, mp.mpf(5) / 3])
            alpha += s5 * s
            beta -= s5 * s * p
        M = _truncated_moments(lo, hi, alpha * w, w, len(poly) - 1)
        total += mp.exp(beta + alpha * alpha * w / 2) * sum(c * mk for c, mk in zip(poly, M))
    return total


def _kpoint(d):
    mp = _mp()
    a = abs(d) * mp.sqrt(5)
    return (1 + a + a * a / 3) * mp.exp(-a)


def _normalised(xs, m, v, l):
    mp = _mp()
    m, v, l = mp.mpf(float(m)), mp.mpf(float(v)), mp.mpf(float(l))
    return [(mp.mpf(float(x)) - m) / l for x in xs], v / (l * l)


def exact_I(x, m, v, l):
    mp = _mp()
    with mp.workdps(DPS):
        (p,), w = _normalised([x], m, v, l)
        return +(_kpoint(p) if w == 0 else _expect([p], w))


def exact_J(x1, x2, m, v, l):
    mp = _mp()
    with mp.workdps(DPS):
        (p, q), w = _normalised([x1, x2], m, v, l)
        return +(_kpoint(p) * _kpoint(q) if w == 0 else _expect([p, q], w))


def quad_J(x1, x2, m, v, l, scale=1, dps=50):
    """The defining integral over `scale` by mpmath.quad, split at the points, at m and a few standard deviations around it
    (quad stops on an absolute error estimate: a caller after a relative error passes the value it expects as `scale`)."""
    mp = _mp()
    with mp.workdps(dps):
        x1, x2, m, v, l = (mp.mpf(float(t)) for t in (x1, x2, m, v, l))
        sd = mp.sqrt(v)
        k = lambda d: (1 + mp.sqrt(5) * abs(d) / l + 5 * d * d / (3 * l * l)) * mp.exp(-mp.sqrt(5) * abs(d) / l)
        f = lambda z: k(x1 - z) * k(x2 - z) * mp.exp(-(z - m) ** 2 / (2 * v)) / (mp.sqrt(2 * mp.pi * v) * scale)
        # where the integrand peaks: the Gaussian shifted by the exponentials' slopes (m, m +- 2 sqrt5 v / l), and the points
        cuts = {x1, x2, m}
        for c in (m, m - 2 * mp.sqrt(5) * v / l, m + 2 * mp.sqrt(5) * v / l, x1, x2):
            for s in (-40, -12, -4, 4, 12, 40):
                cuts.add(c + s * sd)
                cuts.add(c + s * l / 4)
        cuts = [-mp.inf] + sorted(cuts) + [mp.inf]
        return mp.quad(f, cuts, maxdegree=10)


def to_double(x):
    return float(x)


def to_longdouble(x):
    """An mpf as numpy.longdouble: the leading double plus the double of the remainder (mathfn_ref.mp_to_ld's way)."""
    hi = float(x)
    if hi == 0.0 or not np.isfinite(hi):
        return np.longdouble(hi)
    return np.longdouble(hi) + np.longdouble(float(x - _mp().mpf(hi)))


# ------------------------------------------------------------------------------------------------ the fixed algorithm in float64
def _special():
    from scipy.special import erfc, erfcx
    return erfc, erfcx


def _kp(d):
    a = np.abs(d)
    return (1.0 + SQ5 * a + 5.0 * d * d / 3.0) * np.exp(-SQ5 * a)


MILLER_N = 48          # backward-recurrence start of tail_moments
T_FORWARD = 2.5        # below it the forward recurrence loses < 3e-13
B0, B1, B2 = 1.0, SQ5, 5.0 / 3.0
RSQPI = 1.0 / np.sqrt(np.pi)


def tail_moments(X, w, s2):
    """H_k = s2^k g_k(t), k = 0 .. 4, g_k(t) = int_0^inf u^k exp(-u^2 - 2 t u) du, t = X / s2 -- the moments of the Gaussian tail
    beyond a point X / w standard units out -- for t > 0, and exp(-t^2) H_k for t <= 0 (the caller folds exp(t^2) into its
    prefactor's exponent, which it leaves non-positive).  Returns (H, t > 0).

    t <= 0: H_0 = sqrt(pi)/2 erfc(t), H_1 = s2 exp(-t^2)/2 - X H_0, H_{k+1} = k w H_{k-1} - X H_k: every term is positive.
    0 < t < 2.5: the same forward recurrence from erfcx; it loses (2t)^2k / k! and stays below 3e-13.
    t >= 2.5: the g_k are the minimal solution, so the recurrence runs backwards from k = 48 (Miller), in the scaled unknowns
    y_k = g_k (2t)^k / k!: y_{k-1} = y_k + 2 (k + 1) y_{k+1} / (2t)^2, positive terms again, normalised by H_0."""
    erfc, erfcx = _special()
    t = X / s2
    fold = t > 0.0
    with np.errstate(all='ignore'):
        tp = np.where(fold, t, 0.0)
        H0 = 0.5 * np.sqrt(np.pi) * np.where(fold, erfcx(tp), erfc(np.where(fold, 0.0, t)))
        H = [H0, 0.5 * s2 * np.where(fold, 1.0, np.exp(-t * t)) - X * H0]
        for k in range(1, 4):
            H.append(k * w * H[k - 1] - X * H[k])
        tm = np.where(t >= T_FORWARD, t, T_FORWARD)
        u = 0.5 / tm
        u2 = u * u
        y = [None] * (MILLER_N + 2)
        y[MILLER_N + 1], y[MILLER_N] = np.zeros_like(t), np.ones_like(t)
        for k in range(MILLER_N, 0, -1):
            y[k - 1] = y[k] + (2.0 * (k + 1)) * u2 * y[k + 1]
        r = w / np.where(t >= T_FORWARD, X, 1.0)           # s2 / (2t)
        c = H0 / y[0]
        M = [H0]
        for k, f in ((1, 1.0), (2, 2.0), (3, 6.0), (4, 24.0)):
            c = c * r
            M.append(f * c * y[k])
    return [np.where(t >= T_FORWARD, M[k], H[k]) for k in range(5)], fold


def _polyB(a0, a1, a2):
    """(a0 + a1 s + a2 s^2)(1 + sqrt5 s + 5/3 s^2) by powers of s."""
    return (a0, a0 * B1 + a1, a0 * B2 + a1 * B1 + a2, a1 * B2 + a2 * B1, a2 * B2)


def _dot5(q, H):
    return q[0] * H[0] + q[1] * H[1] + q[2] * H[2] + q[3] * H[3] + q[4] * H[4]


def _tail_I(x, w, s2):
    """int over z beyond x of k(x - z) N(z; 0, w): z = x + s, the integrand is (1 + sqrt5 s + 5/3 s^2) exp(-x^2/2w - s (sqrt5 + x/w) - s^2/2w)."""
    H, fold = tail_moments(x + SQ5 * w, w, s2)
    with np.errstate(all='ignore'):
        e = np.exp(np.where(fold, -0.5 * x * x / w, SQ5 * x + 2.5 * w))
    return e * RSQPI * (B0 * H[0] + B1 * H[1] + B2 * H[2])


def fixed_I(x, m, v, l):
    x, m, v, l = (np.asarray(t, dtype=np.float64) for t in (x, m, v, l))
    d = (x - m) / l
    w = np.where(v == 0.0, 1.0, v / (l * l))
    s2 = np.sqrt(2.0 * w)
    return np.where(v == 0.0, _kp(d), _tail_I(d, w, s2) + _tail_I(-d, w, s2))


def _tail_J(dl, x, w, s2):
    """int over z beyond both points of k k N: x the point next to the region (mirrored for the region below), dl >= 0 the other
    one's distance from it; z = x + s, integrand (1 + sqrt5 (s + dl) + 5/3 (s + dl)^2)(1 + sqrt5 s + 5/3 s^2) times
    exp(-sqrt5 dl - x^2/2w - s (2 sqrt5 + x/w) - s^2/2w): a sum of positive terms."""
    H, fold = tail_moments(x + 2.0 * SQ5 * w, w, s2)
    q = _polyB(1.0 + dl * (SQ5 + B2 * dl), SQ5 + 2.0 * B2 * dl, B2)
    with np.errstate(all='ignore'):
        e = np.exp(-SQ5 * dl + np.where(fold, -0.5 * x * x / w, 2.0 * SQ5 * x + 10.0 * w))
    return e * RSQPI * _dot5(q, H)


def _P1(x1, x2, w, sv, s2):
    return _tail_J(x2 - x1, x2, w, s2)


def _P3(x1, x2, w, sv, s2):
    return _tail_J(x2 - x1, -x1, w, s2)


def _erf_difference(ta, tb):
    """erf(tb) - erf(ta), ta <= tb, without cancelling the 1s."""
    from scipy.special import erf
    erfc, _ = _special()
    with np.errstate(under='ignore'):
        return np.where(ta > 0.0, erfc(ta) - erfc(tb), np.where(tb < 0.0, erfc(-tb) - erfc(-ta), erf(tb) - erf(ta)))


def _P2(x1, x2, w, sv, s2):
    """The region between the points."""
    x1s, x2s, x12, xs = x1 * x1, x2 * x2, x1 * x2, x1 + x2
    E0 = 9.0 + 25.0 * x1s * x2s + 3.0 * SQ5 * (3.0 - 5.0 * x12) * (x2 - x1) + 15.0 * (x1s + x2s - 3.0 * x12)
    E1 = 5.0 * (3.0 * SQ5 * (x2s - x1s) + 3.0 * xs - 10.0 * x12 * xs)
    E2 = 5.0 * (5.0 * x1s + 5.0 * x2s - 3.0 - 3.0 * SQ5 * (x2 - x1) + 20.0 * x12)
    E3 = -50.0 * xs
    U = (E0 + w * E2 + 3.0 * w * w * 25.0) / 9.0                     # the moments of N(0, w): 0, w, 0, 3 w^2
    V2 = (E1 + x1 * E2 + (2.0 * w + x1s) * E3 + (x1s * x1 + 3.0 * w * x1) * 25.0) / 9.0
    V3 = (E1 + x2 * E2 + (2.0 * w + x2s) * E3 + (x2s * x2 + 3.0 * w * x2) * 25.0) / 9.0
    with np.errstate(under='ignore'):
        return np.exp(-SQ5 * (x2 - x1)) * (0.5 * U * _erf_difference(x1 / s2, x2 / s2) +
                                           V2 * sv * np.exp(-0.5 * x1s / w) - V3 * sv * np.exp(-0.5 * x2s / w))


def _norm_pair(X1, X2, m, v, l):
    X1, X2, m, v, l = (np.asarray(t, dtype=np.float64) for t in (X1, X2, m, v, l))
    a, b = (np.minimum(X1, X2) - m) / l, (np.maximum(X1, X2) - m) / l
    w = np.where(v == 0.0, 1.0, v / (l * l))
    return a, b, w, np.sqrt(0.5 * w / np.pi), np.sqrt(2.0 * w)


def fixed_Jd(X1, X2, m, v, l):
    a, b, w, sv, s2 = _norm_pair(X1, X2, m, v, l)
    return np.where(np.asarray(v) == 0.0, _kp(a) * _kp(b), _P1(a, b, w, sv, s2) + _P2(a, b, w, sv, s2) + _P3(a, b, w, sv, s2))


def fixed_Jd0(X1, m, v, l):
    a, b, w, sv, s2 = _norm_pair(X1, X1, m, v, l)
    return np.where(np.asarray(v) == 0.0, _kp(a) * _kp(b), _P1(a, a, w, sv, s2) + _P3(a, a, w, sv, s2))


EXP_CLAMP = 600.0      # of the bare exp(+-sqrt5 x) of a record: exact within 268 lengthscales of m, finite beyond


def _tail_T(x, w, s2):
    """T[0..2] of a point x in the larger-point role: the coefficients of exp(sqrt5 lo) lo^a in the region above both points.
    With z = x + s the other point's factor is 1 + sqrt5 (sg - lo) + 5/3 (sg - lo)^2, sg = s + x, by powers of lo."""
    H, fold = tail_moments(x + 2.0 * SQ5 * w, w, s2)
    with np.errstate(all='ignore'):
        e = np.exp(np.minimum(np.where(fold, -SQ5 * x - 0.5 * x * x / w, SQ5 * x + 10.0 * w), EXP_CLAMP)) * RSQPI
    q0 = _polyB(1.0 + x * (SQ5 + B2 * x), SQ5 + 2.0 * B2 * x, B2)
    q1 = _polyB(-SQ5 - 2.0 * B2 * x, -2.0 * B2, 0.0)
    return [e * _dot5(q0, H), e * _dot5(q1, H), e * (B2 * (B0 * H[0] + B1 * H[1] + B2 * H[2]))]


def _middle(x, w, sv, s2, role):
    """The parts of the region between the points that one point carries: (U4[3], V[3], sgn, erfcx(|t|)); role 0 = smaller."""
    _, erfcx = _special()
    sg = 1.0 if role == 0 else -1.0
    p0 = [9.0 + x * (-sg * 9.0 * SQ5 + 15.0 * x), sg * 9.0 * SQ5 + x * (-45.0 + sg * 15.0 * SQ5 * x), 15.0 + x * (-sg * 15.0 * SQ5 + 25.0 * x)]
    p1 = [x * (15.0 - sg * 15.0 * SQ5 * x), 15.0 - 50.0 * x * x, sg * 15.0 * SQ5 - 50.0 * x]
    p2 = [-15.0 + x * (sg * 15.0 * SQ5 + 25.0 * x), -sg * 15.0 * SQ5 + 100.0 * x, 25.0 + 0.0 * x]
    p3 = [-50.0 * x, -50.0 + 0.0 * x, 0.0 * x]
    p4 = [25.0 + 0.0 * x, 0.0 * x, 0.0 * x]
    b2, b3, b4 = x, 2.0 * w + x * x, x * x * x + 3.0 * w * x
    U4 = [(p0[a] + w * p2[a] + 3.0 * w * w * p4[a]) / 9.0 for a in range(3)]
    V = [(p1[a] + b2 * p2[a] + b3 * p3[a] + b4 * p4[a]) / 9.0 for a in range(3)]
    t = x / s2
    return U4, V, np.where(t >= 0.0, 1.0, -1.0), erfcx(np.abs(t))


def _role_S(x, w, sv, s2):
    """S[0..11] and f2 of one point in the smaller-point role (normalised).  f2 is the sign of x: erf(t) = f2 -+ erfc(|t|), and
    the erfc part of the erf difference rides in S[9..11] (and T[6..8]), so that no 1 - 1 is formed."""
    with np.errstate(all='ignore'):
        eP = np.exp(np.minimum(SQ5 * x, EXP_CLAMP))
        e2 = np.exp(SQ5 * x - 0.5 * x * x / w)
    U4, V42, sgn, cx = _middle(x, w, sv, s2, 0)
    T = _tail_T(-x, w, s2)
    out = [None] * 12
    xa = np.ones_like(x)
    for a in range(3):
        out[a] = eP * xa
        out[3 + a] = T[a] if a != 1 else -T[a]
        out[6 + a] = eP * xa
        out[9 + a] = e2 * (sv * V42[a] + sgn * 0.5 * cx * U4[a])
        xa = xa * x
    return out, sgn


def _role_T(x, w, sv, s2):
    """T[0..14] of one point in the larger-point role (normalised)."""
    with np.errstate(all='ignore'):
        eM = np.exp(np.minimum(-SQ5 * x, EXP_CLAMP))
        e2 = np.exp(-SQ5 * x - 0.5 * x * x / w)
    U4, V43, sgn, cx = _middle(x, w, sv, s2, 1)
    T = _tail_T(x, w, s2)
    out = [None] * 15
    xa = np.ones_like(x)
    for a in range(3):
        out[a] = T[a]
        out[3 + a] = eM * xa
        out[6 + a] = e2 * (-sv * V43[a] - sgn * 0.5 * cx * U4[a])
        out[9 + a] = eM * xa
        out[12 + a] = eM * (0.5 * U4[a])
        xa = xa * x
    return out


def _combine(S, f2lo, T, f2hi):
    acc = 0.0
    for c in range(12):
        acc = acc + S[c] * T[c]
    e = 0.0
    for a in range(3):
        e = e + S[6 + a] * T[12 + a]
    return acc + (f2hi - f2lo) * e


def fixed_Jsep(X1, X2, m, v, l):
    a, b, w, sv, s2 = _norm_pair(X1, X2, m, v, l)
    S, f2lo = _role_S(a, w, sv, s2)
    T = _role_T(b, w, sv, s2)
    f2hi = np.where(b / s2 >= 0.0, 1.0, -1.0)
    with np.errstate(under='ignore', invalid='ignore'):
        return np.where(np.asarray(v) == 0.0, _kp(a) * _kp(b), _combine(S, f2lo, T, f2hi))


def fixed_Jsep0(X1, m, v, l):
    return fixed_Jsep(X1, X1, m, v, l)


def fixed(fn, args):
    X1, X2, m, v, l = (args[:, k] for k in range(5))
    with np.errstate(under='ignore'):
        if fn == 'i':
            return fixed_I(X1, m, v, l)
        if fn == 'jd':
            return fixed_Jd(X1, X2, m, v, l)
        if fn == 'jd0':
            return fixed_Jd0(X1, m, v, l)
        if fn == 'jsep':
            return fixed_Jsep(X1, X2, m, v, l)
        return fixed_Jsep0(X1, m, v, l)


def exact_key(fn):
    return {'i': 'exact_i', 'jd': 'exact_j', 'jd0': 'exact_j0', 'jsep': 'exact_j', 'jsep0': 'exact_j0'}[fn]


def relative_error(got, exact):
    """|got - exact| / exact where exact >= TINY; elsewhere 0 if |got| <= 1e-279 and inf if not."""
    got, exact = np.asarray(got, dtype=np.float64), np.asarray(exact, dtype=np.float64)
    big = exact >= TINY
    with np.errstate(divide='ignore', invalid='ignore'):
        rel = np.abs(got - exact) / exact
    small = np.where(np.abs(got) <= 1e-279, 0.0, np.inf)
    out = np.where(big, rel, small)
    return np.where(np.isfinite(got), out, np.inf)


def measure_E_b(args, ratio, exact):
    """E_b (len(BUCKET_EDGES),) and the per-function table {fn: (nb,)}; exact: dict of 'exact_i' / 'exact_j' / 'exact_j0'."""
    b = bucket_of(ratio)
    table = {}
    for fn in FNS:
        rel = relative_error(fixed(fn, args), exact[exact_key(fn)])
        table[fn] = np.array([rel[b == k].max() if (b == k).any() else 0.0 for k in range(len(BUCKET_EDGES))])
    return np.max(np.stack([table[fn] for fn in FNS]), axis=0), table


def exact_rows(args, index):
    """(exact_i, exact_j, exact_j0) as doubles for the cases `index`."""
    ei, ej, e0 = [], [], []
    for k in index:
        X1, X2, m, v, l = args[k]
        ei.append(to_double(exact_I(X1, m, v, l)))
        ej.append(to_double(exact_J(X1, X2, m, v, l)))
        e0.append(to_double(exact_J(X1, X1, m, v, l)))
    return np.array(ei), np.array(ej), np.array(e0)


def erfcx_inputs():
    """Arguments of the device erfcx as linkfun.hpp calls it (t >= 0): the ends, the recurrence switch, a log and a linear grid."""
    edge = [0.0, 5e-324, 1e-300, 2.0 ** -54, 0.5, 1.0, T_FORWARD, np.nextafter(T_FORWARD, 0.0), 26.0, 27.0, 1e8, 1e150, 1e300]
    return np.concatenate((edge, 10.0 ** np.linspace(-20.0, 8.0, 600), np.linspace(0.0, 30.0, 1387)))


def exact_erfcx(t):
    mp = _mp()
    out = []
    with mp.workdps(60):
        for x in t:
            x = mp.mpf(float(x))
            # (beyond 1e6 the two-term asymptotic series is exact to 1e-24; exp(x^2) there has an exponent mpmath need not carry)
            out.append(float(mp.exp(x * x) * mp.erfc(x) if x < 1e6 else (1 - 1 / (2 * x * x)) / (x * mp.sqrt(mp.pi))))
    return np.array(out)


def load():
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def write_fixture():
    args, ratio = cases()
    ei, ej, e0 = exact_rows(args, range(len(args)))
    exact = {'exact_i': ei, 'exact_j': ej, 'exact_j0': e0}
    E_b, table = measure_E_b(args, ratio, exact)
    os.makedirs(GOLDEN, exist_ok=True)
    t = erfcx_inputs()
    np.savez_compressed(FIXTURE, args=args, ratio=ratio, E_b=E_b, erfcx_t=t, erfcx_exact=exact_erfcx(t), **exact)
    print('%d cases -> %s (%d bytes)' % (len(args), FIXTURE, os.path.getsize(FIXTURE)))
    for fn in FNS:
        print('%-6s' % fn, ' '.join('%.1e' % e for e in table[fn]))
    print('E_b   ', ' '.join('%.1e' % e for e in E_b))


# ------------------------------------------------------------------------------------------------ the oracle on the integral
import contextlib


@contextlib.contextmanager
def oracle_on_the_integral(O):
    """Within the block the oracle's three Matern linked factors (matern_I_dim, Jd, Jd0 of oracle/dgp_oracle.py) are the float64
    restatement of the integral above instead of the reference's expression; everything else of the oracle -- how I and J
    are assembled, link_gp's mean and variance, the Vecchia conditioning -- is untouched.  For the GPU tests whose inputs reach
    v/l^2 >~ 0.3: there the reference's expression is wrong beyond those tests' tolerances (6e-4 at 1, 8e4 at 4, not finite
    from 100; test_linkfun_host.py has the figures), the device follows the integral, and the restatement is held to the
    exact values by test_restatement_error_per_bucket."""
    saved = O.matern_I_dim, O.Jd, O.Jd0
    O.matern_I_dim = lambda xk, zm, zv, ell: fixed_I(xk, zm, zv, ell)
    O.Jd = lambda X1, X2, z_m, z_v, ell: fixed_Jd(X1, X2, z_m, z_v, ell)
    O.Jd0 = lambda x1, z_m, z_v, ell: fixed_Jd0(x1, z_m, z_v, ell)
    try:
        yield O
    finally:
        O.matern_I_dim, O.Jd, O.Jd0 = saved


# ------------------------------------------------------------------------------------------------ the kernels end to end
E2E_N, E2E_M, E2E_NUGGET, E2E_SCALE, E2E_PM = 70, 40, 0.05, 1.3, 20
E2E_RATIOS = [1e-8, 0.1, 1.0, 4.0, 25.0, 100.0]
E2E_LENGTH = np.array([0.5, 0.8, 0.3, 0.6])                     # three local dimensions, one global
E2E_CONFIGS = [(1, 0), (3, 0), (1, 1), (3, 1)]                  # (Dw, Dz)
E2E_PAIRS = [(0, 0), (5, 5), (63, 63), (64, 64), (69, 69), (1, 0), (17, 3), (63, 62), (40, 40), (33, 12),
             (64, 0), (64, 63), (69, 5), (65, 64), (69, 68), (66, 31), (68, 64), (50, 49), (12, 12), (69, 0)]   # within / across the 64-tiles


def _frac(a):
    return a - np.floor(a)


def e2e_inputs():
    """Inputs by index (no random numbers): n = 70 training points on [-2, 2]^4 (two 64-blocks), M = 40 test points whose
    dimensions mix the v/l^2 regimes of E2E_RATIOS; every tenth test point sits on a training point."""
    i, t = np.arange(E2E_N)[:, None] + 1.0, np.arange(E2E_M)[:, None] + 1.0
    W = 4.0 * _frac(i * np.sqrt([2.0, 3.0, 5.0, 7.0])[None, :]) - 2.0
    m = 4.4 * _frac(t * np.sqrt([11.0, 13.0, 17.0])[None, :]) - 2.2
    z = 4.0 * _frac(t * np.sqrt(19.0)) - 2.0
    for tt in range(0, E2E_M, 10):
        m[tt] = W[(7 * tt + 3) % E2E_N, :3]
    tk = np.arange(E2E_M)[:, None] + 2 * np.arange(3)[None, :] + np.arange(E2E_M)[:, None] // 6
    ratio = np.array(E2E_RATIOS)[tk % len(E2E_RATIOS)]
    v = ratio * E2E_LENGTH[None, :3] ** 2
    y = np.sin(1.3 * W[:, 0]) + 0.5 * np.cos(2.0 * W[:, 1]) - 0.3 * W[:, 2] * W[:, 3]
    return dict(W=W, m=m, v=v, z=z, y=y, ratio=ratio)


def e2e_drop():
    """The training point each test point leaves out (linkgp_predict's drop=): the first, the last, the point a test point sits on."""
    t = np.arange(E2E_M)
    drop = (11 * t + 5) % E2E_N
    drop[::10] = (7 * t[::10] + 3) % E2E_N
    drop[1], drop[2] = 0, E2E_N - 1
    return drop.astype(np.int32)


def _split(x):
    """A longdouble array as (hi, lo) doubles."""
    x = np.asarray(x, dtype=np.longdouble)
    hi = x.astype(np.float64)
    return hi, (x - hi.astype(np.longdouble)).astype(np.float64)


def join(hi, lo):
    return np.asarray(hi, dtype=np.longdouble) + np.asarray(lo, dtype=np.longdouble)


def _ld_corr(A, B, length):
    """Matern-2.5 product correlation between the rows of A and of B, in longdouble."""
    LDT = np.longdouble
    s5 = np.sqrt(LDT(5))
    r = np.abs(A.astype(LDT)[:, None, :] - B.astype(LDT)[None, :, :]) / np.asarray(length, dtype=LDT)[None, None, :]
    return np.prod(1 + s5 * r + LDT(5) / 3 * r * r, axis=2) * np.exp(-s5 * r.sum(axis=2))


def _ld_inverse(K):
    """Inverse of a symmetric positive definite longdouble matrix by Cholesky."""
    LDT = np.longdouble
    n = len(K)
    L = np.zeros((n, n), dtype=LDT)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - np.dot(L[j, :j], L[j, :j]))
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Li = np.zeros((n, n), dtype=LDT)
    for j in range(n):
        Li[j, j] = 1 / L[j, j]
        for r in range(j + 1, n):
            Li[r, j] = -np.dot(L[r, j:r], Li[j:r, j]) / L[r, r]
    return Li.T @ Li


def link_moments(I, J, Rinv, ry, scale, nugget):
    """mean = I.ry, var = |ry^T J ry - mean^2 + scale (1 + nugget - tr(Rinv J))| in longdouble, and the sums of the absolute
    terms of either expression (what a relative bound multiplies)."""
    LDT = np.longdouble
    I, J, Rinv, ry = (np.asarray(a, dtype=LDT) for a in (I, J, Rinv, ry))
    mean = np.dot(I, ry)
    var = np.abs(ry @ J @ ry - mean * mean + LDT(scale) * (1 + LDT(nugget) - np.sum(Rinv * J)))
    mabs = np.dot(np.abs(I), np.abs(ry))
    vabs = np.abs(ry) @ np.abs(J) @ np.abs(ry) + mean * mean + LDT(scale) * (1 + abs(LDT(nugget)) + np.sum(np.abs(Rinv * J)))
    return mean, var, mabs, vabs


def _e2e_dim_job(job):
    t, k, x, m, v, l = job
    n = len(x)
    Iv = [to_longdouble(exact_I(x[i], m, v, l)) for i in range(n)]
    Jv = np.zeros((n, n), dtype=np.longdouble)
    for i in range(n):
        for j in range(i + 1):
            Jv[i, j] = Jv[j, i] = to_longdouble(exact_J(x[i], x[j], m, v, l))
    return t, k, np.array(Iv, dtype=np.longdouble), Jv


def e2e_exact_factors(inp, processes=8):
    """(I[t, k, i], J[t, k, i, j]) of the exact per-dimension factors as longdouble."""
    import multiprocessing
    jobs = [(t, k, inp['W'][:, k], inp['m'][t, k], inp['v'][t, k], E2E_LENGTH[k]) for t in range(E2E_M) for k in range(3)]
    I = np.zeros((E2E_M, 3, E2E_N), dtype=np.longdouble)
    J = np.zeros((E2E_M, 3, E2E_N, E2E_N), dtype=np.longdouble)
    with multiprocessing.Pool(processes) as pool:
        for t, k, Iv, Jv in pool.imap_unordered(_e2e_dim_job, jobs):
            I[t, k], J[t, k] = Iv, Jv
    return I, J


def e2e_config(inp, Dw, Dz):
    """The training inputs, lengthscales and float64 (Rinv, Rinv y) of one configuration."""
    from oracle import dgp_oracle as O
    X = np.concatenate((inp['W'][:, :Dw], inp['W'][:, 3:3 + Dz]), axis=1)
    length = np.concatenate((E2E_LENGTH[:Dw], E2E_LENGTH[3:3 + Dz]))
    st = O.compute_stats(X, inp['y'], length, E2E_NUGGET, 'matern2.5', Dw)
    return X, length, st['Rinv'], st['Rinv_y']


def e2e_neighbours(inp, Dw, Dz, pm):
    from oracle import dgp_oracle as O
    X, length, _, _ = e2e_config(inp, Dw, Dz)
    q = np.concatenate((inp['m'][:, :Dw], inp['z'][:, :Dz]), axis=1)
    return O.pred_nn(q / length, X / length, pm)


def write_fixture_e2e():
    LDT = np.longdouble
    inp = e2e_inputs()
    Iex, Jex = e2e_exact_factors(inp)
    out = {}
    for (Dw, Dz) in E2E_CONFIGS:
        key = 'w%dz%d_' % (Dw, Dz)
        X, length, Rinv, ry = e2e_config(inp, Dw, Dz)
        out[key + 'Rinv'], out[key + 'ry'] = Rinv, ry
        res = {name: [] for name in ('dense', 'drop', 'vn', 'v20')}
        drop = e2e_drop()
        NN = {'vn': e2e_neighbours(inp, Dw, Dz, E2E_N), 'v20': e2e_neighbours(inp, Dw, Dz, E2E_PM)}
        for t in range(E2E_M):
            Iz = _ld_corr(X[:, Dw:], inp['z'][t:t + 1, :Dz], length[Dw:])[:, 0] if Dz else np.ones(E2E_N, dtype=LDT)
            I = np.prod(Iex[t, :Dw], axis=0) * Iz
            J = np.prod(Jex[t, :Dw], axis=0) * np.outer(Iz, Iz)
            res['dense'].append(link_moments(I, J, Rinv, ry, E2E_SCALE, E2E_NUGGET))
            # without training point d: the downdate of the given (Rinv, Rinv y), in longdouble
            d, keep = drop[t], np.delete(np.arange(E2E_N), drop[t])
            Rl, rl = Rinv.astype(LDT), ry.astype(LDT)
            Rk = Rl[np.ix_(keep, keep)] - np.outer(Rl[keep, d], Rl[d, keep]) / Rl[d, d]
            res['drop'].append(link_moments(I[keep], J[np.ix_(keep, keep)], Rk, rl[keep] - Rl[keep, d] * rl[d] / Rl[d, d], E2E_SCALE, E2E_NUGGET))
            for name in ('vn', 'v20'):
                idx = NN[name][t]
                K = _ld_corr(X[idx], X[idx], length)
                K[np.arange(len(idx)), np.arange(len(idx))] = 1 + LDT(E2E_NUGGET)
                Ki = _ld_inverse(K)
                res[name].append(link_moments(I[idx], J[np.ix_(idx, idx)], Ki, Ki @ inp['y'][idx].astype(LDT), E2E_SCALE, E2E_NUGGET))
        for name, rows in res.items():
            a = np.array(rows, dtype=LDT)
            for c, what in enumerate(('mean', 'var')):
                out[key + name + '_' + what + '_hi'], out[key + name + '_' + what + '_lo'] = _split(a[:, c])
            out[key + name + '_mabs'], out[key + name + '_vabs'] = a[:, 2].astype(np.float64), a[:, 3].astype(np.float64)
    pi, pj = np.array(E2E_PAIRS).T
    out['pair_I'] = Iex[:, 0, pi].astype(np.float64)                   # [t, pair]: I of the pair's first point, first dimension
    out['pair_J'] = Jex[:, 0, pi, pj].astype(np.float64)
    # the far inputs of test_vecchia_predictions_beyond_the_exponent_range: a test point ON a training point, v = 1e-12, l = 1e-5
    out['far_I'] = np.array(_split(to_longdouble(exact_I(0.0, 0.0, 1e-12, 1e-5))))
    out['far_J0'] = np.array(_split(to_longdouble(exact_J(0.0, 0.0, 0.0, 1e-12, 1e-5))))
    np.savez_compressed(FIXTURE_E2E, **out)
    print('%s (%d bytes)' % (FIXTURE_E2E, os.path.getsize(FIXTURE_E2E)))


def load_e2e():
    with np.load(FIXTURE_E2E) as z:
        return {k: z[k] for k in z.files}


if __name__ == '__main__':
    import sys
    if 'e2e' not in sys.argv[1:]:
        write_fixture()
    if 'exact' not in sys.argv[1:]:
        write_fixture_e2e()
