"""Reference for the pick-freeze sums of dgpamd_sobol_tiles / dgpamd_sobol_add (DESIGN I.16).

g = f - shift is formed in f64, the one IEEE subtraction the device does, so both sides sum terms of the same numbers.  Every
term -- g, g^2, g_B (g_AB - g_A), (g_A - g_AB)^2 -- is then taken in exact rational arithmetic (a double is an integer times a
power of two: Python integers over one common power) and so is the sum: the reference carries no rounding at all, and
float() of it is the correctly rounded sum (what math.fsum gives of exact terms).

Bound of a device sum of M terms over ntiles = ceil(M / 64) tiles:
    |device - exact| <= 1.01 (ntiles + 8) 2^-53 sum_j |term_j|.
A term is formed with at most two roundings (the difference of two g, the product); six levels of the wave's tree add one
rounding each to what passes through them; the ntiles sequential additions of dgpamd_sobol_add one each.  (1 + u)^(ntiles + 8)
- 1 <= 1.01 (ntiles + 8) u for every ntiles below 2^45.  The comparison itself is made in rational arithmetic."""
from fractions import Fraction

import numpy as np

U = Fraction(1, 2**53)


def _integers(*gs):
    """Finite doubles as Python integers over one power of two: (lists of integers, e) with g = integer * 2^e exactly."""
    parts = [np.frexp(g) for g in gs]                       # g = mantissa * 2^exponent, |mantissa| < 1 with 53 bits
    e = min(int(ex.min()) for _, ex in parts) - 53
    return [[int(m) << (int(x) - 53 - e) for m, x in zip(np.ldexp(mant, 53), ex)] for mant, ex in parts], e


def _terms(gA, gB, gAB):
    """The exact terms of one (path, output): per sum (list of integers, e), term = integer * 2^e."""
    if gAB is None:
        (a, b), e = _integers(gA, gB)
        return [(a, e), (b, e), ([v * v for v in a], 2 * e), ([v * v for v in b], 2 * e)]
    (a, b, ab), e = _integers(gA, gB, gAB)
    return [([y * (z - x) for x, y, z in zip(a, b, ab)], 2 * e), ([(x - z) * (x - z) for x, z in zip(a, ab)], 2 * e)]


def _fraction(i, e):
    return Fraction(i * 2**e) if e >= 0 else Fraction(i, 2**-e)


def exact_sums(fA, fB, fAB, shift):
    """(sums, magnitudes): object arrays of Fractions (P, K, 4) -- or (P, K, 2) with fAB -- the exact sums of the terms of
    g = f - shift[:, None, :] over the rows and the exact sums of their absolute values.  fA, fB, fAB: (P, M, K) f64."""
    gA, gB = fA - shift[:, None, :], fB - shift[:, None, :]
    gAB = None if fAB is None else fAB - shift[:, None, :]
    P, M, K = fA.shape
    nc = 4 if fAB is None else 2
    sums, mags = np.empty((P, K, nc), dtype=object), np.empty((P, K, nc), dtype=object)
    for p in range(P):
        for k in range(K):
            for c, (t, e) in enumerate(_terms(gA[p, :, k], gB[p, :, k], None if gAB is None else gAB[p, :, k])):
                sums[p, k, c], mags[p, k, c] = _fraction(sum(t), e), _fraction(sum(map(abs, t)), e)
    return sums, mags


def worst_ratio(device, sums, mags, ntiles):
    """max over the entries of |device - exact| / bound (0 / 0 counts as 0: a sum of zeros must come out as zero)."""
    worst = 0.0
    for d, s, m in zip(np.asarray(device).reshape(-1), sums.reshape(-1), mags.reshape(-1)):
        assert np.isfinite(d), d
        err, bound = abs(Fraction(float(d)) - s), Fraction(101, 100) * (ntiles + 8) * U * m
        if err > 0:
            worst = max(worst, float(err / bound) if bound > 0 else np.inf)
    return worst


def check(device, sums, mags, ntiles, what):
    ratio = worst_ratio(device, sums, mags, ntiles)
    print('%s: max error / bound = %.3g' % (what, ratio))
    assert ratio <= 1.0, (what, ratio)
    return ratio


def indices(base, pair, n_base):
    """The three formula lines of sensitivity.indices_from_sums, restated: (first, total, V)."""
    B = n_base
    s1, s2, q1, q2 = (base[..., c] for c in range(4))
    U_, T = pair[..., 0], pair[..., 1]
    V = (q1 + q2) / (2 * B) - ((s1 + s2) / (2 * B))**2
    first = (U_ / B) / V
    total = (T / (2 * B)) / V
    return first, total, V
