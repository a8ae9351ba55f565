"""Inputs so far apart that every correlation between different rows underflows, for the *_beyond_the_exponent_range tests.

Row i = i s (1, 1), s = 1 or 1e4, against a lengthscale of 1e-5: the squared-exponential exponents are 2e10 i^2 (s = 1: far beyond
2^31 ln 2 = 1.4886e9, where the integer part of the device exponentials leaves 32 bits) and beyond 2^63 (s = 1e4), the Matern ones
sqrt5 2e5 i and sqrt5 2e9 i.  Every correlation between different rows is exactly 0 in the oracle's arithmetic (numpy.exp)."""
import numpy as np

FAR_LENGTH, FAR_NUGGET, FAR_SCALE = np.array([1e-5]), 1e-6, 1.1
FAR_ZERO = 1e-300   # what the device may return where the reference is exactly 0


def far_inputs(n, s):
    return np.arange(n, dtype=float)[:, None] * s * np.ones((1, 2))


def check_zeros(a, ref, what=''):
    """Asserts |a| <= FAR_ZERO wherever ref is exactly 0; returns the mask of the other entries, which the caller holds to the
    tolerance of the well-scaled sibling test."""
    a, ref = np.asarray(a, float), np.asarray(ref, float)
    z = ref == 0.0
    bad = ~(np.abs(a[z]) <= FAR_ZERO)
    assert not bad.any(), (what, a[z][bad][:5], int(z.sum()))
    return ~z
