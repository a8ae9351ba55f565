"""Inputs and extended-precision references for the library's own device math functions (tests/test_gpu_mathfn.py probes them
through dgpamd_debug_mathfn; test_host_reference_agrees_with_mpmath there checks this file without a GPU).

The reference is numpy.longdouble (x87 extended, eps = 2^-63) through numpy's exp / cos / sin / sqrt / exp2.  Where the platform's
long double is no wider than that bound allows, HAVE_LONGDOUBLE is False and the tests fall back to mpmath at 40 digits on a subset
chosen by index (subset_index).

Every input set is a fixed function of a seed: structured points first (their number is `n_struct` of the returned pair), random
ones behind them."""
import math

import numpy as np

LD = np.longdouble
HAVE_LONGDOUBLE = bool(np.finfo(LD).eps <= 2.0 ** -63)
LN2 = np.log(LD(2))            # (only place the structured points: each is taken with its neighbouring doubles)
PIO2 = 2 * np.arctan(LD(1))
DBL_MAX = np.finfo(np.float64).max
NRAND = 1000000          # random points per set of the exponentials and the roots
NRAND_COS = 250000       # ... per range of the cosine
BIG = np.array([708.0, 709.5, 745.0, 746.0] + [10.0 ** e for e in range(3, 301)] + [DBL_MAX, np.inf, np.nan])


def neighbours(x, k):
    """Each double of x with its k neighbouring doubles on either side: (len(x) * (2k + 1),)."""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    cols = [x]
    lo = hi = x
    for _ in range(k):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        cols += [lo, hi]
    return np.stack(cols, 1).reshape(-1)


def to_double(v):
    return np.asarray(v, dtype=LD).astype(np.float64)


def log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), size=n))


def _exp_random(rng):
    return [rng.uniform(-1.0, 700.0, size=NRAND), log_uniform(rng, 1e-300, 700.0, NRAND)]


def exp_inputs():
    """exp_negated and exp_negated_v3: (a, n_struct)."""
    rng = np.random.default_rng(20250101)
    k = np.arange(-2, 1011).astype(LD)
    half = neighbours(to_double((k + LD(0.5)) * LN2), 3)
    j = np.arange(1, 5).astype(LD)
    cross = to_double(j * LD(2.0 ** 31) * LN2)
    cross = np.concatenate((neighbours(cross, 3), cross - 1.0, cross + 1.0))
    s = np.concatenate(([0.0, -0.0], half, cross, BIG))
    return np.concatenate([s] + _exp_random(rng)), len(s)


def exp_tab_inputs():
    """exp_negated_tab and its two halves: (a, n_struct)."""
    rng = np.random.default_rng(20250102)
    k = np.arange(-370, 181001).astype(LD)
    half = neighbours(to_double((k + LD(0.5)) * LN2 / LD(256)), 2)
    j = np.arange(1, 9).astype(LD)
    wrap = to_double(j * LD(2.0 ** 31) * LN2 / LD(256))                     # the low word of k wraps (the round-5 fault)
    wrap = np.concatenate((neighbours(wrap, 3), wrap - 1.0, wrap + 1.0))
    p39 = neighbours(to_double(LD(2.0 ** 39) * LN2 / LD(256)), 3)           # |k| = 2^39
    s = np.concatenate(([0.0, -0.0], half, wrap, p39, BIG))
    return np.concatenate([s] + _exp_random(rng)), len(s)


def cos_inputs():
    """cos_reduced_impl, both instantiations: (a, n_struct)."""
    rng = np.random.default_rng(20250103)
    two30 = 2.0 ** 30
    k = np.arange(-200000, 200001).astype(LD)
    near = neighbours(to_double(k * PIO2), 3)
    kmax = int(math.floor(two30 * 2.0 / math.pi))                          # (k pi / 2 < 2^30 for k <= kmax; kmax pi / 2 is 0.3 below)
    ktop = np.arange(kmax - 999, kmax + 1).astype(LD)
    top = neighbours(to_double(ktop * PIO2), 3)
    assert np.all(np.abs(top) < two30)
    below = np.nextafter(two30, 0.0)
    edges = np.array([0.0, -0.0, below, -below, two30, -two30, 1e300, np.inf, -np.inf, np.nan])
    s = np.concatenate((edges, near, top, -top))
    r = [rng.uniform(-w, w, size=NRAND_COS) for w in (10.0, 1e3, 1e6, 1e8, two30 - 1.0)]
    return np.concatenate([s] + r), len(s)


def root_inputs():
    """rsqrt_f64, rsqrt_sqrt, rcp_f64 (rcp_f64 also on the negated set): (a, n_struct)."""
    rng = np.random.default_rng(20250104)
    e = np.arange(-400, 401).astype(np.float64)
    s = np.concatenate((neighbours(np.exp2(e), 2), neighbours(np.exp2(2.0 * e), 2)))
    r = [log_uniform(rng, 1e-290, 1e290, NRAND), rng.uniform(1e-12, 10.0, size=NRAND)]
    return np.concatenate([s] + r), len(s)


def dlog_inputs():
    rng = np.random.default_rng(20250105)
    lu = log_uniform(rng, 1e-300, 1e100, NRAND)
    s = np.array([0.0, -0.0])
    return np.concatenate((s, lu, -lu, rng.uniform(-50.0, 50.0, size=NRAND))), len(s)


def tri_inputs():
    """t: every index below 2^22 and the 1000 largest below 2^31 (int64)."""
    return np.concatenate((np.arange(1 << 22, dtype=np.int64), np.arange((1 << 31) - 1000, 1 << 31, dtype=np.int64)))


def tri_reference(t):
    """(bi, bj) with t = bi (bi + 1) / 2 + bj, 0 <= bj <= bi, in integers: row b of the triangle has b + 1 entries (the dense
    range from 0), math.isqrt for the rest."""
    dense = int(np.searchsorted(t, 1 << 22))
    assert np.array_equal(t[:dense], np.arange(dense))
    rows = math.isqrt(2 * dense) + 2
    bi = np.empty(len(t), dtype=np.int64)
    bi[:dense] = np.repeat(np.arange(rows, dtype=np.int64), np.arange(1, rows + 1))[:dense]
    for i, v in enumerate(t[dense:].tolist()):
        bi[dense + i] = (math.isqrt(8 * v + 1) - 1) // 2
    bj = t - bi * (bi + 1) // 2
    assert np.all((0 <= bj) & (bj <= bi))
    return bi, bj


def subset_index(n, n_struct, nrand=20000):
    """Indices the mpmath fall-back keeps: every structured point and `nrand` of the random ones, by index alone."""
    rest = n - n_struct
    return np.concatenate((np.arange(n_struct), n_struct + (np.arange(min(nrand, rest)) * max(rest // nrand, 1))))


# ---------------------------------------------------------------------------------------------- references
def _ld(a):
    return np.asarray(a, dtype=np.float64).astype(LD)


def _mp(fn, a):
    import mpmath
    out = np.empty(len(a), dtype=LD)
    with mpmath.workdps(40):
        for i, v in enumerate(np.asarray(a, dtype=np.float64).tolist()):
            if math.isnan(v):
                out[i] = np.nan
            elif math.isinf(v):   # (exp(-x); the cosine and the sine have no value there)
                out[i] = {'expn': 0.0 if v > 0 else np.inf}.get(fn, np.nan)
            else:
                out[i] = mp_to_ld(MP_FUNCS[fn](mpmath.mpf(v)))
    return out


def mp_to_ld(m):
    """An mpmath number rounded into numpy.longdouble (two doubles: 106 bits, more than either long double format keeps)."""
    import mpmath
    if m == 0:
        return LD(0.0)
    man, ex = mpmath.frexp(m)
    hi = float(man)
    lo = float(man - mpmath.mpf(hi))
    return np.ldexp(LD(hi) + LD(lo), int(ex))


def ld_to_mp(v):
    """numpy.longdouble -> mpmath, exactly."""
    import mpmath
    man, ex = np.frexp(LD(v))
    hi = float(man)
    lo = float(man - LD(hi))
    return mpmath.ldexp(mpmath.mpf(hi) + mpmath.mpf(lo), int(ex))


def _mp_dlog(t):
    import mpmath
    r, s5 = abs(t), mpmath.sqrt(5)
    return -(mpmath.mpf(5) / 3) * t * (1 + s5 * r) / (1 + s5 * r + (mpmath.mpf(5) / 3) * t * t)


def _mp_funcs():
    import mpmath
    return dict(expn=lambda x: mpmath.exp(-x), cos=mpmath.cos, msin=lambda x: -mpmath.sin(x), rsqrt=lambda x: 1 / mpmath.sqrt(x),
                sqrt=mpmath.sqrt, rcp=lambda x: 1 / x, dlog=_mp_dlog, exp2=lambda x: mpmath.power(2, x))


class _Lazy(dict):
    def __missing__(self, key):
        self.update(_mp_funcs())
        return self[key]


MP_FUNCS = _Lazy()


def _ld_dlog(t):
    r, s5, c = np.abs(t), np.sqrt(LD(5)), LD(5) / LD(3)
    return -c * t * (1 + s5 * r) / (1 + s5 * r + c * t * t)


LD_FUNCS = dict(expn=lambda x: np.exp(-x), cos=np.cos, msin=lambda x: -np.sin(x), rsqrt=lambda x: 1 / np.sqrt(x), sqrt=np.sqrt,
                rcp=lambda x: 1 / x, dlog=_ld_dlog, exp2=np.exp2)


def reference(fn, a, use_longdouble=None):
    """fn in LD_FUNCS at the doubles a, as numpy.longdouble: computed in long double where that has 64 bits, else by mpmath."""
    if HAVE_LONGDOUBLE if use_longdouble is None else use_longdouble:
        with np.errstate(all='ignore'):
            return LD_FUNCS[fn](_ld(a))
    return _mp(fn, a)
