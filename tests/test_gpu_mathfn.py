"""The library's hand-written device math functions, one by one, against extended-precision values (dgpamd_debug_mathfn).

exp_negated / exp_negated_v3 / exp_negated_tab (+ its two halves) of csrc/common.hpp, cos_reduced_impl of csrc/pathfun.hpp, rsqrt_f64 /
rcp_f64 / rsqrt_sqrt of csrc/diagfac.hpp, dlog_factor of csrc/pathfun.hpp and the integer tri_decode of csrc/common.hpp are what
every kernel matrix, Cholesky pivot, Vecchia row and function-valued draw goes through; the kernel tests see them only through
whole results at 1e-10 .. 1e-8.  Here each is evaluated on ~2 .. 4 million arguments (random ones from fixed seeds plus the
structured points where such code goes wrong: half-way points of the rounding of k, quadrant boundaries, word wraps, powers of
two, huge arguments, infinities, NaN) and held to a bound that follows from its operations; each bound's derivation is in the
test's docstring.  The reference is numpy.longdouble (tests/mathfn_ref.py; checked against mpmath at 40 digits by the one test here
that needs no GPU), or mpmath itself on a subset chosen by index where long double has fewer than 64 bits.

Limitation: the probe sees each function as compiled in the probe's own translation units (mathprobe.hip, and mathprobe_trig.hip
for the cosine, built with the flags of the files whose kernels call it).  The functions' arithmetic is explicit
fma, so the operations are those the hot kernels inline, but the instructions around them are not; the kernels themselves are held
to the same huge arguments by the *_beyond_the_exponent_range tests next to their well-scaled siblings.

No case is left out because a device value is large or not finite.  The only arguments outside an accuracy bound are x > 700 for
the exponentials and |a| >= 2^30 for the cosine; both have assertions of their own.  Every test prints the largest error it met and
where, before it asserts.  Needs an MI355X for all but the reference check: -m gpu."""
import ctypes as C
import functools

import numpy as np
import pytest

import mathfn_ref as R

gpu = pytest.mark.gpu
LD = np.longdouble
TWO30 = 2.0 ** 30


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def probe(eng, fn, a):
    out = eng.debug_mathfn(fn, eng.tensor(a))
    if isinstance(out, tuple):
        return tuple(o.cpu().numpy() for o in out)
    return out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def inputs(name):
    a, ns = getattr(R, name + '_inputs')()
    a.setflags(write=False)
    return a, ns


@functools.lru_cache(maxsize=None)
def reference(fn, name, negate=False):
    """(index, reference at a[index]): every input, or mathfn_ref.subset_index's where the reference has to be mpmath."""
    a, ns = inputs(name)
    idx = np.arange(len(a)) if R.HAVE_LONGDOUBLE else R.subset_index(len(a), ns)
    ref = R.reference(fn, -a[idx] if negate else a[idx])
    ref.setflags(write=False)
    return idx, ref


def bits(v):
    return np.ascontiguousarray(v).view(np.int64)


def worst(what, a, err, bound):
    """Print the largest of err and where; non-finite errors count as infinite (nothing is dropped)."""
    err = np.where(np.isfinite(err), err, np.inf).astype(np.float64)
    if len(err) == 0:
        print('%s: no points' % what)
        return
    i = int(np.argmax(err))
    print('%s: largest error %.3g (bound %.3g) at a = %r, over %d points' % (what, err[i], bound, float(a[i]), len(err)))
    assert err[i] <= bound, (what, float(a[i]), float(err[i]), bound)


def rel_err(dev, ref):
    with np.errstate(all='ignore'):
        return np.abs(dev.astype(LD) - ref) / np.abs(ref)


# ------------------------------------------------------------------------------------------------ the reference itself
def test_host_reference_agrees_with_mpmath():
    """numpy.longdouble's exp / cos / sin / sqrt / exp2 (and the rational dlog expression) against mpmath at 40 digits, to 1e-18
    relative (absolute for cos / sin, whose values pass through zero), on 2000 points per function: the named edges of every input
    set, a stride through its structured points, and random ones."""
    mpmath = pytest.importorskip('mpmath')
    assert R.HAVE_LONGDOUBLE, 'long double has fewer than 64 bits here: the GPU tests take mpmath itself as their reference'

    def sample(name, edges):
        a, ns = inputs(name)
        edges = np.asarray(edges, dtype=np.float64)
        k = (2000 - len(edges)) // 2
        return np.concatenate((edges, a[:ns][:: max(ns // k, 1)][:k], a[ns:][:: (len(a) - ns) // k][:k]))

    big = R.BIG
    two39 = float(LD(2.0 ** 39) * R.LN2 / 256)
    wraps = [float(j * LD(2.0 ** 31) * R.LN2 / d) for d in (1, 256) for j in range(1, 9)]
    below = np.nextafter(TWO30, 0.0)
    cases = [('expn', 'exp', np.concatenate(([0.0, -0.0, two39], wraps, big)), False),
             ('expn', 'exp_tab', np.concatenate(([0.0, -0.0, two39], wraps, big)), False),
             ('cos', 'cos', [0.0, -0.0, below, -below, TWO30, -TWO30, 1e300, np.inf, -np.inf, np.nan], True),
             ('msin', 'cos', [0.0, -0.0, below, -below, TWO30, -TWO30, 1e300, np.inf, -np.inf, np.nan], True),
             ('rsqrt', 'root', [1e-290, 1e290, 1.0, 2.0, 4.0], False),
             ('sqrt', 'root', [1e-290, 1e290, 1.0, 2.0, 4.0], False),
             ('rcp', 'root', [1e-290, 1e290, -1e-290, -1e290, 1.0, -1.0], False),
             ('dlog', 'dlog', [0.0, -0.0, 1e-300, -1e-300, 1e100, -1e100, 50.0, -50.0], False)]
    with mpmath.workdps(40):
        for fn, name, edges, absolute in cases:
            a = sample(name, edges)
            assert len(a) <= 2000
            got = R.reference(fn, a, use_longdouble=True)
            top = mpmath.mpf(0)
            for x, g in zip(a.tolist(), got):
                if np.isnan(x) or (np.isinf(x) and fn != 'expn'):
                    assert np.isnan(g), (fn, x, g)
                    continue
                if np.isinf(x):
                    assert g == 0.0, (fn, x, g)
                    continue
                want = R.MP_FUNCS[fn](mpmath.mpf(x))
                if fn == 'expn' and want < mpmath.ldexp(1, -16445):   # (below long double's smallest number)
                    assert g == 0.0, (fn, x, g)
                    continue
                err = abs(R.ld_to_mp(g) - want)
                if not absolute and want != 0:
                    err /= abs(want)
                top = max(top, err)
                assert err <= mpmath.mpf('1e-18'), (fn, x, g, want)
            print('%s on %s: %d points, largest error %s' % (fn, name, len(a), mpmath.nstr(top, 3)))
        j = np.arange(256.0)
        tab = R.reference('exp2', j / 256, use_longdouble=True)
        for x, g in zip(j.tolist(), tab):
            assert abs(R.ld_to_mp(g) / mpmath.power(2, mpmath.mpf(x) / 256) - 1) <= mpmath.mpf('1e-18')


def test_tri_reference_is_the_enumeration():
    t = np.array([0, 1, 2, 3, 5, 6, 2147450879, 2147450880, 2 ** 31 - 1], dtype=np.int64)
    t = np.concatenate((np.arange(1 << 22, dtype=np.int64), t[6:]))
    bi, bj = R.tri_reference(t)
    assert list(zip(bi[:7], bj[:7])) == [(0, 0), (1, 0), (1, 1), (2, 0), (2, 1), (2, 2), (3, 0)]
    assert list(zip(bi[-3:], bj[-3:])) == [(65534, 65534), (65535, 0), (65535, 32767)]


# ------------------------------------------------------------------------------------------------ exponentials
def check_exponential(eng, fn, name, bound):
    a, _ = inputs(name)
    idx, ref = reference('expn', name)
    dev = probe(eng, fn, a)
    x, d = a[idx], dev[idx]
    inside = x <= 700.0                      # (false for NaN)
    worst('%s on [-1.1, 700], relative' % fn, x[inside], rel_err(d[inside], ref[inside]), bound)
    beyond = a >= 700.0
    out = np.flatnonzero(beyond & ~((dev >= 0.0) & (dev <= 1.1e-304)))
    print('%s on [700, inf]: %d of %d values outside [0, 1.1e-304]; largest value inside %.3g' % (
        fn, len(out), beyond.sum(), np.max(np.where(beyond & (dev <= 1.1e-304), dev, 0.0))))
    assert len(out) == 0, (fn, 'first and last offenders (a, value)', a[out[:8]], dev[out[:8]], a[out[-8:]], dev[out[-8:]])
    nan = np.isnan(a)
    assert nan.any() and np.all(np.isnan(dev[nan])), (fn, dev[nan])
    assert np.count_nonzero(inside) + np.count_nonzero(beyond[idx]) + np.count_nonzero(nan[idx]) >= len(idx)   # nothing left out
    return dev


@gpu
@pytest.mark.parametrize('fn', ['exp_negated', 'exp_negated_v3'])
def test_exp_negated(eng, fn):
    """exp(-x), k = round(-x / ln 2), degree-12 Taylor polynomial in r = -x - k ln 2, |r| <= ln 2 / 2.
    x <= 700: relative error <= 4e-16 -- truncation (ln 2 / 2)^13 / 13! = 1.7e-16, the error of r 0.4e-16, the last three Horner
    roundings weighted 1, |r|, r^2 / 2: 1.6e-16; together 3.7e-16.
    x >= 700 up to DBL_MAX and +inf: 0 <= f(x) <= 1.1e-304 (the design's "~1e-308 instead of 0", widened to exp(-700) for the
    stretch before the clamp bites).  f(NaN) is NaN."""
    check_exponential(eng, fn, 'exp', 4e-16)


@gpu
@pytest.mark.parametrize('fn', ['exp_negated_tab', 'exp_negated_tab2'])
def test_exp_negated_tab(eng, fn):
    """exp(-x) = 2^e tab[j] exp(r), k = round(-256 x / ln 2) = 256 e + j, degree-4 polynomial, |r| <= ln 2 / 512 (tab2: the
    _begin / _end halves).  x <= 700: relative error <= 5e-16 -- truncation 3.8e-17, the last Horner step 2^-53, the table entry
    (1 ulp of the library's exp2) 2^-52, the product 2^-53: 4.8e-16.  Beyond 700 and at NaN as test_exp_negated.  The inputs hold
    the points where the low word of k wraps (j 2^31 ln 2 / 256, from 5.8e6) and where k leaves 39 bits (1.4886e9)."""
    check_exponential(eng, fn, 'exp_tab', 5e-16)


@gpu
def test_exp_table_entries(eng):
    """tab[j] = exp2(j / 256) as the kernels build it in LDS: within 2^-52 relative (1 ulp) of 2^(j/256); tab[0] is exactly 1."""
    j = np.arange(256.0)
    dev = probe(eng, 'exp_table', j)
    ref = R.reference('exp2', j / 256)
    worst('table entries, relative', j, rel_err(dev, ref), 2.0 ** -52)
    assert dev[0] == 1.0


@gpu
def test_exponential_forms_agree_bit_for_bit(eng):
    """exp_negated_v3 is exp_negated with pinned instructions, exp_negated_tab_begin / _end is exp_negated_tab in two halves: the same
    operations, so the same bits on every input of both input sets (huge, infinite and NaN ones included)."""
    for name in ('exp', 'exp_tab'):
        a, _ = inputs(name)
        for f, g in (('exp_negated', 'exp_negated_v3'), ('exp_negated_tab', 'exp_negated_tab2')):
            u, v = probe(eng, f, a), probe(eng, g, a)
            diff = np.flatnonzero(bits(u) != bits(v))
            print('%s vs %s on the %s set: %d of %d differ' % (f, g, name, len(diff), len(a)))
            assert len(diff) == 0, (f, g, a[diff[:5]], u[diff[:5]], v[diff[:5]])


# ------------------------------------------------------------------------------------------------ cosine / sine
@gpu
def test_cos_reduced(eng):
    """cos(a) = (-1)^k sin(r), -sin(a) = (-1)^k cos(r), r = a - (k - 1/2) pi by two fused multiply-adds against pi = PI_HI + PI_LO.
    |a| < 2^30: absolute error <= 4e-16 -- the two reduction roundings, each <= ulp(pi / 2) / 2 = 1.1e-16, the final rounding
    1.1e-16, truncation 1.3e-18 (cosine) / 3e-22 (sine).  The inputs hold the doubles around k pi / 2 for |k| <= 200 000 and for the
    1000 largest k with k pi / 2 < 2^30 (where r is all cancellation), and the quadrant bit is checked by every one of them.
    |a| >= 2^30, +-inf, NaN: the library branch -- within 1 ulp of 1 (2.2e-16) of the device library's cos and -sin (torch's, the
    same functions), NaN at +-inf and NaN.  The distance of those values from the extended-precision ones is printed, not bounded:
    it is the library's accuracy, not this code's.
    The branch depends on how its file is built: under -ffp-contract=fast the backend fuses the multiply-adds inside the math
    library's large-argument reduction too, and cos_reduced(1e300) was 0.985380856789356 for -0.5753861119575491 (1.56 against this
    bound).  The files that hold the branch are built with fast-honor-pragmas (csrc/Makefile), the probe's cosine cases among them.
    The cosine of the WITH_SIN instantiation is the plain one's bit for bit."""
    import torch
    a, _ = inputs('cos')
    c0 = probe(eng, 'cos_reduced', a)
    c1, ms = probe(eng, 'cos_sin_reduced', a)
    diff = np.flatnonzero(bits(c0) != bits(c1))
    print('cos_reduced_impl<true> vs <false>: %d of %d cosines differ' % (len(diff), len(a)))
    assert len(diff) == 0, (a[diff[:5]], c0[diff[:5]], c1[diff[:5]])
    nonfinite = ~np.isfinite(a)
    assert nonfinite.sum() == 3 and np.all(np.isnan(c0[nonfinite])) and np.all(np.isnan(ms[nonfinite])), (c0[nonfinite], ms[nonfinite])
    for fn, dev in (('cos', c0), ('msin', ms)):
        idx, ref = reference(fn, 'cos')
        x, d = a[idx], dev[idx]
        small, large = np.abs(x) < TWO30, np.isfinite(x) & (np.abs(x) >= TWO30)
        assert small.sum() + large.sum() + nonfinite[idx].sum() == len(idx)
        worst('%s for |a| < 2^30, absolute' % fn, x[small], np.abs(d[small].astype(LD) - ref[small]), 4e-16)
        assert large.sum() == 3
        al = x[large]
        lib = (torch.cos(eng.tensor(al)) if fn == 'cos' else -torch.sin(eng.tensor(al))).cpu().numpy()
        print('%s for |a| >= 2^30: a %r, values %r, the device library\'s %r, distance from the extended-precision values %r' % (
            fn, al.tolist(), d[large].tolist(), lib.tolist(), np.abs(d[large].astype(LD) - ref[large]).astype(float).tolist()))
        worst('%s for |a| >= 2^30 (library branch) against the device library, absolute' % fn, al, np.abs(d[large] - lib), 2.0 ** -52)


# ------------------------------------------------------------------------------------------------ roots and reciprocals
@gpu
def test_rsqrt_f64(eng):
    """1 / sqrt(d), Goldschmidt (g, h) from v_rsq_f64: relative error <= 5e-16.  Two quadratically convergent rounds from a hardware
    estimate good to 2^-14 leave less than 1e-20 of its error; what remains is the half-weighted roundings of g and h plus the final
    roundings, about 3.5e-16."""
    a, _ = inputs('root')
    idx, ref = reference('rsqrt', 'root')
    worst('rsqrt_f64, relative', a[idx], rel_err(probe(eng, 'rsqrt', a)[idx], ref), 5e-16)


@gpu
def test_rsqrt_sqrt(eng):
    """1 / sqrt(d) and sqrt(d), two Newton rounds on v_rsq_f64 and one correction of the root: relative error of both <= 5e-16, by
    test_rsqrt_f64's argument (the estimate's error squared twice is gone; the last round's half-weighted roundings and the final
    ones remain, about 3.5e-16)."""
    a, _ = inputs('root')
    inv, sd = probe(eng, 'rsqrt_sqrt', a)
    idx, ref = reference('rsqrt', 'root')
    worst('rsqrt_sqrt inv, relative', a[idx], rel_err(inv[idx], ref), 5e-16)
    idx, ref = reference('sqrt', 'root')
    worst('rsqrt_sqrt sd, relative', a[idx], rel_err(sd[idx], ref), 5e-16)


@gpu
def test_rcp_f64(eng):
    """1 / d, two Newton rounds on v_rcp_f64, on the input set and on its negation: relative error <= 5e-16 (the estimate's 2^-14
    squared twice is below 1e-20; the last residual's and the final roundings remain, about 3.5e-16 at most)."""
    a, _ = inputs('root')
    idx, ref = reference('rcp', 'root')
    worst('rcp_f64, relative', a[idx], rel_err(probe(eng, 'rcp', a)[idx], ref), 5e-16)
    idx, ref = reference('rcp', 'root', True)
    worst('rcp_f64 of negative arguments, relative', -a[idx], rel_err(probe(eng, 'rcp', -a)[idx], ref), 5e-16)


# ------------------------------------------------------------------------------------------------ dlog_factor
@gpu
def test_dlog_factor(eng):
    """q(t) = d log(factor) / dt.  matern2.5: -(5/3) t (1 + sqrt5 |t|) / (1 + sqrt5 |t| + (5/3) t^2) within 1e-15 relative -- nine
    roundings of 2^-53 (the two constants, the two fused polynomials' three, the reciprocal's, the three products'): 1e-15 -- and
    exactly -+0 at +-0 (the sign of -(5/3) t).  sexp: exactly -2 t."""
    a, _ = inputs('dlog')
    dev = probe(eng, 'dlog_matern25', a)
    idx, ref = reference('dlog', 'dlog')
    x, d = a[idx], dev[idx]
    nz = x != 0.0
    worst('dlog_factor<matern2.5>, relative', x[nz], rel_err(d[nz], ref[nz]), 1e-15)
    zero = a == 0.0
    assert zero.sum() == 2 and np.all(dev[zero] == 0.0), (a[zero], dev[zero])
    assert np.array_equal(np.signbit(dev[zero]), ~np.signbit(a[zero])), (a[zero], dev[zero])   # (-(5/3) t ...: -0 at +0, +0 at -0)
    dev = probe(eng, 'dlog_sexp', a)
    assert np.array_equal(bits(dev), bits(-2.0 * a))


# ------------------------------------------------------------------------------------------------ tri_decode
@gpu
def test_tri_decode(eng):
    """t -> (bi, bj), t = bi (bi + 1) / 2 + bj: exact for every t below 2^22 and for the 1000 largest below 2^31 (bi = 65535, where
    32-bit products of bi + 1 and bi + 2 no longer fit)."""
    t = R.tri_inputs()
    bi, bj = R.tri_reference(t)
    di, dj = probe(eng, 'tri_decode', t.astype(np.float64))
    bad = np.flatnonzero((di != bi) | (dj != bj))
    print('tri_decode: %d of %d wrong' % (len(bad), len(t)))
    assert len(bad) == 0, (t[bad[:5]], di[bad[:5]], dj[bad[:5]], bi[bad[:5]], bj[bad[:5]])


# ------------------------------------------------------------------------------------------------ arguments
@gpu
def test_bad_arguments(eng):
    import torch
    from dgp_amd._lib import lib
    a = eng.tensor(np.ones(4))
    o0, o1 = eng.empty(4), eng.empty(4)
    p = lambda t: C.c_void_p(t.data_ptr())
    assert lib.dgpamd_debug_mathfn(eng.h, 0, 4, p(a), p(o0), None) == 0
    for fn, count, pa, p0, p1 in ((13, 4, p(a), p(o0), p(o1)), (-1, 4, p(a), p(o0), p(o1)), (0, 0, p(a), p(o0), None),
                                  (0, -4, p(a), p(o0), None), (0, 4, None, p(o0), None), (0, 4, p(a), None, None),
                                  (7, 4, p(a), p(o0), None)):
        assert lib.dgpamd_debug_mathfn(eng.h, fn, count, pa, p0, p1) == 2, (fn, count)
    torch.cuda.synchronize()
    assert np.all(np.abs(o0.cpu().numpy() - np.exp(-1.0)) <= 4e-16 * np.exp(-1.0))   # (the refused calls wrote nothing)
