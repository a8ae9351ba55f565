"""The numpy restatement of the HMC step kernel (tests/boxhmc_ref.py, DESIGN I.20) against posteriors known in closed form,
the reversibility of a trajectory with reflections, its L = 1 case against the MALA restatement, and the host pieces of
calibrate(method='hmc').  No device.

A statistical comparison is test_boxmala_host's z-score: (the chains' average of a quantity - its exact expectation) / its
standard error by the chains' own effective sample size.  The margin is 5."""
import numpy as np
import pytest

import boxhmc_ref as Hm
import boxmala_ref as M
import test_boxmala_host as H

MARGIN = 5.0
EPS = np.finfo(float).eps


def gain(w):
    from dgp_amd import calibrate
    return calibrate.gain(w, calibrate.TARGET_ACCEPT['hmc'])


def run_chains(fun, x0, w, ybar, lo, hi, s, seed, warmup, S, n_leapfrog=8, jitter=True, pv=None, pm=None):
    """R chains on calibrate's schedule, streams and trajectory lengths (P = 1): samples (R, S, D), the chains."""
    from dgp_amd import calibrate
    R, D = x0.shape
    z, logu = calibrate.Streams(seed, 1, R, D).block(1 + warmup + S)
    lengths = calibrate.trajectory_lengths(seed, warmup + S, n_leapfrog, jitter)
    chains = [Hm.sample(fun, x0[r], w, ybar, lo, hi, s, z[:, 0, r], logu[:, 0, r], lengths, warmup, 1, gain, pv, pm) for r in range(R)]
    assert all(c.calls == 1 + lengths.sum() for c in chains)
    return np.array([c.xs for c in chains]), chains


@pytest.mark.parametrize('D', [1, 2, 5])
def test_gaussian_posterior_well_inside_the_box(D):
    """test_boxmala_host's case: f(x) = A x, K = D + 1 outputs, a flat prior on a box 40 posterior standard deviations wide;
    the posterior is N(mu, Sigma).  4 chains of 1500 samples after 300 warm-up iterations, trajectories of 1 .. 8 steps;
    every mean, variance and covariance within 5 standard errors.  Observed (seed 11 + D), largest |z| over the means and
    over the second moments: D = 1: 0.16, 1.21; D = 2: 0.25, 1.18; D = 5: 1.23, 1.68; acceptance 0.73 .. 0.87."""
    rng = np.random.default_rng(100 + D)
    K = D + 1
    A = rng.normal(size=(K, D))
    w = rng.uniform(50.0, 200.0, K)
    ybar = A @ rng.uniform(-0.2, 0.2, D) + rng.normal(size=K) / np.sqrt(w)
    Sigma = np.linalg.inv(A.T @ (w[:, None] * A))
    mu = Sigma @ A.T @ (w * ybar)
    half = 20.0 * np.sqrt(np.diag(Sigma)).max() + np.abs(mu).max()
    lo, hi = np.full(D, -half), np.full(D, half)
    x0 = mu + rng.normal(size=(4, D)) * np.sqrt(np.diag(Sigma))
    xs, chains = run_chains(lambda x: (A @ x, A), x0, w, ybar, lo, hi, hi - lo, 11 + D, 300, 1500)
    assert all(c.status == Hm.OK and c.n_prop == 1800 for c in chains)
    zm = [H.zscore(xs[:, :, d], mu[d]) for d in range(D)]
    zc = [H.zscore((xs[:, :, a] - mu[a]) * (xs[:, :, b] - mu[b]), Sigma[a, b]) for a in range(D) for b in range(a, D)]
    print('D %d: acceptance %s, z of the means %s, of the second moments %s' %
          (D, np.round([c.n_acc / c.n_prop for c in chains], 2), np.round(zm, 2), np.round(zc, 2)))
    assert np.max(np.abs(zm)) <= MARGIN and np.max(np.abs(zc)) <= MARGIN


@pytest.mark.parametrize('m,sd,L', [(0.9, 0.3, 8), (0.8, 0.35, 8), (0.8, 0.35, 1)])
def test_truncated_normal_with_an_active_bound(m, sd, L):
    """f(x) = x on [0, 1]: a normal truncated by an active bound, against scipy.stats.truncnorm; N(0.8, 0.35^2) fills the box
    and the trajectories reflect at both walls.  4 chains of 2000 samples after 300 warm-up iterations, trajectories of
    1 .. L steps.  Observed z (seed 5) of the mean and the variance: (0.9, 0.3, 8): 3.23, -2.76 (seeds 20 .. 27 gave
    means' z of -2.47 .. 1.19 with both signs: no bias); (0.8, 0.35, 8): 1.52, -1.00; (0.8, 0.35, 1): 1.20, 1.03.  The chains reflected
    3488 .. 4505, 2402 .. 3599 and 919 .. 1107 times."""
    from scipy.stats import truncnorm
    exact = truncnorm((0.0 - m) / sd, (1.0 - m) / sd, loc=m, scale=sd)
    lo, hi = np.zeros(1), np.ones(1)
    x0 = np.array([[0.2], [0.5], [0.8], [0.95]])
    xs, chains = run_chains(lambda x: (x.copy(), np.eye(1)), x0, np.array([1.0 / sd ** 2]), np.array([m]), lo, hi, hi - lo, 5, 300, 2000, L)
    assert xs.min() >= 0.0 and xs.max() <= 1.0
    assert sum(c.reflections for c in chains) > 100
    zm, zv = H.zscore(xs[:, :, 0], exact.mean()), H.zscore((xs[:, :, 0] - exact.mean()) ** 2, exact.var())
    print('truncated normal %g %g L %d: acceptance %s, steps %s, reflections %s, z of the mean %.2f, of the variance %.2f' %
          (m, sd, L, np.round([c.n_acc / c.n_prop for c in chains], 2), np.round([c.h for c in chains], 3),
           [c.reflections for c in chains], zm, zv))
    assert abs(zm) <= MARGIN and abs(zv) <= MARGIN


def test_flat_likelihood_gives_the_uniform_distribution():
    """w = 0 (the one output is unobserved: its value and Jacobian hold NaN and are not read) and no prior: the samples
    are uniform on the box by reflection alone: the energy is conserved exactly, and the only rejections are trajectories
    that hit the reflection cap, up to which the warm-up raises the step (4.8 .. 5.0 box widths; acceptance 0.83).  Observed z
    (seed 9): means 2.30, 1.85; variances -0.33, -1.44."""
    lo, hi = np.array([-1.0, 0.0]), np.array([2.0, 1.0])
    x0 = np.random.default_rng(3).uniform(lo, hi, (4, 2))
    nan = lambda x: (np.full(1, np.nan), np.full((1, 2), np.nan))
    xs, chains = run_chains(nan, x0, np.zeros(1), np.full(1, np.nan), lo, hi, hi - lo, 9, 300, 2000)
    assert all(c.status == Hm.OK for c in chains) and np.all(xs >= lo) and np.all(xs <= hi)
    mid, var = 0.5 * (lo + hi), (hi - lo) ** 2 / 12.0
    zm = [H.zscore(xs[:, :, d], mid[d]) for d in range(2)]
    zv = [H.zscore((xs[:, :, d] - mid[d]) ** 2, var[d]) for d in range(2)]
    print('uniform: acceptance %s, steps %s, z of the means %s, of the variances %s' %
          (np.round([c.n_acc / c.n_prop for c in chains], 2), np.round([c.h for c in chains], 3), np.round(zm, 2), np.round(zv, 2)))
    assert np.max(np.abs(zm)) <= MARGIN and np.max(np.abs(zv)) <= MARGIN


# ------------------------------------------------------------------------------------------------ reversibility
def ref_trajectory(x, z, L, fun, args, h):
    """(end point y, end momentum p after the last half kick, logr, reflections) by the restatement."""
    ch = Hm.Chain(x, *args, h0=h)
    ch.step(*fun(ch.trial), z, 0.0, last=L == 1)
    for l in range(1, L + 1):
        end = ch.trial.copy()
        f, J = fun(end)
        if l == L:
            gt = ch.target(end, f, J)[1]
            p = ch.p + (0.5 * (h * ch.s)) * gt
            refl = ch.reflections
        ch.step(f, J, np.zeros(len(x)), 0.0, last=l == L)
    return end, p, ch.logr, refl


def reversal(L, seed, box=5.0, h=0.1, D=3, K=2):
    """A trajectory x -> x' of L steps from the momenta z, then from a fresh chain at x' the L steps from the negated end
    momenta: (the largest of |x'' - x| and |-p'' - z|, logr + logr', the reflections of the forward trajectory)."""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(size=(K, D)), rng.normal(size=K)
    fun = lambda x: (np.sin(a @ x + b), np.cos(a @ x + b)[:, None] * a)
    w, ybar, lo, hi, s = rng.uniform(1.0, 4.0, K), rng.normal(size=K), np.full(D, -box), np.full(D, box), rng.uniform(0.5, 2.0, D)
    x, z = rng.uniform(-1.0, 1.0, D) * min(box, 1.0), rng.normal(size=D)
    args = (w, ybar, lo, hi, s)
    x1, p1, r1, refl = ref_trajectory(x, z, L, fun, args, h)
    x2, p2, r2, back = ref_trajectory(x1, -p1, L, fun, args, h)
    assert back == refl                                     # a drift reflects as often backwards as forwards
    return float(max(np.max(np.abs(x2 - x)), np.max(np.abs(-p2 - z)))), float(r1 + r2), refl


@pytest.mark.parametrize('L', [1, 2, 5, 8])
@pytest.mark.parametrize('box', [5.0, 0.3])
def test_reversibility_of_a_trajectory(L, box):
    """From the end of a trajectory with the momenta negated, the same L steps return to the start (position and momenta)
    and the two log ratios sum to 0.  Measured here over seeds 0 .. 9: in the box of half-width 5 (one reflection in all) the
    return error was at most 1.4e-16, 6.7e-16, 5.6e-16, 6.8e-15 for L = 1, 2, 5, 8 and |logr + logr'| at most 4.4e-16,
    4.4e-16, 1.8e-15, 5.3e-15; in the box of half-width 0.3 (up to 1, 2, 4, 6 reflections per trajectory) 2.2e-16, 5.6e-16,
    1.2e-15, 4.3e-15 and 0, 8.9e-16, 1.8e-15, 8.0e-15.  The bounds are four times the largest: 2.8e-14 and 3.2e-14.  A
    backward trajectory reflects as often as its forward one in every case."""
    worst_x, worst_r, most = 0.0, 0.0, 0
    for seed in range(10):
        dx, dr, refl = reversal(L, seed, box)
        worst_x, worst_r, most = max(worst_x, dx), max(worst_r, abs(dr)), max(most, refl)
    print('L %d box %g: return error %.3g, |logr + logr\'| %.3g, reflections up to %d' % (L, box, worst_x, worst_r, most))
    assert worst_x <= 2.8e-14 and worst_r <= 3.2e-14
    assert most > 0 or box > 1.0


# ------------------------------------------------------------------------------------------------ L = 1 is MALA
def test_one_step_trajectories_are_mala():
    """With L = 1 the proposal is MALA's from the same state and z: x + h s (z + 0.5 h s g) against (x + 0.5 h^2 s^2 g) + h s z,
    a few roundings each on terms of size |x| + h s (|z| + h s |g|): within 4 eps of that (observed: 0.77 eps).  The log ratio
    at MALA's proposal agrees within 64 eps of |lp| + |lp'| + |z|^2 + |z'|^2, the sizes of the terms that either form sums
    (observed: 1.61 eps of it).  And on calibrate's schedule with MALA's gains the two chains make the same 60 decisions."""
    from dgp_amd import calibrate
    rng = np.random.default_rng(4)
    D, K = 3, 2
    a, b = rng.normal(size=(K, D)), rng.normal(size=K)
    fun = lambda x: (np.sin(a @ x + b), np.cos(a @ x + b)[:, None] * a)
    w, ybar, lo, hi, s = rng.uniform(20.0, 60.0, K), rng.normal(size=K) * 0.3, np.full(D, -2.0), np.full(D, 2.0), rng.uniform(0.5, 2.0, D)
    x0 = rng.uniform(-1.0, 1.0, D)
    z, logu = calibrate.Streams(3, 1, 1, D).block(61)
    z, logu = z[:, 0, 0], logu[:, 0, 0]
    mala = M.Chain(x0, w, ybar, lo, hi, s)
    hmc = Hm.Chain(x0, w, ybar, lo, hi, s)
    worst_x, worst_r = 0.0, 0.0
    for c in range(61):
        adapt = 1 <= c <= 30
        up, down = H.gain(c - 1) if adapt else (1.0, 1.0)
        mala.step(*fun(mala.trial), z[c], logu[c], adapt, up, down)
        hmc.step(*fun(hmc.trial), z[c], logu[c], True, adapt, up, down)
        assert not mala.flag and not hmc.bad and not hmc.reflections
        one = Hm.Chain(mala.x, w, ybar, lo, hi, s, h0=mala.h)                    # from MALA's state: one trajectory of one step
        one.step(*fun(mala.x), z[c], 0.0)
        size = np.abs(mala.x) + mala.h * s * (np.abs(z[c]) + mala.h * s * np.abs(mala.g))
        worst_x = max(worst_x, float(np.max(np.abs(mala.trial - one.trial) / size)))
        two = M.Chain(mala.x, w, ybar, lo, hi, s, h0=mala.h)
        two.step(*fun(mala.x), z[c], 0.0)
        assert np.array_equal(two.trial, mala.trial)
        one.trial = two.trial.copy()                                             # decide the same point
        one.step(*fun(one.trial), np.zeros(D), 0.0)
        two.step(*fun(two.trial), np.zeros(D), 0.0)
        back = ((mala.x - two.trial) - (0.5 * mala.h ** 2 * s * s) * one.target(two.trial, *fun(two.trial))[1]) / (mala.h * s)
        size = abs(mala.lp) + abs(one.target(two.trial, *fun(two.trial))[0]) + z[c] @ z[c] + back @ back
        worst_r = max(worst_r, abs(float(one.logr - two.logr)) / size)
    print('L = 1 against MALA: proposals within %.2f eps of their size, log ratios within %.2f eps of theirs; %d of 60 accepted'
          % (worst_x / EPS, worst_r / EPS, sum(hmc.accepts)))
    assert worst_x <= 4 * EPS and worst_r <= 64 * EPS
    assert mala.accepts == hmc.accepts and 10 < sum(hmc.accepts) < 60 and mala.h == hmc.h


# ------------------------------------------------------------------------------------------------ the restatement's edges
def test_the_restatements_edge_cases():
    """A start that is not finite: status NAN, the trial and every saved sample stay the start.  NaN in mid-trajectory: the
    trajectory is rejected with logr NaN, the calls in between evaluate x, and the chain stays live.  A step so large that
    the reflection cap is hit: logr -inf.  A fixed column and a column with s = 0 never move."""
    lo, hi, s = np.array([0.0, 0.0, 0.3]), np.array([1.0, 1.0, 0.3]), np.array([1.0, 0.0, 1.0])
    fun = lambda x: (x[:1].copy(), np.array([[1.0, 0.0, 0.0]]))
    x0 = np.array([0.5, 0.25, 0.3])
    bad = Hm.Chain(x0, np.ones(1), np.zeros(1), lo, hi, s)
    bad.step(np.full(1, np.nan), fun(x0)[1], np.zeros(3), 0.0, save=True)
    bad.step(*fun(bad.trial), np.ones(3), -np.inf, save=True)
    assert bad.status == Hm.NAN and bad.n_prop == 0 and np.array_equal(bad.trial, x0) and np.array_equal(bad.xs, [x0, x0])
    ch = Hm.Chain(x0, np.ones(1), np.zeros(1), lo, hi, s)
    ch.step(*fun(ch.trial), np.array([1.0, 1.0, 1.0]), 0.0, last=False)
    assert ch.trial[0] != x0[0] and np.array_equal(ch.trial[1:], x0[1:]) and np.array_equal(ch.p[1:], [0.0, 0.0])
    ch.step(np.full(1, np.nan), fun(x0)[1], np.zeros(3), 0.0, last=False)          # NaN in mid-trajectory
    assert ch.bad == Hm.NONFINITE and np.array_equal(ch.trial, x0)
    ch.step(*fun(ch.trial), np.zeros(3), 0.0, last=False)
    assert ch.bad == Hm.NONFINITE and np.array_equal(ch.trial, x0)
    ch.step(*fun(ch.trial), np.array([0.5, 0.0, 0.0]), -np.inf, last=True)
    assert np.isnan(ch.logr) and ch.n_prop == 1 and ch.n_acc == 0 and ch.status == Hm.OK and ch.bad == 0
    ch.step(*fun(ch.trial), np.zeros(3), -np.inf, last=True)
    assert ch.n_acc == 1 and np.array_equal(ch.x[1:], x0[1:]) and ch.x[0] != x0[0]
    big = Hm.Chain(x0, np.ones(1), np.zeros(1), lo, hi, s, h0=50.0)                # 50 box widths per unit momentum
    big.step(*fun(big.trial), np.array([1.0, 0.0, 0.0]), 0.0)
    assert big.bad == Hm.WALL and big.reflections == Hm.NREFL and np.array_equal(big.trial, x0)
    big.step(*fun(big.trial), np.array([0.001, 0.0, 0.0]), -np.inf)
    assert big.logr == -np.inf and big.n_acc == 0
    once = Hm.Chain(x0, np.zeros(1), np.zeros(1), lo, hi, s, h0=1.0)               # 0.5 + 0.7 = 1.2 -> 0.8, 0.5 + 1.7 = 2.2 -> -0.2 -> 0.2
    once.step(*fun(once.trial), np.array([0.7, 0.0, 0.0]), 0.0)
    assert once.reflections == 1 and abs(once.trial[0] - 0.8) < 1e-15 and once.p[0] == -0.7
    twice = Hm.Chain(x0, np.zeros(1), np.zeros(1), lo, hi, s, h0=1.0)
    twice.step(*fun(twice.trial), np.array([1.7, 0.0, 0.0]), 0.0)
    assert twice.reflections == 2 and abs(twice.trial[0] - 0.2) < 1e-15 and twice.p[0] == 1.7


def test_status_numbers_and_workspace_match_the_header():
    """Engine.BOXHMC carries the header's DGPAMD_BOXHMC_* status numbers and the restatement's, the reflection cap is the
    header's, and the workspace is x, g, g', p, lp and H0 as doubles and one int32 flag per chain (a host-side formula)."""
    import os
    import re
    from dgp_amd import _lib
    from dgp_amd.ops import Engine
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, 'include', 'dgp_amd.h')).read()
    header = {k.lower(): int(v) for k, v in re.findall(r'#define\s+DGPAMD_BOXHMC_([A-Z]+)\s+(\d+)', src)}
    count, nrefl = header.pop('count'), header.pop('nrefl')
    assert header == Engine.BOXHMC and sorted(header.values()) == list(range(count)) and nrefl == Hm.NREFL == 8
    assert (Engine.BOXHMC['ok'], Engine.BOXHMC['nan']) == (Hm.OK, Hm.NAN) and Engine.BOXMALA == dict(ok=0, nan=1)
    for Q, D in ((1, 1), (130, 5), (800, 64)):
        assert Engine.boxhmc_workspace(Q, D) == Q * (8 * (4 * D + 2) + 4)
    for Q, D in ((0, 5), (4, 0), (4, 65), (1 << 31, 5)):
        with pytest.raises(ValueError):
            Engine.boxhmc_workspace(Q, D)
    # the other host-side checks are exercised by tools/boxchain_args_check.cpp under the sanitizers
    assert _lib.lib.dgpamd_boxhmc_step(None, 1, 1, 1, *[None] * 6, 0.1, 1e-10, 1e2, 1.0, 1.0, 0, 1, 1, -1, 0, *[None] * 9) == _lib.BAD_ARG


# ------------------------------------------------------------------------------------------------ the host pieces
def test_trajectory_lengths_and_streams():
    """The jitter stream is a third child of the seed: it changes no z and no u; the lengths are uniform on 1 .. n_leapfrog,
    the same for equal seeds, and n_leapfrog without jitter.  The streams do not depend on the block size or on R."""
    from dgp_amd import calibrate
    a, b = np.random.SeedSequence(7).spawn(2), np.random.SeedSequence(7).spawn(3)
    assert [c.generate_state(4).tolist() for c in a] == [c.generate_state(4).tolist() for c in b[:2]]
    z, u = calibrate.Streams(7, 3, 4, 2).block(50)
    L = calibrate.trajectory_lengths(7, 4000, 8, True)
    z2, u2 = calibrate.Streams(7, 3, 4, 2).block(50)
    assert np.array_equal(z, z2) and np.array_equal(u, u2)
    assert L.shape == (4000,) and L.min() == 1 and L.max() == 8 and np.array_equal(L, calibrate.trajectory_lengths(7, 4000, 8, True))
    assert np.all(np.abs(np.bincount(L, minlength=9)[1:] - 500.0) < 5.0 * np.sqrt(500.0 * 7.0 / 8.0))
    assert not np.array_equal(L, calibrate.trajectory_lengths(8, 4000, 8, True))
    assert np.array_equal(calibrate.trajectory_lengths(7, 10, 5, False), np.full(10, 5))
    assert np.array_equal(calibrate.trajectory_lengths(7, 10, 1, True), np.ones(10))
    s = calibrate.Streams(7, 3, 4, 2)
    parts = [s.block(n) for n in (1, 7, 42)]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), z) and np.array_equal(np.concatenate([p[1] for p in parts]), u)
    zr, ur = calibrate.Streams(7, 3, 2, 2).block(50)
    assert np.array_equal(zr, z[:, :, :2]) and np.array_equal(ur, u[:, :, :2])


def test_driver_refusals_and_defaults():
    """An unknown method and n_leapfrog < 1 are refused before any device work (the engine here is None); target_accept None
    resolves to 0.574 for 'mala' and 0.8 for 'hmc', and the explicit refusals stay."""
    import inspect
    from dgp_amd import calibrate, pathfun
    box = np.array([[0.0, 1.0], [0.0, 1.0]])

    def call(**kw):
        return calibrate.calibrate(None, 3, 1, 2, None, None, 8, (0.1,), 0.1, box, **kw)
    for kw in (dict(method='nuts'), dict(method=None), dict(method='hmc', n_leapfrog=0), dict(n_leapfrog=-1),
               dict(method='hmc', target_accept=0.0), dict(method='hmc', target_accept=1.0), dict(method='hmc', step=0.0),
               dict(method='hmc', n_chains=0), dict(method='hmc', thin=0)):
        with pytest.raises(ValueError, match='calibrate'):
            call(**kw)
    assert calibrate.TARGET_ACCEPT == dict(mala=0.574, hmc=0.8)
    for method in ('mala', 'hmc'):                                               # None is resolved, not compared: the call
        with pytest.raises(AttributeError):                                      # gets as far as the engine, which is None here
            call(method=method, target_accept=None, x0=np.full((2, 2), 0.5))
    for f in (calibrate.calibrate, pathfun.PathFunctions.calibrate, pathfun.GpPaths.calibrate):
        par = inspect.signature(f).parameters
        assert list(par)[-4:] == ['target_accept', 'method', 'n_leapfrog', 'jitter']
        assert (par['target_accept'].default, par['method'].default, par['n_leapfrog'].default, par['jitter'].default) == (None, 'mala', 8, True)


def test_result_container_fields():
    from dgp_amd import calibrate
    x = np.random.default_rng(0).normal(size=(2, 3, 8, 1))
    args = (x, np.zeros((2, 3, 8)), np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 3), dtype=np.int32), x[:, :, 0], 9)
    old = calibrate.PathPosterior(*args)
    assert (old.method, old.n_leapfrog, old.evaluations, old.rounds) == ('mala', 1, 9, 9)
    new = calibrate.PathPosterior(*args[:-1], 40, 'hmc', 8, 40)
    assert (new.method, new.n_leapfrog, new.evaluations, new.rounds) == ('hmc', 8, 40, 40)
    assert new.rhat.shape == (2, 1) and new.pooled().shape == (48, 1)


def test_line_case_on_the_cpu():
    """tests/test_gpu_calibrate_hmc_model.py::test_line_gp_against_quadrature on the CPU: the restatement, driven by
    pathfun_ref and pathgrad_ref on the same draws, on calibrate's schedule, streams and trajectory lengths.  Per draw the
    mean and variance of 4 chains x 400 samples within 5 standard errors of quadrature on 4001 points.  Observed (seed 1): z of the
    means 1.12, 1.43, 0.51, 0.43, 2.02, -0.48, of the variances 0.62, -0.86, -0.60, -0.12, -2.34, -0.90; ess 933 .. 1372 of
    1600; acceptance 0.74 .. 0.86; split R-hat 0.9988 .. 1.0016, which sets the device test's RHAT_MAX = 1.016, ten times the
    largest distance from 1 seen here."""
    import test_gpu_calibrate_hmc_model as GH
    import test_gpu_calibrate_model as G
    from dgp_amd import calibrate
    L = GH.LINE
    funs, f_grid = G.line_case()
    w, ybar, lo, hi = np.array([1.0 / L['sd'] ** 2]), np.array([L['y']]), np.zeros(1), np.ones(1)
    lp_grid = -0.5 * w[0] * (ybar[0] - f_grid) ** 2                              # (J, 4001): the starts as calibrate picks them
    cand = G.GRID[::16][:, None]
    iterations = L['warmup'] + L['samples']
    z, logu = calibrate.Streams(1, L['J'], L['chains'], 1).block(1 + iterations)
    lengths = calibrate.trajectory_lengths(1, iterations, 8, True)
    zs, rhat, esses, rates = [], [], [], []
    for p, fun in enumerate(funs):
        x0 = cand[np.argsort(-lp_grid[p, ::16], kind='stable')[:L['chains']]]
        chains = [Hm.sample(fun, x0[r], w, ybar, lo, hi, hi - lo, z[:, p, r], logu[:, p, r], lengths, L['warmup'], 1, gain)
                  for r in range(L['chains'])]
        x = np.array([c.xs for c in chains])[:, :, 0]
        zs.append(G.against_the_grid(x, f_grid[p]))
        rhat.append(float(calibrate.split_rhat(x)))
        esses.append(float(calibrate.ess(x)))
        rates += [c.n_acc / c.n_prop for c in chains]
    print('line case on the CPU, hmc: z of the means %s, of the variances %s, rhat %s, ess %s of 1600, acceptance %.2f .. %.2f' %
          (np.round([a for a, _ in zs], 2), np.round([b for _, b in zs], 2), np.round(rhat, 4), np.round(esses), min(rates), max(rates)))
    assert np.max(np.abs(zs)) <= GH.MARGIN and max(rhat) < GH.RHAT_MAX
