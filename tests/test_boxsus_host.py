"""The numpy restatement of subset simulation (tests/boxsus_ref.py, DESIGN I.22) against events of known probability, the
invariance of its move, the properties of its level step, FailureProbability's arithmetic, the streams, the refusals that need
no device, and the spreads that the GPU tests rest on.  No device.

A statistical comparison here runs SEEDS = 32 seeds of R = 1024 particles with 4 moves per stage at level_prob = 0.1 and holds
 - the seeds' average of ln P^ - ln p within 5 standard errors, sd / sqrt(32), sd the seeds' own spread;
 - that spread to at most 2 x cov(), Au and Beck's coefficient of variation without the chains' correlation, a lower bound
   of the true one (this is the condition that the two rejected designs of DESIGN I.22 fail: a step that is adapted from the
   acceptance rate alone gives 3.0, 1.2 and 0.29 against 0.23 at D = 1, 2, 5, a whole-vector walk 0.71 at D = 5);
 - the number of stages to at most ceil(log10(1 / p)) + 1."""
import math

import numpy as np
import pytest

import boxsus_ref as S

SEEDS, R, MARGIN, LEVEL_PROB = 32, 1024, 5.0, 0.1


def run_seeds(fun, threshold, D, lo, hi, pv=None, pm=None, seeds=range(SEEDS), p=0, P=1, n_particles=R, **kw):
    """sus on reliability's streams and calibrate's prior draws, one run per seed: the list of results."""
    from dgp_amd import calibrate, reliability
    out, zero = [], np.zeros(D)
    for seed in seeds:
        streams = reliability.SusStreams(seed, P, n_particles, D)
        x0 = calibrate.prior_draws(streams.prior_uniforms(), lo, hi, zero if pv is None else pv, zero if pm is None else pm)[p]
        out.append(S.sus(fun, x0, lo, hi, threshold, streams, reliability.n_survivors(LEVEL_PROB, n_particles), pv=pv, pm=pm, p=p, **kw))
    return out


def against_exact(res, exact, what):
    """The three conditions of the module's docstring; returns the seeds' sd of ln P^."""
    assert all(r['status'] == S.OK for r in res), what
    lp = np.log([r['prob'] for r in res])
    sd, cov = lp.std(ddof=1), np.mean([r['cov'] for r in res])
    z = (lp.mean() - math.log(exact)) / (sd / math.sqrt(len(lp)))
    stages = [len(r['levels']) for r in res]
    print('%s: exact %.4g, mean of P^ / p %.3f, mean of ln P^ - ln p %.4f (z %.2f), sd of ln P^ %.3f, cov() %.3f, stages %.2f (most %d)'
          % (what, exact, np.mean(np.exp(lp)) / exact, lp.mean() - math.log(exact), z, sd, cov, np.mean(stages), max(stages)))
    assert abs(z) <= MARGIN, what
    assert sd <= 2.0 * cov, what
    assert max(stages) <= math.ceil(math.log10(1.0 / exact) - 1e-9) + 1, what
    for r in res:
        assert r['levels'][-1] == 0.0 and np.all(np.diff(r['levels']) > 0.0) and np.all(r['score'] >= 0.0)
        assert r['prob'] == np.prod(r['cond_prob'])
    return sd


def held(written, measured, what):
    print('%s: written %.4g, measured %.4g' % (what, written, measured))
    assert measured / 1.5 <= written <= measured * 1.5, what             # (the spread of 32 seeds is itself known to an eighth)


# ------------------------------------------------------------------------------------------------- closed-form probabilities
@pytest.mark.parametrize('prob', [1e-3, 1e-6])
@pytest.mark.parametrize('D', [1, 2, 5])
def test_corner_event(D, prob):
    """sum x >= D - a under the uniform prior on [0, 1]^D: a^D / D!.  Measured sd of ln P^ (cov()), stages, at 1e-3:
    D = 1 0.164 (0.161) 3.5, D = 2 0.149 (0.162) 3.6, D = 5 0.169 (0.160) 3.3; at 1e-6: 0.267 (0.229) 6.4, 0.252 (0.229) 6.5,
    0.239 (0.227) 6.3; largest |z| 2.7 (D = 5, 1e-6: subset simulation is biased upwards by O(1 / R), here +0.12 in ln)."""
    import test_gpu_failure_probability_model as G
    fun, threshold, exact = S.corner(D, prob)
    sd = against_exact(run_seeds(fun, threshold, D, np.zeros(D), np.ones(D)), exact, 'corner D %d' % D)
    if (D, prob) == (5, 1e-6):
        held(G.CPU['corner5'], sd, 'corner5')


@pytest.mark.parametrize('D', [2, 5])
def test_halfspace_under_a_truncated_normal_prior(D):
    """sum x / sqrt(D) >= 3 under independent standard normals truncated at +-5: Phi(-3) = 1.35e-3; the truncation moves it
    by less than 2 D Phi(-5) / Phi(-3) = 2.1e-3 D relative, a twentieth of the standard error at D = 5.  Measured sd of ln P^
    (cov()): D = 2 0.166 (0.155), D = 5 0.158 (0.154); 3.1 and 3.0 stages."""
    import test_gpu_failure_probability_model as G
    fun, threshold, exact, (pv, pm), (lo, hi) = S.halfspace(D, 3.0)
    sd = against_exact(run_seeds(fun, threshold, D, lo, hi, pv, pm), exact, 'half-space D %d' % D)
    if D == 2:
        held(G.CPU['normal2'], sd, 'normal2')


def test_line_gp_on_the_cpu():
    """The line gp of tests/test_gpu_failure_probability_model.py, its 6 draws replayed in numpy, 16 seeds each: ln P^ against
    the measure of {f_p >= t} on GRID within 5 standard errors, the quadrature probabilities that the GPU test records, and
    the per-seed spread that its bound is: CPU['line'] there is the largest over the draws.  Measured: 0.114."""
    import test_gpu_calibrate_model as C
    import test_gpu_calibrate_smc_model as M
    import test_gpu_failure_probability_model as G
    funs, f_grid = M.gp_case(*C.line(), C.LINE['seed'], C.LINE['J'], C.LINE['F'])
    exact = np.array([S.grid_measure(f_grid[p], C.GRID, G.LINE_T) for p in range(6)])
    print('quadrature probabilities %s' % exact)
    assert np.allclose(exact, G.LINE_PROB, rtol=1e-6)
    assert np.all(exact >= 1e-4) and np.all(exact <= 0.5) and exact.min() < 1e-2
    sds = []
    for p in range(6):
        res = run_seeds(lambda x, p=p: funs[p](x)[0], G.LINE_T, 1, np.zeros(1), np.ones(1), seeds=range(16))
        assert all(r['status'] == S.OK for r in res)
        lp = np.log([r['prob'] for r in res])
        sd = lp.std(ddof=1)
        z = (lp.mean() - math.log(exact[p])) / (sd / 4.0)
        print('draw %d: quadrature %.4g, mean of ln P^ - ln p %.4f (z %.2f), sd %.3f, stages %s' %
              (p, exact[p], lp.mean() - math.log(exact[p]), z, sd, sorted(set(len(r['levels']) for r in res))))
        assert abs(z) <= MARGIN
        sds.append(sd)
    assert max(len(r['levels']) for r in res) > 1
    held(G.CPU['line'], max(sds), 'line')


# ------------------------------------------------------------------------------------------------------- MOVE's invariance
def moments_within(x, mean, var, what):
    """The sample's mean and variance against the exact ones within 5 standard errors of n independent samples, the fourth
    moment taken from the sample."""
    n = len(x)
    zm = (x.mean() - mean) / math.sqrt(var / n)
    m4 = np.mean((x - mean) ** 4)
    zv = (np.mean((x - mean) ** 2) - var) / math.sqrt((m4 - var * var) / n)
    print('%s: z of the mean %.2f, of the variance %.2f' % (what, zm, zv))
    assert abs(zm) <= MARGIN and abs(zv) <= MARGIN, what


def moved(x0, fun, level, lo, hi, pv=None, pm=None, moves=20, seed=0, lam=1.0):
    """x0 (n, D), drawn exactly from prior(x | f >= level), after `moves` moves of the restatement inside that level set."""
    n, D = x0.shape
    rng = np.random.default_rng(seed)
    pt = S.Particles(x0, n, lo, hi, 0.0, pv=pv, pm=pm)
    sd = x0.std(0)
    pt.move(fun(pt.trial), np.zeros((n, D)), np.zeros((n, D)), level, lam, sd, first=True, last=True)
    for i in range(moves + 1):
        pt.move(fun(pt.trial), rng.standard_normal((n, D)), np.log(rng.uniform(size=(n, D))), level, lam, sd, first=i == 0, last=i == moves)
    assert np.all(pt.score >= level) and np.all(pt.x >= lo) and np.all(pt.x <= hi)
    rate = pt.n_acc.sum() / pt.n_prop.sum()
    assert 0.2 < rate < 0.9 and np.mean(np.any(pt.x != x0, 1)) > 0.9, rate          # (the particles did move)
    return pt.x


def test_the_move_keeps_a_uniform_interval():
    n = 8192
    x0 = 0.7 + 0.3 * np.random.default_rng(1).uniform(size=(n, 1))
    x = moved(x0, lambda x: x[:, :1], 0.7, np.zeros(1), np.ones(1))
    moments_within(x[:, 0], 0.85, 0.09 / 12.0, 'U(0.7, 1)')


def test_the_move_keeps_a_normal_half_space():
    """x ~ N(0, I) on [-5, 5]^2 given s = (x_0 + x_1) / sqrt(2) >= 1.5: s is a standard normal truncated below, with mean
    lam = phi(b) / Phi(-b) and variance 1 + b lam - lam^2; t = (x_0 - x_1) / sqrt(2) stays N(0, 1).  (The box cuts off less
    than 1e-6 of the mass.)"""
    from scipy.special import ndtr, ndtri
    n, b = 8192, 1.5
    rng = np.random.default_rng(2)
    s = -ndtri(rng.uniform(size=n) * ndtr(-b))
    t = rng.standard_normal(n)
    x0 = np.stack([s + t, s - t], 1) / math.sqrt(2.0)
    x0 = x0[np.all(np.abs(x0) < 5.0, 1)]                                         # (given the box: a row outside it is dropped)
    assert len(x0) >= n - 4 and np.all(s >= b)
    fun = lambda x: ((x[:, 0] + x[:, 1]) / math.sqrt(2.0))[:, None]
    x = moved(x0, fun, b, np.full(2, -5.0), np.full(2, 5.0), np.ones(2), np.zeros(2))
    lam = math.exp(-0.5 * b * b) / math.sqrt(2.0 * math.pi) / ndtr(-b)
    moments_within((x[:, 0] + x[:, 1]) / math.sqrt(2.0), lam, 1.0 + b * lam - lam * lam, 'along the normal')
    moments_within((x[:, 0] - x[:, 1]) / math.sqrt(2.0), 0.0, 1.0, 'across it')
    assert len(x) == len(x0)


def test_the_move_keeps_a_corner():
    """x uniform on [0, 1]^5 given sum x >= 5 - a, a = 0.5: y = 1 - x is uniform on the simplex {y >= 0, sum y <= a},
    y = a E_1..5 / sum E_1..6 with E exponential: E y_d = a / 6, Var y_d = 5 a^2 / 252; sum y = a Beta(5, 1): mean 5 a / 6,
    variance 5 a^2 / 252."""
    n, a = 8192, 0.5
    e = np.random.default_rng(3).exponential(size=(n, 6))
    x0 = 1.0 - a * e[:, :5] / e.sum(1, keepdims=True)
    x = moved(x0, lambda x: x.sum(1)[:, None], 5.0 - a, np.zeros(5), np.ones(5))
    for d in range(5):
        moments_within(1.0 - x[:, d], a / 6.0, 5.0 * a * a / 252.0, 'corner column %d' % d)
    moments_within(5.0 - x.sum(1), 5.0 * a / 6.0, 5.0 * a * a / 252.0, 'corner sum')


# ------------------------------------------------------------------------------------------------------ LEVEL's properties
def test_level_properties():
    rng = np.random.default_rng(4)
    x = rng.normal(size=(10, 2))
    sd0 = np.array([0.3, 0.4])
    # b is the k-th largest, with ties; n_b counts the ties; ancestors cycle over the survivors in index order
    s = np.array([-5.0, -1.0, -3.0, -1.0, -2.0, -1.0, -0.5, -4.0, -1.0, -6.0])
    t = S.level(s, x, 0.5, sd0, 2, 1e-12)
    assert t['level'] == -1.0 and t['nsurv'] == 5 and not t['final'] and not t['done'] and t['running'] == 1
    assert np.array_equal(t['anc'], [1, 3, 5, 6, 8, 1, 3, 5, 6, 8]) and t['prob'] == 0.5 * (5.0 / 10.0) and t['status'] == S.OK
    surv = x[[1, 3, 5, 6, 8]]
    assert np.allclose(t['sd'], surv.std(0), rtol=1e-14)
    # the dead are never ancestors, and the divisor stays R
    s2 = s.copy()
    s2[[3, 6]] = np.nan
    t = S.level(s2, x, 1.0, sd0, 2, 1e-12)
    assert t['level'] == -1.0 and t['nsurv'] == 3 and np.array_equal(t['anc'][:4], [1, 5, 8, 1]) and t['prob'] == 3.0 / 10.0
    s3 = np.full(10, np.nan)
    s3[7] = -4.0                                                                 # fewer live particles than n_s: k = the live count
    t = S.level(s3, x, 1.0, sd0, 2, 1e-12)
    assert t['level'] == -4.0 and t['nsurv'] == 1 and np.all(t['anc'] == 7) and t['prob'] == 0.1
    assert np.array_equal(t['sd'], sd0)                                          # one survivor: a spread of 0 keeps the old one
    t = S.level(np.full(10, np.nan), x, 0.25, sd0, 2, 1e-12)
    assert t['status'] == S.NAN and np.isnan(t['prob']) and t['done'] and np.array_equal(t['anc'], np.arange(10)) and t['running'] == 0
    # the final stage sets the level to exactly +0; -0.0 counts as failing, the tiniest negative number does not
    s4 = np.array([0.3, -0.0, 0.0, -5e-324, 2.0, -1.0, -2.0, -3.0, -4.0, -5.0])
    t = S.level(s4, x, 0.01, sd0, 3, 1e-12)
    assert t['final'] and t['done'] and t['level'] == 0.0 and not np.signbit(t['level']) and t['nsurv'] == 4 and t['status'] == S.OK
    assert np.array_equal(t['anc'][:5], [0, 1, 2, 4, 0]) and t['prob'] == 0.01 * (4.0 / 10.0) and t['running'] == 0
    t = S.level(s4, x, 0.01, sd0, 5, 1e-12)                                      # the 5th largest is -5e-324: not final
    assert not t['final'] and t['level'] == -5e-324 and t['nsurv'] == 5
    assert np.array_equal(S.keys([-0.0]), S.keys([0.0])) and S.keys([-5e-324])[0] < S.keys([0.0])[0] < S.keys([5e-324])[0]
    k = S.keys([-np.inf, -1.0, -5e-324, 0.0, 1.0, np.inf, np.nan])
    assert np.all(np.diff(k[:6].astype(object)) > 0) and k[6] == 0 and k[0] > 0
    # below_min: the product falls under min_prob before the event is reached; a final stage is never below_min
    t = S.level(s, x, 1.5e-12, sd0, 2, 1e-12)
    assert t['status'] == S.BELOW_MIN and t['done'] and t['prob'] == 1.5e-12 * 0.5 and t['running'] == 0 and t['nsurv'] == 5
    t = S.level(s4, x, 1.5e-12, sd0, 3, 1e-12)
    assert t['status'] == S.OK and t['done'] and t['final']
    # an all-equal score keeps prob (n_b = R)
    t = S.level(np.full(10, -2.5), x, 0.125, sd0, 2, 1e-12)
    assert t['nsurv'] == 10 and t['prob'] == 0.125 and np.array_equal(t['anc'], np.arange(10)) and t['level'] == -2.5
    # a finished draw: the identity
    t = S.level(s, x, 0.125, sd0, 2, 1e-12, done=True, status=S.BELOW_MIN)
    assert t['level'] is None and t['prob'] == 0.125 and np.array_equal(t['anc'], np.arange(10)) and t['status'] == S.BELOW_MIN
    # +-inf are numbers
    s5 = np.array([np.inf, -np.inf, -1.0, -np.inf, -2.0, -np.inf, -np.inf, -np.inf, -np.inf, -np.inf])
    assert S.level(s5, x, 1.0, sd0, 4, 1e-12)['level'] == -np.inf and S.level(s5, x, 1.0, sd0, 4, 1e-12)['nsurv'] == 10
    assert S.level(s5, x, 1.0, sd0, 1, 1e-12)['final']


def test_the_sums_of_sd_follow_the_device_order():
    """wg_sum adds what a plain sum adds, in another order: equal up to rounding, and exactly for numbers whose sums are exact."""
    rng = np.random.default_rng(5)
    for n in (2, 63, 64, 65, 1000, 1025, 8192):
        v, mask = rng.normal(size=n), rng.uniform(size=n) < 0.6
        assert abs(S.wg_sum(v, mask) - v[mask].sum()) <= 4 * n * 2.0 ** -53 * np.abs(v[mask]).sum()
        k = rng.integers(-1000, 1000, n).astype(np.float64)
        assert S.wg_sum(k, mask) == k[mask].sum() and S.wg_sum(k, np.ones(n, dtype=bool)) == k.sum()
    assert S.n_threads(2) == 64 and S.n_threads(65) == 128 and S.n_threads(1000) == 1024 and S.n_threads(8192) == 1024


# -------------------------------------------------------------------------------------------------- the host side of the driver
def result(prob, cond, status, Rn=4):
    from dgp_amd import reliability
    P, Tn = np.shape(cond)
    x = np.zeros((P, Rn, 2))
    nan = np.full((P, Tn), np.nan)
    return reliability.FailureProbability(np.asarray(prob, dtype=np.float64), nan, np.asarray(cond, dtype=np.float64), nan, nan, x,
                                          np.zeros((P, Rn)), np.asarray(status), Tn, 5 * Tn)


def test_failure_probability_arithmetic():
    res = result([0.02, 0.25, np.nan, 1e-3], [[0.1, 0.2], [0.25, np.nan], [np.nan, np.nan], [0.1, 0.01]], [0, 0, 1, 3])
    assert np.allclose(res.log_prob[[0, 1, 3]], np.log([0.02, 0.25, 1e-3])) and np.isnan(res.log_prob[2])
    want = [math.sqrt(0.9 / (0.1 * 4) + 0.8 / (0.2 * 4)), math.sqrt(0.75 / (0.25 * 4)), np.nan, math.sqrt(0.9 / 0.4 + 0.99 / 0.04)]
    assert np.allclose(res.cov(), want, equal_nan=True, rtol=1e-15)
    s = res.summary(0.5)
    good = np.array([0.02, 0.25, 1e-3])
    assert s['mean'] == good.mean() and s['median'] == 0.02 and s['n_bounded'] == 1
    assert s['lower'] == np.quantile(good, 0.25) and s['upper'] == np.quantile(good, 0.75)
    assert s['mc_cov'] == np.median(np.array(want)[[0, 1, 3]])
    assert result([0.5, 0.1], [[0.5], [0.1]], [2, 3]).summary()['n_bounded'] == 2
    with pytest.raises(ValueError):
        res.summary(1.0)
    with pytest.raises(ValueError):
        result([np.nan], [[np.nan]], [1]).summary()
    assert res.cov()[1] == math.sqrt(0.75)                                       # one stage of c = 0.25, R = 4: plain Monte Carlo's


def test_refusals_without_a_device():
    from dgp_amd import reliability
    box = np.array([[0.0, 1.0], [0.0, 1.0]])
    args = (None, 3, 2, 2, None)
    for kw in (dict(n_particles=1), dict(n_particles=0), dict(n_particles=reliability.MAX_PARTICLES + 1), dict(level_prob=0.0),
               dict(level_prob=1.0), dict(level_prob=float('nan')), dict(level_prob=-0.1), dict(n_moves=0), dict(max_stages=0),
               dict(min_prob=1.0), dict(min_prob=-1e-3), dict(min_prob=float('nan')), dict(output=2), dict(output=-1),
               dict(prior=(np.zeros(2), np.zeros(2))), dict(prior=np.zeros(2)), dict(prior=(np.zeros(3), np.ones(3))),
               dict(step=0.0), dict(step=1e3), dict(step=float('nan')), dict(target_accept=0.0), dict(target_accept=1.0)):
        with pytest.raises(ValueError):
            reliability.failure_probability(*args, 0.5, box, **kw)
    for t, b in ((np.nan, box), (np.inf, box), (0.5, box[:, :1]), (0.5, box[::-1, ::-1]), (0.5, box[:1]),
                 (0.5, np.array([[0.0, np.nan], [0.0, 1.0]]))):
        with pytest.raises(ValueError):
            reliability.failure_probability(*args, t, b)
    assert reliability.MAX_PARTICLES == 8192 and reliability.STATUS == dict(ok=0, nan=1, max_stages=2, below_min=3)
    assert reliability.n_survivors(0.1, 1024) == 102 and reliability.n_survivors(0.1, 5) == 1 and reliability.n_survivors(0.999, 2) == 1
    assert (S.LAM_MIN, S.LAM_MAX) == (reliability.LAM_MIN, reliability.LAM_MAX)


def test_the_streams_of_a_path_do_not_depend_on_P_nor_a_slot_on_R():
    from dgp_amd import reliability
    big, small, more = reliability.SusStreams(11, 5, 7, 3), reliability.SusStreams(11, 2, 7, 3), reliability.SusStreams(11, 2, 9, 3)
    assert np.array_equal(big.prior_uniforms()[:2], small.prior_uniforms())
    assert np.array_equal(more.prior_uniforms()[:, :7], small.prior_uniforms())
    seen = []
    for _ in range(3):
        (zb, lb), (zs, ls), (zm, lm) = big.stage(4), small.stage(4), more.stage(4)
        assert zs.shape == (4, 2, 7, 3) and ls.shape == (4, 2, 7, 3) and np.all(ls <= 0.0)
        assert np.array_equal(zb[:, :2], zs) and np.array_equal(lb[:, :2], ls)
        assert np.array_equal(zm[:, :, :7], zs) and np.array_equal(lm[:, :, :7], ls)
        seen.append(zs)
    assert not np.array_equal(seen[0], seen[1])                                  # a stage has numbers of its own
    assert not np.array_equal(seen[0][:, 0], seen[0][:, 1])                      # and so has a path
    a, c = reliability.SusStreams(None, 1, 2, 1), reliability.SusStreams(None, 1, 2, 1)
    assert not np.array_equal(a.prior_uniforms(), c.prior_uniforms())
    assert not np.array_equal(reliability.SusStreams(12, 2, 7, 3).prior_uniforms(), small.prior_uniforms())
    z = np.concatenate([reliability.SusStreams(s, 4, 8, 2).stage(5)[0].reshape(-1) for s in range(20)])
    assert abs(z.mean()) < 5.0 / np.sqrt(len(z)) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / len(z))
    x0 = np.random.default_rng(0).uniform(size=(3, 50, 2))
    assert np.array_equal(reliability.prior_spread(x0), np.std(x0, axis=1))


def test_the_header_and_the_engine_agree():
    import os
    import re
    from dgp_amd import _lib
    from dgp_amd.ops import Engine
    from test_cabi_symbols import ROOT, declared_functions
    src = open(os.path.join(ROOT, 'include', 'dgp_amd.h')).read()
    header = {k.lower(): int(v) for k, v in re.findall(r'#define\s+DGPAMD_BOXSUS_([A-Z_]+)\s+(\d+)', src)}
    assert header.pop('count') == 4 and header.pop('maxr') == Engine.BOXSUS_MAXR and header == Engine.BOXSUS
    assert (S.OK, S.NAN, S.MAX_STAGES, S.BELOW_MIN) == tuple(Engine.BOXSUS[k] for k in ('ok', 'nan', 'max_stages', 'below_min'))
    assert {'dgpamd_boxsus_move', 'dgpamd_boxsus_level'} <= set(declared_functions())
    # a null context is refused first; the other host-side checks are exercised by tools/boxsus_args_check.cpp under the sanitizers
    assert _lib.lib.dgpamd_boxsus_level(None, 1, 2, 1, 1, 0.0, *([None] * 11)) == _lib.BAD_ARG
    assert _lib.lib.dgpamd_boxsus_move(None, 1, 2, 1, 1, 0, 1.0, 0.0, *([None] * 8), 0, 0, *([None] * 7)) == _lib.BAD_ARG
