"""The numpy restatement of tempered SMC (tests/boxsmc_ref.py, DESIGN I.21) against quadrature, the properties of its
resampling and bisection, ParticlePosterior's arithmetic, the refusals that need no device, the streams, and the margins
that the GPU tests rest on.  No device.

A statistical comparison here runs SEEDS = 16 seeds of R = 512 particles with 4 moves per stage and holds the seeds' average
to the exact value within 5 standard errors, sd / sqrt(16), sd the seeds' own spread."""
import numpy as np
import pytest

import boxmala_ref as M
import boxsmc_ref as S

SEEDS, R, MARGIN = 16, 512, 5.0


def gain(stage, rate):
    from dgp_amd import calibrate
    return calibrate.stage_gain(stage, rate, 0.574)


def run_seeds(fun, D, w, ybar, lo, hi, pv=None, pm=None, seeds=range(SEEDS), p=0, P=1, **kw):
    """smc on calibrate's streams and prior draws, one run per seed: the list of results."""
    from dgp_amd import calibrate
    out = []
    zero = np.zeros(D)
    for seed in seeds:
        streams = calibrate.SmcStreams(seed, P, R, D)
        x0 = calibrate.prior_draws(streams.prior_uniforms(), lo, hi, zero if pv is None else pv, zero if pm is None else pm)[p]
        out.append(S.smc(fun, x0, w, ybar, lo, hi, hi - lo, streams, gain, pv=pv, pm=pm, p=p, **kw))
    return out


def within(values, exact, what):
    values = np.asarray(values, dtype=np.float64)
    sd = values.std(ddof=1)
    z = (values.mean() - exact) / (sd / np.sqrt(len(values)))
    print('%s: mean %.5g, exact %.5g, per-seed sd %.3g, z %.2f' % (what, values.mean(), exact, sd, z))
    assert abs(z) <= MARGIN, what
    return sd


def bimodal_1d(x):
    t = x[:, 0]
    return ((2.0 * t - 1.0) ** 2 + 0.05 * np.sin(7.0 * t))[:, None], (4.0 * (2.0 * t - 1.0) + 0.35 * np.cos(7.0 * t))[:, None, None]


def bimodal_2d(x):
    f = 0.5 * np.sum((2.0 * x - 1.0) ** 2, 1) + 0.05 * np.sin(7.0 * x[:, 0])
    J = 2.0 * (2.0 * x - 1.0)
    J[:, 0] += 0.35 * np.cos(7.0 * x[:, 0])
    return f[:, None], J[:, None, :]


@pytest.mark.parametrize('case', ['1d', '2d', '1d-prior'])
def test_restatement_against_quadrature(case):
    """f(x) = (2 x - 1)^2 + 0.05 sin 7 x on [0, 1] (2-D: the mean of the squares), y = 0.49, sd = 0.02: two modes (2-D: a
    ring that the sine tilts); '1d-prior' adds the prior N(0.3, 0.3^2), which favours the left mode.  The seeds' average of
    log_evidence, of the mass of x_0 < 0.5 and of the particles' mean and variance within 5 standard errors of quadrature.
    Observed per-seed sd (log evidence, mass, mean of x_0, variance of x_0): 1d 0.129, 0.061, 0.042, 0.0030; 2d 0.082, 0.051,
    0.035, 0.0055; 1d-prior 0.106, 0.040, 0.028, 0.0143; 4, 3 and 4 stages; largest |z| 2.19."""
    D = 2 if case == '2d' else 1
    fun = bimodal_2d if D == 2 else bimodal_1d
    w, ybar, lo, hi = np.array([1.0 / 0.02 ** 2]), np.array([0.49]), np.zeros(D), np.ones(D)
    pv, pm = (np.array([1.0 / 0.3 ** 2]), np.array([0.3])) if case == '1d-prior' else (None, None)
    g = np.linspace(0.0, 1.0, 8001 if D == 1 else 801)
    axes = [g] * D
    mesh = np.stack(np.meshgrid(*axes, indexing='ij'), -1).reshape(-1, D)
    f_grid = fun(mesh)[0][:, 0]
    logz, mass = S.grid_evidence(f_grid, axes, ybar, w, pv, pm), S.grid_mass(f_grid, axes, ybar, w, 0.5, pv, pm)
    mean, cov = M.grid_posterior(f_grid, axes, ybar, w, pv, pm)
    res = run_seeds(fun, D, w, ybar, lo, hi, pv, pm)
    assert all(r['status'] == S.OK and r['betas'][-1] == 1.0 for r in res)
    print('%s: stages %s' % (case, [len(r['betas']) for r in res]))
    within([r['log_evidence'] for r in res], logz, 'log evidence')
    within([np.mean(r['x'][:, 0] < 0.5) for r in res], mass, 'mass of x_0 < 0.5')
    within([r['x'][:, 0].mean() for r in res], mean[0], 'mean of x_0')
    within([r['x'][:, 0].var() for r in res], cov[0, 0], 'variance of x_0')
    assert all(np.all(r['x'] >= lo) and np.all(r['x'] <= hi) for r in res)


def gp_on_the_cpu(case, XY, what):
    """16 seeds of the restatement on the numpy replay of the GPU model test's draws: per draw the seeds' average against
    quadrature within 5 standard errors; returns the per-seed standard deviations (draws, quantities)."""
    import test_gpu_calibrate_smc_model as G
    funs, f_grid = G.gp_case(*XY, case['seed'], case['J'], case['F'])
    ybar, w = G.obs(case)
    lo, hi = np.zeros(1), np.ones(1)
    sds = []
    for p in range(case['J']):
        res = run_seeds(funs[p], 1, w, ybar, lo, hi, seeds=range(SEEDS))
        assert all(r['status'] == S.OK for r in res)
        mean, cov = M.grid_posterior(f_grid[p], [G.GRID], ybar, w)
        exact = dict(logz=S.grid_evidence(f_grid[p], [G.GRID], ybar, w), mass=S.grid_mass(f_grid[p], [G.GRID], ybar, w, 0.5),
                     mean=mean[0], var=cov[0, 0])
        got = dict(logz=[r['log_evidence'] for r in res], mass=[np.mean(r['x'][:, 0] < 0.5) for r in res],
                   mean=[r['x'][:, 0].mean() for r in res], var=[r['x'][:, 0].var() for r in res])
        sd = {k: within(got[k], exact[k], 'draw %d %s' % (p, k)) for k in what}
        if 'mean' in sd:
            sd['mean'], sd['var'] = sd['mean'] / np.sqrt(cov[0, 0] / R), sd['var'] / (cov[0, 0] * np.sqrt(2.0 / R))
        sds.append([sd[k] for k in what])
    return np.array(sds)


def held(written, measured, what):
    print('%s: written %.4g, measured %.4g' % (what, written, measured))
    assert measured / 1.5 <= written <= measured * 1.5, what             # (the spread of 16 seeds is itself known to a fifth)


def test_line_gp_on_the_cpu():
    """The line gp of tests/test_gpu_calibrate_smc_model.py, its 6 draws replayed in numpy: log_evidence, mean and variance
    against quadrature, and the per-seed spread that the GPU test's bounds are: CPU['line_logz'], ['line_mean'],
    ['line_var'] there are the largest over the draws, held here to what 16 seeds can tell.  Measured: 0.0869, 1.32, 1.40."""
    import test_gpu_calibrate_model as C
    import test_gpu_calibrate_smc_model as G
    sds = gp_on_the_cpu(G.LINE, C.line(), ('logz', 'mean', 'var')).max(0)
    for k, v in zip(('line_logz', 'line_mean', 'line_var'), sds):
        held(G.CPU[k], v, k)


def test_bimodal_gp_on_the_cpu():
    """The bimodal gp of tests/test_gpu_calibrate_smc_model.py likewise: log_evidence and the mass of x < 0.5.  Measured: 0.141, 0.0737."""
    import test_gpu_calibrate_smc_model as G
    sds = gp_on_the_cpu(G.BIMODAL, G.bimodal(), ('logz', 'mass')).max(0)
    for k, v in zip(('bimodal_logz', 'bimodal_mass'), sds):
        held(G.CPU[k], v, k)


# ---------------------------------------------------------------------------------------------- resampling and bisection
def test_resampling_properties():
    rng = np.random.default_rng(5)
    for n in (1, 2, 7, 64, 513):
        a = rng.exponential(size=n) ** 3
        a[rng.uniform(size=n) < 0.3] = 0.0                                        # dead particles
        if not a.any():
            a[0] = 1.0
        W = a / a.sum()
        total = np.zeros(n)
        us = (np.arange(2000) + 0.5) / 2000
        for u in us:
            anc, counts = S.resample(a, u)
            assert counts.sum() == n and len(anc) == n and np.all(np.diff(anc) >= 0)
            assert np.all(counts >= np.floor(n * W)) and np.all(counts <= np.ceil(n * W) + 1)
            assert np.all(counts[a == 0.0] == 0)
            total += counts
        assert np.all(np.abs(total / len(us) - n * W) <= 1e-3 + 1e-9 * n)         # unbiased: the average over a grid of u
        assert np.array_equal(S.resample(np.ones(n), 0.37)[0], np.arange(n))     # equal weights: the identity


def test_bisection_brackets_the_target():
    rng = np.random.default_rng(6)
    for n, spread, beta in ((64, 1.0, 0.0), (64, 30.0, 0.0), (513, 3000.0, 0.2), (1000, 5.0, 0.9), (7, 100.0, 0.5)):
        ll = -3.0 + spread * rng.normal(size=n)
        ll[::5] = -np.inf
        d = S.choose_dbeta(ll, beta, 0.5)
        target = 0.5 * np.isfinite(ll).sum()
        assert 0.0 < d <= 1.0 - beta and S.ess(S.weights(ll, d)) >= target
        if d < 1.0 - beta:
            assert S.ess(S.weights(ll, d * (1.0 + 1e-9))) < target
        t = S.temper(ll, beta, 0.4, 0.5)
        assert t['dbeta'] == d and t['beta'] == (1.0 if d == 1.0 - beta else beta + d) and np.all(np.isfinite(ll[t['anc']]))
    assert S.choose_dbeta(np.full(5, -np.inf), 0.0, 0.5) == 0.0 and S.temper(np.full(5, np.nan), 0.0, 0.4, 0.5)['status'] == S.NAN
    assert S.temper(np.zeros(5), 1.0, 0.4, 0.5)['dbeta'] == 0.0


def test_the_gpu_operator_inputs_have_no_boundary_inside_the_margin():
    """tests/test_gpu_boxsmc.py compares anc with equality; that is sound where no boundary R C_i - u of the restatement lies
    within the margin of an integer.  The device evaluates at its own step of beta.  Where the full step clears the target
    by more than 1e-6 both take it.  Else both steps solve ESS = target, each within its ESS bound and the bracket's
    2^-52: they differ by at most rel = 2 ess_bound / |d log ESS / d log delta| + 2^-51 relative, the slope taken here by a
    difference quotient.  That moves weight j by rel delta d_j relative, the sum likewise, so a C_i by at most
    2 rel sum_j (a_j / S) delta d_j, and a boundary by R times as much: the margin checked here is the GPU test's plus that."""
    import test_gpu_boxsmc as T
    worst = np.inf
    for n in T.SIZES:
        for pat in T.PATTERNS:
            ll, beta, u, _ = T.temper_case(n, pat)
            t = S.temper(ll, beta, u, T.ESS_FRAC)
            d, live = t['dbeta'], np.isfinite(ll)
            if not d > 0.0 or n == 1:
                continue
            a = S.weights(ll, d)
            margin = T.anc_margin(n)
            target = T.ESS_FRAC * live.sum()                                     # (ESS >= 1 in any arithmetic: a target <= 1 is always met)
            if not (d == 1.0 - beta and (target <= 1.0 or S.ess(a) > target * (1.0 + 1e-6))):
                slope = (np.log(S.ess(S.weights(ll, d * (1.0 + 1e-4)))) - np.log(S.ess(a))) / 1e-4
                assert slope < -0.1, (n, pat, slope)
                rel = 2.0 * T.ess_bound(n) / abs(slope) + 2.0 ** -51
                margin += n * 2.0 * rel * np.sum(a[live] / a.sum() * d * (ll[live].max() - ll[live]))
            v = S.boundaries(a, u)[:-1]
            gap = np.abs(v - np.round(v))[live[:-1]]
            if pat == 'equal':
                assert np.all(np.abs(gap - min(u, 1.0 - u)) < 1e-9)               # (boundaries i + 1 - u: u lies in 0.05 .. 0.95)
            if gap.size:
                worst = min(worst, gap.min() / margin)
                assert gap.min() > margin, (n, pat, gap.min(), margin)
    print('the nearest boundary lies %.3g margins from an integer' % worst)


# -------------------------------------------------------------------------------------------------- the host side of the driver
def posterior(log_evidence, status, P=3, Rn=4):
    from dgp_amd import calibrate
    x = np.arange(P * Rn * 2, dtype=np.float64).reshape(P, Rn, 2)
    z = np.zeros((P, Rn))
    return calibrate.ParticlePosterior(x, z, z, np.asarray(log_evidence, dtype=np.float64), -1.5, np.ones((P, 1)), np.ones((P, 1)),
                                       np.ones((P, 1)), z + 0.1, np.asarray(status), 1, 5)


def test_particle_posterior_weights():
    res = posterior([np.log(1.0), np.log(3.0), np.nan], [0, 0, 1])
    W = res.draw_weights()
    assert np.allclose(W, [0.25, 0.75, 0.0], rtol=1e-15) and abs(res.draw_ess - 1.0 / (0.0625 + 0.5625)) < 1e-14
    assert np.allclose(res.pooled_weights(), np.repeat(W, 4) / 4) and np.allclose(res.pooled_weights('equal'), 1.0 / 12)
    assert res.pooled().shape == (12, 2) and res.per_draw().shape == (3, 4, 2)
    means = res.x.mean(1)
    s = res.summary(0.5, weights='evidence')
    assert np.allclose(s['mean'], 0.25 * means[0] + 0.75 * means[1])
    assert np.allclose(s['draw_sd'], np.sqrt(0.25 * (means[0] - s['mean']) ** 2 + 0.75 * (means[1] - s['mean']) ** 2))
    assert np.all(s['lower'] <= s['mean']) and np.all(s['upper'] <= res.x[1].max(0))     # (draw 2 has no weight)
    e = res.summary(0.5)
    assert np.allclose(e['mean'], res.pooled().mean(0)) and np.allclose(e['draw_sd'], means.std(0, ddof=1))
    drawn = res.resample(200, seed=1)
    assert drawn.shape == (200, 2) and drawn.max() <= res.x[1].max() and np.array_equal(drawn, res.resample(200, seed=1))
    assert res.resample(200, seed=1, weights='equal').max() == res.x.max()
    huge = posterior([-1e4, -1e4 + np.log(3.0), 0.0], [0, 0, 2])                 # (a draw with status max_stages has no weight)
    assert np.allclose(huge.draw_weights(), [0.25, 0.75, 0.0], rtol=1e-12)
    none = posterior([np.nan] * 3, [1, 1, 1])
    assert np.all(none.draw_weights() == 0.0) and none.draw_ess == 0.0
    with pytest.raises(ValueError):
        none.resample(3)
    with pytest.raises(ValueError):
        res.summary(1.0)
    with pytest.raises(ValueError):
        res.pooled_weights('other')


def test_log_norm_with_replicates_and_gaps():
    from dgp_amd import calibrate
    y = np.array([[0.1, 1.0], [0.3, np.nan], [np.nan, np.nan], [0.2, 2.0]])
    sd = np.array([0.1, 0.5])
    ybar, w = calibrate.observation(y, sd, 2)
    want = -0.5 * 3 * np.log(2 * np.pi * 0.01) - 0.5 * 2 * np.log(2 * np.pi * 0.25) \
        - 0.5 * ((0.1 - 0.2) ** 2 + (0.3 - 0.2) ** 2) / 0.01 - 0.5 * (0.5 ** 2 + 0.5 ** 2) / 0.25
    assert abs(calibrate.log_norm(y, sd, 2) - want) <= 1e-13 * abs(want)
    # with it the sufficient statistics give the full log density at any f
    f = np.array([0.27, 1.4])
    full = sum(-0.5 * np.log(2 * np.pi * sd[k] ** 2) - 0.5 * (y[t, k] - f[k]) ** 2 / sd[k] ** 2
               for t in range(4) for k in range(2) if np.isfinite(y[t, k]))
    assert abs(-0.5 * np.sum(w * (ybar - f) ** 2) + calibrate.log_norm(y, sd, 2) - full) <= 1e-12 * abs(full)
    assert abs(calibrate.log_norm(0.3, 0.1, 1) + 0.5 * np.log(2 * np.pi * 0.01)) <= 1e-15


def test_prior_draws():
    from scipy.stats import truncnorm
    from dgp_amd import calibrate
    lo, hi = np.array([0.0, -1.0, 2.0]), np.array([1.0, 3.0, 2.0])
    pv, pm = np.array([0.0, 4.0, 1.0]), np.array([0.0, 2.5, 0.0])
    u = (np.arange(4000) + 0.5)[:, None] / 4000 * np.ones(3)
    x = calibrate.prior_draws(u, lo, hi, pv, pm)
    assert np.all(x >= lo) and np.all(x <= hi) and np.all(x[:, 2] == 2.0) and np.allclose(x[:, 0], u[:, 0])
    exact = truncnorm((-1.0 - 2.5) / 0.5, (3.0 - 2.5) / 0.5, loc=2.5, scale=0.5)
    assert np.allclose(x[:, 1], exact.ppf(u[:, 1]), atol=1e-12)


def test_refusals_without_a_device():
    from dgp_amd import calibrate
    box = np.array([[0.0, 1.0], [0.0, 1.0]])
    args = (None, 3, 1, 2, None, None, 8)
    for kw in (dict(n_particles=0), dict(n_particles=calibrate.MAX_PARTICLES + 1), dict(n_moves=0), dict(ess_frac=0.0), dict(ess_frac=1.0),
               dict(ess_frac=float('nan')), dict(max_stages=0), dict(scale=np.ones(3)), dict(scale=np.array([1.0, -1.0])),
               dict(prior=(np.zeros(2), np.zeros(2))), dict(prior=np.zeros(2)), dict(step=0.0), dict(step=float('nan')),
               dict(target_accept=0.0)):
        with pytest.raises(ValueError):
            calibrate.calibrate_smc(*args, 0.1, 0.1, box, **kw)
    for y, sd, b in ((np.nan, 0.1, box), (0.1, 0.0, box), (np.zeros(2), 0.1, box), (0.1, 0.1, box[:, :1]), (0.1, 0.1, box[::-1, ::-1]),
                     (0.1, 0.1, np.array([[0.0, np.nan], [0.0, 1.0]]))):
        with pytest.raises(ValueError):
            calibrate.calibrate_smc(*args, y, sd, b)
    assert calibrate.MAX_PARTICLES == 8192 and calibrate.SMC_STATUS == dict(ok=0, nan=1, max_stages=2)


def test_the_streams_of_a_path_do_not_depend_on_P():
    from dgp_amd import calibrate
    big, small, more = calibrate.SmcStreams(11, 5, 7, 3), calibrate.SmcStreams(11, 2, 7, 3), calibrate.SmcStreams(11, 2, 9, 3)
    assert np.array_equal(big.prior_uniforms()[:2], small.prior_uniforms())
    assert np.array_equal(more.prior_uniforms()[:, :7], small.prior_uniforms())  # ... nor a slot's on the slots beside it
    seen = []
    for rounds in (4, 4, 2):
        (ub, zb, lb), (us, zs, ls), (um, zm, lm) = big.stage(rounds), small.stage(rounds), more.stage(rounds)
        assert zs.shape == (rounds, 2, 7, 3) and ls.shape == (rounds, 2, 7) and us.shape == (2,) and np.all(ls <= 0.0)
        assert np.array_equal(ub[:2], us) and np.array_equal(zb[:, :2], zs) and np.array_equal(lb[:, :2], ls)
        assert np.array_equal(um, us) and np.array_equal(zm[:, :, :7], zs) and np.array_equal(lm[:, :, :7], ls)
        seen.append(zs)
    assert not np.array_equal(seen[0], seen[1])                                  # a stage has numbers of its own
    a, c = calibrate.SmcStreams(None, 1, 2, 1), calibrate.SmcStreams(None, 1, 2, 1)
    assert not np.array_equal(a.prior_uniforms(), c.prior_uniforms())
    assert not np.array_equal(calibrate.SmcStreams(12, 2, 7, 3).prior_uniforms(), small.prior_uniforms())
    z = np.concatenate([calibrate.SmcStreams(s, 4, 8, 2).stage(5)[1].reshape(-1) for s in range(20)])
    assert abs(z.mean()) < 5.0 / np.sqrt(len(z)) and abs(z.var() - 1.0) < 5.0 * np.sqrt(2.0 / len(z))


def test_the_header_and_the_engine_agree():
    import os
    import re
    from dgp_amd.ops import Engine
    from test_cabi_symbols import ROOT, declared_functions
    src = open(os.path.join(ROOT, 'include', 'dgp_amd.h')).read()
    header = {k.lower(): int(v) for k, v in re.findall(r'#define\s+DGPAMD_BOXSMC_([A-Z_]+)\s+(\d+)', src)}
    assert header.pop('count') == 3 and header.pop('maxr') == Engine.BOXSMC_MAXR and header == Engine.BOXSMC
    assert {'dgpamd_boxsmc_move', 'dgpamd_boxsmc_temper', 'dgpamd_boxsmc_workspace'} <= set(declared_functions())
    from dgp_amd import _lib
    assert _lib.lib.dgpamd_boxsmc_workspace(3, 5, 2) == 15 * 36 and _lib.lib.dgpamd_boxsmc_workspace(1, 8193, 2) == 0
    assert _lib.lib.dgpamd_boxsmc_temper(None, 1, 1, 1, 0.5, *([None] * 11)) == _lib.BAD_ARG
