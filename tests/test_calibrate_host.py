"""The host side of calibrate (dgp_amd/calibrate.py, DESIGN I.19): the diagnostics against series with known answers, the
result's containers, the driver's refusals that need no device, and the invariances of the random streams.  No device."""
import numpy as np
import pytest

import boxmala_ref as M

SEEDS = range(20)


def ar1(rho, seed, R=4, S=5000):
    rng = np.random.default_rng(100 + seed)
    e = rng.normal(size=(R, S))
    x = np.empty_like(e)
    x[:, 0] = e[:, 0] / np.sqrt(1.0 - rho * rho)
    for t in range(1, S):
        x[:, t] = rho * x[:, t - 1] + e[:, t]
    return x


def test_rhat_on_iid_and_on_shifted_chains():
    """4 iid normal chains of 1000 samples, seeds 0 .. 19: split R-hat lay in 0.99918 .. 1.00104, mean 0.99999, standard
    deviation 0.00055.  The threshold for 'mixed' is the mean plus nine of those deviations, 1.005.  With the fourth chain's
    mean shifted by one standard deviation it lay in 1.093 .. 1.120: clearly above."""
    from dgp_amd import calibrate
    for seed in SEEDS:
        x = np.random.default_rng(seed).normal(size=(4, 1000))
        assert abs(float(calibrate.split_rhat(x)) - 1.0) < 0.005
        assert float(calibrate.split_rhat(x + np.array([0.0, 0.0, 0.0, 1.0])[:, None])) > 1.05
    stacked = np.random.default_rng(0).normal(size=(3, 2, 4, 1000))
    assert calibrate.split_rhat(stacked).shape == (3, 2)
    assert np.isnan(calibrate.split_rhat(np.ones((4, 10))))                      # chains that do not move
    with pytest.raises(ValueError):
        calibrate.split_rhat(np.zeros((4, 3)))


@pytest.mark.parametrize('rho,spread', [(0.0, 0.0962), (0.5, 0.1302), (0.9, 0.1645)])
def test_ess_of_ar1_series(rho, spread):
    """4 stationary AR(1) chains of 5000 samples against n (1 - rho) / (1 + rho), n = 20000.  Over seeds 0 .. 19 the largest
    |ess / closed form - 1| seen was 0.0962 (rho 0), 0.1302 (rho 0.5), 0.1645 (rho 0.9); the margin is twice that."""
    from dgp_amd import calibrate
    worst = 0.0
    for seed in SEEDS:
        worst = max(worst, abs(float(calibrate.ess(ar1(rho, seed))) / M.ar1_ess(rho, 20000) - 1.0))
    print('rho %.1f: largest |ratio - 1| %.4f' % (rho, worst))
    assert worst <= 2.0 * spread


def test_ess_shapes_and_still_chains():
    from dgp_amd import calibrate
    x = np.random.default_rng(1).normal(size=(2, 3, 4, 200))
    assert calibrate.ess(x).shape == (2, 3) and np.all(calibrate.ess(x) > 200)
    assert np.isnan(calibrate.ess(np.ones((4, 50))))
    one = calibrate.ess(ar1(0.5, 3, R=1))                                        # one chain: no between-chain term
    assert 0.7 < float(one) / M.ar1_ess(0.5, 5000) < 1.3
    with pytest.raises(ValueError):
        calibrate.ess(np.zeros((4, 3)))


def test_result_containers():
    from dgp_amd import calibrate
    P, R, S, Dx = 3, 4, 50, 2
    rng = np.random.default_rng(2)
    x = rng.normal(size=(P, R, S, Dx)) + np.arange(P)[:, None, None, None]
    res = calibrate.PathPosterior(x, rng.normal(size=(P, R, S)), np.full((P, R), 0.5), np.full((P, R), 0.1), np.zeros((P, R), dtype=np.int32),
                                  x[:, :, 0], 1 + S)
    assert res.pooled().shape == (P * R * S, Dx) and res.per_draw().shape == (P, R * S, Dx)
    assert np.array_equal(res.per_draw()[1], x[1].reshape(-1, Dx)) and np.array_equal(res.pooled()[:S], x[0, 0])
    assert res.rhat.shape == (P, Dx) and res.ess.shape == (P, Dx) and res.rhat is res.rhat
    summ = res.summary(0.9)
    assert all(summ[k].shape == (Dx,) for k in ('mean', 'lower', 'upper', 'draw_sd'))
    assert np.all(summ['lower'] < summ['mean']) and np.all(summ['mean'] < summ['upper'])
    assert np.allclose(summ['mean'], x.mean((0, 1, 2))) and np.allclose(summ['draw_sd'], x.mean((1, 2)).std(0, ddof=1))
    assert np.all(np.abs(summ['draw_sd'] - 1.0) < 0.2)                           # (the draws' means are 0, 1, 2 apart)
    for level in (0.0, 1.0):
        with pytest.raises(ValueError):
            res.summary(level)


def test_observation_statistics():
    from dgp_amd import calibrate
    ybar, w = calibrate.observation([0.5, np.nan, 2.0], 0.1, 3)
    assert np.array_equal(ybar, [0.5, 0.0, 2.0]) and np.array_equal(w, 1.0 / (np.full(3, 0.1) * np.full(3, 0.1)) * np.array([1, 0, 1]))
    y = np.array([[1.0, np.nan], [2.0, np.nan], [np.nan, 4.0], [3.0, 6.0]])
    ybar, w = calibrate.observation(y, [0.5, 2.0], 2)
    assert np.array_equal(ybar, [2.0, 5.0]) and np.array_equal(w, [3 / 0.25, 2 / 4.0])
    rep = np.random.default_rng(0).normal(size=(4, 2))                           # T = 4 replicates: ybar with obs_sd / 2
    a, b = calibrate.observation(rep, 0.3, 2), calibrate.observation(calibrate.observation(rep, 0.3, 2)[0], 0.15, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for bad_y in (np.full(3, np.nan), np.zeros(2), np.zeros((2, 2)), np.zeros((0, 3)), np.array([0.0, np.inf, 0.0]), np.zeros((1, 1, 3))):
        with pytest.raises(ValueError):
            calibrate.observation(bad_y, 0.1, 3)
    for bad_sd in (0.0, -1.0, np.nan, np.inf, [0.1, 0.1], [0.1, 0.0, 0.1], np.ones((1, 3))):
        with pytest.raises(ValueError):
            calibrate.observation(np.zeros(3), bad_sd, 3)


def test_driver_refusals_that_need_no_device():
    from dgp_amd import calibrate
    box = np.array([[0.0, 1.0], [0.0, 1.0]])

    def call(y=(0.1,), obs_sd=0.1, bounds=box, Dx=2, **kw):
        return calibrate.calibrate(None, 3, 1, Dx, None, None, 8, y, obs_sd, bounds, **kw)
    for bounds in (box[0], box[:1], np.array([[0.0, 1.0], [np.nan, 1.0]]), np.array([[0.0, 1.0], [1.0, 0.5]]), box.T[:, :1]):
        with pytest.raises(ValueError, match='calibrate'):
            call(bounds=bounds)
    for kw in (dict(y=[np.nan]), dict(y=[0.1, 0.2]), dict(obs_sd=0.0), dict(obs_sd=[0.1, 0.1]), dict(n_chains=0), dict(n_samples=0),
               dict(thin=0), dict(warmup=-1), dict(scale=[1.0]), dict(scale=[1.0, -1.0]), dict(scale=[1.0, np.nan]), dict(step=0.0),
               dict(step=np.nan), dict(target_accept=0.0), dict(target_accept=1.0), dict(prior=([0.5, 0.5], [1.0, 0.0])),
               dict(prior=([0.5, 0.5], [1.0, -1.0])), dict(prior=([0.5, np.inf], [1.0, 1.0])), dict(prior=([0.5], [1.0])),
               dict(prior=[0.5, 0.5, 0.5])):
        with pytest.raises(ValueError, match='calibrate'):
            call(**kw)
    pv, pm = calibrate.check_prior(([0.2, 0.4], [0.5, np.inf]), 2)
    assert np.array_equal(pv, [4.0, 0.0]) and np.array_equal(pm, [0.2, 0.4])


def test_line_case_on_the_cpu():
    """tests/test_gpu_calibrate_model.py::test_line_gp_against_quadrature on the CPU: the restatement, driven by pathfun_ref
    and pathgrad_ref on the same draws, on calibrate's schedule and streams.  Per draw the mean and variance of 4 chains x
    1000 samples within 5 standard errors of quadrature on 4001 points.  Observed (seed 1): z of the means -0.32, 0.02, 0.02, -0.37,
    2.23, 1.42, of the variances -1.68, 0.64, -0.18, 0.23, -1.01, -1.64; split R-hat 0.9994 .. 1.0010, which sets the device
    test's RHAT_MAX = 1.01, ten times the largest distance from 1 seen here."""
    import test_gpu_calibrate_model as G
    from dgp_amd import calibrate
    L = G.LINE
    funs, f_grid = G.line_case()
    w, ybar, lo, hi = np.array([1.0 / L['sd'] ** 2]), np.array([L['y']]), np.zeros(1), np.ones(1)
    lp_grid = -0.5 * w[0] * (ybar[0] - f_grid) ** 2                              # (J, 4001): the starts as calibrate picks them
    cand = G.GRID[::16][:, None]
    z, logu = calibrate.Streams(1, L['J'], L['chains'], 1).block(1 + L['warmup'] + L['samples'])
    zs, rhat = [], []
    for p, fun in enumerate(funs):
        x0 = cand[np.argsort(-lp_grid[p, ::16], kind='stable')[:L['chains']]]
        chains = [M.sample(fun, x0[r], w, ybar, lo, hi, hi - lo, z[:, p, r], logu[:, p, r], L['warmup'], 1,
                           lambda c: calibrate.gain(c, 0.574)) for r in range(L['chains'])]
        x = np.array([c.xs for c in chains])[:, :, 0]
        zs.append(G.against_the_grid(x, f_grid[p]))
        rhat.append(float(calibrate.split_rhat(x)))
    print('line case on the CPU: z of the means %s, of the variances %s, rhat %s' %
          (np.round([a for a, _ in zs], 2), np.round([b for _, b in zs], 2), np.round(rhat, 4)))
    assert np.max(np.abs(zs)) <= G.MARGIN and max(rhat) < G.RHAT_MAX


def test_gain_is_a_robbins_monro_sequence():
    from dgp_amd import calibrate
    up, down = np.array([calibrate.gain(w, 0.574) for w in range(2000)]).T
    g = np.log(up) - np.log(down)                                                # gamma_w
    assert np.all(up > 1.0) and np.all(down < 1.0) and np.all(np.diff(g) < 0.0) and g[0] == pytest.approx(1.0)
    assert np.allclose(np.log(up) / g, 1.0 - 0.574) and np.allclose(g, (np.arange(2000) + 1.0) ** -0.6)
    # at the target rate the expected move of log h is zero
    assert np.allclose(0.574 * np.log(up) + (1.0 - 0.574) * np.log(down), 0.0, atol=1e-15)


def test_streams_do_not_depend_on_the_blocks_or_on_the_other_chains():
    from dgp_amd import calibrate
    P, R, Dx, rounds = 3, 4, 2, 130
    z, u = calibrate.Streams(7, P, R, Dx).block(rounds)
    assert z.shape == (rounds, P, R, Dx) and u.shape == (rounds, P, R) and np.all(u <= 0.0)
    for size in (1, 7, 64):
        s = calibrate.Streams(7, P, R, Dx)
        parts = [s.block(min(size, rounds - c)) for c in range(0, rounds, size)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), z) and np.array_equal(np.concatenate([p[1] for p in parts]), u)
    z2, u2 = calibrate.Streams(7, P, 2, Dx).block(rounds)                        # the first two chain slots alone
    assert np.array_equal(z2, z[:, :, :2]) and np.array_equal(u2, u[:, :, :2])
    other = calibrate.Streams(8, P, R, Dx).block(rounds)
    assert not np.array_equal(other[0], z)
    # the two streams are independent of each other: no normal draw is a function of a uniform one
    assert abs(np.corrcoef(z[..., 0].ravel(), u.ravel())[0, 1]) < 5.0 / np.sqrt(u.size)
    assert abs(z.mean()) < 5.0 / np.sqrt(z.size) and abs(np.exp(u).mean() - 0.5) < 5.0 / np.sqrt(12 * u.size)
