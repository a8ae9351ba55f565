"""Random streams made on the device (csrc/philox.hip, DESIGN I.23): dgpamd_philox_fill against its numpy restatement
(tests/philox_ref.py) and against the exact value of its transforms, and the three drivers with rng='device' on closed-form
functions given by torch closures, where the answer is known, and on one small gp model.  Needs an MI355X: -m gpu.

The statistical conditions are those of the drivers' own model tests: tests/test_gpu_failure_probability_model.py
(check_seeds, with the spreads that tests/test_philox_host.py measures on the Philox streams), tests/test_gpu_calibrate_model.py
and tests/test_gpu_calibrate_hmc_model.py (the line case: the pooled mean and variance within 5 standard errors by the
samples' own ess, split R-hat, the acceptance window) and tests/test_gpu_calibrate_smc_model.py (the line case: log evidence
and the particles' mean and variance)."""
import math

import numpy as np
import pytest

import philox_ref as X

pytestmark = pytest.mark.gpu
MARGIN = 5.0
KEY = (0xFEDCBA9876543210, 0x8000000000000001)                  # high bits set
SHAPES = {1: (1, 1), 63: (7, 9), 64: (4, 16), 65: (5, 13), 130: (2, 65)}      # Q = P R: below, at and beyond one wave and a workgroup's part
WIDTHS = (1, 3, 4, 5, 8, 64)
ROUNDS = (1, 3)
FIRST = (0, (1 << 32) + 7, 1 << 63)
# The seeds' standard deviation of ln P^ of the restatement on the Philox streams at 1024 particles, 4 moves, level_prob 0.1
# (tests/test_philox_host.py prints them): the D = 2 corner event at 1e-3 and the D = 2 half-space at beta = 3.
CPU = dict(corner2=0.157, normal2=0.176)
# Twice the largest error observed on an MI355X (see test_the_transforms_against_exact_values)
LOG_ULP_MAX = 2 * 0.628
NORMAL_ERR_MAX = 2 * 1.186


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


def cases():
    return [(P, R, D, rounds, c2) for P, R in SHAPES.values() for D in WIDTHS for rounds in ROUNDS for c2 in FIRST]


# ------------------------------------------------------------------------------------------------------------ the fill kernel
@pytest.mark.parametrize('kind', ['bits', 'uniform'])
def test_bits_and_uniforms_equal_the_restatement(eng, kind):
    """Every shape, width, round count and first round: the device's words and uniforms are the restatement's, and the eight
    entries in front of `out` and behind it keep what they held."""
    import torch
    dtype, mark = (torch.int64, -12345) if kind == 'bits' else (torch.float64, -7.5)
    for P, R, D, rounds, c2 in cases():
        n = rounds * P * R * D
        buf = torch.full((n + 16,), mark, dtype=dtype, device=eng.device)
        out = eng.philox_fill(kind, KEY, 2, c2, rounds, P, R, D, out=buf[8:8 + n].view(rounds, P, R, D))
        got = buf.cpu().numpy()
        assert out.data_ptr() == buf.data_ptr() + 64
        assert np.all(got[:8] == mark) and np.all(got[8 + n:] == mark), (P, R, D, rounds, c2)
        assert np.array_equal(got[8:8 + n].reshape(rounds, P, R, D), X.fill(kind, KEY, 2, c2, rounds, P, R, D)), (P, R, D, rounds, c2)
    u = eng.philox_fill('uniform', KEY, 0, 0, 2, 3, 50, 8).cpu().numpy()
    assert np.all(u >= 0.0) and np.all(u < 1.0)


@pytest.mark.parametrize('kind', X.KINDS)
def test_an_entry_does_not_depend_on_the_shape_of_the_call(eng, kind):
    """Bit-equal at P = 1 and P = 3, at R and a smaller R, at D and a smaller D, and with the rounds split over two calls;
    guard entries untouched for the transformed kinds too."""
    import torch
    bits = lambda t: t.contiguous().view(torch.int64).cpu().numpy()
    for D in WIDTHS:
        for c2 in FIRST:
            whole = eng.philox_fill(kind, KEY, 1, c2, 3, 3, 65, D)
            assert np.array_equal(bits(whole[:, :1]), bits(eng.philox_fill(kind, KEY, 1, c2, 3, 1, 65, D))), (D, c2)
            assert np.array_equal(bits(whole[:, :, :7]), bits(eng.philox_fill(kind, KEY, 1, c2, 3, 3, 7, D))), (D, c2)
            two = torch.cat([eng.philox_fill(kind, KEY, 1, c2, 1, 3, 65, D), eng.philox_fill(kind, KEY, 1, c2 + 1, 2, 3, 65, D)])
            assert np.array_equal(bits(whole), bits(two)), (D, c2)
            if D > 3:
                assert np.array_equal(bits(whole[..., :3]), bits(eng.philox_fill(kind, KEY, 1, c2, 3, 3, 65, 3))), (D, c2)
    assert not np.array_equal(bits(eng.philox_fill(kind, KEY, 1, 0, 1, 2, 9, 5)), bits(eng.philox_fill(kind, KEY, 2, 0, 1, 2, 9, 5)))
    assert not np.array_equal(bits(eng.philox_fill(kind, KEY, 1, 0, 1, 2, 9, 5)), bits(eng.philox_fill(kind, (KEY[0], KEY[1] + 1), 1, 0, 1, 2, 9, 5)))
    n = 2 * 5 * 13 * 5
    dtype = torch.int64 if kind == 'bits' else torch.float64
    buf = torch.full((n + 16,), -3, dtype=dtype, device=eng.device)
    eng.philox_fill(kind, KEY, 1, 9, 2, 5, 13, 5, out=buf[8:8 + n].view(2, 5, 13, 5))
    got = buf.cpu().numpy()
    assert np.all(got[:8] == -3) and np.all(got[8 + n:] == -3)
    assert np.array_equal(buf[8:8 + n].view(torch.int64).cpu().numpy().reshape(2, 5, 13, 5), bits(eng.philox_fill(kind, KEY, 1, 9, 2, 5, 13, 5)))


def test_the_transforms_against_exact_values(eng):
    """log_uniform and normal against the exact value of the formula at the exactly known uniforms, by mpmath at 50 digits,
    over Q = 130 and 65, D = 8, 5 and 1, 3 rounds from 2^63: 4485 numbers of each kind.  log_uniform in ulp of the exact value;
    normal as |z - exact| / (2^-52 rho), rho = sqrt(-2 log u1) -- the cosine has no relative accuracy at its zeros.
    Observed on an MI355X: log_uniform at most 0.628 ulp, normal at most 1.186 units; the bounds asserted are twice that."""
    import mpmath
    mpmath.mp.dps = 50
    worst_log, worst_normal = 0.0, 0.0
    for (P, R), D in (((2, 65), 8), ((5, 13), 5), ((2, 65), 1)):
        c2, rounds = 1 << 63, 3
        lu = eng.philox_fill('log_uniform', KEY, 2, c2, rounds, P, R, D).cpu().numpy().reshape(-1)
        u = X.fill('uniform', KEY, 2, c2, rounds, P, R, D).reshape(-1)
        assert np.all(u > 0.0)                                                   # (a zero uniform, one in 2^53, would be -inf)
        exact = [mpmath.log(mpmath.mpf(float(v))) for v in u]
        err = np.array([abs(mpmath.mpf(float(g)) - x) / mpmath.mpf(float(np.spacing(abs(float(x))))) for g, x in zip(lu, exact)], dtype=np.float64)
        worst_log = max(worst_log, err.max())
        z = eng.philox_fill('normal', KEY, 1, c2, rounds, P, R, D).cpu().numpy().reshape(-1, D)
        u1, u2 = (a.reshape(-1, (D + 1) // 2) for a in X.normal_uniforms(KEY, 1, c2, rounds, P, R, D))
        for row in range(len(z)):
            for m in range((D + 1) // 2):
                rho = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(float(u1[row, m]))))
                ang = 2 * mpmath.pi * mpmath.mpf(float(u2[row, m]))
                unit = mpmath.mpf(2) ** -52 * rho
                pair = [rho * mpmath.cos(ang), rho * mpmath.sin(ang)]
                for k in range(min(2, D - 2 * m)):
                    worst_normal = max(worst_normal, float(abs(mpmath.mpf(float(z[row, 2 * m + k])) - pair[k]) / unit) if rho > 0 else
                                       float(abs(z[row, 2 * m + k])))
        assert np.all(np.isfinite(z))
        # and the restatement, whose log, cos and sin are numpy's, stays close: its angle 2 pi u2 carries the rounding of the
        # constant and of the product, at most 2 pi units of 2^-52 together; 12 units with the other roundings and the device's
        zr = X.fill('normal', KEY, 1, c2, rounds, P, R, D).reshape(-1, D)
        assert np.max(np.abs(z - zr)) <= 12 * 2.0 ** -52 * np.sqrt(-2.0 * np.log(u1.min()))
    print('log_uniform: largest error %.3f ulp (bound %.3f); normal: largest error %.3f units of 2^-52 rho (bound %.3f)'
          % (worst_log, LOG_ULP_MAX, worst_normal, NORMAL_ERR_MAX))
    assert worst_log <= LOG_ULP_MAX and worst_normal <= NORMAL_ERR_MAX


def test_moments_on_the_device(eng):
    """10^5 numbers of the device's own normals and log-uniforms: the conditions of tests/test_philox_host.py."""
    n = 100000
    z = eng.philox_fill('normal', X.key_of(2024), 1, 0, 10, 10, 250, 4).cpu().numpy().reshape(-1)
    lu = eng.philox_fill('log_uniform', X.key_of(2024), 2, 0, 10, 10, 250, 4).cpu().numpy().reshape(-1)
    for what, got, exact, var in (('mean of z', z.mean(), 0.0, 1.0), ('variance of z', np.mean(z * z), 1.0, 2.0),
                                  ('fourth moment of z', np.mean(z ** 4), 3.0, 96.0), ('mean of log u', lu.mean(), -1.0, 1.0)):
        assert abs(got - exact) <= MARGIN * math.sqrt(var / n), what


def test_refusals_of_the_engine(eng):
    import torch
    from dgp_amd import _lib
    from dgp_amd.ops import DgpAmdError
    for bad in (dict(kind='gauss'), dict(rounds=0), dict(P=0), dict(R=0), dict(D=0), dict(D=65), dict(c2_first=(1 << 64) - 2)):
        kw = dict(dict(kind='normal', key=KEY, stream=1, c2_first=0, rounds=2, P=2, R=3, D=4), **bad)
        with pytest.raises(ValueError):
            eng.philox_fill(**kw)
    for out in (torch.zeros(2, 2, 3, 4, dtype=torch.float32, device=eng.device), torch.zeros(2, 2, 3, 5, dtype=torch.float64, device=eng.device),
                torch.zeros(2, 2, 3, 8, dtype=torch.float64, device=eng.device)[..., ::2], torch.zeros(2, 2, 3, 4, dtype=torch.float64)):
        with pytest.raises(ValueError):
            eng.philox_fill('normal', KEY, 1, 0, 2, 2, 3, 4, out=out)
    with pytest.raises(ValueError):
        eng.philox_fill('bits', KEY, 1, 0, 2, 2, 3, 4, out=torch.zeros(2, 2, 3, 4, dtype=torch.float64, device=eng.device))
    # the library's own checks, behind the engine's: nothing is launched, the message names the argument
    for args, text in (((7, 1, 2, 1, 0, 1, 1, 1, 1), 'kind'), ((3, 1, 2, 1, 0, 1, 1, 1, 65), 'DGPAMD_MAXD'), ((3, 1, 2, 1, 0, 0, 1, 1, 1), 'rounds'),
                       ((3, 1, 2, 1, 0, 1, 1 << 31, 1, 1), '2^31'), ((3, 1, 2, 1, (1 << 64) - 1, 1, 1, 1, 1), 'wraps')):
        out = torch.zeros(8, dtype=torch.float64, device=eng.device)
        rc = _lib.lib.dgpamd_philox_fill(eng.h, *args, out.data_ptr())
        assert rc == _lib.BAD_ARG and text in _lib.lib.dgpamd_last_error(eng.h).decode() and not out.any()
    assert _lib.lib.dgpamd_philox_fill(eng.h, 3, 1, 2, 1, 0, 1, 1, 1, 1, None) == _lib.BAD_ARG
    assert issubclass(DgpAmdError, RuntimeError)


# ------------------------------------------------------------------------------------------ failure_probability, rng='device'
def sus(eng, P, D, values, threshold, bounds, seed, **kw):
    from dgp_amd import reliability
    return reliability.failure_probability(eng, P, 1, D, values, threshold, bounds, seed=seed, rng='device', **kw)


def corner_values(xt):
    return xt.sum(-1, keepdim=True).contiguous()


def halfspace_values(xt):
    return (xt.sum(-1, keepdim=True) / math.sqrt(2.0)).contiguous()


def check_ladder(res):
    on = np.isfinite(res.cond_prob)
    for p in range(len(res.prob)):
        lev = res.levels[p, on[p]]
        assert lev[-1] == 0.0 and not np.signbit(lev[-1]) and np.all(np.diff(lev) > 0.0) and np.all(lev[:-1] < 0.0)
    assert np.array_equal(res.prob, np.nanprod(res.cond_prob, axis=1)) and res.rng == 'device'


def test_corner_event_with_device_streams(eng):
    """sum x >= 2 - a on [0, 1]^2 at 1e-3: 16 draws of one function are 16 seeds (path p has numbers of its own);
    test_gpu_failure_probability_model.check_seeds, unchanged."""
    import boxsus_ref as S
    import test_gpu_failure_probability_model as G
    _, threshold, exact = S.corner(2, 1e-3)
    box = np.array([[0.0, 1.0]] * 2)
    res = sus(eng, 16, 2, corner_values, threshold, box, 3)
    assert res.x.shape == (16, 1024, 2) and np.all(res.x >= 0.0) and np.all(res.x <= 1.0)
    G.check_seeds(res, exact, CPU['corner2'], 'corner D 2, device streams')
    check_ladder(res)
    assert G.same(res, sus(eng, 16, 2, corner_values, threshold, box, 3))                          # a replay: the same bits
    other = sus(eng, 16, 2, corner_values, threshold, box, 4)
    assert not np.array_equal(res.x, other.x) and not np.array_equal(res.prob, other.prob)
    assert len(set(res.prob.tolist())) > 8                                                          # the draws differ: streams of their own


def test_normal_half_space_with_device_streams(eng):
    import boxsus_ref as S
    import test_gpu_failure_probability_model as G
    _, threshold, exact, (pv, pm), (lo, hi) = S.halfspace(2, 3.0)
    res = sus(eng, 16, 2, halfspace_values, threshold, np.stack([lo, hi], 1), 4, prior=(pm, 1.0 / np.sqrt(pv)))
    G.check_seeds(res, exact, CPU['normal2'], 'half-space D 2, device streams')
    check_ladder(res)


def test_a_draw_of_failure_probability_does_not_depend_on_P(eng):
    """prob, levels, x and everything else of draw 0 are bit-equal at P = 1 and P = 3, with R = 130 (beyond one workgroup's
    waves, no multiple of 64) and with the prior's columns in use."""
    import boxsus_ref as S
    import test_gpu_failure_probability_model as G
    _, threshold, exact, (pv, pm), (lo, hi) = S.halfspace(2, 2.0)
    kw = dict(n_particles=130, n_moves=2, prior=(pm, 1.0 / np.sqrt(pv)))
    one = sus(eng, 1, 2, halfspace_values, threshold, np.stack([lo, hi], 1), 9, **kw)
    # (the larger run goes on until its last draw has finished, moving the others inside F: stop it where the part stops)
    three = sus(eng, 3, 2, halfspace_values, threshold, np.stack([lo, hi], 1), 9, max_stages=one.n_stages, **kw)
    assert np.all(one.status == 0) and G.same(three, one, slice(0, 1))
    assert not np.array_equal(three.x[0], three.x[1])


# ----------------------------------------------------------------------------------------------- calibrate, rng='device'
def line_vj(xt):
    """tests/test_gpu_calibrate_model.line in closed form, every draw the same function: values (P, R, 1), Jacobian (P, R, 1, 1)."""
    import torch
    return (2.0 * xt - 1.0 + 0.2 * torch.sin(3.0 * xt)).contiguous(), (2.0 + 0.6 * torch.cos(3.0 * xt)).unsqueeze(-1).contiguous()


def line_grid():
    import test_gpu_calibrate_model as C
    return 2.0 * C.GRID - 1.0 + 0.2 * np.sin(3.0 * C.GRID)


X0 = np.array([[0.2], [0.4], [0.6], [0.8]])


def chains(eng, P, method, samples, warmup, seed, x0=X0, **kw):
    import test_gpu_calibrate_model as C
    from dgp_amd import calibrate
    return calibrate.calibrate(eng, P, 1, 1, None, line_vj, 1, np.array([[C.LINE['y']]]), C.LINE['sd'], C.BOX1, n_samples=samples, warmup=warmup,
                               x0=x0, seed=seed, method=method, rng='device', **kw)


@pytest.mark.parametrize('method', ['mala', 'hmc'])
def test_line_posterior_by_chains_with_device_streams(eng, method):
    """The line case of the chains' model tests on the line itself: 6 draws x 4 chains, 1000 samples after 500 warm-up rounds
    ('hmc': 400 after 200), per draw the pooled mean and variance within 5 standard errors, by the samples' own ess, of
    quadrature on GRID; split R-hat under that test's bound; the acceptance inside its window."""
    import test_gpu_calibrate_hmc_model as Hm
    import test_gpu_calibrate_model as C
    samples, warmup = (C.LINE['samples'], C.LINE['warmup']) if method == 'mala' else (Hm.LINE['samples'], Hm.LINE['warmup'])
    res = chains(eng, 6, method, samples, warmup, 1)
    assert res.x.shape == (6, 4, samples, 1) and np.all(res.status == 0) and (res.method, res.rng) == (method, 'device')
    f_grid = line_grid()
    z = np.array([C.against_the_grid(res.x[p, :, :, 0], f_grid) for p in range(6)])
    print('line, %s, device streams: acceptance %.2f .. %.2f, ess %.0f .. %.0f, rhat max %.4f' %
          (method, res.accept_rate.min(), res.accept_rate.max(), res.ess.min(), res.ess.max(), res.rhat.max()))
    print('z of the means %s, of the variances %s' % (np.round(z[:, 0], 2), np.round(z[:, 1], 2)))
    assert np.max(np.abs(z)) <= MARGIN
    assert np.all(res.rhat < (C.RHAT_MAX if method == 'mala' else Hm.RHAT_MAX)) and np.all(res.ess > 100)
    lo, hi = (0.3, 0.85) if method == 'mala' else (0.5, 0.98)
    assert np.all(res.accept_rate > lo) and np.all(res.accept_rate < hi)
    assert not np.array_equal(res.x[0], res.x[1])                                # the draws have numbers of their own


@pytest.mark.parametrize('method', ['mala', 'hmc'])
def test_chains_replay_and_do_not_depend_on_P_R_or_the_block(eng, method, monkeypatch):
    import test_gpu_calibrate_model as C
    from dgp_amd import calibrate
    whole = chains(eng, 3, method, 40, 40, 5)
    assert C.same(whole, chains(eng, 3, method, 40, 40, 5))
    assert not np.array_equal(whole.x, chains(eng, 3, method, 40, 40, 6).x)
    one, two = chains(eng, 1, method, 40, 40, 5), chains(eng, 3, method, 40, 40, 5, x0=X0[:2])
    for n in ('x', 'logp', 'accept_rate', 'step', 'status'):
        assert np.array_equal(getattr(whole, n)[:1], getattr(one, n)), n         # P
        assert np.array_equal(getattr(whole, n)[:, :2], getattr(two, n)), n      # R
    for size in (1, 7):
        monkeypatch.setattr(calibrate, '_rounds_per_upload', lambda Q, Dx, size=size: size)
        assert C.same(chains(eng, 3, method, 40, 40, 5), whole), size


# ------------------------------------------------------------------------------------------- calibrate_smc, rng='device'
def smc(eng, P, seed, **kw):
    import test_gpu_calibrate_model as C
    from dgp_amd import calibrate
    return calibrate.calibrate_smc(eng, P, 1, 1, None, line_vj, 1, np.array([[C.LINE['y']]]), C.LINE['sd'], C.BOX1, seed=seed, rng='device', **kw)


def test_line_posterior_by_smc_with_device_streams(eng):
    """The line case of tests/test_gpu_calibrate_smc_model.py on the line itself, its conditions unchanged: 6 draws, 512
    particles, per draw log_evidence within 5 CPU['line_logz'] of grid_evidence, the particles' mean and variance within 5
    standard errors of grid_posterior's, with that file's inflation."""
    import boxmala_ref as M
    import boxsmc_ref as S
    import test_gpu_calibrate_smc_model as G
    res = smc(eng, 6, 1, **G.SMC)
    R = G.SMC['n_particles']
    assert res.x.shape == (6, R, 1) and np.all(res.status == 0) and np.all(res.betas[:, -1] == 1.0) and res.rng == 'device'
    ybar, w = G.obs(G.LINE)
    f_grid = line_grid()
    exact = S.grid_evidence(f_grid, [G.GRID], ybar, w)
    mean, cov = M.grid_posterior(f_grid, [G.GRID], ybar, w)
    for p in range(6):
        x = res.x[p, :, 0]
        zm = (x.mean() - mean[0]) / (np.sqrt(cov[0, 0] / R) * G.CPU['line_mean'])
        zv = (x.var() - cov[0, 0]) / (cov[0, 0] * np.sqrt(2.0 / R) * G.CPU['line_var'])
        print('draw %d: log evidence %.4f, quadrature %.4f (bound %.4f); z of the mean %.2f, of the variance %.2f'
              % (p, res.log_evidence[p], exact, MARGIN * G.CPU['line_logz'], zm, zv))
        assert abs(res.log_evidence[p] - exact) <= MARGIN * G.CPU['line_logz']
        assert abs(zm) <= MARGIN and abs(zv) <= MARGIN
    assert len(set(res.log_evidence.tolist())) == 6                              # the draws have numbers of their own


def test_smc_replays_and_a_draw_does_not_depend_on_P(eng):
    import test_gpu_calibrate_smc_model as G
    kw = dict(n_particles=130, n_moves=2)
    one = smc(eng, 1, 9, **kw)
    assert np.all(one.status == 0) and G.same(one, smc(eng, 1, 9, **kw))
    assert not np.array_equal(one.x, smc(eng, 1, 10, **kw).x)
    # (the larger run goes on until its last draw is at beta = 1: stop it where the part stops)
    three = smc(eng, 3, 9, max_stages=one.n_stages, **kw)
    assert G.same(three, one, slice(0, 1)) and not np.array_equal(three.x[0], three.x[1])


# --------------------------------------------------------------------------------------------------- one gp model, end to end
@pytest.fixture(scope='module')
def gp_paths(eng):
    import test_gpu_boxmin_model as B
    import test_gpu_pathfun as T
    m = T._gp('sexp', *B.bowl())
    np.random.seed(31)
    return m, m.sample_functions(sample_size=3, n_features=64)


def test_gp_model_end_to_end(eng, gp_paths):
    import test_gpu_boxmin_model as B
    import test_gpu_calibrate_model as C
    import test_gpu_calibrate_smc_model as Gs
    import test_gpu_failure_probability_model as Gf
    m, paths = gp_paths
    BOX = B.BOX
    short = dict(n_chains=3, n_samples=20, warmup=20, n_candidates=64)
    for method in ('mala', 'hmc'):
        res = paths.calibrate(0.05, 0.05, BOX, seed=3, method=method, rng='device', **short)
        assert res.x.shape == (3, 3, 20, 2) and res.rng == 'device' and np.all(res.status == 0) and np.all(res.x >= 0.0) and np.all(res.x <= 1.0)
        assert C.same(res, paths.calibrate(0.05, 0.05, BOX, seed=3, method=method, rng='device', **short))
        plain = paths.calibrate(0.05, 0.05, BOX, seed=3, method=method, **short)
        assert plain.rng == 'numpy' and np.array_equal(plain.x0, res.x0) and not np.array_equal(plain.x, res.x)
        assert C.same(plain, paths.calibrate(0.05, 0.05, BOX, seed=3, method=method, rng='numpy', **short))
    res = paths.calibrate_smc(0.05, 0.05, BOX, seed=3, rng='device', **Gs.SMALL)
    assert res.x.shape == (3, 64, 2) and res.rng == 'device' and np.all(res.status == 0)
    assert Gs.same(res, paths.calibrate_smc(0.05, 0.05, BOX, seed=3, rng='device', **Gs.SMALL))
    plain = paths.calibrate_smc(0.05, 0.05, BOX, seed=3, **Gs.SMALL)
    assert plain.rng == 'numpy' and not np.array_equal(plain.x, res.x)
    assert Gs.same(plain, paths.calibrate_smc(0.05, 0.05, BOX, seed=3, rng='numpy', **Gs.SMALL))
    t = Gf.high_value(paths, 0.99)
    res = paths.failure_probability(t, BOX, seed=3, rng='device', **Gf.SMALL)
    Gf.check_result(paths, res, t, 3, Gf.SMALL)
    assert res.rng == 'device' and Gf.same(res, paths.failure_probability(t, BOX, seed=3, rng='device', **Gf.SMALL))
    plain = paths.failure_probability(t, BOX, seed=3, **Gf.SMALL)
    assert plain.rng == 'numpy' and not np.array_equal(plain.x, res.x)
    assert Gf.same(plain, paths.failure_probability(t, BOX, seed=3, rng='numpy', **Gf.SMALL))
    # the model's own entry points pass the keyword on
    np.random.seed(8)
    assert m.failure_probability(t, BOX, sample_size=2, n_features=32, seed=2, rng='device', **Gf.SMALL).rng == 'device'
    np.random.seed(8)
    assert m.calibrate_smc(0.05, 0.05, BOX, sample_size=2, n_features=32, seed=2, rng='device', **Gs.SMALL).rng == 'device'
    np.random.seed(8)
    assert m.calibrate(0.05, 0.05, BOX, sample_size=2, n_features=32, seed=2, rng='device', **short).rng == 'device'
    for bad in ('philox', None, 1):
        with pytest.raises(ValueError, match='rng'):
            paths.calibrate(0.05, 0.05, BOX, rng=bad, **short)
        with pytest.raises(ValueError, match='rng'):
            paths.calibrate_smc(0.05, 0.05, BOX, rng=bad, **Gs.SMALL)
        with pytest.raises(ValueError, match='rng'):
            paths.failure_probability(t, BOX, rng=bad, **Gf.SMALL)
