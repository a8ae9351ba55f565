"""paths.failure_probability, emulator.failure_probability and gp.failure_probability (dgp_amd/reliability.py, DESIGN I.22):
the driver on closed-form functions given by a torch closure, where the exact probability is known; on the 1-D line gp of
tests/test_gpu_calibrate_model.py against the measure of every draw's own event on a grid; and on the 2-D gp and the
emulators of tests/test_gpu_boxmin_model.py: shapes, scores against paths(x), the ladder of levels, replays and invariances,
below, the prior, the refusals.  Needs an MI355X: -m gpu.

The statistical bounds are 5 x the spread over seeds that the numpy restatement (tests/boxsus_ref.py) shows with the same
settings: CPU below, measured by tests/test_boxsus_host.py (test_corner_event, test_halfspace_under_a_truncated_normal_prior,
test_line_gp_on_the_cpu), which also holds these numbers to what it measures."""
import math

import numpy as np
import pytest

import boxsus_ref as S
import test_gpu_boxmin_model as B
import test_gpu_calibrate_model as C
import test_gpu_pathfun as T

pytestmark = pytest.mark.gpu
MARGIN = 5.0
GRID, BOX1, BOX = C.GRID, C.BOX1, C.BOX
# The seeds' standard deviation of ln P^ in the restatement at 1024 particles, 4 moves, level_prob 0.1: the D = 5 corner event
# at 1e-6, the D = 2 half-space under the truncated normal prior, and the largest over the 6 draws of the line gp at LINE_T.
CPU = dict(corner5=0.239, normal2=0.166, line=0.114)
# The threshold of the line gp, chosen on the numpy replay so that every draw's quadrature probability lies in [1e-4, 0.5] and
# some lie under 1e-2 (more than one stage), and those probabilities: the measure of {f_p >= LINE_T} on GRID.
LINE_T = 1.015
LINE_PROB = [0.0147548, 0.01114485, 0.0035432, 0.01090046, 0.00470694, 0.00664848]
SMALL = dict(n_particles=64, n_moves=2)


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import default_engine
    return default_engine(0)


# ------------------------------------------------------------------------------------------ the driver on closed-form functions
def drive(eng, P, D, values, threshold, bounds, seed, **kw):
    from dgp_amd import reliability
    return reliability.failure_probability(eng, P, 1, D, values, threshold, bounds, seed=seed, **kw)


def check_seeds(res, exact, spread, what):
    lp = res.log_prob
    z = (lp.mean() - math.log(exact)) / (lp.std(ddof=1) / math.sqrt(len(lp)))
    print('%s: exact %.4g, ln P^ - ln p in %.3f .. %.3f (bound %.3f), mean %.4f (z %.2f), sd %.3f (restatement %.3f), cov() %.3f, stages %d'
          % (what, exact, (lp - math.log(exact)).min(), (lp - math.log(exact)).max(), MARGIN * spread, lp.mean() - math.log(exact), z,
             lp.std(ddof=1), spread, np.median(res.cov()), res.n_stages))
    assert np.all(res.status == 0)
    assert np.all(np.abs(lp - math.log(exact)) <= MARGIN * spread) and abs(z) <= MARGIN
    assert np.all(res.score >= 0.0) and np.array_equal(res.prob, np.nanprod(res.cond_prob, axis=1))


def test_corner_event_by_the_driver(eng):
    """sum x >= 5 - a on [0, 1]^5 at 1e-6: 16 draws of one function are 16 seeds (path p has streams of its own)."""
    _, threshold, exact = S.corner(5, 1e-6)
    res = drive(eng, 16, 5, lambda xt: xt.sum(-1, keepdim=True).contiguous(), threshold, np.array([[0.0, 1.0]] * 5), 3)
    assert res.x.shape == (16, 1024, 5) and np.all(res.x >= 0.0) and np.all(res.x <= 1.0)
    check_seeds(res, exact, CPU['corner5'], 'corner D 5')


def test_normal_half_space_by_the_driver(eng):
    _, threshold, exact, (pv, pm), (lo, hi) = S.halfspace(2, 3.0)
    res = drive(eng, 16, 2, lambda xt: (xt.sum(-1, keepdim=True) / math.sqrt(2.0)).contiguous(), threshold, np.stack([lo, hi], 1), 4,
                prior=(pm, 1.0 / np.sqrt(pv)))
    check_seeds(res, exact, CPU['normal2'], 'half-space D 2')


# --------------------------------------------------------------------------------------------------------- the 1-D line gp
@pytest.fixture(scope='module')
def line_paths(eng):
    X, Y = C.line()
    m = T._gp('sexp', X, Y)
    np.random.seed(C.LINE['seed'])
    return m.sample_functions(sample_size=C.LINE['J'], n_features=C.LINE['F'])


def test_line_gp_against_quadrature(eng, line_paths):
    """6 draws, 1024 particles: per draw ln P^ within 5 CPU['line'] of the logarithm of the measure of {f_p >= LINE_T} from
    paths(GRID), crossings interpolated linearly; that measure equals the one recorded from the numpy replay."""
    res = line_paths.failure_probability(LINE_T, BOX1, seed=1)
    f_grid = line_paths(GRID[:, None])
    exact = np.array([S.grid_measure(f_grid[:, p], GRID, LINE_T) for p in range(6)])
    assert np.allclose(exact, LINE_PROB, rtol=1e-6)
    print('P^ %s\nquadrature %s\nln ratio %s, bound %.3f; stages %s; cov() %s' % (res.prob, exact, np.round(res.log_prob - np.log(exact), 3),
          MARGIN * CPU['line'], np.sum(np.isfinite(res.cond_prob), 1), np.round(res.cov(), 3)))
    assert np.all(res.status == 0) and res.n_stages > 1
    assert np.all(np.abs(res.log_prob - np.log(exact)) <= MARGIN * CPU['line'])
    s = res.summary()
    assert s['lower'] <= s['median'] <= s['upper'] and s['n_bounded'] == 0 and abs(s['mean'] - res.prob.mean()) < 1e-15
    # below: the same event of the mirrored question, f <= t, has the complementary measure
    low = line_paths.failure_probability(-0.9, BOX1, below=True, seed=1)
    exact_low = np.array([S.grid_measure(f_grid[:, p], GRID, -0.9, -1.0) for p in range(6)])
    assert np.all(low.status == 0) and np.all(np.abs(low.log_prob - np.log(exact_low)) <= MARGIN * CPU['line'])


def test_a_threshold_above_every_draw(eng, line_paths):
    """No grid point of any draw reaches 2: the ladder ends at max_stages = 3 (level_prob = 0.05, so that three stages pass
    the grid's resolution) with an upper bound under the smallest probability the grid resolves, and with min_prob = 0.05
    after two stages of 0.1 as below_min."""
    f_grid = line_paths(GRID[:, None])
    assert f_grid.max() < 2.0
    res = line_paths.failure_probability(2.0, BOX1, seed=1, max_stages=3, level_prob=0.05)
    assert np.all(res.status == 2) and res.n_stages == 3 and np.all(res.prob < 1.0 / (len(GRID) - 1)) and np.all(res.prob > 0.0)
    assert np.all(res.levels < 0.0) and np.all(np.diff(res.levels, axis=1) > 0.0) and res.summary()['n_bounded'] == 6
    assert np.all(res.score >= res.levels[:, -1:])                                # x samples the last level set
    res = line_paths.failure_probability(2.0, BOX1, seed=1, max_stages=5, min_prob=0.05)
    assert np.all(res.status == 3) and res.n_stages == 2 and np.all(res.prob < 0.05)


# ------------------------------------------------------------------------------------------------ 2-D models
@pytest.fixture(scope='module')
def gp_paths(eng):
    X, Y = B.bowl()
    m = T._gp('sexp', X, Y)
    np.random.seed(31)
    return m, m.sample_functions(sample_size=6, n_features=128)


@pytest.fixture(scope='module', params=['two-connect', 'three'])
def emu_paths(request, eng):
    from dgp_amd import emulator
    X, model = T._model(request.param)
    emu = emulator(model.estimate(), N=2, seed=5)
    return request.param, emu, emu.sample_functions(sample_size=3, n_features=100)


NAMES = ('prob', 'levels', 'cond_prob', 'accept_rate', 'step', 'x', 'score', 'status')


def same(a, c, rows=slice(None)):
    return all(np.array_equal(getattr(a, n)[rows], getattr(c, n), equal_nan=True) for n in NAMES) and a.n_stages == c.n_stages


def high_value(obj, q=0.995):
    """A threshold that every draw reaches, and rarely: the smallest over the draws of the q-quantile of the draw's values
    over the box (q < 0.5: the largest, for below)."""
    vals = np.quantile(B.values_of(obj, np.random.default_rng(1).uniform(size=(4096, 2))), q, axis=0)
    return float(vals.min() if q >= 0.5 else vals.max())


def check_result(obj, res, threshold, P, kw, sign=1.0):
    """What every result must satisfy, against the draws' own shared-rows evaluation."""
    R, Tn = kw['n_particles'], res.n_stages
    lo, hi = BOX[:, 0], BOX[:, 1]
    assert res.x.shape == (P, R, 2) and res.score.shape == (P, R) and res.prob.shape == (P,) and res.status.shape == (P,)
    assert all(getattr(res, n).shape == (P, Tn) for n in ('levels', 'cond_prob', 'accept_rate', 'step'))
    assert res.evaluations == Tn * (kw['n_moves'] + 1) and res.cov().shape == (P,)
    assert np.all(res.x >= lo) and np.all(res.x <= hi) and np.all(res.status == 0)
    # score: the draw's own value, as paths(x) gives it at the final particles (row p R + r belongs to path p)
    rows = res.x.reshape(P * R, 2)
    own = np.repeat(np.arange(P), R)
    f = B.values_of(obj, rows)[np.arange(P * R), own]
    bound = B.form_bound(obj, rows)[np.arange(P * R), own] + 4 * np.finfo(float).eps * (np.abs(f) + abs(threshold))
    d = np.abs(res.score.reshape(-1) - sign * (f - threshold))
    print('score against paths(x): largest difference / bound %.3g' % np.max(d / bound))
    assert np.all(d <= bound)
    # every particle of an ok draw lies in F; the levels increase to exactly 0; prob is the product of the stages' shares
    assert np.all(res.score >= 0.0)
    on = np.isfinite(res.cond_prob)
    assert on[:, 0].all() and np.all(on[:, 1:] <= on[:, :-1])                    # NaN once a draw has finished
    for p in range(P):
        lev = res.levels[p, on[p]]
        assert lev[-1] == 0.0 and not np.signbit(lev[-1]) and np.all(np.diff(lev) > 0.0) and np.all(lev[:-1] < 0.0)
    assert np.array_equal(res.prob, np.nanprod(res.cond_prob, axis=1)) and np.all(res.prob > 0.0) and np.all(res.prob <= 1.0)
    assert np.all(res.step[on] >= 1e-3) and np.all(res.step[on] <= 1e2) and np.all(res.accept_rate[on] >= 0.0) and np.all(res.accept_rate[on] <= 1.0)
    assert np.all(np.isnan(res.levels[~on])) and np.all(np.isnan(res.step[~on]))


def test_gp_failure_probability(eng, gp_paths):
    m, paths = gp_paths
    kw = dict(n_particles=256, n_moves=3)
    t = high_value(paths)
    res = paths.failure_probability(t, BOX, seed=3, **kw)
    check_result(paths, res, t, 6, kw)
    assert res.n_stages >= 2 and np.all(res.prob < 0.05)
    assert same(res, paths.failure_probability(t, BOX, seed=3, **kw))                # the same arguments: the same bits
    assert not np.array_equal(res.x, paths.failure_probability(t, BOX, seed=4, **kw).x)
    # plain Monte Carlo through paths(x) on 2^16 rows agrees within 5 of its own standard errors and 5 of cov() (a lower bound
    # of subset simulation's error, so this is the looser of the two honest statements: a factor 2 is allowed on cov())
    rows = np.random.default_rng(5).uniform(size=(1 << 16, 2))
    mc = np.mean(B.values_of(paths, rows) >= t, 0)
    se = np.sqrt(mc * (1.0 - mc) / len(rows)) / np.maximum(mc, 1e-300)
    print('P^ %s, plain Monte Carlo %s, cov() %s' % (res.prob, mc, np.round(res.cov(), 3)))
    assert np.all(mc > 0.0) and np.all(np.abs(res.log_prob - np.log(mc)) <= MARGIN * (2.0 * res.cov() + se))


def test_a_slice_of_the_draws_reproduces_its_part(eng, gp_paths):
    """The driver on the gp's closure with the paths sliced to draws 0 .. 1: their bits are the whole run's."""
    import torch
    from dgp_amd import reliability
    m, paths = gp_paths
    kw = dict(n_particles=130, n_moves=2, seed=9)
    t = high_value(paths, 0.99)
    e, P, K, Dx, values = paths._lane_values(BOX, 'failure_probability')

    def first_two(xt):
        full = torch.cat([xt, xt.new_zeros(P - 2, *xt.shape[1:]) + 0.5], 0)
        return values(full)[:2].contiguous()
    part = reliability.failure_probability(e, 2, K, Dx, first_two, t, BOX, **kw)
    # (the whole run goes on until its last draw has finished, moving the others inside F: stop it where the part stops)
    whole = paths.failure_probability(t, BOX, max_stages=part.n_stages, **kw)
    assert np.all(part.status == 0) and same(whole, part, slice(0, 2))


def test_below_and_prior(eng, gp_paths):
    import copy
    m, paths = gp_paths
    kw = dict(n_particles=256, n_moves=3)
    t = high_value(paths, 0.99)
    up = paths.failure_probability(t, BOX, seed=2, **kw)
    # the negated model: the same draws with the sign of every weight flipped; f <= -t is the same event
    neg = copy.copy(paths)
    neg.node = copy.copy(paths.node)
    flipped = 0
    for name, val in vars(paths.node).items():
        if name in ('theta', 'v'):
            setattr(neg.node, name, -val)
            flipped += 1
    assert flipped == 2
    rows = np.random.default_rng(2).uniform(size=(32, 2))
    assert np.allclose(neg(rows), -paths(rows), rtol=0, atol=1e-12)
    down = neg.failure_probability(-t, BOX, below=True, seed=2, **kw)
    check_result(neg, down, -t, 6, kw, sign=-1.0)
    assert down.n_stages == up.n_stages and np.array_equal(down.cond_prob[:, 0], up.cond_prob[:, 0])
    assert np.all(np.abs(down.log_prob - up.log_prob) <= MARGIN * 2.0 * np.sqrt(up.cov() ** 2 + down.cov() ** 2))
    # a prior concentrated away from F lowers the probability
    far = up.x.reshape(-1, 2).mean(0)
    away = np.clip(1.0 - far, 0.05, 0.95)
    pulled = paths.failure_probability(t, BOX, seed=2, prior=(away, np.array([0.5, 0.5])), **kw)
    print('uniform prior %s\nprior N(%s, 0.5^2) %s, statuses %s' % (up.prob, away, pulled.prob, pulled.status))
    # (a draw whose event the prior makes rarer than min_prob ends as below_min with an upper bound: lower still)
    assert np.all(np.isin(pulled.status, (0, 3))) and np.all(pulled.prob < up.prob)
    if np.all(pulled.status == 0):
        check_result(paths, pulled, t, 6, kw)
    flat = paths.failure_probability(t, BOX, seed=2, prior=(away, np.array([np.inf, np.inf])), **kw)
    assert same(flat, up)                                                        # an infinite sd is the uniform prior


def test_emulator_failure_probability(eng, emu_paths):
    import copy
    which, emu, paths = emu_paths
    kw = dict(n_particles=128, n_moves=2)
    t = high_value(paths, 0.99)
    res = paths.failure_probability(t, BOX, seed=7, **kw)
    check_result(paths, res, t, 6, kw)
    assert same(res, paths.failure_probability(t, BOX, seed=7, **kw))
    assert not np.array_equal(res.x, paths.failure_probability(t, BOX, seed=8, **kw).x)
    low = paths.failure_probability(high_value(paths, 0.01), BOX, below=True, seed=7, **kw)
    check_result(paths, low, high_value(paths, 0.01), 6, kw, sign=-1.0)
    state = copy.deepcopy(emu._sample_rng)
    fresh = emu.failure_probability(t, BOX, sample_size=2, n_features=64, seed=1, **SMALL)       # N = 2: four draws
    assert fresh.x.shape == (4, 64, 2) and np.all(fresh.x >= 0.0) and np.all(fresh.x <= 1.0)
    emu._sample_rng = state
    assert same(emu.failure_probability(t, BOX, sample_size=2, n_features=64, seed=1, **SMALL), fresh)
    with pytest.raises(ValueError):
        paths.failure_probability(t, BOX, output=1, **SMALL)                     # one output
    with pytest.raises(ValueError):
        paths.failure_probability(t, BOX[:1], **SMALL)


def test_refusals(eng, gp_paths):
    from dgp_amd import emulator, reliability
    m, paths = gp_paths
    np.random.seed(8)
    res = m.failure_probability(0.3, BOX, sample_size=5, n_features=64, seed=2, **SMALL)
    assert res.x.shape == (5, 64, 2)
    for bad in (BOX[0], BOX[:1], np.array([[0.0, 1.0], [np.nan, 1.0]]), np.array([[0.0, 1.0], [1.0, 0.5]])):
        with pytest.raises(ValueError):
            paths.failure_probability(0.3, bad, **SMALL)
    for kw in (dict(n_particles=1), dict(n_particles=reliability.MAX_PARTICLES + 1), dict(n_moves=0), dict(level_prob=0.0),
               dict(level_prob=1.0), dict(level_prob=np.nan), dict(max_stages=0), dict(min_prob=1.0), dict(output=1),
               dict(prior=(np.zeros(2), np.zeros(2))), dict(prior=(np.zeros(3), np.ones(3))), dict(step=0.0), dict(target_accept=1.0)):
        with pytest.raises(ValueError):
            paths.failure_probability(0.3, BOX, **dict(SMALL, **kw))
    for t in (np.nan, np.inf):
        with pytest.raises(ValueError):
            paths.failure_probability(t, BOX, **SMALL)
    np.random.seed(1)
    local = m.sample_functions_vecchia(sample_size=2, n_features=16, m=10)
    with pytest.raises(NotImplementedError, match='sample_functions '):
        local.failure_probability(0.3, BOX, **SMALL)
    X, model = T._model('hetero')
    emu = emulator(model.estimate(), N=2, seed=5)
    with pytest.raises(ValueError, match='sampled node'):
        emu.failure_probability(0.1, np.array([[0.0, 1.0]]), sample_size=2, n_features=16, **SMALL)
