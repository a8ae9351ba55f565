"""calibrate_smc's and failure_probability's stage loops on the device against a re-enactment of the restatements' loops
(boxsmc_ref.smc, boxsus_ref.sus; DESIGN I.21, I.22), bit for bit: the drivers' schedule -- which round is a stage's start and
which its end, which stream every round reads, what is recorded per stage, where the step changes and when the loop stops --
is what is held here; the kernels are held call by call in test_gpu_boxsmc.py and test_gpu_boxsus.py.  The re-enactment
follows the restatements' loops line by line, all P draws in lock-step, every step an engine call on the same streams (TEMPER's
exponentials and torch.exp are not restated bitwise on the host, so they run on the device here too); the walk is the
synthetic family of test_gpu_calibrate_schedule.py, single elementwise * and + calls, for subset simulation its values alone.
Every field of ParticlePosterior and FailureProbability must be EQUAL, NaNs in the same places.  The restatements alone, on
the CPU, show that the seeds exercise the schedule: at least two stages per draw, accepted and rejected decisions.
Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import boxsmc_ref as Sm
import boxsus_ref as Su
import philox_ref as X
import test_gpu_calibrate_schedule as CS

pytestmark = pytest.mark.gpu
P, R, DX, K = 2, 5, 3, 2
N_MOVES, MAX_STAGES = 2, 20
PRIOR = np.array([0.4, 0.0, 0.0]), np.array([0.5, np.inf, np.inf])     # a Gaussian prior on column 0 alone
PV, PM = 1.0 / (PRIOR[1] * PRIOR[1]), PRIOR[0]
Y = np.array([0.3, -0.2])
# calibrate_smc: the last column fixed by its scale; an obs_sd that takes at least 2 stages
SMC = dict(seed=11, step=0.25, obs_sd=0.05, ess_frac=0.5, target=0.574, lo=np.array([0.0, -1.0, 0.3]), hi=np.array([1.0, 1.0, 0.9]),
           scale=np.array([1.0, 2.0, 0.0]))
# failure_probability: the last column fixed by its bounds; a threshold that takes at least 2 levels
SUS = dict(seed=10, step=1.0, threshold=-0.4, output=1, sign=-1.0, level_prob=0.4, min_prob=1e-12, target=0.44, lo=np.array([0.0, -1.0, 0.6]),
           hi=np.array([1.0, 1.0, 0.6]))
RNGS = ('numpy', 'device')


def family():
    """a (P, K), b (P, K, 3), c (P, K) of f_pk(x) = a_pk + b_pk0 x_0 + b_pk1 x_1 + b_pk2 x_2 + c_pk (x_0 x_1)."""
    rng = np.random.default_rng(11)
    return rng.normal(size=(P, K)), rng.normal(size=(P, K, DX)), rng.normal(size=(P, K))


def host_fun(a, b, c):
    """fun(x (R, 3)) -> (f (R, K), J (R, K, 3)) of one path: the device's sequence of operations."""
    def fun(x):
        x0, x1, x2 = (x[:, d:d + 1] for d in range(DX))
        f = a + b[:, 0] * x0
        f = f + b[:, 1] * x1
        f = f + b[:, 2] * x2
        f = f + c * (x0 * x1)
        j0, j1 = b[:, 0] + c * x1, b[:, 1] + c * x0
        return f, np.stack((j0, j1, np.broadcast_to(b[:, 2], j0.shape)), -1)
    return fun


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def same(res, ref):
    """Every field of the driver's result EQUAL to the re-enactment's."""
    for name, want in ref.items():
        got = getattr(res, name)
        if isinstance(want, np.ndarray):
            assert isinstance(got, np.ndarray) and got.shape == want.shape and got.dtype == want.dtype, (name, got, want)
            assert np.array_equal(got, want, equal_nan=True), (name, got, want)
        else:
            assert type(got) is type(want) and got == want, (name, got, want)


def on_device(eng, a):
    import torch
    return a if torch.is_tensor(a) else eng.tensor(a)


def on_host(a):
    import torch
    return a.cpu().numpy() if torch.is_tensor(a) else a


def rate_of(state):
    """(rate (P,), accepted, proposed): the stage's acceptance per draw, and its counts over all draws."""
    n_acc, n_prop = state['n_acc'].view(P, R).sum(1), state['n_prop'].view(P, R).sum(1)
    return n_acc.double() / n_prop.clamp(min=1).double(), int(n_acc.sum()), int(n_prop.sum())


# ------------------------------------------------------------------------------------------------------------- calibrate_smc
def smc_restated(rng):
    """boxsmc_ref.smc of every draw, on the numpy streams or on the host twins of the device's."""
    from dgp_amd import calibrate
    a, b, c = family()
    w = np.full(K, 1.0 / (SMC['obs_sd'] * SMC['obs_sd']))
    make = X.SmcStreams if rng == 'device' else calibrate.SmcStreams
    x0 = calibrate.prior_draws(make(SMC['seed'], P, R, DX).prior_uniforms(), SMC['lo'], SMC['hi'], PV, PM)
    gain = lambda stage, rate: calibrate.stage_gain(stage, rate, SMC['target'])
    return [Sm.smc(host_fun(a[p], b[p], c[p]), x0[p], w, Y, SMC['lo'], SMC['hi'], SMC['scale'], make(SMC['seed'], P, R, DX), gain,
                   N_MOVES, SMC['ess_frac'], MAX_STAGES, PV, PM, SMC['step'], p) for p in range(P)]


def smc_reenacted(eng, value_and_jac, rng):
    """boxsmc_ref.smc's loop in engine calls: the fields of ParticlePosterior, and the decisions (accepted, proposed)."""
    import torch
    from dgp_amd import calibrate
    w = np.full(K, 1.0 / (SMC['obs_sd'] * SMC['obs_sd']))
    lo, hi = SMC['lo'], SMC['hi']
    streams = calibrate.DeviceSmcStreams(eng, SMC['seed'], P, R, DX) if rng == 'device' else calibrate.SmcStreams(SMC['seed'], P, R, DX)
    xt = eng.tensor(np.ascontiguousarray(calibrate.prior_draws(on_host(streams.prior_uniforms()), lo, hi, PV, PM)))
    pt = eng.boxsmc_state(P, R, DX, w, Y, lo, hi, SMC['scale'], PV, PM, h0=SMC['step'])
    f, J = value_and_jac(xt)
    eng.boxsmc_move(pt, f, J, xt, eng.zeros(P, R, DX), eng.zeros(P, R), calibrate.HMIN, calibrate.HMAX, first=True, last=True)
    betas, esss, rates, accepted, proposed = [], [], [], 0, 0
    for stage in range(MAX_STAGES):
        u, z, logu = (on_device(eng, t) for t in streams.stage(N_MOVES + 1))
        eng.boxsmc_temper(pt, xt, u, SMC['ess_frac'])
        betas.append(on_host(pt['beta']).copy()), esss.append(on_host(pt['stage_ess']).copy())
        for i in range(N_MOVES + 1):
            f, J = value_and_jac(xt)
            eng.boxsmc_move(pt, f, J, xt, z[i], logu[i], calibrate.HMIN, calibrate.HMAX, first=i == 0, last=i == N_MOVES)
        rate, n_acc, n_prop = rate_of(pt)
        rates.append(on_host(rate))
        accepted, proposed = accepted + n_acc, proposed + n_prop
        pt['h'].view(P, R).mul_(torch.exp(rate - SMC['target'])[:, None]).clamp_(calibrate.HMIN, calibrate.HMAX)
        if not np.any((on_host(pt['beta']) < 1.0) & (on_host(pt['draw_status']) == Sm.OK)):
            break
    beta, status = on_host(pt['beta']), on_host(pt['draw_status']).copy()
    status[(status == Sm.OK) & (beta < 1.0)] = Sm.MAX_STAGES
    T = len(betas)
    ll, lprior = on_host(pt['ll']).reshape(P, R), on_host(pt['lprior']).reshape(P, R)
    ref = dict(x=np.ascontiguousarray(np.moveaxis(on_host(pt['x']).reshape(DX, P, R), 0, 2)), loglik=ll, logp=ll + lprior,
               log_evidence=on_host(pt['log_evidence']), log_norm=calibrate.log_norm(Y, SMC['obs_sd'], K), betas=np.stack(betas, 1),
               stage_ess=np.stack(esss, 1), accept_rate=np.stack(rates, 1), step=on_host(pt['h']).reshape(P, R), status=status,
               n_stages=T, evaluations=T * (N_MOVES + 1), rng=rng)
    return ref, accepted, proposed


@pytest.mark.parametrize('rng', RNGS)
def test_calibrate_smc_follows_the_restatements_schedule(eng, rng):
    """Expected largest difference 0 in every field.  The restatement alone: every draw takes at least 2 stages and ends at
    beta = 1, and its stages' acceptance rates are not all 0 and not all 1."""
    from dgp_amd import calibrate
    runs = smc_restated(rng)
    print('%s: restated stages %s, acceptance %s' % (rng, [len(r['betas']) for r in runs], [np.round(r['accept_rate'], 2) for r in runs]))
    assert all(len(r['betas']) >= 2 and r['status'] == Sm.OK for r in runs)
    assert any(v > 0.0 for r in runs for v in r['accept_rate']) and any(v < 1.0 for r in runs for v in r['accept_rate'])
    value_and_jac = CS.device_fun(eng, *family())
    ref, accepted, proposed = smc_reenacted(eng, value_and_jac, rng)
    print('%s: %d stages, betas %s, %d of %d decisions accepted' % (rng, ref['n_stages'], ref['betas'].tolist(), accepted, proposed))
    assert ref['n_stages'] == max(len(r['betas']) for r in runs) >= 2 and 0 < accepted < proposed
    assert np.all(ref['status'] == Sm.OK) and np.all(ref['betas'][:, -1] == 1.0) and np.all(ref['betas'][:, 0] < 1.0)
    res = calibrate.calibrate_smc(eng, P, K, DX, None, value_and_jac, 8, Y, SMC['obs_sd'], np.stack((SMC['lo'], SMC['hi']), 1),
                                  n_particles=R, n_moves=N_MOVES, ess_frac=SMC['ess_frac'], max_stages=MAX_STAGES, seed=SMC['seed'],
                                  step=SMC['step'], scale=SMC['scale'], prior=PRIOR, target_accept=SMC['target'], rng=rng)
    same(res, ref)
    assert np.all(res.x[..., 2] == res.x[:, :1, 2]) and len(vars(res)) == len(ref)


# ------------------------------------------------------------------------------------------------------- failure_probability
def sus_restated(rng):
    """boxsus_ref.sus of every draw, on the numpy streams or on the host twins of the device's."""
    from dgp_amd import calibrate, reliability
    a, b, c = family()
    make = X.SusStreams if rng == 'device' else reliability.SusStreams
    x0 = calibrate.prior_draws(make(SUS['seed'], P, R, DX).prior_uniforms(), SUS['lo'], SUS['hi'], PV, PM)
    n_s = reliability.n_survivors(SUS['level_prob'], R)
    return [Su.sus(lambda x, p=p: host_fun(a[p], b[p], c[p])(x)[0], x0[p], SUS['lo'], SUS['hi'], SUS['threshold'],
                   make(SUS['seed'], P, R, DX), n_s, N_MOVES, MAX_STAGES, SUS['min_prob'], SUS['step'], SUS['target'], PV, PM, SUS['sign'], SUS['output'], p)
            for p in range(P)]


def sus_reenacted(eng, values, rng):
    """boxsus_ref.sus's loop in engine calls: the fields of FailureProbability, and the decisions (accepted, proposed)."""
    import torch
    from dgp_amd import calibrate, reliability
    lo, hi = SUS['lo'], SUS['hi']
    streams = reliability.DeviceSusStreams(eng, SUS['seed'], P, R, DX) if rng == 'device' else reliability.SusStreams(SUS['seed'], P, R, DX)
    x0 = np.ascontiguousarray(calibrate.prior_draws(on_host(streams.prior_uniforms()), lo, hi, PV, PM))
    xt = eng.tensor(x0)
    pt = eng.boxsus_state(P, R, DX, lo, hi, PV, PM, SUS['step'])
    pt['sd'].copy_(eng.tensor(np.ascontiguousarray(np.std(x0, axis=1))))
    n_s, zero = reliability.n_survivors(SUS['level_prob'], R), eng.zeros(P, R, DX)
    eng.boxsus_move(pt, values(xt), xt, zero, zero, SUS['threshold'], SUS['output'], SUS['sign'], first=True, last=True)
    going, levels, conds, rates, lams, accepted, proposed = [], [], [], [], [], 0, 0
    for stage in range(MAX_STAGES):
        z, logu = (on_device(eng, t) for t in streams.stage(N_MOVES + 1))
        going.append(on_host(pt['done']) == 0)
        eng.boxsus_level(pt, xt, n_s, SUS['min_prob'])
        levels.append(on_host(pt['level']).copy()), conds.append(on_host(pt['nsurv']) / R), lams.append(on_host(pt['lam']).copy())
        for i in range(N_MOVES + 1):
            eng.boxsus_move(pt, values(xt), xt, z[i], logu[i], SUS['threshold'], SUS['output'], SUS['sign'], first=i == 0, last=i == N_MOVES)
        rate, n_acc, n_prop = rate_of(pt)
        rates.append(on_host(rate))
        accepted, proposed = accepted + n_acc, proposed + n_prop
        pt['lam'].mul_(torch.exp(rate - SUS['target'])).clamp_(Su.LAM_MIN, Su.LAM_MAX)
        if np.all(on_host(pt['done']) != 0):
            break
    status = on_host(pt['draw_status']).copy()
    status[(status == Su.OK) & (on_host(pt['done']) == 0)] = Su.MAX_STAGES
    T, going = len(levels), np.stack(going, 1)
    per_stage = lambda rows: np.where(going, np.stack(rows, 1).astype(np.float64), np.nan)
    ref = dict(prob=on_host(pt['prob']), levels=per_stage(levels), cond_prob=per_stage(conds), accept_rate=per_stage(rates),
               step=per_stage(lams), x=np.ascontiguousarray(np.moveaxis(on_host(pt['x']).reshape(DX, P, R), 0, 2)),
               score=on_host(pt['score']).reshape(P, R), status=status, n_stages=T, evaluations=T * (N_MOVES + 1), rng=rng)
    return ref, accepted, proposed


@pytest.mark.parametrize('rng', RNGS)
def test_failure_probability_follows_the_restatements_schedule(eng, rng):
    """Expected largest difference 0 in every field.  The restatement alone: every draw takes at least 2 levels and reaches
    the threshold, and its stages' acceptance rates are not all 0 and not all 1."""
    from dgp_amd import reliability
    runs = sus_restated(rng)
    print('%s: restated levels %s, acceptance %s' % (rng, [np.round(r['levels'], 3) for r in runs], [np.round(r['accept_rate'], 2) for r in runs]))
    assert all(len(r['levels']) >= 2 and r['status'] == Su.OK for r in runs)
    assert any(v > 0.0 for r in runs for v in r['accept_rate']) and any(v < 1.0 for r in runs for v in r['accept_rate'])
    value_and_jac = CS.device_fun(eng, *family())
    values = lambda xt: value_and_jac(xt)[0]
    ref, accepted, proposed = sus_reenacted(eng, values, rng)
    print('%s: %d stages, levels %s, %d of %d decisions accepted' % (rng, ref['n_stages'], ref['levels'].tolist(), accepted, proposed))
    assert ref['n_stages'] == max(len(r['levels']) for r in runs) >= 2 and 0 < accepted < proposed
    assert np.all(ref['status'] == Su.OK) and np.all(np.sum(~np.isnan(ref['levels']), 1) >= 2)
    res = reliability.failure_probability(eng, P, K, DX, values, SUS['threshold'], np.stack((SUS['lo'], SUS['hi']), 1), output=SUS['output'],
                                          below=SUS['sign'] < 0.0,
                                          n_particles=R, level_prob=SUS['level_prob'], n_moves=N_MOVES, max_stages=MAX_STAGES,
                                          min_prob=SUS['min_prob'], seed=SUS['seed'], step=SUS['step'], prior=PRIOR,
                                          target_accept=SUS['target'], rng=rng)
    same(res, ref)
    assert np.all(res.x[..., 2] == SUS['lo'][2]) and len(vars(res)) == len(ref)
