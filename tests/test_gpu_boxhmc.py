"""dgpamd_boxhmc_step on the device (csrc/boxhmc.hip, DESIGN I.20) as an operator: the test computes every chain's values and
Jacobian on the host, in numpy, at the kernel's own trial points, call by call, and uploads them inside (Q, K) / (Q, K, D)
arrays whose unused entries hold NaN.  The numpy restatement tests/boxhmc_ref.py receives the same values, normal draws and
log-uniform draws; every trial point, log ratio, step, count, sample and log density must be EQUAL to its: the largest
difference expected is 0.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import boxhmc_ref as Hm
import test_boxhmc_host as H
import test_gpu_boxmala as G

pytestmark = pytest.mark.gpu
# iteration 0 is INIT; iteration i takes LENGTHS[i - 1] calls (43 calls in all); iterations 1 .. 8 adapt; every second one
# after them is saved: INIT, START, MID and DECIDE all occur, DECIDE + START back to back (L = 1) and after MID calls
LENGTHS = (1, 2, 5, 1, 1, 5, 2, 2, 5, 1, 2, 5, 1, 2, 5, 2)
WARMUP, THIN = 8, 2
SLOTS = (len(LENGTHS) - WARMUP) // THIN
STATE = ('h', 'logr', 'status', 'n_prop', 'n_acc')


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


npy = G.npy
problem = G.problem           # the MALA operator test's chains: z and logu are read per iteration here, the first 17 of 61


def schedule(lengths=LENGTHS):
    """(iteration c, first, last) of every call."""
    calls = [(0, True, lengths[0] == 1)]
    for c, L in enumerate(lengths, 1):
        calls += [(c, False, l == L) for l in range(1, L + 1)]
    return calls


def run(eng, p, rows=slice(None), restate=True, adapt=True, nan_calls=None, h0=0.1, hmin=1e-10, hmax=1e2, lengths=LENGTHS):
    """Drive the chains `rows` of problem p through the schedule.  Checks on the way: every trial lies in the box and equals
    the restatement's, and so do logr and h after every call; at the end the counts, status, samples and log densities.
    nan_calls {chain: (first call, one past the last call) whose values are NaN}.  Returns the results as host arrays,
    'logrs' and 'trials' per call."""
    x0, z, logu = p['x0'][rows], p['z'][:, rows], p['logu'][:, rows]
    Q, D = x0.shape
    nan_calls = nan_calls or {}
    state = eng.boxhmc_state(Q, D, p['w'], p['ybar'], p['lo'], p['hi'], p['s'], p['pv'], p['pm'], n_slots=SLOTS)
    chains = [Hm.Chain(x0[q], p['w'], p['ybar'], p['lo'], p['hi'], p['s'], p['pv'], p['pm'], h0, hmin, hmax) for q in range(Q)] if restate else []
    xt = eng.tensor(x0)
    trial, trials, logrs = x0.copy(), [], []
    for n, (c, first, last) in enumerate(schedule(lengths)):
        f, J = p['fun'](trial, rows)
        for q, (a, b) in nan_calls.items():
            if a <= n < b:
                f[q], J[q] = np.nan, np.nan
        on, j = adapt and last and 1 <= c <= WARMUP, c - WARMUP
        up, down = H.gain(c - 1) if on else (1.0, 1.0)
        slot = j // THIN - 1 if last and j >= 1 and j % THIN == 0 else -1
        eng.boxhmc_step(state, eng.tensor(f), eng.tensor(J), xt, eng.tensor(z[c]), eng.tensor(logu[c]), h0=h0, hmin=hmin, hmax=hmax,
                        up=up, down=down, adapt=on, first=first, last=last, slot=slot)
        trial = npy(xt)
        trials.append(trial)
        logrs.append(npy(state['logr']))
        assert np.all(trial >= p['lo']) and np.all(trial <= p['hi']), 'a trial point left the box'
        for q, ch in enumerate(chains):
            ch.step(f[q], J[q], z[c, q], logu[c, q], last, on, up, down, save=slot >= 0)
        if chains:
            ref = np.array([ch.trial for ch in chains])
            assert np.array_equal(trial, ref), ('call %d: largest |trial - restatement| %.3g' % (n, np.max(np.abs(trial - ref))))
            assert np.array_equal(logrs[-1], np.array([ch.logr for ch in chains]), equal_nan=True), 'call %d: logr' % n
            assert np.array_equal(npy(state['h']), np.array([ch.h for ch in chains])), 'call %d: h' % n
    out = {k: npy(state[k]) for k in STATE}
    out['x'], out['logp'] = npy(state['xs']).transpose(2, 0, 1), npy(state['lps']).T        # (Q, S, D), (Q, S)
    out['trials'], out['logrs'] = np.array(trials), np.array(logrs)
    out['reflections'] = sum(ch.reflections for ch in chains)
    if chains:
        ref = dict(status=[c.status for c in chains], n_prop=[c.n_prop for c in chains], n_acc=[c.n_acc for c in chains],
                   x=[c.xs for c in chains], logp=[c.lps for c in chains])
        saved = len(chains[0].xs)                                                # (a short schedule fills no slot)
        out['x'], out['logp'] = out['x'][:, :saved], out['logp'][:, :saved]
        for k, v in ref.items():
            v = np.array(v, dtype=np.float64).reshape(out[k].shape)
            with np.errstate(invalid='ignore'):
                d = np.abs(out[k] - v)
            assert np.array_equal(out[k], v, equal_nan=True), (k, 'largest difference %.3g' % np.nanmax(d, initial=0.0))
    return out


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('D', [1, 2, 5, 64])
@pytest.mark.parametrize('Q', [1, 63, 64, 65, 130])
def test_chains_equal_the_restatement(eng, Q, D, K):
    """Expected largest difference 0: the kernel and the restatement perform the same roundings.  Observed on an MI355X: 0 in
    all 40 cases; acceptance 0.56 .. 0.94, adapted steps 0.0089 .. 0.22, up to 13654 reflections in a case."""
    p = problem(Q, D, K)
    out = run(eng, p)
    rate = out['n_acc'].sum() / out['n_prop'].sum()
    print('Q %d D %d K %d: acceptance %.2f, steps %.3g .. %.3g, %d reflections' % (Q, D, K, rate, out['h'].min(), out['h'].max(), out['reflections']))
    assert np.all(out['status'] == Hm.OK) and np.all(out['n_prop'] == len(LENGTHS))
    assert np.all(np.isfinite(out['logp']))
    if Q > 1:                                                                    # (both branches of the decision ran, walls were met)
        assert 0 < out['n_acc'].sum() < out['n_prop'].sum() and len(np.unique(out['h'])) > 1 and out['reflections'] > 0


def test_fixed_columns_and_adaptation_limits(eng):
    p = problem(65, 5, 3)
    p['lo'][1] = p['hi'][1] = 0.25                                               # lo = hi
    p['x0'][:, 1] = 0.25
    p['s'] = p['hi'] - p['lo']
    p['s'][3] = 0.0                                                              # s = 0 on an open column
    out = run(eng, p)
    assert np.all(out['x'][:, :, 1] == 0.25) and np.all(out['trials'][:, :, 1] == 0.25)
    assert np.array_equal(out['x'][:, :, 3], np.broadcast_to(p['x0'][:, None, 3], out['x'].shape[:2]))
    assert np.array_equal(out['trials'][:, :, 3], np.broadcast_to(p['x0'][:, 3], out['trials'].shape[:2]))
    assert out['n_acc'].sum() > 0 and np.any(out['x'][:, -1, 0] != p['x0'][:, 0])
    still = run(eng, p, adapt=False)                                             # adapt off: the step stays h0
    assert np.all(still['h'] == 0.1)
    clamped = run(eng, p, hmin=0.09, hmax=0.11)
    assert np.all((clamped['h'] >= 0.09) & (clamped['h'] <= 0.11)) and np.any(clamped['h'] == 0.09) and np.any(clamped['h'] == 0.11)


def test_nan_chains_stay_in_their_lane(eng):
    """Chain 17 of 64 starts at NaN: status NAN, its trial and samples stay its start.  Chain 40 meets NaN at the second of
    the five calls of iteration 3 (call 5 of 43) only: that trajectory is rejected with logr NaN, the calls up to its end
    evaluate x, and the chain stays live and moves again afterwards.  The other chains keep the bits of a run without them."""
    p = problem(64, 5, 1)
    clean = run(eng, p, restate=False)
    out = run(eng, p, nan_calls={17: (0, 999), 40: (5, 6)})
    assert out['status'][17] == Hm.NAN and out['n_prop'][17] == 0
    assert np.all(out['trials'][:, 17] == p['x0'][17]) and np.all(out['x'][17] == p['x0'][17])
    calls = schedule()
    assert [calls[n][0] for n in (4, 8)] == [3, 3] and calls[8][2] and not calls[5][2]
    assert out['status'][40] == Hm.OK and out['n_prop'][40] == len(LENGTHS) and np.isnan(out['logrs'][8, 40])
    assert np.array_equal(out['trials'][:4, 40], clean['trials'][:4, 40])
    held = out['trials'][5, 40]                                                  # x of the chain during the bad trajectory
    assert all(np.array_equal(out['trials'][n, 40], held) for n in (5, 6, 7)) and not np.array_equal(out['trials'][8, 40], held)
    assert np.all(np.isfinite(out['logrs'][9:, 40])) and np.any(out['x'][40, -1] != held)
    others = ~np.isin(np.arange(64), [17, 40])
    for k in STATE + ('x', 'logp'):
        assert np.array_equal(out[k][others], clean[k][others]), k
    assert np.array_equal(out['trials'][:, others], clean['trials'][:, others])


def test_reflections_and_the_reflection_cap(eng):
    """A flat target on [0, 1] (w = 0: the values hold NaN), h = 1, s = 1, from x = 0.5: z = 0.7 drifts to 1.2 and reflects
    once to 0.8; z = 1.7 drifts to 2.2 and reflects twice, to -0.2 and to 0.2; z = -0.3 does not reflect; z = 50 would need 50
    reflections: the cap of 8 is hit, the walk evaluates x, logr = -inf and even log u = -inf does not accept it.  The
    energy of the others is conserved exactly: logr = 0 and log u = -inf accepts."""
    z0 = np.array([[0.7], [1.7], [-0.3], [50.0]])
    p = dict(w=np.zeros(1), ybar=np.full(1, np.nan), lo=np.zeros(1), hi=np.ones(1), s=np.ones(1), pv=np.zeros(1), pm=np.full(1, np.nan),
             x0=np.full((4, 1), 0.5), fun=lambda X, rows: (np.full((len(X), 1), np.nan), np.full((len(X), 1, 1), np.nan)),
             z=np.concatenate([z0[None], np.zeros((2, 4, 1))]), logu=np.full((3, 4), -np.inf))
    out = run(eng, p, h0=1.0, adapt=False, lengths=(1, 1))
    first = out['trials'][0, :, 0]
    assert np.all(np.abs(first[:3] - [0.8, 0.2, 0.2]) < 1e-15) and first[3] == 0.5
    assert np.array_equal(out['logrs'][1], [0.0, 0.0, 0.0, -np.inf])
    assert np.array_equal(out['n_acc'], [2, 2, 2, 1]) and out['reflections'] == 1 + 2 + 0 + Hm.NREFL
    big = run(eng, dict(p, z=np.ones((3, 4, 1))), h0=50.0, adapt=False, lengths=(1, 1))      # a step of 50 box widths
    assert np.all(big['logrs'][1:] == -np.inf) and np.all(big['n_acc'] == 0) and np.all(big['trials'] == 0.5)


def test_slices_of_the_chains_reproduce_the_whole_run(eng):
    """No cross-lane operation: chains [0:1], [1:65], [65:130] of a 130-chain run, each run on its own (other lanes, other
    workgroups, another Q in every address), give the same bits."""
    p = problem(130, 5, 3)
    whole = run(eng, p, restate=False)
    for a, c in ((0, 1), (1, 65), (65, 130)):
        part = run(eng, p, rows=slice(a, c), restate=False)
        for k in STATE + ('x', 'logp'):
            assert np.array_equal(part[k], whole[k][a:c], equal_nan=True), (k, a, c)
        assert np.array_equal(part['trials'], whole['trials'][:, a:c])
        assert np.array_equal(part['logrs'], whole['logrs'][:, a:c], equal_nan=True)


def test_bad_arguments_are_refused(eng):
    from dgp_amd.ops import DgpAmdError, Engine
    lo, hi = -np.ones(2), np.ones(2)
    good = dict(w=np.ones(1), ybar=np.zeros(1), lo=lo, hi=hi, scale=hi - lo)
    state = eng.boxhmc_state(4, 2, n_slots=3, **good)
    assert state['work'].numel() == Engine.boxhmc_workspace(4, 2) == 4 * (8 * (4 * 2 + 2) + 4)
    f, J, xt, z, u = eng.zeros(4, 1), eng.zeros(4, 1, 2), eng.zeros(4, 2), eng.zeros(4, 2), eng.zeros(4)
    eng.boxhmc_step(state, f, J, xt, z, u, first=True, last=True, slot=2)        # (first and last together are accepted)
    for kw in (dict(h0=0.0), dict(h0=float('nan')), dict(h0=float('inf')), dict(hmin=0.0), dict(hmin=-1.0), dict(hmax=float('inf')),
               dict(hmin=1.0, hmax=0.5), dict(up=0.0), dict(up=float('nan')), dict(down=-0.5), dict(down=float('inf')),
               dict(slot=3), dict(slot=-2)):
        with pytest.raises(DgpAmdError):
            eng.boxhmc_step(state, f, J, xt, z, u, first=True, **kw)
    for bad in (dict(w=-np.ones(1)), dict(w=np.full(1, np.nan)), dict(scale=np.array([1.0, -1.0])), dict(scale=np.array([np.nan, 1.0])),
                dict(lo=np.array([0.0, 1.0]), hi=np.array([1.0, 0.5])), dict(lo=np.array([np.nan, 0.0])), dict(hi=np.array([1.0, np.nan])),
                dict(prior_prec=np.array([-1.0, 0.0])), dict(prior_prec=np.array([np.nan, 0.0]))):
        with pytest.raises(DgpAmdError):
            eng.boxhmc_step(eng.boxhmc_state(4, 2, n_slots=3, **dict(good, **bad)), f, J, xt, z, u, first=True)
    with pytest.raises(ValueError):
        eng.boxhmc_state(4, 65, np.ones(1), np.zeros(1), -np.ones(65), np.ones(65), np.ones(65))
    with pytest.raises(ValueError):
        eng.boxhmc_state(4, 2, np.ones(1), np.zeros(1), lo, np.ones(3), hi - lo)
    with pytest.raises(ValueError):
        eng.boxhmc_state(0, 2, **good)
    with pytest.raises(ValueError):
        eng.boxhmc_step(state, f, eng.zeros(4, 1, 3), xt, z, u, first=True)
    with pytest.raises(ValueError):
        eng.boxhmc_step(state, f.float(), J, xt, z, u, first=True)
    with pytest.raises(ValueError):
        eng.boxhmc_step(state, eng.zeros(4, 2)[:, :1], J, xt, z, u, first=True)      # (not contiguous)
    with pytest.raises(ValueError):
        eng.boxhmc_step(state, eng.zeros(4, 2), eng.zeros(4, 2, 2), xt, z, u, first=True)           # (another K than the state's)
    with pytest.raises(ValueError):
        eng.boxhmc_step(state, eng.zeros(5, 1), eng.zeros(5, 1, 2), eng.zeros(5, 2), eng.zeros(5, 2), eng.zeros(5), first=True)
    with pytest.raises(ValueError):                                              # (a MALA state: its workspace is too small)
        eng.boxhmc_step(eng.boxmala_state(4, 2, n_slots=3, **good), f, J, xt, z, u, first=True)
