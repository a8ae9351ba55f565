"""dgpamd_boxmala_step on the device (csrc/boxmala.hip, DESIGN I.19) as an operator: the test computes every chain's values and
Jacobian on the host, in numpy, at the kernel's own trial points, round by round, and uploads them inside (Q, K) / (Q, K, D)
arrays whose unused entries hold NaN.  The numpy restatement tests/boxmala_ref.py receives the same values, normal draws and
log-uniform draws; every trial point, decision, step, sample and log density must be EQUAL to its.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import boxmala_ref as M
import test_boxmala_host as H

pytestmark = pytest.mark.gpu
ROUNDS, WARMUP, THIN = 61, 20, 2          # call 0 is INIT; calls 1 .. 20 adapt; every second call after them is saved


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def problem(Q, D, K, seed=0):
    """Chain q samples the posterior of x given K outputs f_k = sin(a_qk . x + b_qk); with K = 3 the middle output is
    unobserved (w = 0): its ybar, values and Jacobian hold NaN.  Returns a dict of the arguments and fun(X (Q, D), rows)."""
    rng = np.random.default_rng(1000 * Q + 10 * D + K + seed)
    a, b = rng.normal(size=(Q, K, D)) / np.sqrt(D), rng.normal(size=(Q, K))
    w, ybar = rng.uniform(20.0, 60.0, K), rng.uniform(-0.5, 0.5, K)
    if K == 3:
        w[1], ybar[1] = 0.0, np.nan

    def fun(X, rows=slice(None)):
        t = np.einsum('qkd,qd->qk', a[rows], X) + b[rows]
        f, J = np.sin(t), np.cos(t)[:, :, None] * a[rows]
        if K == 3:
            f[:, 1], J[:, 1] = np.nan, np.nan
        return f, J
    lo, hi = np.full(D, -1.0), np.linspace(1.0, 2.0, D)
    pv, pm = np.where(np.arange(D) % 2 == 0, 4.0, 0.0), np.where(np.arange(D) % 2 == 0, 0.1, np.nan)
    return dict(fun=fun, w=w, ybar=ybar, lo=lo, hi=hi, s=hi - lo, pv=pv, pm=pm, x0=rng.uniform(lo, hi, (Q, D)),
                z=rng.normal(size=(ROUNDS, Q, D)), logu=np.log(rng.uniform(size=(ROUNDS, Q))))


def run(eng, p, rows=slice(None), restate=True, adapt=True, nan_from=None, h0=0.1, hmin=1e-10, hmax=1e2):
    """Drive the chains `rows` of problem p through ROUNDS calls.  Checks on the way: every trial lies in the box and equals
    the restatement's; at the end n_prop, n_acc, h, logr, status, the samples and their log densities equal its.
    nan_from {chain: first call with NaN values}.  Returns the results as host arrays."""
    x0, z, logu = p['x0'][rows], p['z'][:, rows], p['logu'][:, rows]
    Q, D = x0.shape
    S = (ROUNDS - 1 - WARMUP) // THIN
    nan_from = nan_from or {}
    state = eng.boxmala_state(Q, D, p['w'], p['ybar'], p['lo'], p['hi'], p['s'], p['pv'], p['pm'], n_slots=S)
    chains = [M.Chain(x0[q], p['w'], p['ybar'], p['lo'], p['hi'], p['s'], p['pv'], p['pm'], h0, hmin, hmax) for q in range(Q)] if restate else []
    xt = eng.tensor(x0)
    trial, trials = x0.copy(), []
    for c in range(ROUNDS):
        f, J = p['fun'](trial, rows)
        for q, c_bad in nan_from.items():
            if c >= c_bad:
                f[q], J[q] = np.nan, np.nan
        on, j = adapt and 1 <= c <= WARMUP, c - WARMUP
        up, down = H.gain(c - 1) if on else (1.0, 1.0)
        slot = j // THIN - 1 if j >= 1 and j % THIN == 0 else -1
        eng.boxmala_step(state, eng.tensor(f), eng.tensor(J), xt, eng.tensor(z[c]), eng.tensor(logu[c]), h0=h0, hmin=hmin, hmax=hmax,
                         up=up, down=down, adapt=on, first=c == 0, slot=slot)
        trial = npy(xt)
        trials.append(trial)
        assert np.all(trial >= p['lo']) and np.all(trial <= p['hi']), 'a trial point left the box'
        for q, ch in enumerate(chains):
            ch.step(f[q], J[q], z[c, q], logu[c, q], on, up, down, save=slot >= 0)
        if chains:
            ref = np.array([ch.trial for ch in chains])
            assert np.array_equal(trial, ref), ('call %d: largest |trial - restatement| %.3g' % (c, np.max(np.abs(trial - ref))))
    out = {k: npy(state[k]) for k in ('h', 'logr', 'status', 'n_prop', 'n_acc')}
    out['x'], out['logp'] = npy(state['xs']).transpose(2, 0, 1), npy(state['lps']).T        # (Q, S, D), (Q, S)
    out['trials'] = np.array(trials)
    if chains:
        ref = dict(h=[c.h for c in chains], logr=[c.logr for c in chains], status=[c.status for c in chains],
                   n_prop=[c.n_prop for c in chains], n_acc=[c.n_acc for c in chains], x=[c.xs for c in chains], logp=[c.lps for c in chains])
        for k, v in ref.items():
            with np.errstate(invalid='ignore'):
                d = np.abs(out[k] - np.array(v, dtype=np.float64))
            assert np.array_equal(out[k], np.array(v), equal_nan=True), (k, 'largest difference %.3g' % np.nanmax(d))
    return out


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('D', [1, 2, 5, 64])
@pytest.mark.parametrize('Q', [1, 63, 64, 65, 130])
def test_chains_equal_the_restatement(eng, Q, D, K):
    """Expected largest difference 0: the kernel and the restatement perform the same roundings."""
    p = problem(Q, D, K)
    out = run(eng, p)
    rate = out['n_acc'].sum() / out['n_prop'].sum()
    print('Q %d D %d K %d: acceptance %.2f, steps %.3g .. %.3g' % (Q, D, K, rate, out['h'].min(), out['h'].max()))
    assert np.all(out['status'] == M.OK) and np.all(out['n_prop'] == ROUNDS - 1)
    assert 0 < out['n_acc'].sum() < out['n_prop'].sum()                          # (both branches of the decision ran)
    assert np.all(np.isfinite(out['logp'])) and len(np.unique(out['h'])) > min(Q, 2) - 1


def test_fixed_columns_and_adaptation_limits(eng):
    p = problem(65, 5, 3)
    p['lo'][1] = p['hi'][1] = 0.25                                               # lo = hi
    p['x0'][:, 1] = 0.25
    p['s'] = p['hi'] - p['lo']
    p['s'][3] = 0.0                                                              # s = 0 on an open column
    out = run(eng, p)
    assert np.all(out['x'][:, :, 1] == 0.25) and np.all(out['trials'][:, :, 1] == 0.25)
    assert np.array_equal(out['x'][:, :, 3], np.broadcast_to(p['x0'][:, None, 3], out['x'].shape[:2]))
    assert out['n_acc'].sum() > 0 and np.any(out['x'][:, -1, 0] != p['x0'][:, 0])
    still = run(eng, p, adapt=False)                                             # adapt off: the step stays h0
    assert np.all(still['h'] == 0.1)
    clamped = run(eng, p, hmin=0.09, hmax=0.11)
    assert np.all((clamped['h'] >= 0.09) & (clamped['h'] <= 0.11)) and np.any(clamped['h'] == 0.09) and np.any(clamped['h'] == 0.11)


def test_nan_chains_stay_in_their_lane(eng):
    """Chain 17 of 65 starts at NaN: status NAN, its trial and samples stay its start.  Chain 40 returns NaN at every trial
    after its start: it never moves and counts only rejections.  The 63 other chains keep the bits of a run without them."""
    p = problem(65, 5, 1)
    clean = run(eng, p, restate=False)
    out = run(eng, p, nan_from={17: 0, 40: 1})
    assert out['status'][17] == M.NAN and out['n_prop'][17] == 0
    assert np.all(out['trials'][:, 17] == p['x0'][17]) and np.all(out['x'][17] == p['x0'][17])
    assert out['status'][40] == M.OK and out['n_prop'][40] == ROUNDS - 1 and out['n_acc'][40] == 0
    assert np.all(out['x'][40] == p['x0'][40]) and np.isnan(out['logr'][40])
    others = ~np.isin(np.arange(65), [17, 40])
    for k in ('h', 'logr', 'status', 'n_prop', 'n_acc', 'x', 'logp'):
        assert np.array_equal(out[k][others], clean[k][others]), k
    assert np.array_equal(out['trials'][:, others], clean['trials'][:, others])


def test_a_proposal_outside_the_box_is_rejected(eng):
    p = problem(64, 2, 1)
    p['z'][30, 5, 0] = 1e300                                                     # call 30 proposes chain 5 far outside
    p['logu'][31, 5] = -np.inf                                                   # (u = 0 would accept anything of positive density)
    out = run(eng, p)                                                            # (the restatement: logr = -inf, a rejection)
    assert np.array_equal(out['trials'][30, 5], out['x'][5, (30 - WARMUP) // THIN - 1])      # the evaluated trial is x, saved at call 30
    clean = run(eng, problem(64, 2, 1), restate=False)
    assert np.array_equal(out['trials'][:30], clean['trials'][:30])
    assert not np.array_equal(out['trials'][30, 5], clean['trials'][30, 5])


def test_slices_of_the_chains_reproduce_the_whole_run(eng):
    """No cross-lane operation: chains [0:1], [1:65], [65:130] of a 130-chain run, each run on its own (other lanes, other
    workgroups, another Q in every address), give the same bits."""
    p = problem(130, 5, 3)
    whole = run(eng, p, restate=False)
    for a, c in ((0, 1), (1, 65), (65, 130)):
        part = run(eng, p, rows=slice(a, c), restate=False)
        for k in ('h', 'logr', 'status', 'n_prop', 'n_acc', 'x', 'logp'):
            assert np.array_equal(part[k], whole[k][a:c], equal_nan=True), (k, a, c)
        assert np.array_equal(part['trials'], whole['trials'][:, a:c])


@pytest.mark.parametrize('seed', range(3))
def test_reversibility_on_the_device(eng, seed):
    def device_step(x, z, fun, args, h):
        w, ybar, lo, hi, s = args
        state = eng.boxmala_state(1, len(x), w, ybar, lo, hi, s)
        xt = eng.tensor(x[None])
        out = []
        for zz in (z, np.zeros(len(x))):
            f, J = fun(npy(xt)[0])
            eng.boxmala_step(state, eng.tensor(f[None]), eng.tensor(J[None]), xt, eng.tensor(zz[None]), eng.zeros(1), h0=h,
                             first=not out)
            out.append(npy(xt)[0])
        return out[0], float(npy(state['logr'])[0])
    r1, r2, bound = H.reversal(device_step, seed=seed)
    ref = H.reversal(H.ref_step, seed=seed)
    print('device log ratios %.17g, %.17g: sum %.3g, bound %.3g' % (r1, r2, r1 + r2, bound))
    assert (r1, r2) == ref[:2] and abs(r1 + r2) <= bound


def test_bad_arguments_are_refused(eng):
    from dgp_amd.ops import DgpAmdError
    lo, hi = -np.ones(2), np.ones(2)
    good = dict(w=np.ones(1), ybar=np.zeros(1), lo=lo, hi=hi, scale=hi - lo)
    state = eng.boxmala_state(4, 2, n_slots=3, **good)
    f, J, xt, z, u = eng.zeros(4, 1), eng.zeros(4, 1, 2), eng.zeros(4, 2), eng.zeros(4, 2), eng.zeros(4)
    eng.boxmala_step(state, f, J, xt, z, u, first=True, slot=2)                  # (the arguments below are otherwise good)
    for kw in (dict(h0=0.0), dict(h0=float('nan')), dict(h0=float('inf')), dict(hmin=0.0), dict(hmin=-1.0), dict(hmax=float('inf')),
               dict(hmin=1.0, hmax=0.5), dict(up=0.0), dict(up=float('nan')), dict(down=-0.5), dict(down=float('inf')),
               dict(slot=3), dict(slot=-2)):
        with pytest.raises(DgpAmdError):
            eng.boxmala_step(state, f, J, xt, z, u, first=True, **kw)
    for bad in (dict(w=-np.ones(1)), dict(w=np.full(1, np.nan)), dict(scale=np.array([1.0, -1.0])), dict(scale=np.array([np.nan, 1.0])),
                dict(lo=np.array([0.0, 1.0]), hi=np.array([1.0, 0.5])), dict(lo=np.array([np.nan, 0.0])), dict(hi=np.array([1.0, np.nan])),
                dict(prior_prec=np.array([-1.0, 0.0])), dict(prior_prec=np.array([np.nan, 0.0]))):
        with pytest.raises(DgpAmdError):
            eng.boxmala_step(eng.boxmala_state(4, 2, n_slots=3, **dict(good, **bad)), f, J, xt, z, u, first=True)
    with pytest.raises(ValueError):
        eng.boxmala_state(4, 65, np.ones(1), np.zeros(1), -np.ones(65), np.ones(65), np.ones(65))
    with pytest.raises(ValueError):
        eng.boxmala_state(4, 2, np.ones(1), np.zeros(1), lo, np.ones(3), hi - lo)
    with pytest.raises(ValueError):
        eng.boxmala_state(0, 2, **good)
    with pytest.raises(ValueError):
        eng.boxmala_step(state, f, eng.zeros(4, 1, 3), xt, z, u, first=True)
    with pytest.raises(ValueError):
        eng.boxmala_step(state, f.float(), J, xt, z, u, first=True)
    with pytest.raises(ValueError):
        eng.boxmala_step(state, eng.zeros(4, 2)[:, :1], J, xt, z, u, first=True)     # (not contiguous)
    with pytest.raises(ValueError):
        eng.boxmala_step(state, eng.zeros(4, 2), eng.zeros(4, 2, 2), xt, z, u, first=True)          # (another K than the state's)
    with pytest.raises(ValueError):
        eng.boxmala_step(state, eng.zeros(5, 1), eng.zeros(5, 1, 2), eng.zeros(5, 2), eng.zeros(5, 2), eng.zeros(5), first=True)
