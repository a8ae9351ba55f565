"""dgpamd_boxsmc_move and dgpamd_boxsmc_temper on the device (csrc/boxsmc.hip, DESIGN I.21) as operators.

MOVE: the test computes every particle's values and Jacobian on the host, in numpy, at the kernel's own trial points, call by
call, and uploads them inside arrays whose unused entries hold NaN; tests/boxsmc_ref.py's Particles receives the same
numbers, and every trial, decision, step, ll, lprior and count must be EQUAL to its.

TEMPER: the device sums in its own fixed order and uses its own exponential, so it is held to the restatement evaluated at
the device's own step of beta by bounds derived here from the operations (u = 2^-53, one rounding):
  a weight: the argument fl(delta fl(m - ll_i)) is the same IEEE operations on both sides, so it is the same number; the two
    exponentials differ by at most EPS_A = 4e-16 (exp_negated, tests/test_gpu_mathfn.py) + 2 u (numpy's, one ulp).  Beyond
    an argument of 700 exp_negated returns at most 1.1e-304 against a sum of at least 1: nothing.
  a sum of R nonnegative terms, in any order: (R - 1) u each side.  S = sum a: EPS_S = EPS_A + 2 (R - 1) u.
  ESS = (S S) / sum a^2: 2 EPS_S + 2 u for the square; a^2 2 EPS_A + 2 u, its sum + 2 (R - 1) u; the quotient + 2 u:
    ESS_BOUND = 4 EPS_A + (6 R) u + 6 u, relative.
  the increment delta m + log(S / R): fl(delta m) is the same number; S / R: EPS_S + 2 u relative, which is absolute on its
    logarithm; the two logarithms within an ulp of it each, the final sum one rounding each:
    INC_BOUND = EPS_S + 2 u + 4 u |log(S / R)| + 2 u (|delta m| + |log(S / R)|), absolute.
  the step of beta, against long double: there the argument's two roundings count, 2 u 707.5 on a weight at most, so
    EPS_LD = 1415 u + 4e-16 and ESS_LD_BOUND = 4 EPS_LD + 3 R u + 6 u.  ESS falls as the step grows, and the bisection ends
    with a bracket of 2^-52 (1 - beta) around its step whose upper end missed the target on the device, so
    ESS_ld(delta) >= target (1 - bound) and, below the full step, ESS_ld(delta (1 + 1e-9)) < target (1 + bound).
  a boundary R C_i - u: C_i is a sum of at most R terms a_j / S, each EPS_A + EPS_S + 2 u apart: 2 EPS_A + 4 R u relative to
    C_i <= 1; times R, and two roundings each side on a number below R: ANC_MARGIN = R (2 EPS_A + 4 R u + 4 u).
The fixed inputs below are such that no boundary of the restatement lies within the margin of an integer
(tests/test_boxsmc_host.py checks it), so anc is compared with equality everywhere.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import boxsmc_ref as S

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
EPS_A = 4e-16 + 2 * U
MAXR = 8192


def eps_s(R):
    return EPS_A + 2 * (R - 1) * U


def ess_bound(R):
    return 4 * EPS_A + 6 * R * U + 6 * U


def ess_ld_bound(R):
    return 4 * (1415 * U + 4e-16) + 3 * R * U + 6 * U


def anc_margin(R):
    return R * (2 * EPS_A + 4 * R * U + 4 * U)


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


# -------------------------------------------------------------------------------------------------------------------- MOVE
CALLS = 20                    # call 0 starts stage 1, call 9 ends it; call 10 starts stage 2 under other betas, call 19 ends it
SHAPES = {1: (1, 1), 63: (63, 1), 64: (64, 1), 65: (5, 13), 130: (2, 65)}


def gain(c):
    from dgp_amd import calibrate
    return calibrate.gain(c, 0.574)


def problem(P, R, D, K, seed=0):
    """Particle q moves under K outputs f_k = sin(a_qk . x + b_qk); with K = 3 the middle output is unobserved (w = 0): its
    ybar, values and Jacobian hold NaN.  betas (2, P): the two stages', mixed, with 1.0, 0 and a tiny one among them."""
    Q = P * R
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
    betas = np.stack([np.resize([0.3, 1e-12, 1.0, 0.0, 0.71], P), np.resize([1.0, 0.5, 1.0, 1e-3, 0.9], P)])
    return dict(P=P, R=R, fun=fun, w=w, ybar=ybar, lo=lo, hi=hi, s=hi - lo, pv=pv, pm=pm, x0=rng.uniform(lo, hi, (Q, D)),
                z=rng.normal(size=(CALLS, Q, D)), logu=np.log(rng.uniform(size=(CALLS, Q))), betas=betas,
                perm=np.concatenate([p * R + rng.integers(0, R, R) for p in range(P)]))


def run(eng, p, draws=slice(None), restate=True, nan_from=None, hmin=1e-10, hmax=1e2):
    """Drive the particles of the draws `draws` of problem p through CALLS calls; check on the way that every trial lies in
    the box and equals the restatement's, and at the end every state field.  nan_from {particle: first call with NaN
    values}.  Returns the results as host arrays."""
    R = p['R']
    rows = np.arange(p['P'] * R).reshape(p['P'], R)[draws].reshape(-1)
    P, Q = len(rows) // R, len(rows)
    x0, z, logu, betas = p['x0'][rows], p['z'][:, rows], p['logu'][:, rows], p['betas'][:, draws]
    D = x0.shape[1]
    K = len(p['w'])
    nan_from = nan_from or {}
    state = eng.boxsmc_state(P, R, D, p['w'], p['ybar'], p['lo'], p['hi'], p['s'], p['pv'], p['pm'], h0=0.1)
    ref = S.Particles(x0, p['w'], p['ybar'], p['lo'], p['hi'], p['s'], p['pv'], p['pm'], 0.1, hmin, hmax) if restate else None
    xt = eng.tensor(x0.reshape(P, R, D))
    trial, trials, moves = x0.copy(), [], 0
    local = np.searchsorted(rows, p['perm'][rows])                               # the gather of stage 2, inside the slice
    for c in range(CALLS):
        stage, i = divmod(c, CALLS // 2)
        first, last = i == 0, i == CALLS // 2 - 1
        if c == CALLS // 2:                                                      # a second stage: gathered particles, other betas
            trial = npy(state['x']).T[local].copy()
            xt = eng.tensor(trial.reshape(P, R, D))
            if ref is not None:
                ref.trial = ref.x[local].copy()
        state['beta'].copy_(eng.tensor(betas[stage]))
        f, J = p['fun'](trial, rows)
        for q, c_bad in nan_from.items():
            if c >= c_bad:
                f[q], J[q] = np.nan, np.nan
        up, down = gain(moves) if i else (1.0, 1.0)
        eng.boxsmc_move(state, eng.tensor(f.reshape(P, R, K)), eng.tensor(J.reshape(P, R, K, D)), xt, eng.tensor(z[c].reshape(P, R, D)),
                        eng.tensor(logu[c].reshape(P, R)), hmin, hmax, up, down, adapt=i > 0, first=first, last=last)
        moves += 1 if i else 0
        trial = npy(xt).reshape(Q, D)
        trials.append(trial)
        assert np.all(trial >= p['lo']) and np.all(trial <= p['hi']), 'a trial point left the box'
        if ref is not None:
            ref.move(f, J, z[c], logu[c], np.repeat(betas[stage], R), first, last, i > 0, up, down)
            assert np.array_equal(trial, ref.trial), ('call %d: largest |trial - restatement| %.3g' % (c, np.max(np.abs(trial - ref.trial))))
            if last:
                assert np.array_equal(trial, ref.x)                              # the stage ends: the walk evaluates x
    out = {k: npy(state[k]) for k in ('h', 'logr', 'status', 'n_prop', 'n_acc', 'll', 'lprior')}
    out['x'], out['trials'] = npy(state['x']).T.copy(), np.array(trials)
    if ref is not None:
        for k in out:
            if k != 'trials':
                assert np.array_equal(out[k], getattr(ref, k), equal_nan=True), k
    return out


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('D', [1, 2, 5, 64])
@pytest.mark.parametrize('Q', [1, 63, 64, 65, 130])
def test_moves_equal_the_restatement(eng, Q, D, K):
    """Expected largest difference 0: the kernel and the restatement perform the same roundings."""
    P, R = SHAPES[Q]
    out = run(eng, problem(P, R, D, K))
    assert np.all(out['status'] == S.OK) and np.all(out['n_prop'] == CALLS // 2 - 1)
    if Q > 1:
        assert 0 < out['n_acc'].sum() < out['n_prop'].sum() and len(np.unique(out['h'])) > 1


def test_fixed_columns_and_clamps(eng):
    p = problem(5, 13, 5, 3)
    p['lo'][1] = p['hi'][1] = 0.25                                               # lo = hi
    p['x0'][:, 1] = 0.25
    p['s'] = p['hi'] - p['lo']
    p['s'][3] = 0.0                                                              # s = 0 on an open column
    out = run(eng, p)
    assert np.all(out['x'][:, 1] == 0.25) and np.all(out['trials'][:, :, 1] == 0.25)
    assert np.array_equal(out['trials'][:10, :, 3], np.broadcast_to(p['x0'][:, 3], (10, 65)))
    clamped = run(eng, p, hmin=0.09, hmax=0.11)
    assert np.all((clamped['h'] >= 0.09) & (clamped['h'] <= 0.11)) and np.any(clamped['h'] == 0.09) and np.any(clamped['h'] == 0.11)


def test_nan_particles_stay_in_their_lane(eng):
    """Particle 17 of 65 returns NaN always: status NAN at both starts, ll NaN (dead for TEMPER), its trial stays its start.
    Particle 40 returns NaN at every trial after the second stage's start: it only rejects.  The others keep the bits of a
    clean run."""
    p = problem(5, 13, 5, 1)
    p['perm'] = np.arange(65)                                                    # (the second stage starts where the first ended)
    clean = run(eng, p, restate=False)
    out = run(eng, p, nan_from={17: 0, 40: CALLS // 2 + 1})
    assert out['status'][17] == S.NAN and out['n_prop'][17] == 0 and np.isnan(out['ll'][17])
    assert np.all(out['trials'][:, 17] == p['x0'][17])
    assert out['status'][40] == S.OK and out['n_prop'][40] == CALLS // 2 - 1 and out['n_acc'][40] == 0 and np.isnan(out['logr'][40])
    assert np.array_equal(out['x'][40], out['trials'][CALLS // 2 - 1, 40])
    others = ~np.isin(np.arange(65), [17, 40])
    for k in clean:
        got, want = (out[k][:, others], clean[k][:, others]) if k == 'trials' else (out[k][others], clean[k][others])
        assert np.array_equal(got, want), k


def test_a_proposal_outside_the_box_is_rejected(eng):
    p = problem(64, 1, 2, 1)
    p['z'][1, 5, 0] = 1e300                                                      # call 1 proposes particle 5 far outside
    p['logu'][2, 5] = -np.inf                                                    # (u = 0 would accept anything of positive density)
    out = run(eng, p)                                                            # (the restatement: logr = -inf, a rejection)
    clean = run(eng, problem(64, 1, 2, 1), restate=False)
    assert np.array_equal(out['trials'][:1], clean['trials'][:1]) and not np.array_equal(out['trials'][1, 5], clean['trials'][1, 5])
    assert np.all(out['trials'][1, 5] >= p['lo']) and np.all(out['trials'][1, 5] <= p['hi'])     # the walk evaluates x, not the proposal


def test_slices_of_the_draws_reproduce_the_whole_run(eng):
    """One lane per particle, beta read per draw: draws [0:1], [1:14], [14:26] of 26 draws of 5 particles, each run on its
    own (other lanes, other workgroups, another Q in every address), give the same bits."""
    p = problem(26, 5, 5, 3)
    whole = run(eng, p, restate=False)
    for a, c in ((0, 1), (1, 14), (14, 26)):
        part = run(eng, p, draws=slice(a, c), restate=False)
        for k in part:
            want = whole[k][:, 5 * a:5 * c] if k == 'trials' else whole[k][5 * a:5 * c]
            assert np.array_equal(part[k], want, equal_nan=True), (k, a, c)


def test_bad_arguments_are_refused(eng):
    from dgp_amd.ops import DgpAmdError
    lo, hi = -np.ones(2), np.ones(2)
    good = dict(w=np.ones(1), ybar=np.zeros(1), lo=lo, hi=hi, scale=hi - lo)
    state = eng.boxsmc_state(2, 3, 2, **good)
    f, J, xt, z, u = eng.zeros(2, 3, 1), eng.zeros(2, 3, 1, 2), eng.zeros(2, 3, 2), eng.zeros(2, 3, 2), eng.zeros(2, 3)
    eng.boxsmc_move(state, f, J, xt, z, u, first=True)                           # (the arguments below are otherwise good)
    eng.boxsmc_temper(state, xt, eng.zeros(2) + 0.5)
    for kw in (dict(hmin=0.0), dict(hmin=-1.0), dict(hmax=float('inf')), dict(hmin=1.0, hmax=0.5), dict(up=0.0), dict(up=float('nan')),
               dict(down=-0.5), dict(down=float('inf'))):
        with pytest.raises(DgpAmdError):
            eng.boxsmc_move(state, f, J, xt, z, u, first=True, **kw)
    for bad in (dict(w=-np.ones(1)), dict(scale=np.array([1.0, -1.0])), dict(lo=np.array([0.0, 1.0]), hi=np.array([1.0, 0.5])),
                dict(lo=np.array([np.nan, 0.0])), dict(prior_prec=np.array([-1.0, 0.0]))):
        with pytest.raises(DgpAmdError):
            eng.boxsmc_move(eng.boxsmc_state(2, 3, 2, **dict(good, **bad)), f, J, xt, z, u, first=True)
    for ess_frac in (0.0, 1.0, -0.5, float('nan')):
        with pytest.raises(DgpAmdError):
            eng.boxsmc_temper(state, xt, eng.zeros(2), ess_frac)
    for P, R, D in ((0, 3, 2), (2, 0, 2), (2, MAXR + 1, 2), (2, 3, 65), (2, 3, 0)):
        with pytest.raises(ValueError):
            eng.boxsmc_workspace(P, R, D)
    assert eng.boxsmc_workspace(2, 3, 2) == 6 * (32 + 4) and eng.BOXSMC_MAXR == MAXR
    with pytest.raises(ValueError):
        eng.boxsmc_state(2, MAXR + 1, 2, **good)
    with pytest.raises(ValueError):
        eng.boxsmc_move(state, f, eng.zeros(2, 3, 1, 3), xt, z, u, first=True)
    with pytest.raises(ValueError):
        eng.boxsmc_move(state, f.float(), J, xt, z, u, first=True)
    with pytest.raises(ValueError):
        eng.boxsmc_move(state, f, J, eng.zeros(3, 2, 2), z, u, first=True)      # (another P and R than the state's)
    with pytest.raises(ValueError):
        eng.boxsmc_temper(state, xt, eng.zeros(3))
    with pytest.raises(ValueError):
        eng.boxsmc_temper(state, eng.zeros(6, 2), eng.zeros(2))


# ------------------------------------------------------------------------------------------------------------------ TEMPER
SIZES = [1, 2, 63, 64, 65, 256, 257, 1000, 4096, MAXR]
PATTERNS = ['equal', 'spread1', 'spread30', 'spread3000', 'dominant', 'dead', 'alldead', 'done']
TRIPLES = [('spread30', 'equal', 'dead'), ('alldead', 'spread3000', 'done'), ('dominant', 'spread1', 'spread30')]
ESS_FRAC, TD = 0.5, 3


def temper_case(R, pattern):
    """(ll (R,), beta, u, status) of one draw: fixed numbers, a function of R and the pattern alone."""
    rng = np.random.default_rng([R, PATTERNS.index(pattern), 7])
    g, u = rng.normal(size=R), rng.uniform(0.05, 0.95)
    beta = {'done': 1.0, 'spread1': 0.5, 'dead': 0.5}.get(pattern, 0.0)
    if pattern == 'equal':
        ll = np.full(R, -3.25)
    elif pattern.startswith('spread'):
        ll = -5.0 + float(pattern[6:]) * g
    elif pattern == 'dominant':
        ll = -900.0 + g
        ll[R // 3] = -1.0
    elif pattern == 'dead':
        ll = -2.0 + 3.0 * g
        ll[::3], ll[1::7] = -np.inf, np.nan
        ll[R - 1] = np.nan if R > 1 else ll[R - 1]
        if not np.isfinite(ll).any():
            ll[0] = -2.0
    elif pattern == 'alldead':
        ll = np.where(np.arange(R) % 2 == 0, np.nan, -np.inf)
    else:
        ll = -1.0 + g
    return ll, beta, u, S.OK


def run_temper(eng, R, patterns):
    """The device's TEMPER of one launch with a draw per pattern: dict of host arrays, and the inputs."""
    P = len(patterns)
    cases = [temper_case(R, pat) for pat in patterns]
    ll, beta, u = np.array([c[0] for c in cases]), np.array([c[1] for c in cases]), np.array([c[2] for c in cases])
    x = np.random.default_rng(R).normal(size=(TD, P * R))
    lo, hi = -np.ones(TD), np.ones(TD)
    state = eng.boxsmc_state(P, R, TD, np.ones(1), np.zeros(1), lo, hi, hi - lo)
    state['ll'].copy_(eng.tensor(ll.reshape(-1)))
    state['x'].copy_(eng.tensor(x))
    state['beta'].copy_(eng.tensor(beta))
    state['log_evidence'].copy_(eng.tensor(np.arange(P) * 0.0))
    state['running'].fill_(99)
    xt = eng.zeros(P, R, TD) - 7.0
    eng.boxsmc_temper(state, xt, eng.tensor(u), ESS_FRAC)
    out = {k: npy(state[k]) for k in ('beta', 'dbeta', 'log_evidence', 'stage_ess', 'draw_status', 'anc', 'running')}
    out['x_trial'] = npy(xt)
    return out, dict(ll=ll, beta=beta, u=u, x=x)


def ess_ld(ll, d):
    return float(S.ess(S.weights(np.asarray(ll, dtype=np.longdouble), np.longdouble(d))))


def check_draw(out, inp, p, R, pattern):
    ll, beta, u = inp['ll'][p], inp['beta'][p], inp['u'][p]
    d, live = out['dbeta'][p], np.isfinite(ll)
    x_p = inp['x'][:, p * R:(p + 1) * R]
    anc = out['anc'][p]
    assert anc.min() >= 0 and anc.max() < R
    assert np.array_equal(out['x_trial'][p], x_p[:, anc].T), 'x_trial is not x gathered by the device\'s anc'
    if pattern in ('done', 'alldead'):
        assert d == 0.0 and out['beta'][p] == beta and np.array_equal(anc, np.arange(R)) and np.isnan(out['stage_ess'][p])
        if pattern == 'done':
            assert out['draw_status'][p] == S.OK and out['log_evidence'][p] == 0.0
        else:
            assert out['draw_status'][p] == S.NAN and np.isnan(out['log_evidence'][p])
        return 0
    assert out['draw_status'][p] == S.OK and 0.0 < d <= 1.0 - beta
    full = d == 1.0 - beta
    assert out['beta'][p] == (1.0 if full else beta + d)
    # the step, by its property in long double
    target, b = ESS_FRAC * live.sum(), ess_ld_bound(R)
    assert ess_ld(ll, d) >= target * (1.0 - b), (pattern, R, ess_ld(ll, d), target)
    if not full:
        assert ess_ld(ll, d * (1.0 + 1e-9)) < target * (1.0 + b), (pattern, R)
    if pattern == 'equal':
        assert full and np.array_equal(anc, np.arange(R))
    if pattern == 'spread3000' and R >= 63:
        assert out['beta'][p] < 1e-2
    if pattern == 'spread1' and R >= 63:
        assert full
    if pattern == 'spread30' and R >= 63:
        assert 1e-3 < out['beta'][p] < 0.9
    # the evidence and the ESS against the restatement at the device's step
    ref = S.temper(ll, beta, u, ESS_FRAC, dbeta=d)
    a = S.weights(ll, d)
    L, dm = np.log(a.sum() / R), d * ll[live].max()
    inc_bound = eps_s(R) + 2 * U + 4 * U * abs(L) + 2 * U * (abs(dm) + abs(L))
    e_ess, e_inc = abs(out['stage_ess'][p] - ref['ess']) / ref['ess'], abs(out['log_evidence'][p] - ref['increment'])
    print('R %d %s: beta\' %.6g, ESS %.1f of %d, ESS error / bound %.3g, increment error / bound %.3g' %
          (R, pattern, out['beta'][p], out['stage_ess'][p], live.sum(), e_ess / ess_bound(R), e_inc / inc_bound))
    assert e_ess <= ess_bound(R) and e_inc <= inc_bound
    # the ancestors: dead particles have none, and they equal the restatement's
    assert np.all(live[anc]) and np.all(a[anc] > 0.0)
    if not np.array_equal(anc, ref['anc']):
        v = S.boundaries(a, u)
        gap = np.abs(v - np.round(v))[:-1]
        tie = gap.size and gap.min() <= anc_margin(R)
        raise AssertionError('%s R %d: %d ancestors differ from the restatement\'s; the nearest boundary lies %.3g from an integer, '
                             'margin %.3g: %s' % (pattern, R, np.sum(anc != ref['anc']), gap.min() if gap.size else np.nan, anc_margin(R),
                                                  'a rounding tie' if tie else 'not a tie: a bug'))
    return int(out['beta'][p] < 1.0)


@pytest.mark.parametrize('R', SIZES)
def test_temper(eng, R):
    """Every pattern alone (P = 1) and three launches of three draws: each draw's checks, the running count, and the bits of a
    draw run alone against the same draw beside others."""
    alone = {}
    for pat in PATTERNS:
        out, inp = run_temper(eng, R, [pat])
        assert out['running'][0] == check_draw(out, inp, 0, R, pat)
        alone[pat] = out
    for triple in TRIPLES:
        out, inp = run_temper(eng, R, list(triple))
        assert out['running'][0] == sum(check_draw(out, inp, p, R, pat) for p, pat in enumerate(triple))
        for p, pat in enumerate(triple):
            for k in ('beta', 'dbeta', 'log_evidence', 'stage_ess', 'draw_status', 'anc'):
                assert np.array_equal(out[k][p], alone[pat][k][0], equal_nan=True), (k, pat)
