"""dgpamd_boxsus_move and dgpamd_boxsus_level on the device (csrc/boxsus.hip, DESIGN I.22) as operators.

MOVE: the test computes every particle's values on the host, in numpy, at the kernel's own trial points, call by call, and
uploads them inside arrays whose unread outputs hold NaN; tests/boxsus_ref.py's Particles receives the same numbers, and
every trial, decision, score and count must be EQUAL to its.

LEVEL: the level is the k-th largest of the same numbers, the counts are integers, the product is one division and one
product, and the restatement's wg_sum adds in the device's order, so level (bits), nsurv, prob, done, status, anc, x_trial and
running must be EQUAL.  sd = sqrt(s / n_b): s / n_b is the same IEEE operations on both sides, hence the same number; numpy's
square root is correctly rounded and the device's is held to one unit in the last place of it (the documented accuracy of the
device library's double sqrt), so |sd - restatement| <= 2^-52 sd; the observed fraction of that bound is printed (0 where
the device's root is correctly rounded too).  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import boxsus_ref as S

pytestmark = pytest.mark.gpu
MAXR = 8192
ULP = 2.0 ** -52


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
CALLS = 20                    # call 0 starts stage 1, call 9 ends it; call 10 starts stage 2 at other levels, call 19 ends it
SHAPES = {1: (1, 1), 63: (63, 1), 64: (32, 2), 65: (5, 13), 130: (2, 65)}        # Q: (P, R)


def problem(P, R, D, K, prior=True, below=False, seed=0):
    """Particle q has K outputs f_k = sin(a_qk . x + b_qk); with K = 3 output 1 is the one read and the others hold NaN.
    levels, lams (2, P): the two stages', mixed: -inf (everything is inside), levels that reject some, +0.0."""
    Q = P * R
    rng = np.random.default_rng(1000 * Q + 10 * D + K + seed)
    a, b = rng.normal(size=(Q, K, D)) / np.sqrt(D), rng.normal(size=(Q, K))
    output = 1 if K == 3 else 0

    def fun(X, rows=slice(None)):
        f = np.sin(np.einsum('qkd,qd->qk', a[rows], X) + b[rows])
        if K == 3:
            f[:, 0], f[:, 2] = np.nan, np.nan
        return f
    lo, hi = np.full(D, -1.0), np.linspace(1.0, 2.0, D)
    even = np.arange(D) % 2 == 0
    pv, pm = (np.where(even, 4.0, 0.0), np.where(even, 0.1, np.nan)) if prior else (None, None)
    levels = np.stack([np.resize([-0.7, -np.inf, -0.2, -1.5, -0.4], P), np.resize([0.0, -0.3, -0.05, -np.inf, -0.6], P)])
    lams = np.stack([np.resize([1.0, 0.3, 2.5], P), np.resize([0.5, 1.0, 0.1, 4.0], P)])
    return dict(P=P, R=R, fun=fun, output=output, threshold=0.15, sign=-1.0 if below else 1.0, lo=lo, hi=hi, pv=pv, pm=pm,
                x0=rng.uniform(lo, hi, (Q, D)), sd=rng.uniform(0.05, 0.6, (P, D)), levels=levels, lams=lams,
                z=rng.normal(size=(CALLS, Q, D)), logu=np.log(rng.uniform(size=(CALLS, Q, D))),
                perm=np.concatenate([p * R + rng.integers(0, R, R) for p in range(P)]))


def run(eng, p, draws=slice(None), restate=True, nan_from=None):
    """Drive the particles of the draws `draws` of problem p through CALLS calls; check on the way that every trial lies in
    the box and equals the restatement's, and at the end every state field.  nan_from {particle: first call with NaN
    values}.  Returns the results as host arrays."""
    R = p['R']
    rows = np.arange(p['P'] * R).reshape(p['P'], R)[draws].reshape(-1)
    P, Q = len(rows) // R, len(rows)
    x0, z, logu = p['x0'][rows], p['z'][:, rows], p['logu'][:, rows]
    levels, lams, sd = p['levels'][:, draws], p['lams'][:, draws], p['sd'][draws]
    D, nan_from = x0.shape[1], nan_from or {}
    state = eng.boxsus_state(P, R, D, p['lo'], p['hi'], p['pv'], p['pm'])
    state['sd'].copy_(eng.tensor(sd))
    ref = S.Particles(x0, R, p['lo'], p['hi'], p['threshold'], p['output'], p['sign'], p['pv'], p['pm']) if restate else None
    xt = eng.tensor(x0.reshape(P, R, D))
    trial, trials = x0.copy(), []
    local = np.searchsorted(rows, p['perm'][rows])                               # the gather of stage 2, inside the slice
    for c in range(CALLS):
        stage, i = divmod(c, CALLS // 2)
        first, last = i == 0, i == CALLS // 2 - 1
        if c == CALLS // 2:                                                      # a second stage: gathered particles, other levels
            trial = npy(state['x']).T[local].copy()
            xt = eng.tensor(trial.reshape(P, R, D))
            if ref is not None:
                ref.trial = ref.x[local].copy()
        state['level'].copy_(eng.tensor(levels[stage]))
        state['lam'].copy_(eng.tensor(lams[stage]))
        f = p['fun'](trial, rows)
        for q, c_bad in nan_from.items():
            if c >= c_bad:
                f[q] = np.nan
        eng.boxsus_move(state, eng.tensor(f.reshape(P, R, -1)), xt, eng.tensor(z[c].reshape(P, R, D)),
                        eng.tensor(logu[c].reshape(P, R, D)), p['threshold'], p['output'], p['sign'], first=first, last=last)
        trial = npy(xt).reshape(Q, D)
        trials.append(trial)
        assert np.all(trial >= p['lo']) and np.all(trial <= p['hi']), 'a trial point left the box'
        if ref is not None:
            ref.move(f, z[c], logu[c], levels[stage], lams[stage], sd, first, last)
            assert np.array_equal(trial, ref.trial), ('call %d: largest |trial - restatement| %.3g' % (c, np.max(np.abs(trial - ref.trial))))
            if last:
                assert np.array_equal(trial, ref.x)                              # the stage ends: the walk evaluates x
    out = {k: npy(state[k]) for k in ('score', 'status', 'n_prop', 'n_acc')}
    out['moved'] = npy(state['moved']) != 0
    out['x'], out['trials'] = npy(state['x']).T.copy(), np.array(trials)
    if ref is not None:
        for k in out:
            if k != 'trials':
                assert np.array_equal(out[k], getattr(ref, k), equal_nan=True), k
    return out


@pytest.mark.parametrize('prior', [True, False])
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('D', [1, 2, 5, 64])
@pytest.mark.parametrize('Q', [1, 63, 64, 65, 130])
def test_moves_equal_the_restatement(eng, Q, D, K, prior):
    """Expected largest difference 0: the kernel and the restatement perform the same roundings."""
    P, R = SHAPES[Q]
    out = run(eng, problem(P, R, D, K, prior))
    assert np.all(out['status'] == S.OK) and np.all(out['n_prop'] == CALLS // 2 - 1)
    if Q > 1:
        assert 0 < out['n_acc'].sum() < out['n_prop'].sum()


def test_below_flips_the_score(eng):
    """sign = -1: the event is f <= threshold.  Both runs equal their restatements; a particle that accepted a move in the
    second stage holds a score at or above its draw's level."""
    p, m = problem(5, 13, 5, 3), problem(5, 13, 5, 3, below=True)
    up, down = run(eng, p), run(eng, m)
    assert not np.array_equal(up['score'], down['score'])
    for out in (up, down):
        took = out['n_acc'] > 0
        assert took.any() and np.all(out['score'][took] >= np.repeat(p['levels'][1], 13)[took])


def test_fixed_columns(eng):
    p = problem(5, 13, 5, 3)
    p['lo'][1] = p['hi'][1] = 0.25                                               # lo = hi
    p['x0'][:, 1] = 0.25
    p['sd'][:, 3] = 0.0                                                          # sd = 0 on an open column, every draw
    p['sd'][2, 0] = 0.0                                                          # and on one draw's column 0
    out = run(eng, p)
    assert np.all(out['x'][:, 1] == 0.25) and np.all(out['trials'][:, :, 1] == 0.25)
    assert np.array_equal(out['trials'][:10, :, 3], np.broadcast_to(p['x0'][:, 3], (10, 65)))
    assert np.array_equal(out['trials'][:10, 26:39, 0], np.broadcast_to(p['x0'][26:39, 0], (10, 13)))
    assert not np.array_equal(out['trials'][1, :26, 0], p['x0'][:26, 0])


def test_nan_particles_stay_in_their_lane(eng):
    """Particle 17 of 65 returns NaN always: status NAN at both starts, score NaN (dead for LEVEL), its trial stays its
    start.  Particle 40 returns NaN at every trial after the second stage's start: it only rejects.  The others keep the bits
    of a clean run."""
    p = problem(5, 13, 5, 1)
    p['perm'] = np.arange(65)                                                    # (the second stage starts where the first ended)
    clean = run(eng, p, restate=False)
    out = run(eng, p, nan_from={17: 0, 40: CALLS // 2 + 1})
    assert out['status'][17] == S.NAN and out['n_prop'][17] == 0 and np.isnan(out['score'][17])
    assert np.all(out['trials'][:, 17] == p['x0'][17])
    assert out['status'][40] == S.OK and out['n_prop'][40] == CALLS // 2 - 1 and out['n_acc'][40] == 0
    assert np.array_equal(out['x'][40], out['trials'][CALLS // 2 - 1, 40]) and not np.isnan(out['score'][40])
    others = ~np.isin(np.arange(65), [17, 40])
    for k in clean:
        got, want = (out[k][:, others], clean[k][:, others]) if k == 'trials' else (out[k][others], clean[k][others])
        assert np.array_equal(got, want), k


def run_calls(eng, p, n):
    """The counts and the moved flags after the first n calls of stage 1 (first on call 0, no last)."""
    P, R, D = p['P'], p['R'], p['x0'].shape[1]
    state = eng.boxsus_state(P, R, D, p['lo'], p['hi'], p['pv'], p['pm'])
    state['sd'].copy_(eng.tensor(p['sd']))
    state['level'].copy_(eng.tensor(p['levels'][0]))
    state['lam'].copy_(eng.tensor(p['lams'][0]))
    xt = eng.tensor(p['x0'].reshape(P, R, D))
    for c in range(n):
        f = p['fun'](npy(xt).reshape(P * R, D))
        eng.boxsus_move(state, eng.tensor(f.reshape(P, R, -1)), xt, eng.tensor(p['z'][c].reshape(P, R, D)),
                        eng.tensor(p['logu'][c].reshape(P, R, D)), p['threshold'], p['output'], p['sign'], first=c == 0)
    return {k: npy(state[k]) for k in ('n_prop', 'n_acc', 'moved')}


def test_a_proposal_with_every_column_thrown_out_is_a_rejection(eng):
    """Call 1 proposes particle 5 far outside the box in every column: no column is kept, the moved flag stays down, the walk
    evaluates x, and call 2 counts a rejection although the level (-inf) lets everything in."""
    p = problem(32, 2, 2, 1)
    p['levels'][0, :] = -np.inf
    p['z'][1, 5] = 1e300
    out = run(eng, p)                                                            # (the restatement agrees call by call)
    assert np.array_equal(out['trials'][1, 5], out['trials'][0, 5])              # x after call 1's decision, not the proposal
    two, three = run_calls(eng, p, 2), run_calls(eng, p, 3)
    assert two['moved'][5] == 0 and two['moved'].sum() > 0
    assert three['n_prop'][5] == 2 and three['n_acc'][5] == two['n_acc'][5]
    others = np.arange(64) != 5
    assert np.array_equal(three['n_acc'][others], two['n_acc'][others] + two['moved'][others])


def test_slices_of_the_draws_reproduce_the_whole_run(eng):
    """One lane per particle, level, lam and sd read per draw: draws [0:1], [1:14], [14:26] of 26 draws of 5 particles, each
    run on its own (other lanes, other workgroups, another Q in every address), give the same bits."""
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
    state = eng.boxsus_state(2, 3, 2, lo, hi)
    f, xt, z, u = eng.zeros(2, 3, 1), eng.zeros(2, 3, 2), eng.zeros(2, 3, 2), eng.zeros(2, 3, 2)
    eng.boxsus_move(state, f, xt, z, u, 0.0, first=True)                         # (the arguments below are otherwise good)
    eng.boxsus_level(state, xt, 1)
    for kw in (dict(output=1), dict(output=-1), dict(sign=0.5), dict(sign=float('nan')), dict(threshold=float('inf')),
               dict(threshold=float('nan'))):
        with pytest.raises(DgpAmdError):
            eng.boxsus_move(state, f, xt, z, u, **dict(dict(threshold=0.0, first=True), **kw))
    for bad in (dict(lo=np.array([0.0, 1.0]), hi=np.array([1.0, 0.5])), dict(lo=np.array([np.nan, 0.0]), hi=hi),
                dict(lo=lo, hi=hi, prior_prec=np.array([-1.0, 0.0])), dict(lo=lo, hi=hi, prior_prec=np.array([np.nan, 0.0]))):
        with pytest.raises(DgpAmdError):
            eng.boxsus_move(eng.boxsus_state(2, 3, 2, **dict(dict(lo=lo, hi=hi), **bad)), f, xt, z, u, 0.0, first=True)
    for n_s, min_prob in ((0, 1e-12), (3, 1e-12), (-1, 1e-12), (1, -0.1), (1, 1.0), (1, float('nan'))):
        with pytest.raises(DgpAmdError):
            eng.boxsus_level(state, xt, n_s, min_prob)
    for P, R, D in ((0, 3, 2), (2, 0, 2), (2, MAXR + 1, 2), (2, 3, 65), (2, 3, 0), (1 << 18, MAXR, 1)):
        with pytest.raises(ValueError):
            eng.boxsus_state(P, R, D, np.zeros(max(D, 0)), np.ones(max(D, 0)))
    assert eng.BOXSUS_MAXR == MAXR and eng.BOXSUS == dict(ok=0, nan=1, max_stages=2, below_min=3)
    with pytest.raises(ValueError):
        eng.boxsus_move(state, eng.zeros(2, 3), xt, z, u, 0.0, first=True)
    with pytest.raises(ValueError):
        eng.boxsus_move(state, f.float(), xt, z, u, 0.0, first=True)
    with pytest.raises(ValueError):
        eng.boxsus_move(state, f, xt, z, eng.zeros(2, 3), 0.0, first=True)      # (log u per column, not per particle)
    with pytest.raises(ValueError):
        eng.boxsus_move(state, f, eng.zeros(3, 2, 2), z, u, 0.0, first=True)    # (another P and R than the state's)
    with pytest.raises(ValueError):
        eng.boxsus_level(state, eng.zeros(6, 2), 1)
    with pytest.raises(DgpAmdError):                                             # (one particle has no level to take: n_s < R)
        eng.boxsus_level(eng.boxsus_state(2, 1, 2, lo, hi), eng.zeros(2, 1, 2), 1)


# ------------------------------------------------------------------------------------------------------------------- LEVEL
SIZES = [2, 3, 63, 64, 65, 256, 257, 1000, 4096, MAXR]
PATTERNS = ['distinct', 'equal', 'blocks', 'ulps', 'zeros', 'infs', 'dead', 'alldead', 'final', 'done', 'below_min']
TRIPLES = [('distinct', 'equal', 'dead'), ('alldead', 'blocks', 'done'), ('zeros', 'ulps', 'below_min'), ('infs', 'final', 'distinct')]
LEVEL_PROB, MIN_PROB, TD = 0.1, 1e-12, 3


def level_case(R, pattern):
    """(score (R,), prob, done) of one draw: fixed numbers, a function of R and the pattern alone."""
    rng = np.random.default_rng([R, PATTERNS.index(pattern), 11])
    g = rng.normal(size=R)
    n_s = max(1, R // 10)
    prob, done = 1e-3, 0
    if pattern == 'distinct':
        s = -3.0 + g
    elif pattern == 'equal':
        s = np.full(R, -2.5)
    elif pattern == 'blocks':                          # what cloning leaves behind: runs of duplicates, one run straddling the level
        s = np.repeat(-3.0 + np.sort(g[:(R + 6) // 7])[::-1], 7)[:R]
        s = s[rng.permutation(R)]
    elif pattern == 'ulps':                            # values one ulp apart around the level
        s = np.nextafter(-1.0, 0.0) + np.zeros(R)
        s[::2], s[1::3] = -1.0, np.nextafter(np.nextafter(-1.0, 0.0), 0.0)
    elif pattern == 'zeros':                           # +-0 and tiny values around 0; the n_s-th largest is a zero of either sign
        pool = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-300, -1e-300, -1.0])
        s = pool[rng.integers(0, len(pool), R)]
        s[:2] = [-0.0, -5e-324]
    elif pattern == 'infs':
        s = -3.0 + g
        s[::4], s[1::9] = -np.inf, np.inf
    elif pattern == 'dead':
        s = -3.0 + g
        s[::3] = np.nan
        s[R - 1] = np.nan
        s[1] = -2.0
    elif pattern == 'alldead':
        s = np.full(R, np.nan)
    elif pattern == 'final':
        s = 1.0 + g                                    # most scores are >= 0 already
        s[0] = 0.5
    elif pattern == 'done':
        s, done = -3.0 + g, 1
    else:                                              # below_min
        s, prob = -3.0 + g, 1.5e-12
    return s, prob, done, n_s


def run_level(eng, R, patterns):
    """The device's LEVEL of one launch with a draw per pattern: dict of host arrays, and the inputs."""
    P = len(patterns)
    cases = [level_case(R, pat) for pat in patterns]
    score, prob, done = np.array([c[0] for c in cases]), np.array([c[1] for c in cases]), np.array([c[2] for c in cases])
    rng = np.random.default_rng(R)
    x = rng.normal(size=(P, TD, R)) * np.array([1.0, 1e-3, 50.0])[:, None] + np.array([0.0, 7.0, -3.0])[:, None]
    x[:, 2] = np.round(x[:, 2])                        # a column of few values: survivors that all agree give sd = 0
    sd0 = rng.uniform(0.1, 0.2, (P, TD))
    lo, hi = np.full(TD, -1e3), np.full(TD, 1e3)
    state = eng.boxsus_state(P, R, TD, lo, hi)
    state['score'].copy_(eng.tensor(score.reshape(-1)))
    state['x'].copy_(eng.tensor(np.ascontiguousarray(x.transpose(1, 0, 2).reshape(TD, P * R))))
    state['prob'].copy_(eng.tensor(prob))
    state['done'].copy_(eng.tensor(done.astype(np.float64)).int())
    state['sd'].copy_(eng.tensor(sd0))
    state['level'].fill_(-77.0)
    state['nsurv'].fill_(-5)
    state['running'].fill_(99)
    xt = eng.zeros(P, R, TD) - 7.0
    eng.boxsus_level(state, xt, cases[0][3], MIN_PROB)
    out = {k: npy(state[k]) for k in ('level', 'nsurv', 'prob', 'done', 'draw_status', 'anc', 'sd', 'running')}
    out['x_trial'] = npy(xt)
    return out, dict(score=score, prob=prob, done=done, x=x, sd=sd0, n_s=cases[0][3])


def check_draw(out, inp, p, R, pattern):
    """Draw p of a launch against the restatement; returns what it adds to the running count and the worst sd error."""
    x_p = inp['x'][p].T                                # (R, D)
    ref = S.level(inp['score'][p], x_p, inp['prob'][p], inp['sd'][p], inp['n_s'], MIN_PROB, bool(inp['done'][p]))
    anc = out['anc'][p]
    assert anc.min() >= 0 and anc.max() < R
    assert np.array_equal(anc, ref['anc']), pattern
    assert np.array_equal(out['x_trial'][p], x_p[anc]), 'x_trial is not x gathered by the device\'s anc'
    assert np.array_equal(out['prob'][p:p + 1].view(np.uint64), np.array([ref['prob']]).view(np.uint64)), (pattern, out['prob'][p], ref['prob'])
    assert out['done'][p] == int(ref['done']) and out['draw_status'][p] == ref['status'], pattern
    if ref['level'] is None:                           # finished before, or no live particle
        assert out['level'][p] == -77.0 and out['nsurv'][p] == (-5 if ref['nsurv'] is None else 0)
        assert np.array_equal(out['sd'][p], inp['sd'][p])
        return 0, 0.0
    assert out['level'][p:p + 1].view(np.uint64)[0] == np.array([ref['level']]).view(np.uint64)[0], (pattern, out['level'][p], ref['level'])
    assert out['nsurv'][p] == ref['nsurv']
    live = ~np.isnan(inp['score'][p])
    assert np.all(live[anc]) and np.all(inp['score'][p][anc] >= out['level'][p])
    err = np.abs(out['sd'][p] - ref['sd']) / (ULP * ref['sd'])
    assert np.all(err <= 1.0), (pattern, err)
    if pattern in ('final', 'zeros'):
        assert out['level'][p:p + 1].view(np.uint64)[0] == 0 and out['done'][p] == 1 and out['draw_status'][p] == S.OK
        assert out['nsurv'][p] == np.sum(inp['score'][p] >= 0.0)                 # (-0.0 and +0.0 are in F, -5e-324 is not)
    if pattern == 'equal':
        assert out['nsurv'][p] == R and out['prob'][p] == inp['prob'][p] and np.array_equal(anc, np.arange(R))
    if pattern == 'below_min':
        assert out['draw_status'][p] == S.BELOW_MIN and out['done'][p] == 1 and out['prob'][p] < MIN_PROB
    if pattern == 'blocks' and R >= 63:
        assert out['nsurv'][p] == 7 * -(-inp['n_s'] // 7)                        # the run that straddles the level survives whole
    return ref['running'], float(err.max())


@pytest.mark.parametrize('R', SIZES)
def test_level(eng, R):
    """Every pattern alone (P = 1) and four launches of three draws: each draw's checks, the running count, and the bits of a
    draw run alone against the same draw beside others (sd included)."""
    alone, worst = {}, 0.0
    for pat in PATTERNS:
        out, inp = run_level(eng, R, [pat])
        running, err = check_draw(out, inp, 0, R, pat)
        assert out['running'][0] == running, pat
        alone[pat], worst = out, max(worst, err)
    for triple in TRIPLES:
        out, inp = run_level(eng, R, list(triple))
        assert out['running'][0] == sum(check_draw(out, inp, p, R, pat)[0] for p, pat in enumerate(triple))
    print('R %d: largest |sd - restatement| / (2^-52 sd) = %.3g' % (R, worst))


@pytest.mark.parametrize('R', SIZES)
def test_a_draw_does_not_depend_on_the_draws_beside_it(eng, R):
    """P = 1 against P = 3, the same draw in the middle: the x columns are the draw's own, so every output agrees bit for bit."""
    for pat in ('distinct', 'blocks', 'dead', 'infs'):
        one, inp1 = run_level_fixed_x(eng, R, [pat], [0])
        three, inp3 = run_level_fixed_x(eng, R, ['equal', pat, 'zeros'], [1, 0, 2])
        for k in ('level', 'nsurv', 'prob', 'done', 'draw_status', 'anc', 'sd', 'x_trial'):
            assert np.array_equal(one[k][0:1].view(np.uint8), three[k][1:2].view(np.uint8)), (k, pat)


def run_level_fixed_x(eng, R, patterns, ids):
    """run_level with draw i's particles and starting sd a function of ids[i], not of its place in the launch."""
    P = len(patterns)
    cases = [level_case(R, pat) for pat in patterns]
    x = np.stack([np.random.default_rng([R, i]).normal(size=(TD, R)) for i in ids])
    sd0 = np.stack([np.random.default_rng([R, i, 1]).uniform(0.1, 0.2, TD) for i in ids])
    state = eng.boxsus_state(P, R, TD, np.full(TD, -1e3), np.full(TD, 1e3))
    state['score'].copy_(eng.tensor(np.array([c[0] for c in cases]).reshape(-1)))
    state['x'].copy_(eng.tensor(np.ascontiguousarray(x.transpose(1, 0, 2).reshape(TD, P * R))))
    state['prob'].copy_(eng.tensor(np.array([c[1] for c in cases])))
    state['sd'].copy_(eng.tensor(sd0))
    xt = eng.zeros(P, R, TD)
    eng.boxsus_level(state, xt, cases[0][3], MIN_PROB)
    out = {k: npy(state[k]) for k in ('level', 'nsurv', 'prob', 'done', 'draw_status', 'anc', 'sd')}
    out['x_trial'] = npy(xt)
    return out, None
