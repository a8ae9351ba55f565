"""dgpamd_boxsites_fold on the device (csrc/boxsites.hip, DESIGN I.24) as an operator: its outputs EQUAL those of the numpy
restatement tests/boxsites_ref.py at every shape at which the kernel takes another path -- one site, a partial wave, whole
waves and one thread more, the largest T; one chunk of staged columns, a partial second one, eight full ones -- and the chain
kernels driven through it equal their restatements call by call.  Needs an MI355X: -m gpu."""
import functools

import numpy as np
import pytest

import boxhmc_ref as HM
import boxmala_ref as M
import boxsites_ref as B
import test_boxmala_host as H

pytestmark = pytest.mark.gpu
QMAX = 65
COLS = {(2, 1): [1], (5, 2): [3, 0], (5, 4): [4, 0, 2, 1], (64, 63): [c for c in range(63, -1, -1) if c != 31]}


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=2)
def case(T, K, Dx, Dt, kind):
    """(f (65, T, K), J (65, T, K, Dx), W (K, T, T), cols, the restatement's (ft, Jt)) -- made once for the 65 chains; a test
    with fewer takes the first of them (a chain's outputs are its own).  kind: 'dense' a full lower triangle; 'diagonal';
    'gaps' the dense one with two sites unobserved (one where T < 4, none where T = 1): their rows and columns of W are zero
    and their f and J hold NaN."""
    rng = np.random.default_rng(1000 * T + 100 * K + Dx + len(kind))
    f, J = rng.normal(size=(QMAX, T, K)), rng.normal(size=(QMAX, T, K, Dx))
    W = np.tril(rng.normal(size=(K, T, T)))
    gone = []
    if kind == 'diagonal':
        W = W * np.eye(T)
    elif kind == 'gaps':
        gone = sorted({1, T - 2} & set(range(1, T)))
        W[:, gone], W[:, :, gone] = 0.0, 0.0
        f[:, gone], J[:, gone] = np.nan, np.nan
    cols = COLS[Dx, Dt]
    for a in (f, J, W):
        a.setflags(write=False)
    return f, J, W, cols, gone, B.fold(f, J, W, cols)


@pytest.mark.parametrize('Q', [1, 3, 65])                  # (the fastest: the three share one case)
@pytest.mark.parametrize('kind', ['dense', 'diagonal', 'gaps'])
@pytest.mark.parametrize('Dx,Dt', sorted(COLS))
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('T', [1, 2, 63, 64, 65, 256])
def test_fold_equals_the_restatement(eng, Q, T, K, Dx, Dt, kind):
    """Expected largest difference 0: the kernel and the restatement perform the same roundings in the same order."""
    f, J, W, cols, gone, (ft_ref, Jt_ref) = case(T, K, Dx, Dt, kind)
    ft, Jt = eng.boxsites_fold(eng.tensor(f[:Q]), eng.tensor(J[:Q]), eng.tensor(W), cols)
    ft, Jt = npy(ft), npy(Jt)
    assert ft.shape == (Q, T * K) and Jt.shape == (Q, T * K, Dt)
    assert np.array_equal(ft, ft_ref[:Q]), 'largest |ft - restatement| %.3g' % np.max(np.abs(ft - ft_ref[:Q]))
    assert np.array_equal(Jt, Jt_ref[:Q]), 'largest |Jt - restatement| %.3g' % np.max(np.abs(Jt - Jt_ref[:Q]))
    assert np.all(np.isfinite(ft)) and np.all(np.isfinite(Jt))                   # no NaN of an unobserved site leaks
    if gone:
        assert np.all(ft.reshape(Q, T, K)[:, gone] == 0.0) and np.all(Jt.reshape(Q, T, K, Dt)[:, gone] == 0.0)
    if kind == 'gaps' and T > 4:
        assert np.all(ft.reshape(Q, T, K)[:, [0, T - 1]] != 0.0)
    # the values alone: the same ft, no Jacobian read
    only = eng.boxsites_fold(eng.tensor(f[:Q]), None, eng.tensor(W))
    assert only[1] is None and np.array_equal(npy(only[0]), ft)


def test_a_slice_of_the_chains_is_the_slice_of_the_fold(eng):
    """An element depends on its own chain's inputs alone: the fold of chains [a:b] equals rows [a:b] of the fold of all, with a
    plan made once and with outputs given."""
    f, J, W, cols, _, _ = case(65, 3, 5, 4, 'gaps')
    plan = eng.boxsites_plan(W, cols)
    whole = [npy(t) for t in eng.boxsites_fold(eng.tensor(f), eng.tensor(J), plan)]
    for a, b in ((0, 1), (1, 64), (64, 65), (7, 40)):
        out = (eng.empty(b - a, 65 * 3), eng.empty(b - a, 65 * 3, 4))
        got = eng.boxsites_fold(eng.tensor(f[a:b]), eng.tensor(J[a:b]), plan, out=out)
        assert got[0] is out[0] and got[1] is out[1]
        assert np.array_equal(npy(out[0]), whole[0][a:b]) and np.array_equal(npy(out[1]), whole[1][a:b])


# ----------------------------------------------------------------------------- the chain kernels behind the fold, call by call
ROUNDS, WARMUP, THIN = 61, 20, 2          # test_gpu_boxmala's schedule: call 0 is INIT; calls 1 .. 20 adapt; every second one after is saved
SITES = 5


def field_problem(Q, K, seed=0):
    """Chain q calibrates theta (2 columns: 0 and 2 of the walk's input (theta_0, c, theta_1)) of f_k(c, theta) =
    sin(a_qk . (theta_0, c, theta_1) + b_qk) at T = 5 known c, under a dense covariance per output; with K = 3 entry (2, 1)
    is unobserved: its y, f and J hold NaN.  K' = 5 K pseudo-outputs."""
    rng = np.random.default_rng(77 * Q + K + seed)
    T, D = SITES, 2
    c = np.linspace(0.1, 0.9, T)
    a, b = rng.normal(size=(Q, K, 3)) / np.sqrt(3.0), rng.normal(size=(Q, K))
    cov = np.array([s * s * np.exp(-(c[:, None] - c[None]) ** 2 / (2.0 * 0.3 ** 2)) for s in rng.uniform(0.1, 0.3, K)])
    y = rng.uniform(-0.5, 0.5, (T, K))
    if K == 3:
        y[2, 1] = np.nan
    W, ybar, w, _ = B.whiten(y, rng.uniform(0.1, 0.2, (T, K)), cov)

    def fun(theta, rows=slice(None)):
        """theta (Q, 2) -> the walk's f (Q, T, K) and J (Q, T, K, 3)."""
        x = np.stack([np.broadcast_to(theta[:, None, 0], (len(theta), T)), np.broadcast_to(c, (len(theta), T)),
                      np.broadcast_to(theta[:, None, 1], (len(theta), T))], -1)          # (Q, T, 3)
        t = np.einsum('qkd,qtd->qtk', a[rows], x) + b[rows][:, None]
        f, J = np.sin(t), np.cos(t)[..., None] * a[rows][:, None]
        if K == 3:
            f[:, 2, 1], J[:, 2, 1] = np.nan, np.nan
        return f, J
    lo, hi = np.array([-1.0, -1.0]), np.array([1.0, 1.5])
    return dict(fun=fun, W=W, w=w, ybar=ybar, lo=lo, hi=hi, s=hi - lo, cols=[0, 2], x0=rng.uniform(lo, hi, (Q, D)),
                z=rng.normal(size=(ROUNDS, Q, D)), logu=np.log(rng.uniform(size=(ROUNDS, Q))))


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('method', ['mala', 'hmc'])
def test_chains_behind_the_device_fold_equal_the_restatement(eng, method, K):
    """A 61-call run of 65 chains: f(c, theta) and J in numpy at the kernel's own trial points, the device fold between the
    walk and the step, K' = 5 and 15.  Every trial, decision, h, sample and logp equal those of the restatement's chain on
    boxsites_ref.fold's output.  HMC: every third call closes a trajectory."""
    Q = 65
    p = field_problem(Q, K)
    hmc = method == 'hmc'
    S = (ROUNDS - 1 - WARMUP) // THIN
    state = (eng.boxhmc_state if hmc else eng.boxmala_state)(Q, 2, p['w'], p['ybar'], p['lo'], p['hi'], p['s'], n_slots=S)
    chains = [(HM.Chain if hmc else M.Chain)(p['x0'][q], p['w'], p['ybar'], p['lo'], p['hi'], p['s']) for q in range(Q)]
    plan = eng.boxsites_plan(p['W'], p['cols'])
    xt = eng.tensor(p['x0'])
    trial, slots = p['x0'].copy(), []
    for c in range(ROUNDS):
        f, J = p['fun'](trial)
        ft, Jt = eng.boxsites_fold(eng.tensor(f), eng.tensor(J), plan)
        ft_ref, Jt_ref = B.fold(f, J, p['W'], p['cols'])
        assert np.array_equal(npy(ft), ft_ref) and np.array_equal(npy(Jt), Jt_ref), 'call %d: the fold' % c
        last = not hmc or c % 3 == 0
        on, j = last and 1 <= c <= WARMUP, c - WARMUP
        up, down = H.gain(c - 1) if on else (1.0, 1.0)
        slot = j // THIN - 1 if last and j >= 1 and j % THIN == 0 else -1
        kw = dict(up=up, down=down, adapt=on, first=c == 0, slot=slot)
        slots += [slot] if slot >= 0 else []
        if hmc:
            eng.boxhmc_step(state, ft, Jt, xt, eng.tensor(p['z'][c]), eng.tensor(p['logu'][c]), last=last, **kw)
        else:
            eng.boxmala_step(state, ft, Jt, xt, eng.tensor(p['z'][c]), eng.tensor(p['logu'][c]), **kw)
        trial = npy(xt)
        for q, ch in enumerate(chains):
            if hmc:
                ch.step(ft_ref[q], Jt_ref[q], p['z'][c, q], p['logu'][c, q], last, on, up, down, save=slot >= 0)
            else:
                ch.step(ft_ref[q], Jt_ref[q], p['z'][c, q], p['logu'][c, q], on, up, down, save=slot >= 0)
        ref = np.array([ch.trial for ch in chains])
        assert np.array_equal(trial, ref), 'call %d: largest |trial - restatement| %.3g' % (c, np.max(np.abs(trial - ref)))
    out = {k: npy(state[k]) for k in ('h', 'logr', 'status', 'n_prop', 'n_acc')}
    out['x'], out['logp'] = npy(state['xs']).transpose(2, 0, 1)[:, slots], npy(state['lps']).T[:, slots]   # (HMC fills every third slot)
    assert len(slots) == (S if not hmc else len([c for c in range(WARMUP + THIN, ROUNDS, THIN) if c % 3 == 0])) and len(slots) >= 6
    ref = dict(h=[c.h for c in chains], logr=[c.logr for c in chains], status=[c.status for c in chains],
               n_prop=[c.n_prop for c in chains], n_acc=[c.n_acc for c in chains], x=[c.xs for c in chains], logp=[c.lps for c in chains])
    for k, v in ref.items():
        assert np.array_equal(out[k], np.array(v), equal_nan=True), k
    assert np.all(out['status'] == 0) and 0 < out['n_acc'].sum() < out['n_prop'].sum() and np.all(np.isfinite(out['logp']))


def test_bad_arguments_are_refused(eng):
    from dgp_amd.ops import DgpAmdError
    f, J, W = eng.zeros(4, 5, 3), eng.zeros(4, 5, 3, 6), eng.zeros(3, 5, 5)
    eng.boxsites_fold(f, J, W, [0, 5])                                           # (the arguments below are otherwise good)
    for cols in ([0, 6], [-1, 2], [2, 2], [0, 1, 2, 3, 4, 5, 0]):                # out of range, named twice, more than Dx
        with pytest.raises(DgpAmdError):
            eng.boxsites_fold(f, J, W, cols)
    with pytest.raises(DgpAmdError):
        eng.boxsites_fold(eng.zeros(2, 257, 1), eng.zeros(2, 257, 1, 2), eng.zeros(1, 257, 257), [0])   # T > 256
    with pytest.raises(DgpAmdError):
        eng.boxsites_fold(eng.zeros(2, 3, 1), eng.zeros(2, 3, 1, 70), eng.zeros(1, 3, 3), list(range(65)))   # Dt > 64
    with pytest.raises(DgpAmdError):
        eng.boxsites_fold(eng.zeros(0, 5, 3), eng.zeros(0, 5, 3, 6), W, [0])                          # no chain
    for bad in (lambda: eng.boxsites_fold(f, J, eng.zeros(3, 5, 4), [0]), lambda: eng.boxsites_fold(f, J, eng.zeros(2, 5, 5), [0]),
                lambda: eng.boxsites_fold(f, J, eng.zeros(3, 4, 4), [0]), lambda: eng.boxsites_fold(f, eng.zeros(4, 5, 2, 6), W, [0]),
                lambda: eng.boxsites_fold(f.float(), J, W, [0]), lambda: eng.boxsites_fold(f, J.transpose(0, 1), W, [0]),
                lambda: eng.boxsites_fold(f, J, W, [0], out=(eng.empty(4, 15), eng.empty(4, 15, 2))),
                lambda: eng.boxsites_fold(f, J, W.float(), [0])):
        with pytest.raises(ValueError):
            bad()
