"""The I-step's queue driver without a device: run_queue_windows (dgp_amd/imputation.py) driven by a numpy stand-in for the
queue plan that follows the device state machine of train.hip section a7 (ess_begin_kernel, ess_prepare, ess_decide,
ess_end_kernel, the resume entry), against the sequential sampler's rule (imputation.py:79-119); the cached device
description of a Vecchia node upstairs; the dgpamd_node filler of the two ESS plans."""
import itertools
import time
import types

import numpy as np
import pytest
import torch

from oracle import dgp_oracle as O

TWO_PI = 2.0 * np.pi
THETA, LO, HI, PENDING, CURSOR, STATUS, INFO, LL, LOGY, PROPOSALS, BATCHES, UPDATES = range(12)
LL_START = -0.3   # log-likelihood of every layer's first state


def synthetic_ll(l, k, theta):
    """Log-likelihood of update number k of hidden layer l at angle theta: 0 at theta = 0, which every slice threshold is
    below (log_y = ll + log u < 0) -- the shrinking bracket always ends in acceptance."""
    return -abs(np.sin(3.0 * theta)) * 5.0 * (1 + l) * (1 + k % 3)


class StandInPlan:
    """dgpamd_ess_queue on a numpy state: what _EssQueue offers the driver, with the latents replaced by `ll_now` (the
    log-likelihood of the layer's current state) and `count` (updates of this layer so far; picks the target)."""
    FIELDS = ('theta', 'lo', 'hi', 'pending', 'cursor', 'status', 'info', 'll', 'log_y', 'proposals', 'batches', 'updates')

    def __init__(self, layer, b0, log):
        self.layer, self.b0, self.log = layer, b0, log
        self.ll_now, self.count = LL_START, 0
        self.state, self.udev = np.zeros(16), None

    def share_with(self, other):
        self.state, self.udev = other.state, other.udev

    def upload_uniforms(self, uniforms):
        if self.udev is None or self.udev[0] is not uniforms:
            self.udev = (uniforms, np.asarray(uniforms, dtype=float))

    def reset_state(self, cursor=0, ll=None):
        self.state[:] = 0.0
        self.state[CURSOR], self.state[LL] = cursor, 0.0 if ll is None else ll

    def resume_state(self, st, ll=None):
        self.state[:] = 0.0
        self.state[[THETA, LO, HI, PENDING]] = st['theta'], st['lo'], st['hi'], st['pending']
        self.state[LL], self.state[LOGY] = st['ll'] if ll is None else ll, st['log_y']

    def note_info(self, info):
        raise AssertionError('no factorisation is queued here')

    def fetch(self):
        self.log['status'].append(int(self.state[STATUS]))
        return dict(zip(self.FIELDS, self.state[:12].copy()))

    def queue(self, F, NU, scales, uniforms, cursor, ll, compute_ll0, batch_next, max_batches, fresh=True):
        self.upload_uniforms(uniforms)
        if fresh:
            self.reset_state(cursor, ll)
        st, u = self.state, self.udev[1]
        bn = batch_next if 0 < batch_next <= self.b0 else self.b0
        sc = dict(done=0, nb=0, th=[], br=[])   # (hipMemsetAsync of the scratch)
        if int(compute_ll0) == 1 and st[STATUS] == 0.0:   # ess_set_ll_kernel
            st[LL] = self.ll_now
        nupd = len(NU)
        for upd in range(nupd):
            self._begin(sc, u, upd, int(compute_ll0) == 2)
            for j in range(max(1, max_batches)):
                if j > 0:
                    self._prepare(sc, u, bn)
                self._decide(sc)
            if upd == nupd - 1 and not sc['done'] and st[STATUS] == 0.0:   # ess_end_kernel
                st[STATUS] = 3.0

    def _begin(self, sc, u, upd, resume):
        st = self.state
        if resume and upd == 0:
            sc['done'] = 0
            return self._prepare(sc, u, self.b0)
        if upd > 0 and not sc['done'] and st[STATUS] == 0.0:
            st[STATUS] = 3.0
        sc['nb'] = 0
        if st[STATUS] != 0.0:
            sc['done'] = 1
            return
        cur = int(st[CURSOR])
        if cur + 2 > len(u):
            st[STATUS], sc['done'] = 4.0, 1
            return
        st[LOGY] = st[LL] + np.log(u[cur])
        theta = TWO_PI * u[cur + 1]
        st[[THETA, LO, HI, PENDING]] = theta, theta - TWO_PI, theta, 0.0
        st[CURSOR] = cur + 2
        sc['done'] = 0
        self._prepare(sc, u, self.b0)

    def _prepare(self, sc, u, B):
        st = self.state
        sc['nb'] = 0
        if sc['done']:
            return
        cur = int(st[CURSOR])
        theta, lo, hi = st[THETA], st[LO], st[HI]
        if st[PENDING] != 0.0:
            if cur >= len(u):
                st[STATUS], sc['done'] = 1.0, 1
                return
            lo, hi = (theta, hi) if theta < 0.0 else (lo, theta)
            theta = lo + (hi - lo) * u[cur]
            cur += 1
            st[[THETA, LO, HI, PENDING]] = theta, lo, hi, 0.0
            st[CURSOR] = cur
        sc['th'], sc['br'] = [theta], [(lo, hi)]
        while len(sc['th']) < B and cur + len(sc['th']) - 1 < len(u):
            lo, hi = (theta, hi) if theta < 0.0 else (lo, theta)
            theta = lo + (hi - lo) * u[cur + len(sc['th']) - 1]
            sc['th'].append(theta)
            sc['br'].append((lo, hi))
        sc['nb'] = len(sc['th'])

    def _decide(self, sc):
        st = self.state
        if sc['done']:
            return
        nb, cur = sc['nb'], int(st[CURSOR])
        st[BATCHES] += 1
        for b in range(nb):
            ll = synthetic_ll(self.layer, self.count, sc['th'][b])
            if ll > st[LOGY]:
                st[CURSOR] = cur + b
                st[PROPOSALS] += b + 1
                st[[THETA, LO, HI, PENDING]] = sc['th'][b], sc['br'][b][0], sc['br'][b][1], 0.0
                st[LL] = ll
                st[UPDATES] += 1
                sc['done'] = 1
                self.accepted(sc['th'][b], ll)
                return
        st[CURSOR] = cur + nb - 1
        st[PROPOSALS] += nb
        st[[THETA, LO, HI, PENDING]] = sc['th'][-1], sc['br'][-1][0], sc['br'][-1][1], 1.0

    def accepted(self, theta, ll):
        self.log['accepted'].append((self.layer, theta))
        self.ll_now, self.count = ll, self.count + 1


def host_finish(plan, draws, stats, ll_cache, resume, B):
    """one_sample_block(l, resume=...) with the stand-in's target: the host loop's speculative batches of B from the device's
    bracket (imputation.one_sample_block, the general loop)."""
    from dgp_amd.imputation import shrink, speculative_angles
    log_y, theta, lo, hi = resume['log_y'], resume['theta'], resume['lo'], resume['hi']
    stats['updates'] += 1
    if resume['pending']:
        theta, lo, hi = shrink(theta, lo, hi, draws.uniform_take(1)[0])
    while True:
        thetas, brackets = speculative_angles(theta, lo, hi, draws.uniform_peek(B - 1))
        stats['batches'] += 1
        for b, t in enumerate(thetas):
            ll = synthetic_ll(plan.layer, plan.count, t)
            if ll > log_y:
                draws.uniform_take(b)
                stats['proposals'] += b + 1
                plan.accepted(t, ll)
                ll_cache[plan.layer] = ll
                return
        draws.uniform_take(len(thetas) - 1)
        stats['proposals'] += len(thetas)
        theta, (lo, hi) = thetas[-1], brackets[-1]
        theta, lo, hi = shrink(theta, lo, hi, draws.uniform_take(1)[0])


def batches_of(i, b0, bn, qmax, resume_on_device):
    """Speculative batches an update accepted at its proposal number i (from 0) takes: b0 then bn, qmax per window; an open
    update goes on with a new window's sizes (on the device) or with the host loop's min(b0, bn) = bn."""
    window = [b0] + [bn] * (qmax - 1)
    later = itertools.cycle(window) if resume_on_device else itertools.repeat(min(b0, bn))
    seen = 0
    for count, size in enumerate(itertools.chain(window, later), 1):
        seen += size
        if seen > i:
            return count


def sequential(u, ops, b0, bn, qmax, resume_on_device):
    """The sequential sampler on the uniforms u: per operation log_y = ll + log u, the angles of O.ess_angles, the first one
    whose log-likelihood exceeds log_y.  Returns (accepted [(layer, theta)], stats, uniforms consumed)."""
    ll_now, count, acc = {}, {}, []
    stats = dict(proposals=0, updates=0, batches=0)
    cur = 0
    for _, l in ops:
        k = count.get(l, 0)
        log_y = ll_now.get(l, LL_START) + np.log(u[cur])
        th = O.ess_angles(u[cur + 1:cur + 400])
        i = next(i for i, t in enumerate(th) if synthetic_ll(l, k, t) > log_y)
        acc.append((l, th[i]))
        ll_now[l], count[l] = synthetic_ll(l, k, th[i]), k + 1
        cur += 1 + (i + 1)   # the threshold's uniform, theta0's, one per rejection
        stats['proposals'] += i + 1
        stats['updates'] += 1
        stats['batches'] += batches_of(i, b0, bn, qmax, resume_on_device)
    return acc, stats, cur


def drive(draws, sweeps, hidden, b0, bn, qmax, resume_on_device):
    """run_queue_windows over stand-in plans, wired as imputer._sample_queued wires it."""
    from dgp_amd.imputation import run_queue_windows, _resume_args
    log = dict(status=[], accepted=[])
    plans = {l: StandInPlan(l, b0, log) for l in range(hidden)}
    ops = [(s, l) for s in range(sweeps) for l in range(hidden)]
    stats, ll_cache = dict(proposals=0, updates=0, batches=0), {}
    one = hidden == 1

    def args_of(j, lead):
        return None, np.zeros((len(ops) - j if one else 1, 1, 1)), [1.0]

    def finish(j, st):
        host_finish(plans[ops[j][1]], draws, stats, ll_cache, _resume_args(st), min(b0, bn))

    run_queue_windows(ops, plans, {l: (b0, bn, qmax) for l in plans}, draws, stats, ll_cache, args_of, finish, resume_on_device)
    return ops, log, stats


SIZES = [(1, 1, 1), (2, 2, 2), (3, 2, 1), (12, 4, 2), (6, 3, 5)]
POLICIES = [(1, True), (1, False), (2, False)]   # (hidden layers, open updates continued on the device); several layers: host only


@pytest.mark.parametrize('hidden,resume_on_device', POLICIES)
@pytest.mark.parametrize('b0,bn,qmax', SIZES)
def test_driver_takes_the_sequential_decisions(b0, bn, qmax, hidden, resume_on_device):
    """Every update accepts the proposal the sequential rule accepts, the counters match, and the uniform stream is left
    exactly where the sequential sampler leaves it -- 40 chains of 5 sweeps per case."""
    from dgp_amd.imputation import DrawStream
    rng = np.random.default_rng(1000 * b0 + 10 * qmax + hidden)
    statuses = []
    for trial in range(40):
        u = rng.random(4000)
        draws = DrawStream(z=[], u=list(u))
        ops, log, stats = drive(draws, 5, hidden, b0, bn, qmax, resume_on_device)
        acc, ref_stats, used = sequential(u, ops, b0, bn, qmax, resume_on_device)
        assert log['accepted'] == acc
        assert stats == ref_stats
        assert len(u) - len(draws._ubuf) == used
        statuses += log['status']
    if (b0, bn, qmax) in ((1, 1, 1), (2, 2, 2), (3, 2, 1)):   # the narrow queues leave updates open all the time
        assert 3 in statuses


@pytest.mark.parametrize('hidden,resume_on_device', POLICIES)
def test_each_open_update_policy_meets_status_3(hidden, resume_on_device):
    """The grid above cannot pass without windows that end with an update left open, under each policy."""
    from dgp_amd.imputation import DrawStream
    u = np.random.default_rng(7).random(4000)
    _, log, _ = drive(DrawStream(z=[], u=list(u)), 5, hidden, 2, 2, 2, resume_on_device)
    assert log['status'].count(3) >= 1


# theta0 = 2 pi 0.26 and the angle 0.5 places in its bracket are both rejected under log_y = LL_START + log 0.99
SHORT = [((1, 1, 1), []),                   # status 4, empty peek: no update can begin
         ((1, 1, 1), [0.5]),                # status 4 with one uniform left, which no window can consume
         ((1, 1, 1), [0.99, 0.26]),         # status 3, then the closing shrink is due with nothing left (status 1, empty peek)
         ((2, 2, 2), [0.99, 0.26, 0.5])]    # status 1 inside a window, then the same


@pytest.mark.parametrize('hidden,resume_on_device', POLICIES)
@pytest.mark.parametrize('sizes,u', SHORT)
def test_short_injected_stream_is_reported(hidden, resume_on_device, sizes, u):
    """An injected uniform stream that ends before or inside an update: RuntimeError, not a loop."""
    from dgp_amd.imputation import DrawStream
    for t in (O.ess_angles(u[1:]) if len(u) > 1 else []):   # (the proposals these streams reach are all rejected)
        assert synthetic_ll(0, 0, t) <= LL_START + np.log(0.99)
    t0 = time.perf_counter()
    with pytest.raises(RuntimeError, match='injected uniform stream exhausted'):
        drive(DrawStream(z=[], u=u), 5, hidden, *sizes, resume_on_device)
    assert time.perf_counter() - t0 < 1.0


@pytest.mark.parametrize('hidden,resume_on_device', POLICIES)
@pytest.mark.parametrize('b0,bn,qmax', [(2, 2, 2), (12, 4, 2)])
def test_exact_injected_stream_is_used_up(b0, bn, qmax, hidden, resume_on_device):
    """A stream that ends with the last accepted update's last uniform: the driver completes and leaves it empty."""
    from dgp_amd.imputation import DrawStream
    rng = np.random.default_rng(17)
    for trial in range(40):
        u = rng.random(4000)
        ops = [(s, l) for s in range(3) for l in range(hidden)]
        acc, ref_stats, used = sequential(u, ops, b0, bn, qmax, resume_on_device)
        draws = DrawStream(z=[], u=list(u[:used]))
        _, log, stats = drive(draws, 3, hidden, b0, bn, qmax, resume_on_device)
        assert log['accepted'] == acc and stats == ref_stats
        assert draws._ubuf == []


def test_a_window_without_progress_raises():
    """A queue that reports an open update (status 3) having consumed no uniform and finished no update can never make
    progress: the driver raises instead of queueing the same window for ever."""
    from dgp_amd.imputation import DrawStream, run_queue_windows

    class Stuck(StandInPlan):
        def queue(self, *a, **kw):
            self.state[STATUS] = 3.0

    for resume_on_device in (True, False):
        plan = Stuck(0, 2, dict(status=[], accepted=[]))
        t0 = time.perf_counter()
        with pytest.raises(RuntimeError, match='without consuming a uniform'):
            run_queue_windows([(0, 0), (1, 0)], {0: plan}, {0: (2, 2, 2)}, DrawStream(seed=1), dict(proposals=0, updates=0, batches=0), {},
                              lambda j, lead: (None, np.zeros((1, 1, 1)), [1.0]), lambda j, st: None, resume_on_device)
        assert time.perf_counter() - t0 < 1.0
        assert plan.log['status'] == [3]


# ---------------------------------------------------------------------------- the device description of a node upstairs
def _vecchia_setup(n=7, rep=False):
    """An imputer over plain objects: one hidden layer of two columns, one Vecchia node upstairs with observed outputs."""
    from dgp_amd.imputation import imputer
    node = types.SimpleNamespace(ord=np.random.default_rng(0).permutation(n), NNarray=np.arange(n * 3).reshape(n, 3) % n,
                                 input_dim=np.array([1, 0]), rep=np.arange(n) if rep else None, W_diag=np.linspace(1.0, 2.0, n))
    node.ord_dev = lambda: torch.as_tensor(node.ord)
    node.nn_dev = lambda: torch.as_tensor(node.NNarray)
    imp = imputer.__new__(imputer)
    imp.all_layer = [[None, None], [node]]
    imp._engine = types.SimpleNamespace(tensor=lambda a, dtype=torch.float64: torch.as_tensor(np.asarray(a), dtype=dtype))
    imp.F = [torch.zeros(n, 2, dtype=torch.float64)]
    imp._yy = {0: torch.arange(n, dtype=torch.float64)}
    return imp, node


def test_upper_node_description_is_cached_and_rebuilt():
    imp, node = _vecchia_setup(rep=True)
    v = imp._upper_vecch(1, 0)
    assert v['cm'].dtype == torch.long and v['cm'].tolist() == [1, 0]
    assert torch.equal(v['ord'], torch.as_tensor(node.ord)) and torch.equal(v['nn'], torch.as_tensor(node.NNarray))
    assert torch.equal(v['nd'], torch.as_tensor(node.W_diag)) and torch.equal(v['y'], imp._yy[0][torch.as_tensor(node.ord)])
    keep = {key: v[key] for key in ('ord', 'nn', 'nd', 'cm', 'y')}
    again = imp._upper_vecch(1, 0)
    assert all(again[key] is keep[key] for key in keep)   # the same objects on a second call
    for name, fresh in (('NNarray', node.NNarray.copy()), ('ord', node.ord[::-1].copy()), ('W_diag', node.W_diag * 2.0)):
        setattr(node, name, fresh)
        new = imp._upper_vecch(1, 0)
        assert all(new[key] is not keep[key] for key in keep), name
        assert torch.equal(new['y'], imp._yy[0][torch.as_tensor(node.ord)])
        assert torch.equal(new['nd'], torch.as_tensor(node.W_diag)) and torch.equal(new['nn'], torch.as_tensor(node.NNarray))
        keep = {key: new[key] for key in keep}
    imp._yy[0] = imp._yy[0] + 1.0   # the outputs replaced: only their ordered copy is made again
    new = imp._upper_vecch(1, 0)
    assert new['y'] is not keep['y'] and torch.equal(new['y'], imp._yy[0][new['ord']])
    assert all(new[key] is keep[key] for key in ('ord', 'nn', 'nd', 'cm'))


def test_upper_node_description_without_replicates_has_unit_weights():
    imp, node = _vecchia_setup()
    assert torch.equal(imp._upper_vecch(1, 0)['nd'], torch.ones(7, dtype=torch.float64))


def test_fill_gp_node_fields():
    """The dgpamd_node of a GP node upstairs, as _EssQueue and _EssPlan fill it (include/dgp_amd.h)."""
    from dgp_amd import _lib
    from dgp_amd.ops import _fill_gp_node, KIND
    n, M = 5, 4
    Xglob, W, y = torch.zeros(n, 2, dtype=torch.float64), torch.ones(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    nd = _lib.Node()
    keep = _fill_gp_node(nd, 'matern2.5', [2, 0, 3], Xglob, [0.5, 0.6, 0.7, 0.8, 0.9], 1e-6, W, y, M)
    assert (nd.kind, nd.Dl, nd.Dg, nd.nlen, nd.ldloc, nd.nugget) == (KIND['matern2.5'], 3, 2, 5, M, 1e-6)
    assert nd.nugget_est == 0 and nd.Xloc is None
    colmap, length = keep[0], keep[1]
    assert colmap.dtype == np.int32 and colmap.tolist() == [2, 0, 3] and nd.colmap == colmap.ctypes.data
    assert length.dtype == np.float64 and length.tolist() == [0.5, 0.6, 0.7, 0.8, 0.9] and nd.length == length.ctypes.data
    assert (nd.Xglob, nd.W, nd.y) == (Xglob.data_ptr(), W.data_ptr(), y.data_ptr())
    assert all(any(k is t for k in keep) for t in (Xglob, W, y))   # (alive as long as the struct)
    assert (nd.vecch_ord, nd.vecch_m, nd.lik_kind) == (None, 0, 0)
    nd2 = _lib.Node()
    _fill_gp_node(nd2, 'sexp', [0], None, [1.5], 0.25, None, y, 1)
    assert (nd2.kind, nd2.Dl, nd2.Dg, nd2.nlen, nd2.ldloc, nd2.nugget) == (KIND['sexp'], 1, 0, 1, 1, 0.25)
    assert nd2.Xglob is None and nd2.W is None
