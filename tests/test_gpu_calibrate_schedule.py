"""calibrate.calibrate's lock-step loop on the device against the restatements' sample(), bit for bit (DESIGN I.19, I.20): the
driver's schedule -- which round is INIT, which adapt with which gain, which are saved, where a trajectory ends, which draws
a round reads and how the uploads are cut into blocks -- is what is held here; the step kernels are held call by call in
test_gpu_boxmala.py and test_gpu_boxhmc.py.  In place of a model the walk is a synthetic family
    f_pk(x) = a_pk + b_pk0 x_0 + b_pk1 x_1 + b_pk2 x_2 + c_pk (x_0 x_1),
evaluated on the device by single elementwise * and + calls, left to right, each rounded once: numpy performing the same
sequence gives the same doubles, so every sample, log density, step and status must be EQUAL.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import boxhmc_ref as Hm
import boxmala_ref as M

pytestmark = pytest.mark.gpu
P, R, DX, K = 2, 3, 3, 2
WARMUP, SAMPLES, THIN = 5, 4, 2
TOTAL = 1 + WARMUP + SAMPLES * THIN               # 14 iterations
SEED, STEP, OBS_SD = 5, 0.25, 0.15
LO, HI = np.array([0.0, -1.0, 0.3]), np.array([1.0, 1.0, 0.9])
SCALE = np.array([1.0, 2.0, 0.0])                 # hi - lo, the last column fixed by its scale
PRIOR = np.array([0.4, 0.0, 0.0]), np.array([0.5, np.inf, np.inf])     # a Gaussian prior on column 0 alone
CASES = {'mala': dict(method='mala'), 'hmc-jitter': dict(method='hmc', n_leapfrog=3, jitter=True),
         'hmc-fixed': dict(method='hmc', n_leapfrog=3, jitter=False)}


def family():
    """a (P, K), b (P, K, 3), c (P, K), y (K,), x0 (P, R, DX)."""
    rng = np.random.default_rng(11)
    a, b, c = rng.normal(size=(P, K)), rng.normal(size=(P, K, DX)), rng.normal(size=(P, K))
    x0 = rng.uniform(LO, HI, (P, R, DX))
    y = np.array([0.3, -0.2])
    return a, b, c, y, x0


def host_fun(a, b, c):
    """fun(x (3,)) -> (f (K,), J (K, 3)) of one path: the device's sequence of operations."""
    def fun(x):
        f = a + b[:, 0] * x[0]
        f = f + b[:, 1] * x[1]
        f = f + b[:, 2] * x[2]
        f = f + c * (x[0] * x[1])
        return f, np.stack((b[:, 0] + c * x[1], b[:, 1] + c * x[0], b[:, 2]), 1)
    return fun


def device_fun(eng, a, b, c):
    """value_and_jac(xt (P, R, 3)) -> (f (P, R, K), J (P, R, K, 3)), one torch call per operation."""
    import torch
    ad, cd = eng.tensor(a[:, None, :]), eng.tensor(c[:, None, :])
    bd = [eng.tensor(np.ascontiguousarray(b[:, None, :, d])) for d in range(DX)]

    def value_and_jac(xt):
        x0, x1, x2 = (xt[:, :, d:d + 1] for d in range(DX))
        f = torch.add(ad, torch.mul(bd[0], x0))
        f = torch.add(f, torch.mul(bd[1], x1))
        f = torch.add(f, torch.mul(bd[2], x2))
        f = torch.add(f, torch.mul(cd, torch.mul(x0, x1)))
        j0, j1 = torch.add(bd[0], torch.mul(cd, x1)), torch.add(bd[1], torch.mul(cd, x0))
        return f.contiguous(), torch.stack((j0, j1, bd[2].expand_as(j0)), -1).contiguous()
    return value_and_jac


class Walls(M.Chain):
    """boxmala_ref.Chain that counts the proposals thrown out of the box."""
    walls = 0

    def step(self, *args, **kw):
        super().step(*args, **kw)
        self.walls += int(self.flag)


def restated(case, monkeypatch):
    """The P x R chains of the restatement on calibrate's streams, trajectory lengths and gains."""
    from dgp_amd import calibrate
    kw = CASES[case]
    a, b, c, y, x0 = family()
    w, pv = np.full(K, 1.0 / (OBS_SD * OBS_SD)), 1.0 / (PRIOR[1] * PRIOR[1])
    z, logu = calibrate.Streams(SEED, P, R, DX).block(TOTAL)
    gain = lambda n: calibrate.gain(n, calibrate.TARGET_ACCEPT[kw['method']])
    monkeypatch.setattr(M, 'Chain', Walls)
    chains = []
    for p in range(P):
        for r in range(R):
            args = (host_fun(a[p], b[p], c[p]), x0[p, r], w, y, LO, HI, SCALE, z[:, p, r], logu[:, p, r])
            if kw['method'] == 'mala':
                ch = M.sample(*args, WARMUP, THIN, gain, pv, PRIOR[0], STEP)
                ch.calls = TOTAL
            else:
                lengths = calibrate.trajectory_lengths(SEED, TOTAL - 1, kw['n_leapfrog'], kw['jitter'])
                ch = Hm.sample(*args, lengths, WARMUP, THIN, gain, pv, PRIOR[0], STEP)
                ch.walls = ch.reflections
            chains.append(ch)
    return chains


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def never(*args):
    raise AssertionError('x0 is given: no candidate is screened')


@pytest.mark.parametrize('case', list(CASES))
def test_the_driver_follows_the_restatements_schedule(eng, case, monkeypatch):
    """Expected largest difference 0 in x, logp, step and status; the acceptance rate is the restatement's mean over the
    decisions after warm-up; rounds and evaluations are its calls.  Uploads of 4 iterations: the 14 cross three block edges.
    The restatement alone (no device) shows that the case exercises the schedule: accepted and rejected decisions after
    warm-up, and proposals out of the box ('mala') or reflections ('hmc')."""
    from dgp_amd import calibrate
    kw = CASES[case]
    chains = restated(case, monkeypatch)
    accepts = np.array([ch.accepts for ch in chains])
    print('%s: %d of %d decisions accepted, %d after warm-up of %d; walls met %s; steps %s; calls %d' %
          (case, accepts.sum(), accepts.size, accepts[:, WARMUP:].sum(), accepts[:, WARMUP:].size, [ch.walls for ch in chains],
           np.round([float(ch.h) for ch in chains], 4), chains[0].calls))
    assert accepts.shape == (P * R, TOTAL - 1) and 0 < accepts[:, WARMUP:].sum() < accepts[:, WARMUP:].size
    assert sum(ch.walls for ch in chains) > 0 and all(ch.status == M.OK for ch in chains)
    a, b, c, y, x0 = family()
    monkeypatch.setattr(calibrate, '_rounds_per_upload', lambda Q, Dx: 4)
    res = calibrate.calibrate(eng, P, K, DX, never, device_fun(eng, a, b, c), 8, y, OBS_SD, np.stack((LO, HI), 1), n_samples=SAMPLES,
                              warmup=WARMUP, thin=THIN, x0=x0, seed=SEED, step=STEP, scale=SCALE, prior=PRIOR, **kw)
    shape = (P, R)
    for name, ref in (('x', [ch.xs for ch in chains]), ('logp', [ch.lps for ch in chains]), ('step', [ch.h for ch in chains]),
                      ('status', [ch.status for ch in chains])):
        got, ref = getattr(res, name), np.array(ref, dtype=np.float64)
        ref = ref.reshape(shape + ref.shape[1:])
        assert got.shape == ref.shape
        assert np.array_equal(got, ref), (name, 'largest difference %.3g' % np.max(np.abs(got - ref)))
    assert np.array_equal(res.accept_rate, accepts[:, WARMUP:].mean(1).reshape(shape))
    assert np.array_equal(res.x0, x0) and np.all(res.x[..., 2] == x0[:, :, None, 2])
    assert res.rounds == res.evaluations == chains[0].calls and all(ch.calls == chains[0].calls for ch in chains)
    assert (res.method, res.n_leapfrog) == (kw['method'], kw.get('n_leapfrog', 1))
