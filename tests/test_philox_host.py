"""The counter-based random streams without a device (DESIGN I.23): the numpy restatement of dgpamd_philox_fill
(tests/philox_ref.py) against numpy.random.Philox and against csrc/philox.hpp compiled for the host (tools/philox_check.cpp),
the independence of a number from the shape of the call, the moments of the transforms, subset simulation and tempered SMC on
the Philox streams against events and posteriors of known answers, the refusals that need no device, and the keyword's
default.  No device.

The statistical conditions on subset simulation are test_boxsus_host.py's, unchanged (32 seeds x 1024 particles: |z| of the
mean of ln P^ - ln p <= 5, the seeds' sd <= 2 cov(), stages <= ceil(log10(1 / p)) + 1), those on SMC test_boxsmc_host.py's
(16 seeds x 512 particles, every average within 5 standard errors of quadrature)."""
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import philox_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = np.uint64
TOP = 1 << 64
# keys and counter words with high bits set, and c0 across a carry into c1, c2 and c3
KEYS = [(0, 0), (0xFEDCBA9876543210, 0x8000000000000001), (TOP - 1, TOP - 1)]
COUNTERS = [(0, 0, 0, 0), (0, (5 << 32) | 7, (1 << 63) + 3, 2), (0, TOP - 1, TOP - 1, TOP - 1), (TOP - 2, 3, 4, 5),
            (TOP - 2, TOP - 1, 5, TOP - 1), (TOP - 3, TOP - 1, TOP - 1, 1 << 63)]


def numpy_raw(key, counter, n):
    return np.random.Philox(counter=np.array(counter, dtype=U), key=np.array(key, dtype=U)).random_raw(n)


def advanced(counter, k):
    """The counter k steps on, as 256-bit arithmetic with the carry."""
    v = (sum(int(c) << (64 * i) for i, c in enumerate(counter)) + k) % (1 << 256)
    return tuple((v >> (64 * i)) & (TOP - 1) for i in range(4))


# ---------------------------------------------------------------------------------------------------------------------- bits
@pytest.mark.parametrize('key', KEYS)
def test_the_restatement_is_numpys_philox(key):
    for counter in COUNTERS:
        steps = [advanced(counter, k) for k in (1, 2, 3, 4)]        # (numpy increments before it generates)
        parts = [np.array([s[i] for s in steps], dtype=U) for i in range(4)]
        mine = np.stack(X.philox(*parts, *key), -1).reshape(-1)
        assert np.array_equal(mine, numpy_raw(key, counter, 16)), (key, counter)


def test_mulhilo_against_python_integers():
    rng = np.random.default_rng(0)
    a = np.concatenate([rng.integers(0, TOP, 200, dtype=U), np.array([0, 1, TOP - 1, 1 << 63, (1 << 32) - 1, 1 << 32], dtype=U)])
    b = np.concatenate([rng.integers(0, TOP, 200, dtype=U), np.array([TOP - 1, TOP - 1, TOP - 1, 1 << 63, (1 << 32) + 1, 1 << 32], dtype=U)])
    hi, lo = X.mulhilo(a, b)
    for x, y, h, l in zip(a.tolist(), b.tolist(), hi.tolist(), lo.tolist()):
        assert (h << 64) | l == x * y


@pytest.mark.parametrize('key', KEYS[1:])
def test_an_element_is_the_eth_output_of_numpys_generator(key):
    """The counter contract: element e of slot (p, r) in round c2 of stream s is the e-th output of
    numpy.random.Philox(counter=[0, (p << 32) | r, c2, s], key=key); the uniform is Generator.random()'s."""
    P, R, D, rounds, c2_first = 3, 2, 7, 2, (1 << 63) + 5
    for stream in (0, 3, TOP - 1):
        bits = X.fill('bits', key, stream, c2_first, rounds, P, R, D).view(U)
        unif = X.fill('uniform', key, stream, c2_first, rounds, P, R, D)
        for i in range(rounds):
            for p in range(P):
                for r in range(R):
                    counter = (0, (p << 32) | r, c2_first + i, stream)
                    assert np.array_equal(bits[i, p, r], numpy_raw(key, counter, D))
                    g = np.random.Generator(np.random.Philox(counter=np.array(counter, dtype=U), key=np.array(key, dtype=U)))
                    assert np.array_equal(unif[i, p, r], g.random(D))
    # high path and slot numbers: the two fields of c1
    w = X.words(key, 1, 0, 1, 1, 1, 4, p0=(1 << 31) - 1, r0=(1 << 32) - 1)
    assert np.array_equal(w[0, 0, 0], numpy_raw(key, (0, (((1 << 31) - 1) << 32) | ((1 << 32) - 1), 0, 1), 4))


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    cxx = next((c for c in ('c++', 'g++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler found (tried c++, g++, clang++, /opt/rocm/lib/llvm/bin/clang++)'
    exe = str(tmp_path_factory.mktemp('philox') / 'philox_check')
    subprocess.run([cxx, '-O2', '-std=c++17', os.path.join(ROOT, 'tools', 'philox_check.cpp'), '-o', exe], check=True)
    return exe


def test_the_header_compiled_for_the_host_prints_the_same_blocks(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.rstrip().endswith('philox_check: ok'), r.stdout + r.stderr
    for key in KEYS:
        args = [str(v) for c in COUNTERS for v in c]
        r = subprocess.run([checker, hex(key[0]), str(key[1])] + args, capture_output=True, text=True, check=True)
        rows = [[int(v, 16) for v in line.split()] for line in r.stdout.splitlines()]
        assert len(rows) == len(COUNTERS)
        for counter, row in zip(COUNTERS, rows):
            # (the tool prints the block of the counter itself; numpy's first block is the counter's successor's)
            mine = [int(v[0]) for v in X.philox(*(np.array([c], dtype=U) for c in counter), *key)]
            assert row == mine
            before = advanced(counter, -1)
            assert row == numpy_raw(key, before, 4).tolist()


# -------------------------------------------------------------------------------------------------------------- independence
def test_a_number_does_not_depend_on_the_shape_of_the_call():
    key = X.key_of(7)
    for kind in X.KINDS:
        big = X.fill(kind, key, 1, 10, 5, 4, 6, 7)
        assert np.array_equal(X.fill(kind, key, 1, 10, 5, 2, 3, 7), big[:, :2, :3])                   # P and R
        assert np.array_equal(X.fill(kind, key, 1, 12, 2, 4, 6, 7), big[2:4])                         # rounds and their split
        assert np.array_equal(X.fill(kind, key, 1, 10, 5, 4, 6, 7, p0=0, r0=2)[:, :, :4], big[:, :, 2:])
        assert np.array_equal(X.fill(kind, key, 1, 10, 5, 4, 6, 3), big[..., :3])                     # D
        assert not np.array_equal(X.fill(kind, key, 2, 10, 5, 4, 6, 7), big)                          # the stream
        assert not np.array_equal(X.fill(kind, X.key_of(8), 1, 10, 5, 4, 6, 7), big)                  # the seed
    # an odd D: the last normal is the cosine of its pair, whatever D
    assert np.array_equal(X.fill('normal', key, 1, 10, 5, 4, 6, 5), X.fill('normal', key, 1, 10, 5, 4, 6, 7)[..., :5])
    assert np.array_equal(X.fill('normal', key, 1, 10, 5, 4, 6, 4), X.fill('normal', key, 1, 10, 5, 4, 6, 7)[..., :4])


def test_the_streams_do_not_depend_on_P_R_rounds_block_size_or_n_moves():
    big, small = X.Streams(3, 5, 7, 3), X.Streams(3, 2, 4, 3)
    zb, ub = big.block(6)
    parts = [small.block(n) for n in (1, 3, 2)]                                   # another block size
    zs, us = np.concatenate([a for a, _ in parts]), np.concatenate([b for _, b in parts])
    assert zs.shape == (6, 2, 4, 3) and us.shape == (6, 2, 4) and np.all(us <= 0.0)
    assert np.array_equal(zb[:, :2, :4], zs) and np.array_equal(ub[:, :2, :4], us)
    assert np.array_equal(big.block(2)[0][:, :2, :4], small.block(2)[0])          # and the blocks go on where they stopped
    for cls in (X.SmcStreams, X.SusStreams):
        big, small = cls(3, 5, 7, 3), cls(3, 2, 4, 3)
        assert np.array_equal(big.prior_uniforms()[:2, :4], small.prior_uniforms())
        seen = []
        for t in range(3):
            b, s = big.stage(5), small.stage(3)                                   # n_moves = 4 beside n_moves = 2
            if cls is X.SmcStreams:
                assert b[0].shape == (5,) and np.array_equal(b[0][:2], s[0]) and np.all((b[0] >= 0.0) & (b[0] < 1.0))
                b, s = b[1:], s[1:]
                assert b[1].shape == (5, 5, 7)
            else:
                assert b[1].shape == (5, 5, 7, 3)
            assert b[0].shape == (5, 5, 7, 3)
            for x, y in zip(b, s):
                assert np.array_equal(x[:3, :2, :4], y)
            seen.append(s[0])
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[0][0], seen[0][1])
        assert not np.array_equal(seen[0][:, 0], seen[0][:, 1]) and not np.array_equal(seen[0][:, :, 0], seen[0][:, :, 1])
    assert not np.array_equal(X.SusStreams(None, 1, 2, 1).prior_uniforms(), X.SusStreams(None, 1, 2, 1).prior_uniforms())


def test_the_device_streams_and_their_twins_share_the_layout():
    """The stream ids and the round of a stage, which the twins restate, are the driver's."""
    from dgp_amd import calibrate, reliability
    assert (X.STREAM_PRIOR, X.STREAM_NORMAL, X.STREAM_LOGU, X.STREAM_RESAMPLE) == \
        (calibrate.STREAM_PRIOR, calibrate.STREAM_NORMAL, calibrate.STREAM_LOGU, calibrate.STREAM_RESAMPLE) == (0, 1, 2, 3)
    assert X.stage_round(3, 2) == calibrate.stage_round(3, 2) == (3 << 32) | 2

    class Recorder:
        """An engine that records what the device streams ask for, and answers from the restatement."""
        device = None

        def __init__(self):
            self.calls = []

        def philox_fill(self, kind, key, stream, c2_first, rounds, P, R, D):
            import torch
            self.calls.append((kind, stream, c2_first, rounds, P, R, D))
            return torch.from_numpy(X.fill(kind, key, stream, c2_first, rounds, P, R, D))
    for dev, ref in ((calibrate.DeviceStreams, X.Streams), (calibrate.DeviceSmcStreams, X.SmcStreams),
                     (reliability.DeviceSusStreams, X.SusStreams)):
        d, r = dev(Recorder(), 11, 3, 4, 2), ref(11, 3, 4, 2)
        assert d.key == r.key == X.key_of(11)
        if ref is not X.Streams:
            assert np.array_equal(d.prior_uniforms().numpy(), r.prior_uniforms())
        for rounds in (3, 2):
            got = d.block(rounds) if ref is X.Streams else d.stage(rounds)
            want = r.block(rounds) if ref is X.Streams else r.stage(rounds)
            assert len(got) == len(want)
            for a, b in zip(got, want):
                assert a.is_contiguous() and np.array_equal(a.numpy(), b)


# ---------------------------------------------------------------------------------------------------------------- transforms
def test_moments_of_the_transforms():
    """10^5 numbers each: the mean, variance and fourth moment of the normals (0, 1, 3; standard errors sqrt(1 / n),
    sqrt(2 / n), sqrt(96 / n)) and the mean of log u (-1; sqrt(1 / n)) within 5 standard errors; the uniforms' likewise."""
    n, key = 100000, X.key_of(2024)
    z = X.fill('normal', key, 1, 0, 10, 10, 250, 4).reshape(-1)
    lu = X.fill('log_uniform', key, 2, 0, 10, 10, 250, 4).reshape(-1)
    u = X.fill('uniform', key, 0, 0, 10, 10, 250, 4).reshape(-1)
    assert len(z) == len(lu) == len(u) == n
    figures = {'mean of z': (z.mean(), 0.0, 1.0), 'variance of z': (np.mean(z * z), 1.0, 2.0), 'fourth moment of z': (np.mean(z ** 4), 3.0, 96.0),
               'mean of log u': (lu.mean(), -1.0, 1.0), 'mean of u': (u.mean(), 0.5, 1.0 / 12.0),
               'cosine against sine': (np.mean(z[0::2] * z[1::2]) * math.sqrt(0.5), 0.0, 1.0)}
    for what, (got, exact, var) in figures.items():
        zscore = (got - exact) / math.sqrt(var / n)
        print('%s: %.5f, exact %g, z %.2f' % (what, got, exact, zscore))
        assert abs(zscore) <= 5.0, what
    assert np.all(np.isfinite(z)) and np.all(lu <= 0.0) and np.all((u >= 0.0) & (u < 1.0))
    # the ends of the two mappings: u1 never 0 (rho finite), u never 1
    w = np.array([0, 2047, 2048, TOP - 1], dtype=U)
    assert np.array_equal(X.to_uniform(w), [0.0, 0.0, 2.0 ** -53, 1.0 - 2.0 ** -53])
    assert np.array_equal(X.to_uniform_open0(w), [2.0 ** -53, 2.0 ** -53, 2.0 ** -52, 1.0])


# ------------------------------------------------------------------------------------- subset simulation on the Philox streams
def sus_seeds(fun, threshold, D, lo, hi, pv=None, pm=None):
    import boxsus_ref as S
    import test_boxsus_host as H
    from dgp_amd import calibrate, reliability
    out, zero = [], np.zeros(D)
    for seed in range(H.SEEDS):
        streams = X.SusStreams(seed, 1, H.R, D)
        x0 = calibrate.prior_draws(streams.prior_uniforms(), lo, hi, zero if pv is None else pv, zero if pm is None else pm)[0]
        out.append(S.sus(fun, x0, lo, hi, threshold, streams, reliability.n_survivors(H.LEVEL_PROB, H.R), pv=pv, pm=pm, p=0))
    return out


@pytest.mark.parametrize('D,prob', [(1, 1e-3), (2, 1e-3), (5, 1e-3), (5, 1e-6)])
def test_corner_event_on_the_philox_streams(D, prob):
    """test_boxsus_host.against_exact, unchanged, on the restatement's schedule with the Philox twin of SusStreams."""
    import boxsus_ref as S
    import test_boxsus_host as H
    fun, threshold, exact = S.corner(D, prob)
    H.against_exact(sus_seeds(fun, threshold, D, np.zeros(D), np.ones(D)), exact, 'corner D %d on Philox' % D)


def test_halfspace_on_the_philox_streams():
    import boxsus_ref as S
    import test_boxsus_host as H
    fun, threshold, exact, (pv, pm), (lo, hi) = S.halfspace(2, 3.0)
    H.against_exact(sus_seeds(fun, threshold, 2, lo, hi, pv, pm), exact, 'half-space D 2 on Philox')


# -------------------------------------------------------------------------------------------- tempered SMC on the Philox streams
def test_smc_on_the_philox_streams_against_quadrature():
    """test_boxsmc_host's smallest closed-form case, '1d', and its conditions: 16 seeds x 512 particles, the seeds' average of
    the log evidence, of the mass of x < 0.5 and of the particles' mean and variance within 5 standard errors of quadrature."""
    import boxmala_ref as M
    import boxsmc_ref as S
    import test_boxsmc_host as H
    from dgp_amd import calibrate
    fun = H.bimodal_1d
    w, ybar, lo, hi = np.array([1.0 / 0.02 ** 2]), np.array([0.49]), np.zeros(1), np.ones(1)
    axes = [np.linspace(0.0, 1.0, 8001)]
    f_grid = fun(axes[0][:, None])[0][:, 0]
    logz, mass = S.grid_evidence(f_grid, axes, ybar, w, None, None), S.grid_mass(f_grid, axes, ybar, w, 0.5, None, None)
    mean, cov = M.grid_posterior(f_grid, axes, ybar, w, None, None)
    res = []
    for seed in range(H.SEEDS):
        streams = X.SmcStreams(seed, 1, H.R, 1)
        x0 = calibrate.prior_draws(streams.prior_uniforms(), lo, hi, np.zeros(1), np.zeros(1))[0]
        res.append(S.smc(fun, x0, w, ybar, lo, hi, hi - lo, streams, H.gain))
    assert all(r['status'] == S.OK and r['betas'][-1] == 1.0 for r in res)
    H.within([r['log_evidence'] for r in res], logz, 'log evidence on Philox')
    H.within([np.mean(r['x'][:, 0] < 0.5) for r in res], mass, 'mass of x_0 < 0.5 on Philox')
    H.within([r['x'][:, 0].mean() for r in res], mean[0], 'mean of x_0 on Philox')
    H.within([r['x'][:, 0].var() for r in res], cov[0, 0], 'variance of x_0 on Philox')
    assert all(np.all(r['x'] >= lo) and np.all(r['x'] <= hi) for r in res)


# ------------------------------------------------------------------------------------------------------------------ the rest
def test_refusals_without_a_device():
    from dgp_amd import calibrate, reliability
    from dgp_amd.ops import Engine
    ok = dict(kind='normal', key=(1, 2), stream=1, c2_first=0, rounds=3, P=2, R=5, D=7)
    assert Engine.philox_check(**ok) == (3, 1, 2, 1, 0, 3, 2, 5, 7)
    assert Engine.philox_check(**dict(ok, c2_first=TOP - 4, key=(TOP - 1, 0), stream=TOP - 1))[4] == TOP - 4
    for bad in (dict(kind='gamma'), dict(kind=3), dict(key=(1,)), dict(key=3), dict(key=(-1, 0)), dict(key=(0, TOP)), dict(stream=-1),
                dict(stream=TOP), dict(c2_first=-1), dict(c2_first=TOP), dict(rounds=0), dict(P=0), dict(R=0), dict(D=0), dict(D=65),
                dict(P=1 << 31), dict(R=1 << 32), dict(c2_first=TOP - 3), dict(c2_first=TOP - 1, rounds=1),
                dict(rounds=1 << 55, P=1, R=3), dict(P=(1 << 31) - 1, R=(1 << 32) - 1)):
        with pytest.raises(ValueError):
            Engine.philox_check(**dict(ok, **bad))
    assert Engine.philox_key(5) == X.key_of(5) == tuple(int(k) for k in np.random.SeedSequence(5).generate_state(2, np.uint64))
    assert Engine.philox_key(None) != Engine.philox_key(None)
    # the keyword: anything but 'numpy' and 'device' is refused before a device is needed
    box = np.array([[0.0, 1.0], [0.0, 1.0]])
    for rng in ('philox', 'cpu', None, 0, ''):
        with pytest.raises(ValueError, match='rng'):
            reliability.failure_probability(None, 3, 2, 2, None, 0.5, box, rng=rng)
        with pytest.raises(ValueError, match='rng'):
            calibrate.calibrate_smc(None, 3, 2, 2, None, None, 1, np.zeros(2), 0.1, box, rng=rng)
        with pytest.raises(ValueError, match='rng'):
            calibrate.calibrate(None, 3, 2, 2, None, None, 1, np.zeros(2), 0.1, box, rng=rng)
    assert calibrate.RNGS == ('numpy', 'device')
    assert not calibrate.check_rng('numpy', 'x') and calibrate.check_rng('device', 'x')


def test_the_header_and_the_engine_agree():
    from dgp_amd import _lib
    from dgp_amd.ops import Engine
    from test_cabi_symbols import declared_functions
    src = open(os.path.join(ROOT, 'include', 'dgp_amd.h')).read()
    header = {k.lower(): int(v) for k, v in re.findall(r'#define\s+DGPAMD_PHILOX_([A-Z_]+)\s+(\d+)', src)}
    assert header.pop('count') == 4 and header == Engine.PHILOX and tuple(sorted(header, key=header.get)) == X.KINDS
    assert 'dgpamd_philox_fill' in declared_functions() and 'dgpamd_philox_fill' in _lib.SIGNATURES
    hpp = open(os.path.join(ROOT, 'dgp_amd', 'csrc', 'philox.hpp')).read()
    consts = {k: int(v, 16) for k, v in re.findall(r'#define\s+PHILOX_([MW][01])\s+(0x[0-9A-Fa-f]+)ULL', hpp)}
    assert consts == dict(M0=int(X.M0), M1=int(X.M1), W0=int(X.W0), W1=int(X.W1))
    assert int(re.search(r'#define\s+PHILOX_ROUNDS\s+(\d+)', hpp).group(1)) == X.ROUNDS == 10
    # a null context is refused first; the other host-side checks are exercised by tools/philox_check.cpp
    assert _lib.lib.dgpamd_philox_fill(None, 3, 1, 2, 1, 0, 1, 1, 1, 1, None) == _lib.BAD_ARG
    # philox.hip is one of the files that are compiled without contraction
    mk = open(os.path.join(ROOT, 'dgp_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^philox\.o: override FLAGS \+= -ffp-contract=off$', mk, flags=re.M)


def test_rng_numpy_is_the_default_of_every_entry_point():
    """rng is a keyword with default 'numpy' on the three drivers and on both containers: the last one of calibrate_smc and
    failure_probability; in calibrate it stands in front of target_accept, method, n_leapfrog and jitter, the tail that
    tests/test_boxhmc_host.py pins.  The numpy streams are the classes they were, so rng='numpy' is the code path of a call
    without the keyword."""
    from dgp_amd import calibrate, pathfun, reliability
    owners = [(calibrate, ('calibrate', 'calibrate_smc')), (reliability, ('failure_probability',)),
              (pathfun.PathFunctions, ('calibrate', 'calibrate_smc', 'failure_probability')),
              (pathfun.GpPaths, ('calibrate', 'calibrate_smc', 'failure_probability'))]
    for owner, names in owners:
        for name in names:
            par = list(inspect.signature(getattr(owner, name)).parameters.values())
            at = -5 if name == 'calibrate' else -1
            assert par[at].name == 'rng' and par[at].default == 'numpy', (owner, name)
            if name == 'calibrate':
                assert [q.name for q in par[-6:]] == ['prior', 'rng', 'target_accept', 'method', 'n_leapfrog', 'jitter']
    for cls, args in ((calibrate.PathPosterior, [None] * 7), (calibrate.ParticlePosterior, [None] * 12),
                      (reliability.FailureProbability, [None] * 10)):
        assert cls(*args).rng == 'numpy' and cls(*args, rng='device').rng == 'device'
    # the numpy streams' numbers, pinned: what a seed gave before the keyword existed
    z, lu = calibrate.Streams(5, 2, 3, 2).block(2)
    ref = np.random.default_rng(np.random.SeedSequence(5).spawn(2)[0].spawn(3)[1]).standard_normal((2, 2, 2))
    assert np.array_equal(z[:, :, 1], ref) and lu.shape == (2, 2, 3)
    u = reliability.SusStreams(5, 2, 3, 2).prior_uniforms()
    assert np.array_equal(u[1], np.random.default_rng(np.random.SeedSequence(5, spawn_key=(0, 1))).random((3, 2)))
    import torch
    t = torch.ones(2)
    assert calibrate.upload(None, t) is t                                        # (what a device stream returns is not uploaded)
