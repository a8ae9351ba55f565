"""dgpamd_vpathfun_update (Engine.vpathfun_update; DESIGN I.14) against the numpy restatement tests/vpathfun_ref.py.

Bound per (path, row), on out / sqrt(scale): 1e-8 sum_j |b_j r_j| + 1e-10 with b from float64 numpy -- the project's gp_vecch
mean tolerances (rtol 1e-8, atol 1e-10) applied to the magnitude of the sum, because a sum of residuals can cancel.  Every
test prints its worst ratio to the bound before it asserts.  Needs an MI355X: -m gpu."""
import functools

import numpy as np
import pytest

import vpathfun_ref as V
from test_gpu_ops import engine_under

pytestmark = pytest.mark.gpu
npy = lambda t: t.cpu().numpy()


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)

# (kind, lengths, omega, n, pm, D, P, M): pm 51 | 52 and D 16 | 17 are the register | LDS boundaries; n < pm: padded sets
SHARED = [('sexp', 'one', True, 70, 3, 1, 1, 1),
          ('matern2.5', 'D', False, 70, 51, 5, 64, 4),
          ('sexp', 'D', True, 70, 52, 16, 65, 5),
          ('matern2.5', 'one', True, 70, 64, 17, 130, 257),
          ('sexp', 'one', False, 70, 51, 16, 130, 257),
          ('matern2.5', 'D', True, 70, 51, 17, 65, 5),
          ('sexp', 'D', False, 5, 51, 5, 65, 5),
          ('matern2.5', 'D', True, 5, 64, 5, 64, 4),
          ('matern2.5', 'one', True, 1, 1, 1, 1, 4),
          ('sexp', 'one', False, 1, 3, 5, 130, 1)]
# per-path rows, three groups (three training sets, one call each, as the host makes them): P is the paths of ONE group
PER_PATH = [('sexp', 'D', True, 70, 51, 5, 1, 257),
            ('matern2.5', 'one', False, 70, 52, 16, 64, 4),
            ('sexp', 'one', True, 70, 64, 17, 65, 5),
            ('matern2.5', 'D', True, 70, 3, 1, 130, 1),
            ('matern2.5', 'D', False, 5, 51, 16, 65, 5),
            ('sexp', 'one', True, 1, 1, 5, 1, 4)]


@functools.lru_cache(maxsize=None)
def problem(kind, nlen, with_omega, n, pm, D, P, M, per_path, nugget, seed=0):
    """One training set and its rows, scaled coordinates, with the float64 reference: (xs, Ws, NN, omega, r, prior, ref,
    mag, scale).  Shared rows: xs (M, D), r (P, n), prior / ref / mag (P, M).  Per-path rows: xs (P, M, D) and NN of the
    P * M stacked rows.  Row 0 lies on a training row."""
    rng = np.random.default_rng([seed, n, pm, D, P, M])
    length = np.array([0.8]) if nlen == 'one' else rng.uniform(0.5, 1.2, size=D)
    W = rng.uniform(size=(n, D))
    x = rng.uniform(size=(P, M, D) if per_path else (M, D))
    x.reshape(-1, D)[0] = W[min(3, n - 1)]
    omega = 1.0 / rng.integers(1, 4, size=n) if with_omega else None
    r, prior = rng.normal(size=(P, n)), rng.normal(size=(P, M))
    xs, Ws = x / length, W / length
    flat = xs.reshape(-1, D)
    NN = V.neighbours(flat, Ws, pm, pad=pm)
    B = V.coefficients(flat, Ws, NN, kind, nugget, omega)
    if per_path:
        s, mag = (np.stack([a[p, p * M:(p + 1) * M] for p in range(P)]) for a in V.update(B, NN, r))
    else:
        s, mag = V.update(B, NN, r)
    return xs, Ws, NN, omega, r, prior, prior + s, mag, 1.7


def run(e, kind, prob, per_path, nugget, jitters=(0.0, 1e-10, 1e-8)):
    """Engine.vpathfun_update on a problem: (out / sqrt(scale) as (P, M), info)."""
    import torch
    xs, Ws, NN, omega, r, prior, _, _, scale = prob
    t = e.tensor
    om = None if omega is None else t(omega)
    if per_path:
        out, info = e.vpathfun_update(kind, t(xs), t(Ws), t(NN, dtype=torch.int64), t(r), t(prior), scale, nugget, jitters, om)
        return npy(out) / np.sqrt(scale), npy(info)
    out, info = e.vpathfun_update(kind, t(xs), t(Ws), t(NN, dtype=torch.int64), t(np.ascontiguousarray(r.T)),
                                  t(np.ascontiguousarray(prior.T)), scale, nugget, jitters, om)
    return npy(out).T / np.sqrt(scale), npy(info)


def check(tag, got, prob):
    ref, mag = prob[6], prob[7]
    bound = 1e-8 * mag + 1e-10
    print('%s: max |device - numpy| / bound = %.3g' % (tag, (np.abs(got - ref) / bound).max()))
    assert np.all(np.abs(got - ref) <= bound)


@pytest.mark.parametrize('nugget', [1e-2, 1e-3])
@pytest.mark.parametrize('case', SHARED, ids=lambda c: '-'.join(map(str, c)))
def test_shared_rows_equal_numpy(eng, case, nugget):
    got, info = run(eng, case[0], problem(*case, False, nugget), False, nugget)
    assert list(info) == [0, -1]
    check('shared %s nugget %g' % (case, nugget), got, problem(*case, False, nugget))


@pytest.mark.parametrize('nugget', [1e-2, 1e-3])
@pytest.mark.parametrize('case', PER_PATH, ids=lambda c: '-'.join(map(str, c)))
def test_per_path_rows_equal_numpy(eng, case, nugget):
    for g in range(3):
        prob = problem(*case, True, nugget, seed=g)
        got, info = run(eng, case[0], prob, True, nugget)
        assert list(info) == [0, -1]
        check('per-path %s group %d nugget %g' % (case, g, nugget), got, prob)


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_default_nugget_against_a_longdouble_solve(eng, kind):
    """Nugget 1e-6, the default: the blocks' condition numbers reach 1e7 and 1e-8 relative is not what float64 gives.  The
    reference is a long-double Cholesky solve of the same float64 blocks; E is the float64 numpy solve's worst deviation from it,
    relative to sum_j |b_j r_j| with the long-double b; the device gets 10 E (it eliminates in another order than LAPACK, so a
    bound at numpy's own error would test the order and not the arithmetic).  Measured: DESIGN I.14."""
    case, nugget = (kind, 'D', True, 70, 51, 5, 65, 33), 1e-6
    prob = problem(*case, False, nugget)
    xs, Ws, NN, omega, r, prior = prob[:6]
    Bl = V.coefficients_longdouble(xs, Ws, NN, kind, nugget, omega)
    t = Bl[None] * r[:, np.where(NN >= 0, NN, 0)].astype(np.longdouble)
    ref, mag = prior + t.sum(-1), np.abs(t).sum(-1).astype(float)
    E = (np.abs(prob[6] - ref).astype(float) / mag).max()
    got, info = run(eng, kind, prob, False, nugget)
    dev = (np.abs(got - ref).astype(float) / mag).max()
    print('%s nugget 1e-6: numpy float64 E = %.3g, device %.3g (bound 10 E = %.3g)' % (kind, E, dev, 10 * E))
    assert list(info) == [0, -1] and dev <= 10 * E


@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_one_path_of_y_is_vecchia_gp(eng, kind):
    """prior = 0, one path, residual = y: out / sqrt(scale) is dgpamd_vecchia_gp's mean on the same conditioning sets, at that
    family's rtol 1e-8, atol 1e-10."""
    import torch
    rng = np.random.default_rng(12)
    n, M, D, pm, scale, nugget = 70, 40, 3, 20, 1.7, 1e-3
    length = np.array([0.6, 1.1, 0.9])
    W, x, y = rng.uniform(size=(n, D)), rng.uniform(size=(M, D)), rng.normal(size=n)
    omega = 1.0 / rng.integers(1, 4, size=n)
    t = eng.tensor
    xs, Ws = t(x / length), t(W / length)
    NN = eng.nn_query(xs, Ws, pm)
    out, _ = eng.vpathfun_update(kind, xs, Ws, NN, t(y[:, None]), eng.zeros(M, 1), scale, nugget, (0.0,), t(omega))
    mean, _ = eng.vecchia_gp(kind, t(x), t(W), NN, t(y), scale, length, nugget, t(omega))
    np.testing.assert_allclose(npy(out)[:, 0] / np.sqrt(scale), npy(mean), rtol=1e-8, atol=1e-10)


@pytest.mark.parametrize('per_path', [False, True])
@pytest.mark.parametrize('kind', ['sexp', 'matern2.5'])
def test_register_and_lds_forms_agree(eng, kind, per_path):
    """Sizes the register form takes, once more under DGPAMD_VECCHIA_LDS=1 with NaNs in every CU's LDS first: test_gpu_ops' bound
    for the sibling kernels' two forms, at nugget 1e-2 (condition numbers up to 5e3: the forms differ by 1e-12 of the sum's
    magnitude, which leaves three digits for cancellation)."""
    nugget = 1e-2
    for case in [(kind, 'D', True, 70, 51, 16, 65, 33), (kind, 'one', False, 70, 20, 3, 3, 70), (kind, 'D', True, 5, 51, 8, 2, 9)]:
        prob = problem(*case, per_path, nugget)
        reg, _ = run(eng, kind, prob, per_path, nugget)
        with engine_under(VECCHIA_LDS=1, POISON_LDS=1) as e:
            lds, info = run(e, kind, prob, per_path, nugget)
        assert list(info) == [0, -1]
        np.testing.assert_allclose(lds, reg, rtol=1e-9, atol=1e-11)
        check('lds %s' % (case,), lds, prob)


@pytest.mark.parametrize('lds', [None, 1])
@pytest.mark.parametrize('per_path', [False, True])
def test_a_row_does_not_depend_on_the_rows_of_its_call(eng, lds, per_path):
    """Slices [0:1], [1:65], [65:257] of a 257-row call, neighbour search included (the slice is queried alone), reproduce it bit
    for bit in both forms and both storages."""
    import torch
    from dgp_amd import vpathfun
    rng = np.random.default_rng(5)
    n, M, D, pm, P, scale, nugget = 70, 257, 4, 12, 3, 1.7, 1e-3
    W = rng.uniform(size=(n, D))
    r = rng.normal(size=(P, n))
    with engine_under(VECCHIA_LDS=lds) as e:
        t = e.tensor
        Ws = t(W)

        def call(x, prior):   # x (rows, D) for shared rows; (P, rows, D) per path
            xs = t(x)
            NN = vpathfun.neighbours(e, xs.reshape(-1, D), Ws, pm)
            if per_path:
                return e.vpathfun_update('matern2.5', xs, Ws, NN, t(r), t(prior), scale, nugget, (0.0, 1e-10), None)[0]
            return e.vpathfun_update('matern2.5', xs, Ws, NN, t(np.ascontiguousarray(r.T)), t(np.ascontiguousarray(prior.T)), scale,
                                     nugget, (0.0, 1e-10), None)[0].T
        x = rng.uniform(size=(P, M, D) if per_path else (M, D))
        prior = rng.normal(size=(P, M))
        whole = call(x, prior)
        for lo, hi in ((0, 1), (1, 65), (65, 257)):
            part = call(np.ascontiguousarray(x[..., lo:hi, :]), np.ascontiguousarray(prior[:, lo:hi]))
            assert torch.equal(part, whole[:, lo:hi]), (lo, hi)


@pytest.mark.parametrize('lds', [None, 1])
def test_jitter_ladder_is_a_property_of_the_row(eng, lds):
    """Two identical neighbours and nugget 0: the block is singular, the row is redone with the next rung by its own wave --
    a finite value and info[0] == 1; the same row among well-posed rows has the same bits, and their bits do not change
    by its presence.  With a one-rung ladder the row is reported in info[1] (1 + its index), not raised or faulted on."""
    import torch
    from dgp_amd import vpathfun
    rng = np.random.default_rng(9)
    n, D, pm, P = 40, 3, 8, 5
    W = rng.uniform(size=(n, D))
    W[7] = W[3] = 3.0    # two identical training rows, far from the others: no other row has them in its set
    good = rng.uniform(size=(6, D))
    twin = W[3] + 0.01   # its two nearest neighbours are rows 3 and 7
    r, prior = rng.normal(size=(n, P)), rng.normal(size=(7, P))
    with engine_under(VECCHIA_LDS=lds) as e:
        t = e.tensor
        Ws = t(W)

        def call(x, pr, ladder=(0.0, 1e-10, 1e-8)):
            xs = t(x)
            out, info = e.vpathfun_update('sexp', xs, Ws, vpathfun.neighbours(e, xs, Ws, pm), t(r), t(pr), 1.3, 0.0, ladder, None)
            return out, list(npy(info))
        alone, info = call(twin[None], prior[3:4])
        assert info == [1, -1] and bool(torch.isfinite(alone).all())
        x = np.concatenate((good[:3], twin[None], good[3:]))
        mixed, info = call(x, prior)
        assert info == [1, -1] and torch.equal(mixed[3:4], alone)
        clean, info = call(good, np.delete(prior, 3, 0))
        assert info == [0, -1] and torch.equal(clean, mixed[[0, 1, 2, 4, 5, 6]])
        _, info = call(x, prior, ladder=(0.0,))
        assert info == [0, 4]


def test_a_block_beyond_the_lds_is_refused_before_any_launch(eng):
    import torch
    from dgp_amd.ops import DgpAmdError
    n, D, pm = 200, 2, 150   # (151 * 152 doubles: 184 KB)
    z = eng.zeros
    with pytest.raises(DgpAmdError, match='LDS'):
        eng.vpathfun_update('sexp', z(1, D), z(n, D), torch.zeros(1, pm, dtype=torch.int64, device=eng.device), z(n, 1), z(1, 1), 1.0,
                            1e-3, (0.0,))
