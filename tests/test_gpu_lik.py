"""The likelihood nodes' log-densities on the device (lik_point and its helpers, lik_partial_kernel / lik_sum_kernel, reached
through dgpamd_lik_loglik and the I-step queue's ess_liknode_ll_kernel) against exact values: tests/lik_ref.py, mpmath from the
definitions.  Needs an MI355X: -m gpu.

Bound (lik_ref's docstring): |got - exact| <= C 2^-53 T + 2^-1074 per value, C = 4 x the constant measured for a stable float64
form on the CPU (tests/test_lik_host.py); a sum adds (ceil(per / 256) + 8 + 32) 2^-53 sum |exact_i| for the kernel's own order of
additions.  Every test prints its worst error / bound as a PARITY line before it asserts.

Per-point values: one call takes one observation (nobs = n = 1) and 64 candidate blocks of one latent row, so it returns 64
single log-densities; the two- and three-column kinds need 121 rows for every pairing of the wild values alone, so their grid
is three such calls per count.  Latent rows are 70 wide, the columns read through a permuted `cols`, every other entry NaN."""
import math

import numpy as np
import pytest

import lik_ref as R

pytestmark = pytest.mark.gpu

M = 70
COLS = {'Poisson': [41], 'NegBin': [69, 3], 'ZIP': [17, 0], 'ZINB': [5, 68, 33], 'logit': [69], 'probit': [0]}


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def class_cols(K):
    return np.random.default_rng(K).permutation(M)[:K].tolist()


def device_points(eng, kind, y, F, cols, K=0):
    """The log-density of observation y at every row of F (R x ncol), 64 rows per call."""
    import torch
    yd = eng.tensor(np.array([float(y)]))
    lik = dict(kind=kind, y=yd, rep=None, classes=K, par=R.EPS)
    out = []
    for s in range(0, len(F), 64):
        rows = F[s:s + 64]
        FP = np.full((len(rows), 1, M), np.nan)
        FP[:, 0, cols] = rows
        out.append(eng.lik_loglik(lik, np.asarray(cols, dtype=np.int32), eng.tensor(FP)))
    return torch.cat(out).cpu().numpy()


def check_points(tag, kind, got, ex, lo, T):
    assert np.all(np.isfinite(ex)), (tag, 'the grid holds only inputs with a finite exact value')
    assert np.all(np.isfinite(got)), (tag, np.nonzero(~np.isfinite(got))[0])
    ratio = np.abs((got - ex) - lo) / R.point_bound(kind, T)
    return float(ratio.max()), int(ratio.argmax())


@pytest.mark.parametrize('kind', ['Poisson', 'NegBin', 'ZIP', 'ZINB', 'logit', 'probit'])
def test_point_values_against_exact(eng, kind):
    """Counts 0 .. 10^6 (the rising sum's ends 63, 64, 65; the lgamma difference beyond) and both classes of logit / probit, at
    the wild latents in every pairing, logaddexp's a == b case and the probit switch points with their neighbouring doubles:
    finite wherever the exact value is, and inside the bound."""
    worst, where = 0.0, None
    for y in R.point_ys(kind):
        F, ex, lo, T = R.point_reference(kind, y)
        assert len(F) % 64 == 0
        got = device_points(eng, kind, y, F, COLS[kind])
        w, i = check_points((kind, y), kind, got, ex, lo, T)
        if w > worst:
            worst, where = w, (y, F[i].tolist(), got[i], ex[i])
    print('PARITY point %-9s worst |error| / (C 2^-53 T) = %.3f  (C = %.2f) at y, f, got, exact = %s' % (kind, worst, R.C[kind], where))
    assert worst <= 1.0, where


def test_equal_arguments_of_logaddexp_give_log_2_to_the_last_bit(eng):
    """lik_logaddexp's a == b case returns a + log 2 from a constant.  At f = 0 the logit density of y = 0 is -logaddexp(0, 0),
    and 0 + c is exact: the result must be the double nearest to -log 2 (a constant off in its last digit is one ulp, which the
    bound of the point test, C 2^-53 T with C = 5.68, does not see)."""
    got = device_points(eng, 'logit', 0.0, np.array([[0.0], [-0.0]]), COLS['logit'])
    want = R.to_float(R.exact('logit', 0.0, [0.0]))
    assert want == -0.6931471805599453
    assert got[0] == want and got[1] == want, (got.tolist(), want)


@pytest.mark.parametrize('K', [2, 3, 4, 64])
@pytest.mark.parametrize('kind', ['softmax', 'robustmax'])
def test_class_values_against_exact(eng, kind, K):
    """Softmax: the top column first, last and in the middle, 0, 1, 700 and 1500 above the rest (exp of the difference
    underflows, the answer stays finite), around 0, -800 and 1000.  Robustmax: single, tied (the first index wins) and
    all-equal maxima, a maximum by one subnormal.  Columns through a permuted `cols` of a 70-wide row."""
    cols = class_cols(K)
    worst, where = 0.0, None
    for y in R.class_ys(K):
        F, ex, lo, T = R.class_reference(kind, K, y)
        got = device_points(eng, kind, y, F, cols, K)
        w, i = check_points((kind, K, y), kind, got, ex, lo, T)
        if w > worst:
            worst, where = w, (y, i, got[i], ex[i])
    print('PARITY class %-9s K=%-2d worst |error| / (C 2^-53 T) = %.3f  (C = %.2f) at y, row, got, exact = %s' % (kind, K, worst, R.C[kind], where))
    assert worst <= 1.0, where


def test_non_finite_inputs_keep_their_class(eng):
    """Inputs at which the definition is no finite double (lik_ref.NONFINITE: a NaN latent in any column that is read, e^f
    beyond the double range at f = 710) give NaN / -inf as the definition does; robustmax with NaN latents follows
    numpy.argmax (the first NaN is the maximum) and stays finite; softmax with a NaN latent is NaN."""
    for kind, y, row, cls in R.NONFINITE:
        assert R.same_class(R.to_float(R.exact(kind, y, row)), cls)
        got = device_points(eng, kind, y, np.array([row]), COLS[kind])
        assert R.same_class(got[0], cls), (kind, y, row, got)
    for K in (2, 3, 4, 64):
        F, winners = R.nan_class_rows(K)
        for y in R.class_ys(K):
            ex = np.array([R.to_float(R.exact('robustmax', y, r, classes=K, eps=R.EPS)) for r in F])
            assert np.array_equal(ex < -1.0, np.asarray(winners) != y)
            got = device_points(eng, 'robustmax', y, F, class_cols(K), K)
            assert np.all(np.abs(got - ex) <= R.point_bound('robustmax', np.abs(ex))), (K, y, got, ex)
            assert np.all(np.isnan(device_points(eng, 'softmax', y, F, class_cols(K), K)))


def run_sum(eng, kind, case):
    import torch
    ncol = R.NCOL[kind]
    cols = [4, 0, 2][:ncol]
    B, n, _ = case['FP'].shape
    FP = np.full((B, n, 5), np.nan)
    FP[:, :, cols] = case['FP']
    lik = dict(kind=kind, y=eng.tensor(case['y']), rep=None if case['rep'] is None else torch.as_tensor(case['rep'], device='cuda'),
               classes=0, par=0.0)
    FPd = eng.tensor(FP)
    got = eng.lik_loglik(lik, np.asarray(cols, dtype=np.int32), FPd).cpu().numpy()
    again = eng.lik_loglik(lik, np.asarray(cols, dtype=np.int32), FPd).cpu().numpy()
    assert np.array_equal(got, again), 'two calls, two results'
    return got


@pytest.mark.parametrize('nobs', R.SUM_NOBS)
@pytest.mark.parametrize('kind', ['Poisson', 'ZINB'])
def test_sums_against_exact(eng, kind, nobs):
    """The chunked sum: 300 distinct (y, latent row) pairs tiled through a replicate map that is a permutation with repeats to
    nobs observations -- fewer than the 32 chunks, one per chunk, one more, and (8161, 8192, 8193, 20000) the sizes at which
    the 256-stride loop of a chunk stops after one step, fills it exactly, and takes a second and a third -- for 1, 3 and 64
    candidate blocks of different latents, against math.fsum of the exact values; and the same bits from a second call."""
    worst = 0.0
    for B in (1, 3, 64):
        case = R.sum_case(kind, nobs, B)
        got = run_sum(eng, kind, case)
        assert np.all(np.isfinite(got))
        ratio = np.abs(got - case['want']) / case['bound']
        worst = max(worst, float(ratio.max()))
    print('PARITY sum %-8s nobs %-6d worst |error| / bound = %.3f' % (kind, nobs, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('kind', ['Poisson', 'ZINB'])
def test_sums_without_a_map(eng, kind):
    """nobs = n = 8193 latent rows read directly (per = 257: the stride loop's second step), 1 and 3 blocks."""
    worst = 0.0
    for B in (1, 3):
        case = R.sum_case(kind, 8193, B, mapped=False)
        got = run_sum(eng, kind, case)
        worst = max(worst, float((np.abs(got - case['want']) / case['bound']).max()))
    print('PARITY sum %-8s nobs = n = 8193, no map: worst |error| / bound = %.3f' % (kind, worst))
    assert worst <= 1.0


@pytest.mark.parametrize('kind', ['Poisson', 'ZINB'])
def test_queue_and_stand_alone_give_the_same_bits(eng, kind):
    """csrc/train.hip promises "the same bits from the queue and from dgpamd_lik_loglik".  One update of a 200-row block under a
    likelihood node through Engine.ess_queue_plan: (a) a threshold far below (u = 1e-300) -- the first proposal is accepted, and
    the log-likelihood the queue leaves in its state (candidate block 0 of 8, summed by ess_liknode_ll_kernel) has the bits of
    dgpamd_lik_loglik on the latents the queue left; (b) proposals along a direction that no threshold admits -- the update stays
    open, the latents are untouched, and the state holds the log-likelihood of the current latents (the queue's one-block
    pass) with the bits of the stand-alone call."""
    n, B = 200, 8
    ncol = R.NCOL[kind]
    cols = np.asarray([3, 0, 2][:ncol], dtype=np.int32)
    rng = np.random.default_rng(5)
    F0 = rng.normal(size=(n, 4))
    y = rng.poisson(3.0, size=n).astype(float)
    y[::7] = 0.0
    y[3], y[50] = 70.0, 64.0
    lik = dict(kind=kind, y=eng.tensor(y), rep=None, classes=0, par=0.0)
    plan = eng.ess_queue_plan(n, 4, [dict(lik=lik, colmap=cols)], B)
    for accepted, u0, nu_scale in ((True, 1e-300, 1.0), (False, 1.0 - 2.0 ** -53, 400.0)):
        F = eng.tensor(F0)
        NU = eng.tensor(nu_scale * rng.normal(size=(1, n, 4)))
        uniforms = np.concatenate(([u0], rng.uniform(0.2, 0.8, size=15)))
        plan.queue(F, NU, [1.0], uniforms, 0, None, 1, B, 1)
        st = plan.fetch()
        alone = eng.lik_loglik(lik, cols, F[None]).cpu().numpy()[0]
        assert st['info'] == 0 and math.isfinite(st['ll'])
        if accepted:
            assert st['status'] == 0 and st['proposals'] == 1 and not np.array_equal(F.cpu().numpy(), F0)
        else:
            assert st['status'] == 3 and st['proposals'] == B and np.array_equal(F.cpu().numpy(), F0)
        assert np.float64(st['ll']).tobytes() == np.float64(alone).tobytes(), (accepted, st['ll'], alone)
