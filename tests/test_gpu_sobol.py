"""The pick-freeze sums on the device (dgpamd_sobol_tiles, dgpamd_sobol_add; DESIGN I.16) against the exact sums of
tests/sobol_ref.py, within its derived bound 1.01 (ntiles + 8) 2^-53 sum |term|.  Every comparison prints the largest
error / bound it met before it asserts.  Needs an MI355X: -m gpu."""
import numpy as np
import pytest

import sobol_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def device_sums(eng, fA, fB, fAB, shift, cuts=()):
    """The running sums over the rows of (P, M, K) host arrays, one sobol_tiles + sobol_add per piece of rows between cuts."""
    P, M, K = fA.shape
    sums = eng.zeros(P, K, 4 if fAB is None else 2)
    sd = eng.tensor(shift)
    edges = [0, *cuts, M]
    for a, c in zip(edges, edges[1:]):
        piece = [None if f is None else eng.tensor(f[:, a:c]) for f in (fA, fB, fAB)]
        part = eng.sobol_tiles(*piece, sd)
        assert part.shape == (-(-(c - a) // 64), P, K, sums.shape[-1])
        eng.sobol_add(part, sums)
    return npy(sums)


def values(rng, P, M, K, offset):
    """fA, fB, fAB (P, M, K) and the shift: N(0, 1) values around a per-path level -- of order 1, or 1e8 -- and f_A at row 0."""
    level = offset * (1.0 + rng.uniform(size=(P, 1, K)))
    fA, fB, fAB = (level + rng.normal(size=(P, M, K)) for _ in range(3))
    return fA, fB, fAB, fA[:, 0, :].copy()


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('M', [1, 63, 64, 65, 300])
@pytest.mark.parametrize('P', [1, 3, 65])
def test_sums_within_the_bound(eng, P, M, K):
    """All six sums, for values of order 1 and for 1e8 + N(0, 1) (the shift leaves g of order 1: without it sum g^2 would sit at
    1e16 M and the variance would come out of a cancellation of 16 digits)."""
    ntiles = -(-M // 64)
    for offset in (1.0, 1e8):
        rng = np.random.default_rng(1000 * P + 10 * M + K)
        fA, fB, fAB, shift = values(rng, P, M, K, offset)
        base, pair = device_sums(eng, fA, fB, None, shift), device_sums(eng, fA, fB, fAB, shift)
        assert base.shape == (P, K, 4) and pair.shape == (P, K, 2)
        R.check(base, *R.exact_sums(fA, fB, None, shift), ntiles, 'base P=%d M=%d K=%d level %g' % (P, M, K, offset))
        R.check(pair, *R.exact_sums(fA, fB, fAB, shift), ntiles, 'pair P=%d M=%d K=%d level %g' % (P, M, K, offset))
        if offset == 1e8:   # what the shift is for: g is of order 1, so is every sum of squares per row
            assert np.all(base[..., 2:] < 40.0 * M)


def test_the_shift_is_one_subtraction(eng):
    """Sums of g = f - shift for a shift that is not a value of the path: the reference forms g the same way."""
    rng = np.random.default_rng(3)
    fA, fB, fAB, _ = values(rng, 3, 130, 2, 1e8)
    shift = 1e8 + rng.normal(size=(3, 2))
    R.check(device_sums(eng, fA, fB, None, shift), *R.exact_sums(fA, fB, None, shift), 3, 'base, free shift')
    R.check(device_sums(eng, fA, fB, fAB, shift), *R.exact_sums(fA, fB, fAB, shift), 3, 'pair, free shift')


@pytest.mark.parametrize('K', [1, 3])
def test_tile_aligned_splits_change_no_bit(eng, K):
    """M = 300 in one call and split at rows 64, 128 and 256 across calls: the running sum continues, tile by tile."""
    rng = np.random.default_rng(7)
    fA, fB, fAB, shift = values(rng, 5, 300, K, 1e8)
    for f3 in (None, fAB):
        whole = device_sums(eng, fA, fB, f3, shift)
        assert np.array_equal(device_sums(eng, fA, fB, f3, shift, cuts=(64, 128, 256)), whole)
        assert np.array_equal(device_sums(eng, fA, fB, f3, shift, cuts=(192,)), whole)
        assert np.array_equal(device_sums(eng, fA, fB, f3, shift), whole)       # and a second call the same bits


def test_nan_stays_in_its_path(eng):
    rng = np.random.default_rng(8)
    fA, fB, fAB, shift = values(rng, 4, 150, 2, 1.0)
    clean = [device_sums(eng, fA, fB, None, shift), device_sums(eng, fA, fB, fAB, shift)]
    fA2 = fA.copy()
    fA2[2, 70, 1] = np.nan
    for f3, ref in zip((None, fAB), clean):
        out = device_sums(eng, fA2, fB, f3, shift)
        hit = np.zeros(out.shape, dtype=bool)
        hit[2, 1, [0, 2] if f3 is None else [0, 1]] = True       # sum g_A and sum g_A^2; both pair sums
        assert np.all(np.isnan(out[hit])) and np.array_equal(out[~hit], ref[~hit])
    fAB2 = fAB.copy()
    fAB2[0, 149, 0] = np.nan                                       # in the short last tile
    out = device_sums(eng, fA, fB, fAB2, shift)
    assert np.all(np.isnan(out[0, 0])) and np.array_equal(out[1:], clean[1][1:]) and np.array_equal(out[0, 1], clean[1][0, 1])


def test_bad_arguments_raise(eng):
    from dgp_amd import _lib
    from dgp_amd.ops import DgpAmdError
    f, shift = eng.zeros(2, 10, 1), eng.zeros(2, 1)
    part = eng.sobol_tiles(f, f, None, shift)
    with pytest.raises(DgpAmdError, match='need P >= 1, M >= 1, K >= 1'):
        eng.sobol_tiles(eng.zeros(2, 0, 1), eng.zeros(2, 0, 1), None, shift)
    with pytest.raises(DgpAmdError, match='need P >= 1, M >= 1, K >= 1'):
        eng.sobol_tiles(eng.zeros(0, 10, 1), eng.zeros(0, 10, 1), None, eng.zeros(0, 1))
    with pytest.raises(DgpAmdError, match='null pointer'):
        eng._chk(_lib.lib.dgpamd_sobol_tiles(eng.h, 2, 10, 1, f.data_ptr(), None, None, shift.data_ptr(), part.data_ptr()))
    with pytest.raises(DgpAmdError, match='need ntiles >= 1, count >= 1'):
        eng._chk(_lib.lib.dgpamd_sobol_add(eng.h, 0, 8, part.data_ptr(), eng.zeros(8).data_ptr()))
    with pytest.raises(DgpAmdError, match='null pointer'):
        eng._chk(_lib.lib.dgpamd_sobol_add(eng.h, 1, 8, part.data_ptr(), None))
    # what the Python front refuses itself: shapes that would read or write out of bounds
    with pytest.raises(ValueError, match='one shape'):
        eng.sobol_tiles(f, eng.zeros(2, 9, 1), None, shift)
    with pytest.raises(ValueError, match='one shape'):
        eng.sobol_tiles(f, f, None, eng.zeros(2, 2))
    with pytest.raises(ValueError, match='shape of one tile'):
        eng.sobol_add(part, eng.zeros(2, 1, 2))
