"""The gradient second-moment sums on the device (dgpamd_gradmom_tiles, added by dgpamd_sobol_add; DESIGN I.18) against the
longdouble sums of tests/gradmom_ref.py within its bound (n + 3) 2^-53 sum |term|, and the bits that must not depend on how
the rows are split over calls or on the paths that share a launch.  Every comparison prints the largest error / bound it met
before it asserts.  Needs an MI355X: -m gpu.

The kernel has one form, its block count ceil(Dx / 16) changes at 16 | 17, 32 | 33 and 48 | 49: those widths and their
neighbours are in WIDTHS beside the ones every caller meets."""
import numpy as np
import pytest

import gradmom_ref as R

pytestmark = pytest.mark.gpu

WIDTHS = [1, 2, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64]
ROWS = [1, 63, 64, 65, 200]


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def inputs(rng, P, M, K, Dx, level=1e8):
    """f (P, M, K): N(0, 1) around a per-path level of order 1e8, so that the shift matters; J (P, M, K, Dx): mixed signs,
    magnitudes 10^U(-3, 3), column Dx // 2 all zero where there are two columns or more; shift = f at row 0."""
    f = level * (1.0 + rng.uniform(size=(P, 1, K))) + rng.normal(size=(P, M, K))
    J = rng.choice([-1.0, 1.0], size=(P, M, K, Dx)) * 10.0**rng.uniform(-3.0, 3.0, size=(P, M, K, Dx))
    if Dx >= 2:
        J[..., Dx // 2] = 0.0
    return f, J, f[:, 0, :].copy()


def device_sums(eng, f, J, shift, cuts=()):
    """The running sums over the rows of host arrays, one gradmom_tiles + sobol_add per piece of rows between cuts."""
    P, M, K = f.shape
    Dx = J.shape[3]
    sums = eng.zeros(P, K, R.n_sums(Dx))
    sd = eng.tensor(shift)
    edges = [0, *cuts, M]
    for a, c in zip(edges, edges[1:]):
        part = eng.gradmom_tiles(eng.tensor(f[:, a:c]), eng.tensor(J[:, a:c]), sd)
        assert part.shape == (-(-(c - a) // 64), P, K, R.n_sums(Dx))
        eng.sobol_add(part, sums)
    return npy(sums)


def zero_entries(Dx):
    """The entries of a (NC,) vector of sums that involve column z = Dx // 2: its sum and the products (d, z), (z, e)."""
    z, iu = Dx // 2, np.triu_indices(Dx)
    hit = np.zeros(R.n_sums(Dx), dtype=bool)
    hit[2 + z] = True
    hit[2 + Dx:] = (iu[0] == z) | (iu[1] == z)
    return hit


def check_zero_column(out, Dx):
    if Dx >= 2:
        z = out[..., zero_entries(Dx)]
        assert z.size and np.all(z == 0.0) and not np.any(np.signbit(z))
        assert np.all(out[..., ~zero_entries(Dx)][..., 2:] != 0.0)      # (sum g and sum g^2 are 0 at one row: g = f - f)


@pytest.mark.parametrize('M', ROWS)
@pytest.mark.parametrize('Dx', WIDTHS)
def test_sums_within_the_bound(eng, Dx, M):
    """Every width at every row count, three paths and three outputs."""
    P, K = 3, 3
    f, J, shift = inputs(np.random.default_rng(1000 * Dx + M), P, M, K, Dx)
    out = device_sums(eng, f, J, shift)
    assert out.shape == (P, K, R.n_sums(Dx))
    R.check(out, f, J, shift, 'P=%d M=%d K=%d Dx=%d' % (P, M, K, Dx))
    check_zero_column(out, Dx)
    assert np.all(out[..., 1] < 40.0 * M)      # what the shift is for: g is of order 1, so is its square


@pytest.mark.parametrize('M,Dx', [(1, 5), (65, 17), (200, 5), (65, 64)])
@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('P', [1, 70])
def test_paths_and_outputs(eng, P, K, M, Dx):
    """One path and more paths than a launch has waves to a workgroup, one output and three: the decoding of (tile, path,
    output) from the workgroup's index."""
    f, J, shift = inputs(np.random.default_rng(7 * P + 3 * K + M + Dx), P, M, K, Dx)
    out = device_sums(eng, f, J, shift)
    R.check(out, f, J, shift, 'P=%d M=%d K=%d Dx=%d' % (P, M, K, Dx))
    check_zero_column(out, Dx)


def test_the_shift_is_one_subtraction(eng):
    """Sums of g = f - shift for a shift that is not a value of the path: the reference forms g the same way."""
    rng = np.random.default_rng(3)
    f, J, _ = inputs(rng, 3, 130, 2, 5)
    shift = 1e8 + rng.normal(size=(3, 2))
    R.check(device_sums(eng, f, J, shift), f, J, shift, 'free shift')


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('Dx', [5, 16, 17, 33, 49, 64])
def test_tile_aligned_splits_change_no_bit(eng, Dx, K):
    """Rows [0:64], [64:192] and [192:M] computed separately and added in order, against one call over all rows; and a second
    call the same bits."""
    import torch
    for M in (200, 300):
        f, J, shift = inputs(np.random.default_rng(Dx + K + M), 5, M, K, Dx)
        whole = device_sums(eng, f, J, shift)
        assert np.array_equal(device_sums(eng, f, J, shift, cuts=(64, 192)), whole)
        assert np.array_equal(device_sums(eng, f, J, shift), whole)
    fd, Jd, sd = eng.tensor(f), eng.tensor(J), eng.tensor(shift)
    assert torch.equal(eng.gradmom_tiles(fd, Jd, sd), eng.gradmom_tiles(fd, Jd, sd))


@pytest.mark.parametrize('Dx', [5, 17, 64])
def test_a_path_does_not_depend_on_its_neighbours(eng, Dx):
    """P = 1 against the matching slice of P = 3, and of P = 70: another grid, other neighbours, the same bits."""
    f, J, shift = inputs(np.random.default_rng(40 + Dx), 70, 200, 3, Dx)
    whole = device_sums(eng, f, J, shift)
    three = device_sums(eng, f[4:7], J[4:7], shift[4:7])
    assert np.array_equal(three, whole[4:7])
    for p in (4, 5, 6):
        assert np.array_equal(device_sums(eng, f[p:p + 1], J[p:p + 1], shift[p:p + 1]), three[p - 4:p - 3])
    # one output alone: another row stride of J, the same rows
    assert np.array_equal(device_sums(eng, f[:3, :, 1:2].copy(), J[:3, :, 1:2].copy(), shift[:3, 1:2].copy()), whole[:3, 1:2])


def test_nan_stays_in_its_path_and_output(eng):
    f, J, shift = inputs(np.random.default_rng(8), 4, 150, 2, 17)
    clean = device_sums(eng, f, J, shift)
    J2 = J.copy()
    J2[2, 140, 1, 3] = np.nan                       # in the short last tile
    out = device_sums(eng, f, J2, shift)
    hit = np.zeros(out.shape, dtype=bool)
    hit[2, 1, 2:] = True
    assert np.array_equal(out[~hit], clean[~hit]) and np.isnan(out[2, 1, 2 + 3])
    assert np.all(np.isnan(out[2, 1, 2:]) | (out[2, 1, 2:] == clean[2, 1, 2:]))


def test_bad_arguments_raise(eng):
    from dgp_amd import _lib
    from dgp_amd.ops import DgpAmdError
    f, J, shift = eng.zeros(2, 10, 1), eng.zeros(2, 10, 1, 3), eng.zeros(2, 1)
    part = eng.gradmom_tiles(f, J, shift)
    assert part.shape == (1, 2, 1, 11) and not np.any(npy(part))
    ptr = [t.data_ptr() for t in (f, J, shift, part)]
    for Dx in (0, 65, -1):
        with pytest.raises(DgpAmdError, match='need 1 <= Dx <= 64'):
            eng._chk(_lib.lib.dgpamd_gradmom_tiles(eng.h, 2, 10, 1, Dx, *ptr))
    for P, M, K in ((0, 10, 1), (2, 0, 1), (2, 10, 0)):
        with pytest.raises(DgpAmdError, match='need P >= 1, M >= 1, K >= 1'):
            eng._chk(_lib.lib.dgpamd_gradmom_tiles(eng.h, P, M, K, 3, *ptr))
    for i in range(4):
        with pytest.raises(DgpAmdError, match='null pointer'):
            eng._chk(_lib.lib.dgpamd_gradmom_tiles(eng.h, 2, 10, 1, 3, *[None if j == i else q for j, q in enumerate(ptr)]))
    with pytest.raises(DgpAmdError, match='beyond 2\\^31'):
        eng._chk(_lib.lib.dgpamd_gradmom_tiles(eng.h, 2**20, 2**20, 1, 3, *ptr))
    with pytest.raises(DgpAmdError, match='beyond 2\\^31'):
        eng._chk(_lib.lib.dgpamd_gradmom_tiles(eng.h, 2**40, 10, 1, 3, *ptr))
    # what the Python front refuses itself: shapes that would read or write out of bounds
    with pytest.raises(ValueError, match='1 to 64 columns'):
        eng.gradmom_tiles(f, eng.zeros(2, 10, 1, 0), shift)
    with pytest.raises(ValueError, match='1 to 64 columns'):
        eng.gradmom_tiles(f, eng.zeros(2, 10, 1, 65), shift)
    with pytest.raises(ValueError, match='contiguous float64'):
        eng.gradmom_tiles(f, eng.zeros(2, 10, 1, 6)[..., ::2], shift)
    with pytest.raises(ValueError, match='contiguous float64'):
        eng.gradmom_tiles(f, eng.zeros(2, 9, 1, 3), shift)
    with pytest.raises(ValueError, match='contiguous float64'):
        eng.gradmom_tiles(f, J, eng.zeros(2, 2))
    with pytest.raises(ValueError, match='contiguous float64'):
        eng.gradmom_tiles(f, J.float(), shift)
    with pytest.raises(ValueError, match=r'\(P, M, K, Dx\)'):
        eng.gradmom_tiles(f, J[0], shift)
