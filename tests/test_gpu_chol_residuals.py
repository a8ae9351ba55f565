"""The dense factorisation (csrc/chol.hip, csrc/potrf_step.hpp, csrc/potrf_mega.hpp, csrc/diagfac.hpp: dgpamd_potrf, dgpamd_potrf_inv, dgpamd_potri_batched) held to
backward-error bounds and to LAPACK's info, in both modes (per-step graphs, one launch).  Needs an MI355X: -m gpu.

The forward comparisons of tests/test_gpu_ops.py (rtol 1e-7 .. 1e-9 against LAPACK's factor) cannot be tighter on kernel
matrices of cond 1e4 .. 1e9, so a factor that lost six digits passes them.  Residuals do not depend on the conditioning
(tests/chol_ref.py, checked on its own by tests/test_chol_ref_host.py): every measure of the device is held to
4 x max(LAPACK's value on the same input, 1 u), u = 2^-53; one lost digit, or one missing Newton round of rsqrt_f64 / rcp_f64
(about 90 u), fails."""
import numpy as np
import pytest

import chol_ref as R

pytestmark = pytest.mark.gpu

FAMILIES = ('well', 'matern', 'sexp')
FULL_NS = (1, 2, 17, 63, 64, 65, 128, 129, 320)      # full residual matrices
PROBE_NS = (449, 511, 1000, 2000)                    # +-1 probes, double-double


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


def families_of(n):
    """Three matrices per call, one per family; at n = 2000 one: matern with nugget 1e-4."""
    return [('matern', 1e-4)] if n == 2000 else [(f, None) for f in FAMILIES]


def nan_buffers(eng, B, Np, count):
    import torch
    # (the engine's stream is the thread's current torch stream: the fills are ordered ahead of the library's launches)
    return [torch.full((B, Np, Np), float('nan'), dtype=torch.float64, device=eng.device) for _ in range(count)]


_device = {}


def run_device(eng, mode, n):
    """potrf, potri from its factor, potrf_inv on fresh copies, in `mode`; T, S and potri's output pre-filled with NaN.  The
    outputs as numpy arrays (kept for the sizes the two modes are compared at)."""
    if (mode, n) in _device:
        return _device[mode, n]
    fams = families_of(n)
    B, Np = len(fams), eng.padded_dim(n)
    Ms = np.stack([R.buffer(*R.family(f, n, nugget=g), Np) for f, g in fams])
    try:
        eng.set_potrf_mode(mode)
        A1, A2 = eng.tensor(Ms), eng.tensor(Ms)
        Ainv, T, S = nan_buffers(eng, B, Np, 3)
        work = eng.potrf_workspace(n, B)
        ld1, info1 = eng.potrf(n, A1, batch=B, work=work)
        factored = A1.clone()   # (potri works in its input)
        eng.potri(n, A1, Ainv, 1, work, batch=B)
        ld2, info2 = eng.potrf_inv(n, A2, T, S, batch=B, work=work)
        eng.sync()
        out = dict(A1=npy(factored), A2=npy(A2), Ainv=npy(Ainv), T=npy(T), S=npy(S), ld1=npy(ld1), ld2=npy(ld2),
                   info1=npy(info1), info2=npy(info2))
    finally:
        eng.set_potrf_mode(1)
    if n <= R.FULL_MAX:
        _device[mode, n] = out
    return out


def defined_parts(out, n):
    """Every output where the entry points define it (n+1 rows of the factor buffers and of the inverses, T on tr <= tc, S on
    tr >= tc), the rest zeroed: what the two modes, or two calls, must agree on bit for bit."""
    tr, tc = R.tiles(n)
    parts = {}
    for k in ('A1', 'A2'):
        if k in out:
            parts[k] = np.tril(out[k][:, :n + 1, :n + 1])
    if 'Ainv' in out:
        parts['Ainv'] = out['Ainv'][:, :n + 1, :n]
    if 'T' in out:
        parts['T'] = np.where(tr <= tc, out['T'][:, :n, :n], 0.0)
        parts['S'] = np.where(tr >= tc, out['S'][:, :n, :n], 0.0)
        parts['S_row'] = out['S'][:, n, :n]
    for k in ('ld1', 'ld2'):
        if k in out:
            parts[k] = out[k]
    return parts


def assert_same_bits(a, b, which=None, what=''):
    for k in a:
        x, y = (a[k], b[k]) if which is None else (a[k][which], b[k][which])
        assert np.isfinite(x).all(), (what, k)
        assert x.tobytes() == y.tobytes(), (what, k, float(np.abs(x - y).max()))


@pytest.mark.parametrize('n', FULL_NS + PROBE_NS)
@pytest.mark.parametrize('mode', [0, 1])
def test_backward_errors_against_lapack(eng, mode, n):
    """Every measure of tests/chol_ref.py, for potrf, potri from its factor and potrf_inv, three families per call (well: cond 9;
    matern, sexp: cond up to 3e10), at the 16- and 64-pivot edges in full and at 449 .. 2000 through probes: device <= 4 x
    max(LAPACK, 1 u); the corner within its a-priori (n + 2) u; info == 0; potri's inverse equal to its transpose bit for bit.
    eps_L of matern and sexp: the larger of that and 4 x LAPACK x max_k kappa_2(L_kk) (chol_ref.bound_eps_L: the panels are
    multiplied by the explicit inverse of the diagonal block's factor; the block columns of the residual are printed for
    64 < n <= 320 and show the excess in the first panel alone, DESIGN.md, accuracy of the factorisation).
    The figures of every case are printed (device / LAPACK, units of u).

    Observed on an MI355X, both modes alike, device (LAPACK), over all n:
        eps_L      well 0.54 .. 3.54 (0.54 .. 1.55), at most 0.75 of its bound (n = 128); matern 0.23 .. 4.08 (0.23 .. 6.97),
                   sexp 1.25 .. 21.5 (0.71 .. 6.32): the plain 4 x is exceeded by sexp at n = 128 only (21.5 against 4 x 2.24,
                   kappa_2(L_00) = 4.4e3)
        eps_w      0.001 .. 1.21 (0.001 .. 0.35)          corner     0 .. 9.6, at most 0.85 of (n + 2)
        eps_T      0.001 .. 1.80 (0.005 .. 0.41)          eps_S      0.10 .. 1.83 (0.10 .. 1.19)
        eps_alpha  0.12 .. 2.90 (0.10 .. 0.62), worst 0.72 of its bound (sexp, n = 449)
        eps_logdet 0.004 .. 0.66 (0.02 .. 0.67)
    This test found the trailing updates accumulating every product onto the tile's own value: eps_L of `well` was 5.32, 5.93,
    7.86 u at n = 449, 511, 1000 against LAPACK's 1.32, 1.39, 1.55 u (4.03 x, 4.27 x, 5.07 x) in both modes.  The updates now sum
    each half tile of products from zero (tile.hpp, FROM_ZERO): 3.35, 3.26, 3.54 u."""
    out = run_device(eng, mode, n)
    assert not out['info1'].any() and not out['info2'].any()
    lines, over = [], []

    def hold(fam, what, got, lapack, limit=None):
        limit = R.bound(lapack) if limit is None else limit
        lines.append('%-7s %-22s device %8.3f  LAPACK %8.3f  bound %8.3f' % (fam, what, got, lapack, limit))
        if not got <= limit:   # (a NaN is over the bound)
            over.append(lines[-1])

    for b, (fam, nug) in enumerate(families_of(n)):
        K, y = R.family(fam, n, nugget=nug)
        ref = R.lapack_values(n, fam, nug)
        factors = {}
        for entry, A, ld in (('potrf', out['A1'][b], out['ld1'][b]), ('potrf_inv', out['A2'][b], out['ld2'][b])):
            L, w = np.tril(A[:n, :n]), A[n, :n].copy()
            factors[entry] = L
            hold(fam, entry + ' eps_L', R.eps_L(K, L), ref['eps_L'], R.bound_eps_L(fam, ref['eps_L'], ref['L']))
            if entry == 'potrf' and 64 < n <= R.FULL_MAX:   # (printed, not asserted: where the residual sits, block column by block column)
                lines.append('%-7s panel residuals: device %s  LAPACK %s  max kappa_2(L_kk) %.3g' % (
                    fam, ' '.join('%.2f' % v for v in R.panel_residuals(K, L)),
                    ' '.join('%.2f' % v for v in R.panel_residuals(K, ref['L'])), R.kappa_diag_blocks(ref['L'])))
            hold(fam, entry + ' eps_w', R.eps_w(L, w, y), ref['eps_w'])
            c, limit = R.corner(A[n, n], w)
            hold(fam, entry + ' corner', c, float('nan'), limit)
            if fam == 'well':
                hold(fam, entry + ' eps_logdet', R.eps_logdet(ld, ref['logdet_ref'], n), ref['eps_logdet'])
        Si = out['Ainv'][b][:n, :n]
        assert Si.tobytes() == np.ascontiguousarray(Si.T).tobytes(), 'potri: not symmetric bit for bit'
        hold(fam, 'potri eps_S', R.eps_S(K, Si), ref['eps_S'])
        hold(fam, 'potri eps_alpha', R.eps_alpha(K, -out['Ainv'][b][n, :n], y), ref['eps_alpha'])
        L = factors['potrf_inv']
        right, left = R.eps_T(L, R.mask_T(out['T'][b], n))
        lr, ll = R.lapack_eps_T(L)
        hold(fam, 'potrf_inv eps_T right', right, lr)
        hold(fam, 'potrf_inv eps_T left', left, ll)
        hold(fam, 'potrf_inv eps_S', R.eps_S(K, R.complete_S(out['S'][b], n)), ref['eps_S'])
        hold(fam, 'potrf_inv eps_alpha', R.eps_alpha(K, -out['S'][b][n, :n], y), ref['eps_alpha'])
    print('\nmode %d, n = %d (units of u = 2^-53)\n' % (mode, n) + '\n'.join(lines))
    assert not over, '\n' + '\n'.join(over)


@pytest.mark.parametrize('n', FULL_NS)
def test_the_two_modes_agree_bit_for_bit(eng, n):
    """Per-step graphs and the one launch run the same arithmetic in the same order: L, w, the log-determinants, potri's
    inverse, T and S are equal bit for bit at every edge size (tests/test_gpu_ops.py ties them at n = 300 only)."""
    a, b = run_device(eng, 0, n), run_device(eng, 1, n)
    assert_same_bits(defined_parts(a, n), defined_parts(b, n), what='n = %d' % n)


# ------------------------------------------------------------------------------------------------ failure reports
# n = 130: blocks of 64, 64 and 2 pivots (the last block runs the partial-block elimination); n = 128: the last block carries
# the right-hand side only; n = 1.
POSITIONS = {130: (1, 2, 16, 17, 63, 64, 65, 80, 128, 129, 130), 128: (64, 65, 128), 1: (1,)}
KINDS = ('neg', 'zero', 'nan_diag', 'nan_row')


def healthy(n, tag):
    return R.family('well', n, seed=31000 + tag)


def fresh_workspace(eng, n, B):
    import torch
    from dgp_amd import ops
    return torch.empty(int(ops.lib.dgpamd_potrf_workspace(n, B)), dtype=torch.uint8, device=eng.device)


def call(eng, entry, n, mats, work=None):
    """One batched call of `entry` on the (K, y) pairs `mats`; outputs as numpy arrays."""
    B, Np = len(mats), eng.padded_dim(n)
    A = eng.tensor(np.stack([R.buffer(K, y, Np) for K, y in mats]))
    work = eng.potrf_workspace(n, B) if work is None else work
    if entry == 'potrf':
        ld, info = eng.potrf(n, A, batch=B, work=work)
        eng.sync()
        return dict(A1=npy(A), ld1=npy(ld), info=npy(info))
    T, S = nan_buffers(eng, B, Np, 2)
    ld, info = eng.potrf_inv(n, A, T, S, batch=B, work=work)
    eng.sync()
    return dict(A2=npy(A), T=npy(T), S=npy(S), ld2=npy(ld), info=npy(info))


def in_mode(eng, mode, body):
    try:
        eng.set_potrf_mode(mode)
        return body()
    finally:
        eng.set_potrf_mode(1)


@pytest.mark.parametrize('n', sorted(POSITIONS))
@pytest.mark.parametrize('entry', ['potrf', 'potrf_inv'])
@pytest.mark.parametrize('mode', [0, 1])
def test_info_is_the_first_pivot_that_is_not_positive(eng, mode, entry, n):
    """LAPACK's info (1-based order of the first leading minor that is not positive; tests/test_chol_ref_host.py holds
    scipy's dpotrf to the same positions) from the per-step path (diag_logdet) and the one-launch chain (k * 64 + bad), at
    the 16- and 64-pivot edges and in the last, partial block, for a negative, a zero and a NaN pivot (`!(d > 0)`) and a NaN that
    reaches the pivot through the elimination.  Per kind one batched call, failing matrices at the even indices, healthy ones
    at the odd: their info is 0 and their L, w, logdet, T, S equal, bit for bit, those of the same call with every failing
    matrix replaced by a healthy one.  'neg' also alone at every position.  Nothing is asserted about the outputs of a failed
    matrix."""
    def body():
        for kind in KINDS:
            ps = [p for p in POSITIONS[n] if not (kind == 'nan_row' and p < 2)]
            if not ps:
                continue
            bad, good = [], []
            for i, p in enumerate(ps):
                K, y = healthy(n, 2 * i)
                bad += [(R.failing(K, p, kind), y), healthy(n, 2 * i + 1)]
                good += [(K, y), healthy(n, 2 * i + 1)]
            got, want = call(eng, entry, n, bad), call(eng, entry, n, good)
            assert got['info'][0::2].tolist() == ps, (kind, got['info'].tolist())
            assert not got['info'][1::2].any() and not want['info'].any(), (kind, got['info'].tolist(), want['info'].tolist())
            assert_same_bits(defined_parts(got, n), defined_parts(want, n), which=slice(1, None, 2), what=kind)
            if kind == 'neg':
                for (A, y), p in zip(bad[0::2], ps):
                    assert call(eng, entry, n, [(A, y)])['info'].tolist() == [p], (kind, p)
    in_mode(eng, mode, body)


@pytest.mark.parametrize('entry', ['potrf', 'potrf_inv'])
@pytest.mark.parametrize('mode', [0, 1])
def test_the_first_of_two_failures_is_reported(eng, mode, entry):
    """Two pivots fail in one matrix -- in two 64-blocks (20, 70) and in two 16-blocks of one 64-block (70, 100): the first is
    reported, in a batch among healthy matrices and alone."""
    n = 130

    def body():
        mats, first = [], []
        for i, (p, q) in enumerate(((20, 70), (70, 100))):
            K, y = healthy(n, 50 + i)
            mats += [(R.failing(R.failing(K, q, 'neg'), p, 'neg'), y), healthy(n, 60 + i)]
            first += [p, 0]
        assert call(eng, entry, n, mats)['info'].tolist() == first
        for m, p in zip(mats[0::2], first[0::2]):
            assert call(eng, entry, n, [m])['info'].tolist() == [p]
    in_mode(eng, mode, body)


@pytest.mark.parametrize('entry', ['potrf', 'potrf_inv'])
@pytest.mark.parametrize('mode', [0, 1])
def test_a_healthy_call_after_a_failed_one_on_the_same_workspace(eng, mode, entry):
    """The info word lives in the workspace between the launches: a failing call followed by a healthy call of the same shape on
    the same workspace reports 0, and every output equals, bit for bit, that of the healthy call alone on a fresh workspace."""
    n, B = 130, 2

    def body():
        good = [healthy(n, 70), healthy(n, 71)]
        bad = [(R.failing(good[0][0], 65, 'neg'), good[0][1]), (R.failing(good[1][0], 2, 'nan_row'), good[1][1])]
        alone = call(eng, entry, n, good, fresh_workspace(eng, n, B))
        work = fresh_workspace(eng, n, B)
        assert call(eng, entry, n, bad, work)['info'].tolist() == [65, 2]
        after = call(eng, entry, n, good, work)
        assert after['info'].tolist() == [0, 0] and alone['info'].tolist() == [0, 0]
        assert_same_bits(defined_parts(after, n), defined_parts(alone, n))
    in_mode(eng, mode, body)
