"""Linked-GP predictions with the inputs moved away from the origin.  Needs an MI355X: -m gpu.

Adding one constant per column to the training inputs W and the test means m (and to Wg and z) leaves a linked-GP
prediction unchanged.  tests/linkshift_ref.py generates problems on dyadic grids for which such a shift is exact in float64
(offsets 0, 2^6, 2^10, 2^14, 2^20, -2^10 and one per-column vector), computes the exact prediction once, at offset 0, in
long double, and states the bound that the SExp forms and gp_predict are held to at every shift (the list of what each form
is held to is below),

    |var - var_exact|   <= eps (c_a A_t + c_s (mean_t^2 + scale (1 + nugget))),      A_t = sum_ij |C_ij| J_ij (1 + E_ij)
    |mean - mean_exact| <= eps c_m B_t,                                               B_t = sum_i |ry_i| I_i (1 + e_i)

with c_a, c_s, c_m counted from the kernels' source there; nothing about the shift enters it.  tests/test_linkshift_host.py
shows that the bound can fail: a float64 restatement of the expanded pair exponent breaks it from offset 2^6 on, on each of
these shapes.  As a second, coarser condition every output meets the suite's linked-GP tolerances (mean rtol 1e-8 atol 1e-10,
variance rtol 1e-6 atol 1e-8) at every shift.  Every test prints its worst error / bound per shift before it asserts.

The same float64 (R^-1, R^-1 y), fitted at offset 0, are handed to the device at every shift.

Where a form takes differences before anything else an exact shift changes none of its operands, and its outputs are held
bit-equal to its own offset-0 run as well.  That is every form (read from the code, form by form):
  SExp direct           linkgp_J_kernel: wi = w_i - 2 m, sgm = wi + w_j; base from w_i - w_j; globals (wg - z) / l
  the means             linkgp_mean_kernel: d = w_i - m; matern_I_dim: (x - m) / l
  Matern separable      matern_role_S / _T: x = (X - m) / l; the order classes compare raw coordinates, which a common
                        shift keeps in order; globals (wg - z) * (1 / l)
  Matern direct         matern_Jd / matern_Jd0: (min(X1, X2) - m) / l, (max(X1, X2) - m) / l
  leave-one-out         the direct kernels with weights from Rinv, ry alone
  Vecchia, LDS form     vecchia_linkgp_kernel: raw neighbours in LDS, (x_r - x_c) / l for K, x - m for I and J
  Vecchia, registers    SExp: u = (w - m) / l and ug = (wg - z) / l, everything from u; Matern: the same u for K, the
                        records from (x - m) / l
  SExp first, second    linkgp_Jsexp_kernel, sexp_records_kernel + linkgp_Jsexp2_kernel: w - W[0] and m - W[0] where they are
                        staged (column by column, so a per-column shift drops out as well), the expanded terms from those
  gp_predict            cross_corr_kernel: (w - W[0]) / l and (x - W[0]) / l
(the subtractions are exact on the generator's grids; on arbitrary data they round once, relative to the data's diameter).

What each form is held to, at every shape and every shift:
  the sharp bound, the suite's tolerances against the long-double values, the offset-0 bits
      SExp second form, first form, direct form, leave-one-out (the bound on the long-double downdate of the given
      statistics), gp_predict SExp (its own counts, linkshift_ref.gp_bounds), functions.link_gp; Matern separable, direct
      and leave-one-out at Dw <= 3 (their own bound, below)
  the offset-0 bits and the suite's tolerances only -- NOT the sharp bound
      Matern separable, direct, leave-one-out at Dw = 14, 15, and gp_predict Matern: the exact integrals of
      tests/linkfun_ref.py are mpmath at 120 digits, 34 Dw n (n + 1) / 2 of them per shape (7e4 at (65, 1, 0), 4e6 at
      (130, 15, 0)); they are recorded for (Dw, Dz) = (1, 0) and (3, 2) at both n (tests/golden/linkshift_matern.npz), where
      the three dense Matern forms get a bound of their own (linkshift_ref.matern_bounds: 32 E_b per factor, what
      tests/test_gpu_linkfn.py allows the device's factors, plus the counts of the sums).  At the wide shapes the reference
      is the float64 oracle on the integral at offset 0 (leave-one-out: its refit at the first four test points), and the
      shift is checked by the bits: an output that equals its offset-0 run bit for bit meets at every offset whatever it
      meets at offset 0.
      Vecchia, LDS and register forms, both kernels: the kernel factorises the conditioning block itself (cond <= 1e4), so
      its error carries cond(K) eps ~ 1e-12 and no count of the pair path bounds it; the references are the long-double
      prediction with K inverted in long double (SExp) and the oracle on the integral (Matern), at the suite's tolerances.
      The register form holds at most 50 neighbours, so it runs with the 50 nearest, not with pm = n.
"""
import numpy as np
import pytest

import linkshift_ref as R
from test_gpu_ops import engine_under, integral_oracle
from test_linkshift_host import loo_drop, seed_of

pytestmark = pytest.mark.gpu

CASES = [(n, Dw, Dz) for n in R.SIZES for (Dw, Dz) in R.SHAPES]


@pytest.fixture(scope='module')
def eng():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    from dgp_amd.ops import Engine
    return Engine(0)


def npy(t):
    return t.detach().cpu().numpy()


_cache = {}


def cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def matern_case(n, Dw, Dz):
    """(problem, exact dense, exact leave-one-out); the exact values are None where none are recorded (R.MATERN_EXACT_CASES)."""
    return cached(('mc', n, Dw, Dz), lambda: R.matern_problem(n, Dw, Dz))


def problem_of(name, n, Dw, Dz):
    if name != 'sexp':
        return matern_case(n, Dw, Dz)[0]
    return cached(('p', name, n, Dw, Dz), lambda: R.problem(name, n, Dw, Dz, seed_of(n, Dw, Dz)))


def sexp_exact(n, Dw, Dz, loo=False):
    p = problem_of('sexp', n, Dw, Dz)
    return p, cached(('x', n, Dw, Dz, loo), lambda: R.exact_sexp(p, drop=loo_drop(n) if loo else None))


def matern_reference(n, Dw, Dz):
    """(problem, (mean, var)) of the oracle on the integral at offset 0."""
    from oracle import dgp_oracle as O
    p = problem_of('matern2.5', n, Dw, Dz)

    def make():
        with integral_oracle():
            return O.link_gp_predict(p['m0'], p['v'], p['z0'] if Dz else None, p['W0'], p['Wg0'] if Dz else None, p['Rinv'], p['ry'],
                                     p['scale'], p['length'], p['nugget'], 'matern2.5')
    return p, cached(('m', n, Dw, Dz), make)


def linkgp(e, p, off, drop=None):
    import torch
    W, m, Wg, z = R.shifted(p, off)
    Dz = p['Dz']
    mo, vo = e.linkgp_predict(p['name'], e.tensor(m), e.tensor(p['v']), e.tensor(z) if Dz else None, e.tensor(W), e.tensor(Wg) if Dz else None,
                              p['length'], e.tensor(p['Rinv']), p['n'], e.tensor(p['ry']), p['scale'], p['nugget'],
                              drop=None if drop is None else e.tensor(drop, dtype=torch.int32))
    return npy(mo), npy(vo)


def coarse(mean, var, mean_ref, var_ref):
    """The suite's linked-GP tolerances, as booleans."""
    mr, vr = np.asarray(mean_ref, float), np.asarray(var_ref, float)
    return (bool(np.all(np.abs(mean - mr) <= 1e-10 + 1e-8 * np.abs(mr))), bool(np.all(np.abs(var - vr) <= 1e-8 + 1e-6 * np.abs(vr))))


def sweep(label, p, run, exact=None, bounds=None, reference=None, bit_equal=False):
    """run(off) -> (mean, var) at every shift of R.shifts.  exact + bounds: the sharp bound, and the coarse tolerances against
    exact; reference (mean, var): the coarse tolerances against it; bit_equal: every shift returns the offset-0 bits.  Prints
    a line per shift, then asserts."""
    failures, first = [], None
    ref = (exact['mean'], exact['var']) if exact is not None else reference
    for name, off in R.shifts(p['Dw'] + p['Dz']).items():
        mean, var = run(off)
        line = '%s n %d Dw %d Dz %d shift %-9s' % (label, p['n'], p['Dw'], p['Dz'], name)
        if exact is not None:
            rm, rv = R.worst_ratio(mean, exact['mean'], bounds[0]), R.worst_ratio(var, exact['var'], bounds[1])
            line += ' mean err/bound %.3g var err/bound %.3g' % (rm, rv)
            if not (rm <= 1.0 and rv <= 1.0):
                failures.append((name, 'bound', rm, rv))
        okm, okv = coarse(mean, var, *ref)
        line += ' max |dmean| %.3g max |dvar| %.3g' % (float(np.max(np.abs(mean - np.asarray(ref[0], float)))),
                                                     float(np.max(np.abs(var - np.asarray(ref[1], float)))))
        if not (okm and okv):
            failures.append((name, 'tolerance', okm, okv))
        if first is None:
            first = (mean, var)
        same = np.array_equal(mean, first[0]) and np.array_equal(var, first[1])
        line += ' bits %s' % ('same' if same else 'differ')
        if bit_equal and not same:
            failures.append((name, 'bits', int(np.sum(mean != first[0])), int(np.sum(var != first[1]))))
        print(line)
    assert not failures, failures


def sexp_bounds(ex, p):
    return R.mean_bound(ex, p), R.var_bound(ex, p)


# ------------------------------------------------------------------------------------------------ SExp, dense
@pytest.mark.parametrize('n,Dw,Dz', [c for c in CASES if c[1] <= 14])
def test_sexp_second_form(eng, n, Dw, Dz):
    """sexp_records_kernel + linkgp_Jsexp2_kernel, the default to Dw = 14 (k-steps 1, 2 and 4 at Dw = 1, 3, 14)."""
    p, ex = sexp_exact(n, Dw, Dz)
    sweep('sexp2', p, lambda off: linkgp(eng, p, off), exact=ex, bounds=sexp_bounds(ex, p), bit_equal=True)


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_sexp_first_form(eng, n, Dw, Dz):
    """linkgp_Jsexp_kernel: the default at Dw = 15, under DGPAMD_SEXP_FORM1 below."""
    p, ex = sexp_exact(n, Dw, Dz)
    if Dw >= 15:
        sweep('sexp1', p, lambda off: linkgp(eng, p, off), exact=ex, bounds=sexp_bounds(ex, p), bit_equal=True)
    else:
        with engine_under(SEXP_FORM1=1) as e1:
            sweep('sexp1', p, lambda off: linkgp(e1, p, off), exact=ex, bounds=sexp_bounds(ex, p), bit_equal=True)


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_sexp_direct_form(eng, n, Dw, Dz):
    """linkgp_J_kernel<SEXP, false> (set_linkgp_direct)."""
    p, ex = sexp_exact(n, Dw, Dz)
    eng.set_linkgp_direct(True)
    try:
        sweep('sexp-direct', p, lambda off: linkgp(eng, p, off), exact=ex, bounds=sexp_bounds(ex, p), bit_equal=True)
    finally:
        eng.set_linkgp_direct(False)


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_sexp_leave_one_out(eng, n, Dw, Dz):
    """dgpamd_linkgp_loo, SExp: drop = 0, 63, 64, n - 1 and on.  Exact values: the long-double downdate of the float64
    statistics the device is given (test_linkshift_host.py holds it to the refit at the suite's tolerances)."""
    p, ex = sexp_exact(n, Dw, Dz, loo=True)
    drop = loo_drop(n)
    sweep('sexp-loo', p, lambda off: linkgp(eng, p, off, drop=drop), exact=ex, bounds=sexp_bounds(ex, p), bit_equal=True)


# ------------------------------------------------------------------------------------------------ Matern, dense
@pytest.mark.parametrize('direct', [False, True])
@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_matern_forms(eng, n, Dw, Dz, direct):
    """The separable form (records + linkgp_Jsep_kernel) and the direct kernel: bit-equal across the shifts; where exact values
    are recorded (Dw <= 3) the bound of linkshift_ref.matern_bounds and the suite's tolerances against them, elsewhere the
    suite's tolerances against the oracle on the integral."""
    p, dense, _ = matern_case(n, Dw, Dz)
    label = 'matern-direct' if direct else 'matern-sep'
    eng.set_linkgp_direct(direct)
    try:
        if dense is not None:
            sweep(label, p, lambda off: linkgp(eng, p, off), exact=dense, bounds=R.matern_bounds(dense, p), bit_equal=True)
        else:
            sweep(label, p, lambda off: linkgp(eng, p, off), reference=matern_reference(n, Dw, Dz)[1], bit_equal=True)
    finally:
        eng.set_linkgp_direct(False)


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_matern_leave_one_out(eng, n, Dw, Dz):
    """dgpamd_linkgp_loo, Matern: bit-equal across the shifts; where exact values are recorded (the long-double downdate of the
    given statistics, Dw <= 3) the bound of linkshift_ref.matern_bounds; everywhere the first four test points (drop = 0, 63,
    64, n - 1) against the oracle on the integral with the statistics refitted on the other n - 1 points."""
    from oracle import dgp_oracle as O
    p, _, loo = matern_case(n, Dw, Dz)
    drop = loo_drop(n)
    X0 = np.concatenate((p['W0'], p['Wg0']), 1)
    mean0, var0 = linkgp(eng, p, np.zeros(Dw + Dz), drop=drop)
    if loo is not None:
        sweep('matern-loo', p, lambda off: linkgp(eng, p, off, drop=drop), exact=loo, bounds=R.matern_bounds(loo, p), bit_equal=True)
    else:
        sweep('matern-loo', p, lambda off: linkgp(eng, p, off, drop=drop), reference=(mean0, var0), bit_equal=True)
    for t in range(4):
        keep = np.delete(np.arange(n), drop[t])
        s2 = O.compute_stats(X0[keep], p['y'][keep], p['length'], p['nugget'], 'matern2.5', Dw)
        with integral_oracle():
            mr, vr = O.link_gp_predict(p['m0'][t:t + 1], p['v'][t:t + 1], p['z0'][t:t + 1] if Dz else None, p['W0'][keep],
                                       p['Wg0'][keep] if Dz else None, s2['Rinv'], s2['Rinv_y'], p['scale'], p['length'], p['nugget'],
                                       'matern2.5')
        assert coarse(mean0[t:t + 1], var0[t:t + 1], mr, vr) == (True, True), (t, mean0[t], mr, var0[t], vr)


# ------------------------------------------------------------------------------------------------ Vecchia
def vecchia_run(e, p, NN, off):
    import torch
    W, m, Wg, z = R.shifted(p, off)
    Dz = p['Dz']
    mo, vo = e.vecchia_linkgp(p['name'], e.tensor(m), e.tensor(p['v']), e.tensor(z) if Dz else None, e.tensor(W), e.tensor(Wg) if Dz else None,
                              e.tensor(NN, dtype=torch.int64), e.tensor(p['y']), p['scale'], p['length'], p['nugget'], e.tensor(np.ones(p['n'])))
    return npy(mo), npy(vo)


def vecchia_case(name, Dw, Dz, pm):
    """n = 65; pm = 65: the full conditioning set (the dense prediction); pm = 50: the 50 nearest training points."""
    from oracle import dgp_oracle as O
    p = problem_of(name, 65, Dw, Dz)
    X0 = np.concatenate((p['W0'], p['Wg0']), 1)
    NN = O.pred_nn(np.concatenate((p['m0'], p['z0']), 1) / p['length'], X0 / p['length'], pm)

    def make():
        if name == 'sexp':
            return R.exact_sexp_vecchia(p, NN)
        with integral_oracle():
            return O.link_gp_vecch(p['m0'], p['v'], p['z0'] if Dz else None, p['W0'], p['Wg0'] if Dz else None, NN, p['y'], p['scale'],
                                   p['length'], p['nugget'], np.ones(65), name)
    return p, NN, cached(('v', name, Dw, Dz, pm), make)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
@pytest.mark.parametrize('Dw,Dz', R.SHAPES)
def test_vecchia_lds_form(eng, name, Dw, Dz):
    """vecchia_linkgp_kernel with the full conditioning set pm = n = 65 (past the register form's 50): the dense prediction.
    Reference: SExp the long-double prediction with the correlation matrix inverted in long double, Matern the oracle on the
    integral; the kernel factorises K itself (cond <= 1e4), so the suite's tolerances, and bit-equality across the shifts."""
    p, NN, ref = vecchia_case(name, Dw, Dz, 65)
    sweep('vecchia-lds-' + name, p, lambda off: vecchia_run(eng, p, NN, off), reference=ref, bit_equal=True)


@pytest.mark.parametrize('name', ['sexp', 'matern2.5'])
@pytest.mark.parametrize('Dw,Dz', [(1, 0), (3, 2)])
def test_vecchia_register_form(eng, name, Dw, Dz):
    """vecchia_linkgp_sexp_reg_kernel / _matern_reg_kernel (pm <= 50, Dw <= 8) with the 50 nearest training points."""
    p, NN, ref = vecchia_case(name, Dw, Dz, 50)
    sweep('vecchia-reg-' + name, p, lambda off: vecchia_run(eng, p, NN, off), reference=ref, bit_equal=True)


# ------------------------------------------------------------------------------------------------ gp_predict at deterministic inputs
@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_gp_predict_sexp(eng, n, Dw, Dz):
    """Engine.gp_predict with the test means as deterministic inputs (v = 0), SExp: the bound of linkshift_ref.gp_bounds, and
    bit-equal across the shifts."""
    p = problem_of('sexp', n, Dw, Dz)
    ex = cached(('g', n, Dw, Dz), lambda: R.exact_gp(p))

    def run(off):
        W, m, Wg, z = R.shifted(p, off)
        mo, vo = eng.gp_predict('sexp', eng.tensor(np.concatenate((m, z), 1)), eng.tensor(np.concatenate((W, Wg), 1)), p['length'],
                                eng.tensor(p['Rinv']), n, eng.tensor(p['ry']), p['scale'], p['nugget'])
        return npy(mo), npy(vo)
    sweep('gp-sexp', p, run, exact=ex, bounds=R.gp_bounds(ex, p), bit_equal=True)


@pytest.mark.parametrize('n,Dw,Dz', CASES)
def test_gp_predict_matern(eng, n, Dw, Dz):
    """... Matern: the suite's tolerances against O.gp_predict at offset 0."""
    from oracle import dgp_oracle as O
    p = problem_of('matern2.5', n, Dw, Dz)
    X0, x0 = np.concatenate((p['W0'], p['Wg0']), 1), np.concatenate((p['m0'], p['z0']), 1)
    ref = O.gp_predict(x0, X0, p['Rinv'], p['ry'], p['scale'], p['length'], p['nugget'], 'matern2.5')

    def run(off):
        W, m, Wg, z = R.shifted(p, off)
        mo, vo = eng.gp_predict('matern2.5', eng.tensor(np.concatenate((m, z), 1)), eng.tensor(np.concatenate((W, Wg), 1)), p['length'],
                                eng.tensor(p['Rinv']), n, eng.tensor(p['ry']), p['scale'], p['nugget'])
        return npy(mo), npy(vo)
    sweep('gp-matern', p, run, reference=ref, bit_equal=True)


# ------------------------------------------------------------------------------------------------ the public wrapper
def test_functions_link_gp_at_offset_1024(eng):
    """dgp_amd.functions.link_gp (numpy in, numpy out) at offset 2^10 against offset 0 and the exact values."""
    from dgp_amd.functions import link_gp
    p, ex = sexp_exact(130, 3, 2)
    out = []
    for off in (np.zeros(5), np.full(5, 2.0 ** 10)):
        W, m, Wg, z = R.shifted(p, off)
        out.append(link_gp(m, p['v'], z, W, Wg, p['Rinv'], p['ry'], None, None, p['scale'], p['length'], p['nugget'], 'sexp', engine=eng))
    bm, bv = sexp_bounds(ex, p)
    for (mean, var), what in zip(out, ('offset 0', 'offset 1024')):
        rm, rv = R.worst_ratio(mean, ex['mean'], bm), R.worst_ratio(var, ex['var'], bv)
        print('functions.link_gp %s mean err/bound %.3g var err/bound %.3g' % (what, rm, rv))
        assert rm <= 1.0 and rv <= 1.0, (what, rm, rv)
        assert coarse(mean, var, ex['mean'], ex['var']) == (True, True), what
    assert coarse(out[1][0], out[1][1], out[0][0], out[0][1]) == (True, True)
