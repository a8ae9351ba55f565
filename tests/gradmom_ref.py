"""Reference for the gradient second-moment sums of dgpamd_gradmom_tiles / dgpamd_sobol_add and for the formulas of
sensitivity.ActiveSubspaceResult (DESIGN I.18).

sums(f, J, shift, dtype): per (path, output) the NC = 2 + Dx + Dx (Dx + 1) / 2 sums over the rows, in the device's order of
entries: sum g, sum g^2, sum J_d, sum J_d J_e for d <= e (the upper triangle row-major).  g = f - shift is formed in f64, the one
IEEE subtraction the device does, so both sides sum terms of the same numbers; the terms and the sums are then taken in
`dtype`: np.float64 (numpy's pairwise order -- a restatement, not the device's bits) or np.longdouble, the reference of the
bound.

Bound of a device sum of n terms (n the rows summed), entry by entry:
    |device - reference| <= (n + 3) 2^-53 sum_rows |term|.
A term is a product rounded once, or fused into the addition that takes it; whatever the order of the additions -- the order
inside an MFMA is the instruction's own -- a term passes through at most n - 1 of them, tile sums included, so the computed
sum is sum term_j (1 + d_j) with |d_j| <= (1 + u)^n - 1, u = 2^-53: the any-order bound of a rounded-product sum.  The three
extra u cover the second-order terms (n^2 u^2 / 2) and the reference's own rounding (64-bit significands: at most n 2^-64
relative to the same sum of magnitudes, 2^-11 of the bound) for every n below 4096; the tests sum a few hundred rows."""
import numpy as np

U = 2.0**-53


def n_sums(Dx):
    return 2 + Dx + Dx * (Dx + 1) // 2


def _terms(f, J, shift, dtype):
    """Per path: (M, K, NC) terms in `dtype`."""
    Dx = J.shape[-1]
    iu = np.triu_indices(Dx)
    for p in range(f.shape[0]):
        g = (f[p] - shift[p][None, :]).astype(dtype)
        Jp = J[p].astype(dtype)
        yield np.concatenate((g[..., None], (g * g)[..., None], Jp, Jp[..., iu[0]] * Jp[..., iu[1]]), -1)


def sums(f, J, shift, dtype=np.float64):
    """(P, K, NC) in `dtype`.  f (P, M, K), J (P, M, K, Dx), shift (P, K): f64 host arrays."""
    return np.stack([t.sum(0) for t in _terms(f, J, shift, dtype)])


def magnitudes(f, J, shift):
    """(P, K, NC) longdouble: sum over the rows of |term|."""
    return np.stack([np.abs(t).sum(0) for t in _terms(f, J, shift, np.longdouble)])


def worst_ratio(device, f, J, shift):
    """max over the entries of |device - longdouble sums| / ((n + 3) 2^-53 sum |term|); 0 / 0 counts as 0 (a sum of zeros must
    come out as zero), a non-zero error over a zero bound as inf."""
    assert np.all(np.isfinite(device))
    n = f.shape[1]
    err = np.abs(np.asarray(device).astype(np.longdouble) - sums(f, J, shift, np.longdouble))
    bound = (n + 3) * np.longdouble(U) * magnitudes(f, J, shift)
    with np.errstate(divide='ignore', invalid='ignore'):
        ratio = np.where(err > 0, err / bound, 0.0)
    return float(ratio.max())


def check(device, f, J, shift, what):
    ratio = worst_ratio(device, f, J, shift)
    print('%s: max error / bound = %.3g' % (what, ratio))
    assert ratio <= 1.0, (what, ratio)
    return ratio


def from_gradients(f, G, shift=None):
    """The sums dictionary ActiveSubspaceResult takes, from values f (P, M, K) and gradients G (P, M, K, Dx) in f64."""
    shift = f[:, 0, :].copy() if shift is None else shift
    return {'sums': sums(f, G, shift), 'shift': shift}


def formulas(S, shift, n_rows, bounds=None):
    """ActiveSubspaceResult's quantities restated from sums S (P, K, NC): a dict of C (K, P, Dx, Dx), dgsm, mean_grad
    (K, Dx, P), mean, variance (K, P), scale (Dx,), scaled = S C S (K, P, Dx, Dx) and, with bounds, total_bound (K, Dx, P)."""
    P, K, NC = S.shape
    Dx = next(d for d in range(1, 65) if n_sums(d) == NC)
    C = np.zeros((K, P, Dx, Dx))
    c = 2 + Dx
    for d in range(Dx):
        for e in range(d, Dx):
            C[:, :, d, e] = C[:, :, e, d] = S[:, :, c].T / n_rows
            c += 1
    s1, s2 = S[..., 0] / n_rows, S[..., 1] / n_rows
    out = dict(C=C, dgsm=np.stack([C[:, :, d, d] for d in range(Dx)], 1), mean_grad=(S[..., 2:2 + Dx] / n_rows).transpose(1, 2, 0),
               mean=(shift + s1).T, variance=(s2 - s1**2).T)
    out['scale'] = np.ones(Dx) if bounds is None else 0.5 * (np.asarray(bounds)[:, 1] - np.asarray(bounds)[:, 0])
    out['scaled'] = C * out['scale'][:, None] * out['scale'][None, :]
    if bounds is not None:
        width = np.asarray(bounds)[:, 1] - np.asarray(bounds)[:, 0]
        with np.errstate(divide='ignore', invalid='ignore'):
            V = np.where(out['variance'] == 0.0, np.nan, out['variance'])
            out['total_bound'] = out['dgsm'] * (width**2)[None, :, None] / (np.pi**2 * V[:, None, :])
    return out
