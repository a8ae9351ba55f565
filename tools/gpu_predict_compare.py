"""Compare two dumps of tools/gpu_predict_dump.py (a parent checkout's and its refactoring's): every array must be numpy.array_equal,
except where the refactoring moved an aggregation over the S imputations from numpy's mean to the device's accumulate / finalise pair --
predict(full_layer=True) of a Vecchia-mode emulator, and metric('ALM') under a likelihood, which reads it.  There two differently
ordered S-term sums may differ by their rounding: per element |d mean| <= 2 (S + 2) 2^-53 mean_s |mu_s| and |d var| <= 2 (S + 2) 2^-53
max_s (mu_s^2 + var_s).  The dump holds the aggregated moments only, so the scales used here are |mean| <= mean_s |mu_s| and
var + mean^2 = mean_s (mu_s^2 + var_s) <= max_s (...): never wider than those bounds.
The last full_layer entry of an emulator with a Categorical top is no such sum: its class probabilities are computed on the host
from the aggregated moments (m, v) of the feeding latent, which are held to the bounds above, dm and dv.  Its bound is those
propagated through the link to first order, plus the rounding of evaluating it twice (u = 2^-53, an operation within 1 ulp, expit
within 2).  Two classes, link 'logit' (likelihood_class.Categorical.prediction): den = 1 + pi/8 v, t = m / sqrt(den), p = expit(t),
pv = clip(q^2 r, 0, q) with q = p (1 - p), r = v / den:
    dt = dm / sqrt(den) + |m| pi/16 dv / den^1.5 + 8 u |t|          dp = q dt + 4 u p
    dq = |1 - 2p| dp + 4 u q      dr = dv / den^2 + 6 u r           dpv = max(2 q r dq + q^2 dr + 4 u q^2 r, dq)
Any other link has no bound stated here and a difference there is a defect.  Prints the report; exit status 1 on a defect.
usage: gpu_predict_compare.py PARENT.npz CHILD.npz"""
import re
import sys

import numpy as np

EXCEPTED = re.compile(r'^([a-e])\.(vecchia_\w+)\.(predict_full\.([01])\.(\d+)|metric_ALM)$')


def bound_scale(P, key):
    """The scale of the rounding bound per element of an excepted array, from the parent's dump (None: no such layer)."""
    case, mode, _, which, layer = EXCEPTED.match(key).groups()
    full = '%s.%s.predict_full' % (case, mode)
    if layer is None:   # metric ALM under a likelihood: the variance of the last GP layer of predict_full
        layer = next((k.rsplit('.', 1)[1] for k in P.files if k.startswith(full + '.1.') and np.array_equal(P[k], P[key])), None)
        which = '1'
        if layer is None:
            return None
    mean, var = P['%s.0.%s' % (full, layer)], P['%s.1.%s' % (full, layer)]
    return np.abs(mean) if which == '0' else var + mean ** 2


def categorical_bound(P, case, mode, which, layer, eps):
    """The bound of the docstring on the class probabilities (which '0') or their variances ('1'), or None where none is stated."""
    if str(P[case + '.categorical_link']) != '2:logit':
        return None
    col = P[case + '.categorical_input_dim']
    m, v = (P['%s.%s.predict_full.%d.%d' % (case, mode, w, int(layer) - 1)][:, col].reshape(-1) for w in (0, 1))
    u, dm, dv = 2.0 ** -53, eps * np.abs(m), eps * (v + m ** 2)
    den = 1.0 + np.pi / 8.0 * v
    t = m / np.sqrt(den)
    p = 1.0 / (1.0 + np.exp(-t))
    q, r = p * (1.0 - p), v / den
    dp = q * (dm / np.sqrt(den) + np.abs(m) * np.pi / 16.0 * dv / den ** 1.5 + 8 * u * np.abs(t)) + 4 * u * p
    dq = np.abs(1.0 - 2.0 * p) * dp + 4 * u * q
    dpv = np.maximum(2 * q * r * dq + q ** 2 * (dv / den ** 2 + 6 * u * r) + 4 * u * q ** 2 * r, dq)
    return (dp if which == '0' else dpv).reshape(-1, 1)


def main(parent, child):
    P, C = np.load(parent), np.load(child)
    bad, worst, n_exc = [], (0.0, None), 0
    if sorted(P.files) != sorted(C.files):
        bad.append('the dumps hold different arrays: %s' % sorted(set(P.files) ^ set(C.files)))
    for key in sorted(set(P.files) & set(C.files)):
        a, b = P[key], C[key]
        if a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == 'f'):
            continue
        hit = EXCEPTED.match(key)
        if hit and hit.group(4) is None and not bool(P[hit.group(1) + '.likelihood']):
            hit = None   # (without a likelihood on top ALM reads the plain predict: nothing excepted)
        if hit and a.shape == b.shape and a.dtype.kind == 'f':
            case, mode, _, which, layer = hit.groups()
            eps = 2 * (int(P[case + '.N']) + 2) * 2.0 ** -53
            top = bool(P[case + '.categorical']) and layer is not None and '%s.%s.predict_full.0.%d' % (case, mode, int(layer) + 1) not in P.files
            bound = categorical_bound(P, case, mode, which, layer, eps) if top else bound_scale(P, key)
            bound = bound if top or bound is None else eps * bound
            if bound is not None and bound.shape == a.shape:
                n_exc += 1
                with np.errstate(invalid='ignore', divide='ignore'):
                    ratio = float(np.nanmax(np.where(a == b, 0.0, np.abs(a - b) / bound)))
                worst = max(worst, (ratio, key))
                if ratio <= 1.0:
                    continue
                bad.append('%s: %.3g times its rounding bound (%s)' % (key, ratio, 'a Categorical top: the propagated bound' if top else
                                                                       'an S = %d term sum' % int(P[case + '.N'])))
                continue
        bad.append('%s differs%s' % (key, '' if a.dtype.kind != 'f' or a.shape != b.shape else
                                     ': max |difference| %.3g' % float(np.nanmax(np.abs(a - b)))))
    raised = [k for k in P.files if P[k].dtype.kind == 'U' and not k.endswith('.categorical_link')]
    print('%d arrays compared (%d of them the text of a refusal); %d differ within the excepted aggregation, largest ratio to its '
          'bound %.3g (%s); %d defects' % (len(P.files), len(raised), n_exc, worst[0], worst[1], len(bad)))
    for line in bad:
        print('DEFECT ' + line)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:3]))
