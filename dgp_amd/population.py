"""What the population methods over a box share on the host (calibrate.calibrate_smc, DESIGN I.21;
reliability.failure_probability, DESIGN I.22), and the plumbing that calibrate.calibrate takes too: the prior over the box and
its particles, where the random numbers come from, and the one stage loop.  Both methods are the same machine: P draws with R
particles each; a stage is one per-draw step on the device (csrc/boxpop.hpp), then n_moves + 1 walk evaluations with a move
behind each, then the step's adaptation.  What the per-draw step selects by, what a move is and what a step means are the
callers'."""
import numpy as np
import torch

from .ops import Engine

RNGS = ('numpy', 'device')
STREAM_PRIOR, STREAM_NORMAL, STREAM_LOGU, STREAM_RESAMPLE = 0, 1, 2, 3      # c3 of dgpamd_philox_fill's counter (DESIGN I.23)


def check_rng(rng, what):
    if rng not in RNGS:
        raise ValueError("%s: rng must be 'numpy' or 'device'" % what)
    return rng == 'device'


def check_prior(prior, Dx):
    """(precision (Dx,), mean (Dx,)) of prior = None or (mean (Dx,), sd (Dx,)); an infinite sd is a flat column."""
    if prior is None:
        return np.zeros(Dx), np.zeros(Dx)
    try:
        mean, sd = (np.asarray(a, dtype=np.float64) for a in prior)
    except (TypeError, ValueError):
        raise ValueError('calibrate: prior must be None or (mean (Dx,), sd (Dx,))') from None
    if mean.shape != (Dx,) or sd.shape != (Dx,) or not np.all(np.isfinite(mean)) or np.any(np.isnan(sd)) or not np.all(sd > 0.0):
        raise ValueError('calibrate: prior must be (mean, sd), (%d,) each, mean finite and sd > 0 (inf: flat)' % Dx)
    return 1.0 / (sd * sd), mean


def prior_draws(u, lo, hi, pv, pm):
    """x (..., Dx) in the box with the prior's distribution from uniforms u (..., Dx) in [0, 1), by the inverse cdf: a flat
    column (pv_d = 0) is lo + u (hi - lo); another one is N(pm_d, 1 / pv_d) truncated to [lo_d, hi_d]; lo_d = hi_d keeps it."""
    from scipy.special import ndtr, ndtri
    x = lo + u * (hi - lo)
    for d in np.nonzero((pv > 0.0) & (hi > lo))[0]:
        sd = 1.0 / np.sqrt(pv[d])
        a, b = ndtr((lo[d] - pm[d]) / sd), ndtr((hi[d] - pm[d]) / sd)
        x[..., d] = pm[d] + sd * ndtri(a + u[..., d] * (b - a))
    return np.minimum(np.maximum(x, lo), hi)


def stage_round(t, i=0):
    """The round c2 of move i of stage t in calibrate_smc and failure_probability: (t << 32) | i."""
    return (int(t) << 32) | int(i)


def upload(e, a):
    """e.tensor for what a numpy stream returns; what a device stream returns is on the device already."""
    return a if torch.is_tensor(a) else e.tensor(a)


def host_uniforms(u):
    """The prior uniforms on the host: a device stream's visit it once, for prior_draws."""
    return u.cpu().numpy() if torch.is_tensor(u) else u


class HostStreams:
    """The numpy random numbers of a population run: children of np.random.SeedSequence(seed) by spawn key, one generator per
    key.  Which keys there are and what each fills is the subclass's layout (calibrate.SmcStreams, reliability.SusStreams)."""

    def __init__(self, seed, P, R, Dx):
        self.entropy = np.random.SeedSequence(seed).entropy
        self.P, self.R, self.Dx, self.t = P, R, Dx, 0

    def _rng(self, *key):
        return np.random.default_rng(np.random.SeedSequence(self.entropy, spawn_key=key))


class DeviceStageStreams:
    """The host streams' twin for rng='device' (Engine.philox_fill under the key of the seed, DESIGN I.23): the prior uniforms
    are stream 0 at round 0; stage t reads z from stream 1, Dx elements, and log u from stream 2, logu_elements of them, at
    c2 = (t << 32) | i for move i; with resample its resampling uniform from stream 3 at (c2 = t << 32, r = 0).  Particle
    (p, r)'s numbers depend on nothing but the seed, p, r, t and i."""

    def __init__(self, e, seed, P, R, Dx, logu_elements, resample):
        self.e, self.key, self.P, self.R, self.Dx, self.t = e, Engine.philox_key(seed), P, R, Dx, 0
        self.logu_elements, self.resample = logu_elements, resample

    def prior_uniforms(self):
        """(P, R, Dx) uniforms in [0, 1), on the device."""
        return self.e.philox_fill('uniform', self.key, STREAM_PRIOR, 0, 1, self.P, self.R, self.Dx)[0]

    def stage(self, rounds):
        """([u (P,),] z (rounds, P, R, Dx), log u (rounds, P, R[, Dx])) of the next stage, on the device."""
        t, self.t = self.t, self.t + 1
        c2, fill = stage_round(t), self.e.philox_fill
        u = (fill('uniform', self.key, STREAM_RESAMPLE, c2, 1, self.P, 1, 1).view(self.P),) if self.resample else ()
        logu = fill('log_uniform', self.key, STREAM_LOGU, c2, rounds, self.P, self.R, self.logu_elements)
        return u + (fill('normal', self.key, STREAM_NORMAL, c2, rounds, self.P, self.R, self.Dx),
                    logu.view(rounds, self.P, self.R) if self.logu_elements == 1 else logu)


def prior_particles(streams, lo, hi, pv, pm):
    """x0 (P, R, Dx), contiguous: the run's particles under the prior on the box, from the streams' prior uniforms."""
    return np.ascontiguousarray(prior_draws(host_uniforms(streams.prior_uniforms()), lo, hi, pv, pm))


def run_stages(e, streams, state, n_moves, max_stages, target_accept, select, move, adapt):
    """The stage loop of both methods.  state: the engine's, with P, R, n_prop, n_acc (P R) and running.  A stage fetches its
    streams -- (z, log u) of n_moves + 1 rounds, before them what the per-draw step draws --, calls select(*that), the
    per-draw step with what the caller records around it, then move(z_i, logu_i, first, last), first on round 0 and last on
    round n_moves; the stage's acceptance rate per draw over all its particles goes to adapt(exp(rate - target_accept)), which
    scales and clamps the caller's step, and the loop ends when no draw is running.  Returns the rates, (P,) per stage."""
    P, R, accept = state['P'], state['R'], []
    for stage in range(max_stages):
        *u, zb, ub = (upload(e, a) for a in streams.stage(n_moves + 1))
        select(*u)
        for i in range(n_moves + 1):
            move(zb[i], ub[i], first=i == 0, last=i == n_moves)
        rate = state['n_acc'].view(P, R).sum(1).double() / state['n_prop'].view(P, R).sum(1).clamp(min=1).double()
        accept.append(rate)
        adapt(torch.exp(rate - target_accept))
        if int(state['running'].item()) == 0:
            break
    return accept


def particles(x, P, R):
    """(P, R, Dx), contiguous, from the moves' state x (Dx, P R) on the host."""
    return np.ascontiguousarray(x.reshape(-1, P, R).transpose(1, 2, 0))


def draw_status(codes, status, unfinished):
    """status (P,) with 'max_stages' for the ok draws that the last stage left unfinished."""
    status = status.copy()
    status[(status == codes['ok']) & unfinished] = codes['max_stages']
    return status
