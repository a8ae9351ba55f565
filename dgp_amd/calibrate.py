"""Bayesian calibration with function-valued posterior draws, on the device (paths.calibrate, emulator.calibrate,
gp.calibrate; DESIGN I.19): which inputs x produced the observation y?

Conditional on one draw f_p of the emulated function, the posterior of x over a box is
    p(x | y, f_p)  proportional to  prior(x) N(y; f_p(x), obs_sd^2),
and every draw has a closed-form Jacobian, so each of these posteriors can be sampled by a gradient-informed chain.  Sampling
it for every draw and pooling the samples with equal weights gives the MODULAR (cut) posterior of Liu, Bayarri and Berger
(2009): the emulator's uncertainty is carried into the calibration, the observation is not fed back into the emulator.
P draws with R chains each are P R independent Metropolis-adjusted Langevin chains.  They advance in lock-step: a round
evaluates every chain's trial point through the layer walk at per-path rows (P, R, Dx), values and Jacobian, and
dgpamd_boxmala_step (one lane per chain) decides the proposals, adapts the steps during warm-up, stores the samples and writes
the next trial points.  The normal and uniform draws come from numpy generators, uploaded in blocks of rounds; nothing visits
the host until the end.  The starts are the best of n_candidates rows in the box, screened through the shared-rows walk.
method='hmc' (DESIGN I.20) runs the same loop with dgpamd_boxhmc_step: an iteration is a trajectory of L leapfrog steps, one
round each, with the walls of the box reflecting; L is n_leapfrog, or with jitter uniform on 1 .. n_leapfrog per iteration.
"""
import warnings

import numpy as np
import torch

from . import optimize, pathfun
from .ops import Engine

STATUS = Engine.BOXMALA
HMIN, HMAX = 1e-10, 1e2       # the clamp of a chain's step, in units of `scale`
TARGET_ACCEPT = dict(mala=0.574, hmc=0.8)      # what target_accept=None means
GAIN_DECAY = 0.6              # gamma_w = (w + 1)^-GAIN_DECAY: sum gamma = inf, sum gamma^2 < inf (Robbins and Monro)
UPLOAD_BYTES = 1 << 25        # the normal and uniform draws of one upload


def gain(w, target_accept):
    """(up, down) of warm-up round w = 0, 1, ...: log h moves by gamma_w (accepted - target_accept), gamma_w = (w + 1)^-0.6."""
    g = (w + 1.0) ** -GAIN_DECAY
    return float(np.exp(g * (1.0 - target_accept))), float(np.exp(-g * target_accept))


def _rounds_per_upload(Q, Dx):
    return max(1, UPLOAD_BYTES // (8 * Q * (Dx + 1)))


def observation(y, obs_sd, K):
    """(ybar (K,), w (K,)): the sufficient statistics of y (K,) or (T, K) replicates at one x, NaN an unobserved entry, under
    independent N(0, obs_sd^2) errors, obs_sd a positive scalar or (K,): ybar_k the mean of output k's T_k finite entries
    (0 where there is none), w_k = T_k / obs_sd_k^2."""
    y = np.atleast_1d(np.asarray(y, dtype=np.float64))          # (a number is (1,): one output)
    if y.ndim == 1:
        y = y[None]
    if y.ndim != 2 or y.shape[0] < 1 or y.shape[1] != K:
        raise ValueError('calibrate: y must be (K,) or (T, K) with K = %d outputs' % K)
    if np.any(np.isinf(y)):
        raise ValueError('calibrate: y must be finite (NaN marks an unobserved entry)')
    seen = ~np.isnan(y)
    if not seen.any():
        raise ValueError('calibrate: y has no finite entry')
    sd = np.asarray(obs_sd, dtype=np.float64)
    if sd.ndim > 1 or (sd.ndim == 1 and sd.shape[0] != K) or not np.all(np.isfinite(sd)) or not np.all(sd > 0.0):
        raise ValueError('calibrate: obs_sd must be a positive number or (K,) = (%d,) positive numbers' % K)
    T = seen.sum(0)
    ybar = np.where(seen, y, 0.0).sum(0) / np.maximum(T, 1)
    return ybar, T / (np.broadcast_to(sd, (K,)) * np.broadcast_to(sd, (K,)))


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


def check_counts(n_chains, n_samples, warmup, thin):
    n_chains, n_samples, warmup, thin = int(n_chains), int(n_samples), int(warmup), int(thin)
    if n_chains < 1 or n_samples < 1 or thin < 1 or warmup < 0:
        raise ValueError('calibrate: need n_chains >= 1, n_samples >= 1, thin >= 1 and warmup >= 0')
    return n_chains, n_samples, warmup, thin


def trajectory_lengths(seed, iterations, n_leapfrog, jitter):
    """(iterations,) int: the leapfrog steps of every HMC iteration, shared by all chains.  With jitter uniform on
    1 .. n_leapfrog, from the third child of np.random.SeedSequence(seed).spawn(3), whose first two are Streams'; else
    n_leapfrog."""
    if not jitter:
        return np.full(iterations, n_leapfrog, dtype=np.int64)
    return np.random.default_rng(np.random.SeedSequence(seed).spawn(3)[2]).integers(1, n_leapfrog + 1, iterations)


class Streams:
    """The random numbers of a run: two independent streams, z (standard normal) and u (uniform), from
    np.random.SeedSequence(seed).spawn(2).  Each stream spawns one child generator per chain slot r, so that the numbers of
    chain (p, r) do not depend on how many chains run beside it; a slot's generator is drawn in round order, (rounds, P, Dx)
    and (rounds, P) per block, so the block size does not change a number."""

    def __init__(self, seed, P, R, Dx):
        sz, su = np.random.SeedSequence(seed).spawn(2)
        self.z = [np.random.default_rng(s) for s in sz.spawn(R)]
        self.u = [np.random.default_rng(s) for s in su.spawn(R)]
        self.P, self.Dx = P, Dx

    def block(self, rounds):
        """(z (rounds, P, R, Dx), log u (rounds, P, R)) of the next `rounds` rounds."""
        z = np.stack([g.standard_normal((rounds, self.P, self.Dx)) for g in self.z], 2)
        with np.errstate(divide='ignore'):
            logu = np.log(np.stack([g.random((rounds, self.P)) for g in self.u], 2))
        return z, logu


# ---------------------------------------------------------------------------------------------- diagnostics (host numpy)
def split_rhat(x):
    """The split potential scale reduction of x (..., R, S), S >= 4 samples of R chains: every chain is cut in two halves,
    R-hat = sqrt(((n - 1) / n W + B / n) / W) over the 2 R half chains of n = S // 2 samples (Gelman et al., BDA3 11.4).
    NaN where the chains do not move."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[-1] // 2
    if n < 2:
        raise ValueError('rhat: need at least 4 samples per chain')
    halves = np.concatenate([x[..., :n], x[..., x.shape[-1] - n:]], -2)
    W = halves.var(-1, ddof=1).mean(-1)
    B_n = halves.mean(-1).var(-1, ddof=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.sqrt(((n - 1.0) / n * W + B_n) / W)


def _autocov(x):
    """The biased autocovariances (divided by S) of the rows of x (R, S), by FFT."""
    S = x.shape[-1]
    c = x - x.mean(-1, keepdims=True)
    F = np.fft.rfft(c, 2 * S, axis=-1)
    return np.fft.irfft(F * np.conj(F), 2 * S, axis=-1)[..., :S] / S


def ess(x):
    """The effective sample size of the mean of x (..., R, S) from the chains' autocorrelations: rho_t = 1 - (W - mean over
    the chains of their autocovariance at lag t) / var+, summed by Geyer's initial monotone sequence of pairs
    rho_2t + rho_2t+1 (BDA3 11.5); ess = R S / (-1 + 2 sum of the pairs).  NaN where the chains do not move."""
    x = np.asarray(x, dtype=np.float64)
    if x.shape[-1] < 4:
        raise ValueError('ess: need at least 4 samples per chain')
    out = np.empty(x.shape[:-2])
    for idx in np.ndindex(*x.shape[:-2]):
        out[idx] = _ess_one(x[idx])
    return out


def _ess_one(x):
    R, S = x.shape
    acov = _autocov(x)
    W = (acov[:, 0] * S / (S - 1.0)).mean()
    var_plus = W * (S - 1.0) / S + (x.mean(1).var(ddof=1) if R > 1 else 0.0)
    if not var_plus > 0.0:
        return np.nan
    rho = 1.0 - (W - acov.mean(0)) / var_plus
    rho[0] = 1.0
    pairs = rho[:S - S % 2].reshape(-1, 2).sum(1)
    stop = np.nonzero(pairs <= 0.0)[0]
    pairs = np.minimum.accumulate(pairs[:stop[0] if len(stop) else len(pairs)])
    tau = -1.0 + 2.0 * pairs.sum()
    return R * S / max(tau, 1.0 / np.log10(max(R * S, 10)))     # (antithetic chains: ess is capped at R S log10(R S), as Stan does)


class PathPosterior:
    """The input posteriors of P function-valued draws, R chains of S samples each.  x (P, R, S, Dx), logp (P, R, S): the
    samples and their log posterior density up to a constant, -1/2 sum_k w_k (ybar_k - f_k(x))^2 + the log prior.
    accept_rate, step, status (P, R): the acceptance rate after warm-up, the adapted step in units of `scale`, and the
    numbers of calibrate.STATUS (= Engine.BOXMALA, DGPAMD_BOXMALA_*; Engine.BOXHMC carries the same): ok 0; nan 1 the start's
    value or gradient was not finite (the chain repeats its start).  x0 (P, R, Dx): the starts.  rounds: the evaluations of
    the lock-step loop.  method 'mala' or 'hmc'; n_leapfrog: the (largest) trajectory length of 'hmc', 1 for 'mala';
    evaluations: the walk evaluations of the run (None: rounds).
    rhat, ess (P, Dx): the split R-hat over a draw's R chains and the effective sample size of a draw's posterior mean.
    Row p is path p of the draws' container (s * sample_size + j for an emulator)."""

    def __init__(self, x, logp, accept_rate, step, status, x0, rounds, method='mala', n_leapfrog=1, evaluations=None):
        self.x, self.logp, self.accept_rate, self.step, self.status, self.x0, self.rounds = x, logp, accept_rate, step, status, x0, rounds
        self.method, self.n_leapfrog, self.evaluations = method, n_leapfrog, rounds if evaluations is None else evaluations
        self._rhat = self._ess = None

    @property
    def rhat(self):
        if self._rhat is None:
            self._rhat = split_rhat(self.x.transpose(0, 3, 1, 2))
        return self._rhat

    @property
    def ess(self):
        if self._ess is None:
            self._ess = ess(self.x.transpose(0, 3, 1, 2))
        return self._ess

    def pooled(self):
        """(P R S, Dx): every sample of every draw with equal weight, the modular posterior of x."""
        return self.x.reshape(-1, self.x.shape[-1])

    def per_draw(self):
        """(P, R S, Dx): the samples of each draw's own posterior p(x | y, f_p)."""
        return self.x.reshape(self.x.shape[0], -1, self.x.shape[-1])

    def summary(self, level=0.95):
        """{'mean', 'lower', 'upper', 'draw_sd'} (Dx,) each: the mean and the equal-tailed interval of probability `level`
        of the pooled samples, and the standard deviation over the draws of their own posterior means -- what the
        emulator's uncertainty contributes to the spread of x."""
        if not 0.0 < level < 1.0:
            raise ValueError('summary: level must lie in (0, 1)')
        tail = 0.5 * (1.0 - level)
        pooled, means = self.pooled(), self.per_draw().mean(1)
        return {'mean': pooled.mean(0), 'lower': np.quantile(pooled, tail, axis=0), 'upper': np.quantile(pooled, 1.0 - tail, axis=0),
                'draw_sd': means.std(0, ddof=1) if len(means) > 1 else np.zeros(means.shape[1])}


def calibrate(e, P, K, Dx, values, value_and_jac, width, y, obs_sd, bounds, n_chains=4, n_samples=500, warmup=500, thin=1,
              n_candidates=2048, x0=None, seed=None, qmc=False, step=0.1, scale=None, prior=None, target_accept=None, method='mala',
              n_leapfrog=8, jitter=True):
    """The driver behind PathFunctions.calibrate and GpPaths.calibrate; values, value_and_jac and width as in
    optimize.minimize."""
    if method not in TARGET_ACCEPT:
        raise ValueError("calibrate: method must be 'mala' or 'hmc'")
    n_leapfrog = int(n_leapfrog)
    if n_leapfrog < 1:
        raise ValueError('calibrate: need n_leapfrog >= 1')
    if target_accept is None:
        target_accept = TARGET_ACCEPT[method]
    lo, hi = optimize.check_bounds(bounds, Dx, 'calibrate')
    Dx = len(lo)
    ybar, w = observation(y, obs_sd, K)
    pv, pm = check_prior(prior, Dx)
    R, S, warmup, thin = check_counts(n_chains, n_samples, warmup, thin)
    scale = hi - lo if scale is None else np.asarray(scale, dtype=np.float64)
    if scale.shape != (Dx,) or not np.all(np.isfinite(scale)) or np.any(scale < 0.0):
        raise ValueError('calibrate: scale must be (%d,) finite numbers >= 0' % Dx)
    if not (np.isfinite(step) and HMIN <= step <= HMAX) or not 0.0 < target_accept < 1.0:
        raise ValueError('calibrate: need %g <= step <= %g and 0 < target_accept < 1' % (HMIN, HMAX))
    seen = torch.as_tensor(np.nonzero(w > 0.0)[0], device=e.device)
    wd, yd, pvd, pmd = e.tensor(w[w > 0.0]), e.tensor(ybar[w > 0.0]), e.tensor(pv), e.tensor(pm)

    def neg_lp(xd):
        r = yd - values(xd)[:, :, seen]
        return 0.5 * (r * r * wd).sum(2) + 0.5 * ((xd - pmd) ** 2 * pvd).sum(1)
    if x0 is None:
        cand = optimize.candidates(lo, hi, n_candidates, seed, qmc, 'calibrate')
        if R > len(cand):
            raise ValueError('calibrate: n_chains = %d is more than n_candidates = %d' % (R, len(cand)))
        x0 = optimize.best_candidates(e, neg_lp, cand, P, R, width, 1.0)
    else:
        x0 = np.asarray(x0, dtype=np.float64)
        if x0.ndim == 2:
            x0 = np.broadcast_to(x0, (P,) + x0.shape)
        if x0.ndim != 3 or x0.shape[0] != P or x0.shape[1] < 1 or x0.shape[2] != Dx or np.any(np.isnan(x0)):
            raise ValueError('calibrate: x0 must be (R, Dx) or (P, R, Dx) = (%d, R, %d) without NaN' % (P, Dx))
        x0 = np.minimum(np.maximum(x0, lo), hi)     # (a start outside the box begins at its projection)
        R = x0.shape[1]
    Q = P * R
    xt = e.tensor(np.ascontiguousarray(x0))
    # The lock-step loop.  Iteration 0 is INIT; iterations 1 .. warmup adapt; every thin-th one after them is saved.  An
    # iteration reads the streams once, z_c and log u_c, and takes L_c rounds: 1 for 'mala'; for 'hmc' L_0 = 1 and then the
    # trajectory's lengths[c - 1], of which the last round decides it with log u_c, adapts, saves and starts the next
    # trajectory with the momenta z_c.
    hmc = method == 'hmc'
    state = (e.boxhmc_state if hmc else e.boxmala_state)(Q, Dx, w, ybar, lo, hi, scale, pv, pm, n_slots=S)
    streams = Streams(seed, P, R, Dx)
    total = 1 + warmup + S * thin
    lengths = trajectory_lengths(seed, total - 1, n_leapfrog, jitter) if hmc else None
    block = _rounds_per_upload(Q, Dx)
    before, rounds = None, 0
    for c0 in range(0, total, block):
        zb, ub = map(e.tensor, streams.block(min(block, total - c0)))
        for i in range(len(zb)):
            c = c0 + i
            adapt, j = 1 <= c <= warmup, c - warmup
            up, down = gain(c - 1, target_accept) if adapt else (1.0, 1.0)
            L = int(lengths[c - 1]) if hmc and c > 0 else 1
            for l in range(1, L + 1):
                f, J = value_and_jac(xt)
                last = l == L
                kw = dict(h0=step, hmin=HMIN, hmax=HMAX, up=up, down=down, adapt=adapt and last, first=c == 0,
                          slot=j // thin - 1 if last and j >= 1 and j % thin == 0 else -1)
                if hmc:
                    e.boxhmc_step(state, f, J, xt, zb[i], ub[i], last=last, **kw)
                else:
                    e.boxmala_step(state, f, J, xt, zb[i], ub[i], **kw)
            rounds += L
            if c == warmup:
                before = state['n_prop'].clone(), state['n_acc'].clone()
    host = {k: state[k].cpu().numpy() for k in ('xs', 'lps', 'h', 'status', 'n_prop', 'n_acc')}
    n_prop, n_acc = host['n_prop'] - before[0].cpu().numpy(), host['n_acc'] - before[1].cpu().numpy()
    return PathPosterior(np.ascontiguousarray(host['xs'].reshape(S, Dx, P, R).transpose(2, 3, 0, 1)),
                         np.ascontiguousarray(host['lps'].reshape(S, P, R).transpose(1, 2, 0)),
                         (n_acc / np.maximum(n_prop, 1)).reshape(P, R), host['h'].reshape(P, R), host['status'].reshape(P, R),
                         np.array(x0), rounds, method, n_leapfrog if hmc else 1, rounds)
