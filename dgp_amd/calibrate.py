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
the next trial points.  The normal and uniform draws come from numpy generators, uploaded in blocks of rounds, or with
rng='device' from counter-based streams filled on the device (dgpamd_philox_fill, DESIGN I.23); nothing visits the host until
the end.  The starts are the best of n_candidates rows in the box, screened through the shared-rows walk.
method='hmc' (DESIGN I.20) runs the same loop with dgpamd_boxhmc_step: an iteration is a trajectory of L leapfrog steps, one
round each, with the walls of the box reflecting; L is n_leapfrog, or with jitter uniform on 1 .. n_leapfrog per iteration.
calibrate_smc (DESIGN I.21) samples the same posteriors by adaptive likelihood tempering: R particles per draw from the prior,
reweighted, resampled (dgpamd_boxsmc_temper) and moved (dgpamd_boxsmc_move) until beta = 1; the product of the mean incremental
weights is the draw's evidence, and ParticlePosterior can weigh the draws by it.
"""
import warnings

import numpy as np
import torch

from . import optimize, pathfun
from .ops import Engine
# (the plumbing shared with reliability.py; its names stay importable from here)
from .population import (RNGS, STREAM_LOGU, STREAM_NORMAL, STREAM_PRIOR, STREAM_RESAMPLE, DeviceStageStreams, HostStreams, check_prior,
                         check_rng, draw_status, host_uniforms, particles, prior_draws, prior_particles, run_stages, stage_round, upload)

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


def check_counts(n_chains, n_samples, warmup, thin):
    n_chains, n_samples, warmup, thin = int(n_chains), int(n_samples), int(warmup), int(thin)
    if n_chains < 1 or n_samples < 1 or thin < 1 or warmup < 0:
        raise ValueError('calibrate: need n_chains >= 1, n_samples >= 1, thin >= 1 and warmup >= 0')
    return n_chains, n_samples, warmup, thin


def check_step(what, lo, hi, scale, step, target_accept):
    """scale (Dx,), hi - lo for None, after the refusals that the chains and the SMC moves share."""
    Dx = len(lo)
    scale = hi - lo if scale is None else np.asarray(scale, dtype=np.float64)
    if scale.shape != (Dx,) or not np.all(np.isfinite(scale)) or np.any(scale < 0.0):
        raise ValueError('%s: scale must be (%d,) finite numbers >= 0' % (what, Dx))
    if not (np.isfinite(step) and HMIN <= step <= HMAX) or not 0.0 < target_accept < 1.0:
        raise ValueError('%s: need %g <= step <= %g and 0 < target_accept < 1' % (what, HMIN, HMAX))
    return scale


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


# ------------------------------------------------------------------------- random streams made on the device (DESIGN I.23)
class DeviceStreams:
    """Streams' twin for rng='device': the same method, device tensors, the numbers Philox4x64-10 under the key
    SeedSequence(seed).generate_state(2, uint64) (Engine.philox_fill).  z is stream 1 with Dx elements per slot, log u stream 2
    with one; the round c2 is the iteration index, so chain (p, r)'s numbers of iteration c depend on nothing else: not on
    P, R or the block size."""

    def __init__(self, e, seed, P, R, Dx):
        self.e, self.key, self.P, self.R, self.Dx, self.c = e, Engine.philox_key(seed), P, R, Dx, 0

    def block(self, rounds):
        """(z (rounds, P, R, Dx), log u (rounds, P, R)) of the next `rounds` rounds, on the device."""
        c, self.c = self.c, self.c + rounds
        return (self.e.philox_fill('normal', self.key, STREAM_NORMAL, c, rounds, self.P, self.R, self.Dx),
                self.e.philox_fill('log_uniform', self.key, STREAM_LOGU, c, rounds, self.P, self.R, 1).view(rounds, self.P, self.R))


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
    evaluations: the walk evaluations of the run (None: rounds).  rng: 'numpy' or 'device', where the run's normal and uniform
    numbers were made.
    rhat, ess (P, Dx): the split R-hat over a draw's R chains and the effective sample size of a draw's posterior mean.
    Row p is path p of the draws' container (s * sample_size + j for an emulator)."""

    columns = controls = None     # (with controls: the calibration columns of the walk's input (Dx,) and the sites' settings (T, Dc))

    def __init__(self, x, logp, accept_rate, step, status, x0, rounds, method='mala', n_leapfrog=1, evaluations=None, rng='numpy'):
        self.x, self.logp, self.accept_rate, self.step, self.status, self.x0, self.rounds = x, logp, accept_rate, step, status, x0, rounds
        self.method, self.n_leapfrog, self.evaluations = method, n_leapfrog, rounds if evaluations is None else evaluations
        self.rng = rng
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
              n_candidates=2048, x0=None, seed=None, qmc=False, step=0.1, scale=None, *, problem=None, prior=None, rng='numpy',
              target_accept=None, method='mala', n_leapfrog=8, jitter=True):
    """The driver behind PathFunctions.calibrate and GpPaths.calibrate; values, value_and_jac and width as in
    optimize.minimize.  rng='device': the chains' normals and uniforms are made on the device (DeviceStreams) instead of by
    numpy generators and an upload; the candidate design and HMC's trajectory lengths stay numpy's.  problem: a prepared
    fieldcal.FieldProblem (DESIGN I.24) -- its K, Dx, closures, width and pseudo-observation stand for the arguments' and for
    observation(y, obs_sd, K), and the result carries its columns and controls."""
    if method not in TARGET_ACCEPT:
        raise ValueError("calibrate: method must be 'mala' or 'hmc'")
    device_rng = check_rng(rng, 'calibrate')
    n_leapfrog = int(n_leapfrog)
    if n_leapfrog < 1:
        raise ValueError('calibrate: need n_leapfrog >= 1')
    if target_accept is None:
        target_accept = TARGET_ACCEPT[method]
    if problem is not None:
        K, Dx, values, value_and_jac, width = problem.K, problem.Dx, problem.values, problem.value_and_jac, problem.width
    lo, hi = optimize.check_bounds(bounds, Dx, 'calibrate')
    Dx = len(lo)
    ybar, w = observation(y, obs_sd, K) if problem is None else (problem.ybar, problem.w)
    pv, pm = check_prior(prior, Dx)
    R, S, warmup, thin = check_counts(n_chains, n_samples, warmup, thin)
    scale = check_step('calibrate', lo, hi, scale, step, target_accept)
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
    streams = DeviceStreams(e, seed, P, R, Dx) if device_rng else Streams(seed, P, R, Dx)
    total = 1 + warmup + S * thin
    lengths = trajectory_lengths(seed, total - 1, n_leapfrog, jitter) if hmc else None
    block = _rounds_per_upload(Q, Dx)
    before, rounds = None, 0
    for c0 in range(0, total, block):
        zb, ub = (upload(e, a) for a in streams.block(min(block, total - c0)))
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
    res = PathPosterior(np.ascontiguousarray(host['xs'].reshape(S, Dx, P, R).transpose(2, 3, 0, 1)),
                        np.ascontiguousarray(host['lps'].reshape(S, P, R).transpose(1, 2, 0)),
                        (n_acc / np.maximum(n_prop, 1)).reshape(P, R), host['h'].reshape(P, R), host['status'].reshape(P, R),
                        np.array(x0), rounds, method, n_leapfrog if hmc else 1, rounds, rng)
    if problem is not None:
        res.columns, res.controls = problem.columns, problem.controls
    return res


# ------------------------------------------------------------------------- tempered SMC with per-draw evidence (DESIGN I.21)
SMC_STATUS = Engine.BOXSMC
MAX_PARTICLES = Engine.BOXSMC_MAXR


def log_norm(y, obs_sd, K):
    """The constant that observation's sufficient statistics drop from log N(y; f, obs_sd^2):
    -sum_k T_k / 2 log(2 pi sd_k^2) - 1/2 sum_k sum_t (y_tk - ybar_k)^2 / sd_k^2 over the finite entries of y."""
    ybar, w = observation(y, obs_sd, K)
    y = np.atleast_1d(np.asarray(y, dtype=np.float64))
    y = y[None] if y.ndim == 1 else y
    seen = ~np.isnan(y)
    sd2 = np.broadcast_to(np.asarray(obs_sd, dtype=np.float64), (K,)) ** 2
    T = seen.sum(0)
    within = np.where(seen, (np.where(seen, y, 0.0) - ybar) ** 2, 0.0).sum(0)
    return float(-0.5 * np.sum(T * np.log(2.0 * np.pi * sd2)) - 0.5 * np.sum(within / sd2))


def stage_gain(stage, rate, target_accept):
    """The factor on a draw's step after stage `stage` whose moves were accepted at `rate`: exp(rate - target_accept).  The
    step is held fixed within a stage and is one number per draw, set from the acceptance of all the draw's particles: every
    move is then invariant for its pi_beta.  (Adapting a slot's step after each of its own decisions, as the chains' warm-up
    does, is not: over the 10 to 20 moves of a run the gain does not get small, the step follows the particle's own last
    outcome, and the restatement's particle variance came out 5 % low on the line case of DESIGN I.21.)  The gain does not
    decay: every stage has another target."""
    return float(np.exp(rate - target_accept))


class SmcStreams(HostStreams):
    """The random numbers of an SMC run, children of np.random.SeedSequence(seed) by spawn key: (0, r) the prior uniforms of
    particle slot r, (P, Dx); (1, r, t) and (2, r, t) the normal and the uniform draws of slot r in stage t, (P, rounds, Dx)
    and (P, rounds), path first; (3, t) the resampling uniforms of stage t, (P,).  A generator is read path by path, so
    path p's numbers do not depend on P, nor a slot's on R."""

    def prior_uniforms(self):
        """(P, R, Dx) uniforms in [0, 1)."""
        return np.stack([self._rng(0, r).random((self.P, self.Dx)) for r in range(self.R)], 1)

    def stage(self, rounds):
        """(u (P,), z (rounds, P, R, Dx), log u (rounds, P, R)) of the next stage."""
        t, self.t = self.t, self.t + 1
        z = np.stack([self._rng(1, r, t).standard_normal((self.P, rounds, self.Dx)) for r in range(self.R)], 1)
        with np.errstate(divide='ignore'):
            logu = np.log(np.stack([self._rng(2, r, t).random((self.P, rounds)) for r in range(self.R)], 1))
        return self._rng(3, t).random(self.P), np.ascontiguousarray(z.transpose(2, 0, 1, 3)), np.ascontiguousarray(logu.transpose(2, 0, 1))


class DeviceSmcStreams(DeviceStageStreams):
    """SmcStreams' twin for rng='device': population.DeviceStageStreams with one log u per particle and round and the
    resampling uniform; stage(rounds) gives (u (P,), z (rounds, P, R, Dx), log u (rounds, P, R))."""

    def __init__(self, e, seed, P, R, Dx):
        super().__init__(e, seed, P, R, Dx, logu_elements=1, resample=True)


def _weighted_quantile(v, wt, q):
    """The q-quantile of the columns of v (n, Dx) under the weights wt (n,): the smallest value whose cumulative weight
    reaches q."""
    out = np.empty(v.shape[1])
    for d in range(v.shape[1]):
        order = np.argsort(v[:, d], kind='stable')
        c = np.cumsum(wt[order])
        out[d] = v[order[min(np.searchsorted(c, q * c[-1]), len(order) - 1)], d]
    return out


class ParticlePosterior:
    """The input posteriors of P function-valued draws as R weighted-equal particles each, with every draw's evidence
    (calibrate_smc, DESIGN I.21).  x (P, R, Dx): the particles at beta = 1, equally weighted samples of p(x | y, f_p);
    loglik, logp (P, R): ll = -1/2 sum_k w_k (ybar_k - f_k(x))^2 and ll + the unnormalised log prior (PathPosterior.logp's
    quantity).  log_evidence (P,): the estimate of log of the integral of prior(x) exp(ll_p(x)) over the box, prior the
    NORMALISED prior on the box; log_norm: the constant the sufficient statistics drop, so that log_evidence + log_norm
    estimates log p(y | f_p).  betas, stage_ess, accept_rate (P, T): per stage the temperature reached, the effective sample
    size of the incremental weights and the mean acceptance of the moves; after a draw reached beta = 1, betas is 1 and
    stage_ess NaN.  step (P, R): the adapted steps.  status (P,): calibrate.SMC_STATUS (= Engine.BOXSMC): ok 0; nan 1 no
    particle had a finite likelihood; max_stages 2 the draw ended below beta = 1 (its particles sample pi_beta, its
    evidence is partial).  n_stages; evaluations: the walk evaluations of the stages, n_stages (n_moves + 1) -- the one of
    the prior particles comes on top.  rng: 'numpy' or 'device', where the run's random numbers were made.
    Evidence weighting: draw_weights() is the softmax of log_evidence over the ok draws.  The draws f_p are P samples of the
    emulator's prior-predictive functions, so weighting them by p(y | f_p) is a self-normalised importance estimate of the
    posterior that feeds the observation back to the emulator -- over P functions only.  draw_ess = 1 / sum W^2 says how
    many of them carry it: when it is small, the weighted answer rests on few draws and more of them are needed; pooled()
    with equal weights stays the modular (cut) posterior."""

    columns = controls = None     # (as PathPosterior's)

    def __init__(self, x, loglik, logp, log_evidence, log_norm, betas, stage_ess, accept_rate, step, status, n_stages, evaluations,
                 rng='numpy'):
        self.rng = rng
        self.x, self.loglik, self.logp, self.log_evidence, self.log_norm = x, loglik, logp, log_evidence, log_norm
        self.betas, self.stage_ess, self.accept_rate, self.step, self.status = betas, stage_ess, accept_rate, step, status
        self.n_stages, self.evaluations = n_stages, evaluations

    def draw_weights(self):
        """(P,): softmax of log_evidence over the draws with status ok, 0 elsewhere (all 0 if there is none)."""
        good = (self.status == SMC_STATUS['ok']) & np.isfinite(self.log_evidence)
        W = np.zeros(len(self.status))
        if good.any():
            e = np.exp(self.log_evidence[good] - self.log_evidence[good].max())
            W[good] = e / e.sum()
        return W

    @property
    def draw_ess(self):
        W = self.draw_weights()
        return 1.0 / np.sum(W * W) if W.any() else 0.0

    def pooled(self):
        """(P R, Dx): every particle of every draw with equal weight, the modular posterior of x."""
        return self.x.reshape(-1, self.x.shape[-1])

    def per_draw(self):
        """(P, R, Dx): the particles of each draw's own posterior p(x | y, f_p)."""
        return self.x

    def pooled_weights(self, kind='evidence'):
        """(P R,): the weights of pooled()'s rows, summing to 1: 'evidence' W_p / R, 'equal' 1 / (P R)."""
        P, R = self.x.shape[:2]
        if kind not in ('evidence', 'equal'):
            raise ValueError("weights must be 'evidence' or 'equal'")
        return np.repeat(self.draw_weights() if kind == 'evidence' else np.full(P, 1.0 / P), R) / R

    def resample(self, n, seed=None, weights='evidence'):
        """(n, Dx): rows of pooled() drawn with replacement under pooled_weights(weights)."""
        wt = self.pooled_weights(weights)
        if not wt.any():
            raise ValueError('resample: no draw with status ok')
        return self.pooled()[np.random.default_rng(seed).choice(len(wt), size=int(n), p=wt / wt.sum())]

    def summary(self, level=0.95, weights='equal'):
        """{'mean', 'lower', 'upper', 'draw_sd'} (Dx,) each: the mean and the equal-tailed interval of probability `level` of
        the pooled particles under pooled_weights(weights), and the (weighted) standard deviation over the draws of their
        own posterior means."""
        if not 0.0 < level < 1.0:
            raise ValueError('summary: level must lie in (0, 1)')
        tail = 0.5 * (1.0 - level)
        pooled, means = self.pooled(), self.x.mean(1)
        if weights == 'equal':
            return {'mean': pooled.mean(0), 'lower': np.quantile(pooled, tail, axis=0), 'upper': np.quantile(pooled, 1.0 - tail, axis=0),
                    'draw_sd': means.std(0, ddof=1) if len(means) > 1 else np.zeros(means.shape[1])}
        wt, W = self.pooled_weights(weights), self.draw_weights()
        if not wt.any():
            raise ValueError('summary: no draw with status ok')
        mean = wt @ pooled
        return {'mean': mean, 'lower': _weighted_quantile(pooled, wt, tail), 'upper': _weighted_quantile(pooled, wt, 1.0 - tail),
                'draw_sd': np.sqrt(W @ (means - mean) ** 2)}


def calibrate_smc(e, P, K, Dx, values, value_and_jac, width, y, obs_sd, bounds, n_particles=1024, n_moves=4, ess_frac=0.5,
                  max_stages=100, seed=None, step=0.1, scale=None, prior=None, target_accept=0.574, *, problem=None, rng='numpy'):
    """The driver behind PathFunctions.calibrate_smc and GpPaths.calibrate_smc: adaptive likelihood tempering (Del Moral,
    Doucet and Jasra 2006) on population.run_stages.  A stage is dgpamd_boxsmc_temper, then n_moves + 1 walk evaluations with
    dgpamd_boxsmc_move behind each: the start of the stage at the resampled particles, then n_moves decisions.  Only the count
    of draws below beta = 1 visits the host, once per stage.  rng='device': every random number is made on the device
    (DeviceSmcStreams); the prior uniforms visit the host once, for prior_draws.  problem: as in calibrate; its log_norm is the
    result's."""
    device_rng = check_rng(rng, 'calibrate_smc')
    if problem is not None:
        K, Dx, value_and_jac = problem.K, problem.Dx, problem.value_and_jac
    lo, hi = optimize.check_bounds(bounds, Dx, 'calibrate_smc')
    Dx = len(lo)
    ybar, w = observation(y, obs_sd, K) if problem is None else (problem.ybar, problem.w)
    pv, pm = check_prior(prior, Dx)
    R, n_moves, max_stages = int(n_particles), int(n_moves), int(max_stages)
    if not 1 <= R <= MAX_PARTICLES:
        raise ValueError('calibrate_smc: need 1 <= n_particles <= %d' % MAX_PARTICLES)
    if n_moves < 1 or max_stages < 1:
        raise ValueError('calibrate_smc: need n_moves >= 1 and max_stages >= 1')
    if not 0.0 < ess_frac < 1.0:
        raise ValueError('calibrate_smc: ess_frac must lie in (0, 1)')
    scale = check_step('calibrate_smc', lo, hi, scale, step, target_accept)
    streams = DeviceSmcStreams(e, seed, P, R, Dx) if device_rng else SmcStreams(seed, P, R, Dx)
    xt = e.tensor(prior_particles(streams, lo, hi, pv, pm))
    state = e.boxsmc_state(P, R, Dx, w, ybar, lo, hi, scale, pv, pm, h0=step)
    betas, stage_ess = [], []

    move = lambda z, logu, first, last: e.boxsmc_move(state, *value_and_jac(xt), xt, z, logu, HMIN, HMAX, first=first, last=last)

    def temper(u):
        e.boxsmc_temper(state, xt, u, ess_frac)
        betas.append(state['beta'].clone()), stage_ess.append(state['stage_ess'].clone())
    # the likelihood of the prior particles: a stage's start under beta = 0 that ends at once (z and log u are not read)
    move(e.zeros(P, R, Dx), e.zeros(P, R), first=True, last=True)
    # the draw's step for the next stage follows this stage's acceptance over all its particles (see stage_gain)
    accept = run_stages(e, streams, state, n_moves, max_stages, target_accept, temper, move,
                        lambda gain: state['h'].view(P, R).mul_(gain[:, None]).clamp_(HMIN, HMAX))
    host = {k: state[k].cpu().numpy() for k in ('x', 'll', 'lprior', 'h', 'beta', 'log_evidence', 'draw_status')}
    T = len(betas)
    stack = lambda ts: np.ascontiguousarray(torch.stack(ts, 1).cpu().numpy())
    ll = host['ll'].reshape(P, R)
    res = ParticlePosterior(particles(host['x'], P, R), ll, ll + host['lprior'].reshape(P, R), host['log_evidence'],
                            log_norm(y, obs_sd, K) if problem is None else problem.log_norm, stack(betas), stack(stage_ess),
                            stack(accept), host['h'].reshape(P, R),
                            draw_status(SMC_STATUS, host['draw_status'], host['beta'] < 1.0), T, T * (n_moves + 1), rng)
    if problem is not None:
        res.columns, res.controls = problem.columns, problem.controls
    return res
